#!/usr/bin/env python3
"""Cost of the per-env Fried parameter on the hot path, at the C2 geometry (8 m, 20 x 20 Shack-Hartmann, 256 envs, float32,
run_integrator): env-steps per second with set_r0_per_env active against the same build with the feature off.
    python scripts/time_r0_env.py [n_envs] [steps] [repeats]
Each figure is the median over `repeats` timed runs of `steps` on-device integrator steps after a warm-up run,
torch.cuda.synchronize() on both sides; the two states alternate so that clock drift hits both alike.  One JSON line."""
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rlao_amd.env import BatchedAOEnv  # noqa: E402

GEOMETRY = dict(diameter=8.0, nSubaperture=20, nPixelPerSubap=6, r0=0.13, L0=30.0, windSpeed=[10.0], windDirection=[72.0],
                fractionalR0=[1.0], altitude=[0.0], nModes=50, nLoop=64)


def run_ms(env, steps):
    n_loop = int(env.param.nLoop)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    done = 0
    while done < steps:
        k = min(n_loop, steps - done)
        env.run_integrator(0, k, 0.5)
        done += k
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0)


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 256
    steps = int(sys.argv[2]) if len(sys.argv) > 2 else 512
    repeats = max(5, int(sys.argv[3]) if len(sys.argv) > 3 else 9)
    env = BatchedAOEnv(n_envs=n, device=0, dtype="f32", return_frame=False)
    env.set_params(GEOMETRY, camera="ideal", wfs_type="shackhartmann")
    r0 = np.exp(np.random.RandomState(0).uniform(np.log(0.05), np.log(0.25), n))      # a seeing sweep, log-uniform
    t = {"off": [], "per_env_r0": []}
    for rep in range(repeats + 1):
        for state in ("off", "per_env_r0"):
            if state == "off":
                env.atm.r0 = GEOMETRY["r0"]
            else:
                env.set_r0_per_env(r0)
            env.generate_new_phase_screen(100 + rep)
            env.dm.coefs = 0
            env.dm_prev = 0
            env.measure()
            env.reset_soft()
            ms = run_ms(env, steps)
            if rep:                                                 # (the first round is the warm-up)
                t[state].append(ms)
    out = {"n_envs": n, "steps": steps, "repeats": repeats, "fused_step": bool(env.fused_step)}
    for state, v in t.items():
        v = np.array(v)
        out[state] = {"env_steps_per_s": round(n * steps / (1e-3 * float(np.median(v)))), "median_ms": round(float(np.median(v)), 3),
                      "min_ms": round(float(v.min()), 3), "max_ms": round(float(v.max()), 3)}
    out["finite"] = bool(torch.isfinite(env._obs).all())
    env.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
