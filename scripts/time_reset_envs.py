#!/usr/bin/env python3
"""Cost of an episode reset at the C2 geometry (8 m, 20 x 20 Shack-Hartmann, 256 envs, float32): the full reset
(generate_new_phase_screen) against reset_envs of 1, 32 and all envs.
    python scripts/time_reset_envs.py [n_envs] [calls]
Median wall time of `calls` (>= 20) calls after warm-up, torch.cuda.synchronize() on both sides of every call; one JSON line.
reset_envs includes its measurement and reset_soft(); the full reset is timed bare and with the same epilogue
(dm.coefs = 0, dm_prev = 0, measure, reset_soft), which is what reset_envs replaces.  The shard runs per-env clocks after the
first reset_envs, so the full resets are timed first, on the shared clock, and once more at the end on per-env clocks."""
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


def median_ms(fn, calls, warmup=3):
    t = []
    for k in range(warmup + calls):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn(k)
        torch.cuda.synchronize()
        t.append(1e3 * (time.perf_counter() - t0))
    t = np.array(t[warmup:])
    return {"median_ms": round(float(np.median(t)), 3), "min_ms": round(float(t.min()), 3), "max_ms": round(float(t.max()), 3)}


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 256
    calls = max(20, int(sys.argv[2]) if len(sys.argv) > 2 else 20)
    env = BatchedAOEnv(n_envs=n, device=0, dtype="f32", return_frame=False)
    env.set_params(GEOMETRY, camera="ideal", wfs_type="shackhartmann")

    def full(k):
        env.generate_new_phase_screen(100 + k)

    def full_episode(k):
        env.generate_new_phase_screen(200 + k)
        env.dm.coefs = 0
        env.dm_prev = 0
        env.measure()
        env.reset_soft()

    out = {"n_envs": n, "calls": calls, "full_reset": median_ms(full, calls), "full_reset_with_prologue": median_ms(full_episode, calls)}
    if hasattr(env, "reset_envs"):
        for m in sorted({1, min(32, n), n}):
            ids = np.linspace(0, n - 1, m).round().astype(np.int64)          # spread over the shard
            out[f"reset_envs_{m}"] = median_ms(lambda k: env.reset_envs(ids, seed=300 + k), calls)
        out["full_reset_per_env_clocks"] = median_ms(full, calls)
    # the loop still runs
    obs = env.reset_soft()
    for i in range(4):
        obs = env.step(i, 0.5 * obs)[0]
    out["finite"] = bool(torch.isfinite(obs).all())
    env.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
