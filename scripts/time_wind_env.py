#!/usr/bin/env python3
"""Cost of per-env winds above one pixel per frame (AOENV_OPT_ENV_WIND_PIXELS, the whole-pixel ring rounds) at the C2 geometry
(8 m, 20 x 20 Shack-Hartmann, 256 envs, float32, ideal camera, run_integrator on per-env clocks).
    python scripts/time_wind_env.py [--parent-lib libaoenv.so] [--out file.json] [n_envs] [steps] [repeats]
(a) slow winds (every env below a pixel per frame): ceiling 4 against ceiling 1 -- with --parent-lib, ceiling 1 is run on THAT
    library (a build of the commit before the feature, loaded beside this one in the same process), twice, as two shards "A" and
    "B": their difference is the A/A spread of the session, and it is the pass mark for "ceiling 4 on this library costs
    nothing".  Without --parent-lib the A/A pair and the ceiling-1 side are this library's.
(b) the same winds, but env 0 at 0.x, 1.x, 2.x and 3.x pixels per frame (ceiling 4): the time per step, and so the cost of one
    more round (prepare + GEMM over the whole shard + scatter with the min / max pass).
Each figure is the median over `repeats` timed runs of `steps` on-device integrator steps after a warm-up round,
torch.cuda.synchronize() on both sides; the states alternate inside every round so that clock drift hits all alike.  One JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rlao_amd import _lib as L  # noqa: E402
from rlao_amd.env import BatchedAOEnv  # noqa: E402

GEOMETRY = dict(diameter=8.0, nSubaperture=20, nPixelPerSubap=6, r0=0.13, L0=30.0, windSpeed=[10.0], windDirection=[72.0],
                fractionalR0=[1.0], altitude=[0.0], nModes=50, nLoop=64)
PX_PER_FRAME = 8.0 / 120 / 0.002                                   # one pixel per frame [m/s]: 6.67 cm at 500 Hz


def make_env(n, lib_path=None):
    """a shard on libaoenv at lib_path (None: this tree's); every call of a shard goes through the library it was created on"""
    if lib_path is not None:
        L._lib, L.LIB_PATH = None, os.path.abspath(lib_path)
    env = BatchedAOEnv(n_envs=n, device=0, dtype="f32", return_frame=False)
    env.set_params(GEOMETRY, camera="ideal", wfs_type="shackhartmann")
    return env


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


def episode(env, seed, speed, direction):
    env.generate_new_phase_screen(seed)
    env.set_wind_per_env(speed, direction, reset=True)
    env.dm.coefs = 0
    env.dm_prev = 0
    env.measure()
    env.reset_soft()


def summary(v, n, steps):
    v = np.array(v)
    med = float(np.median(v))
    return {"env_steps_per_s": round(n * steps / (1e-3 * med)), "us_per_step": round(1e3 * med / steps, 3), "median_ms": round(med, 3),
            "min_ms": round(float(v.min()), 3), "max_ms": round(float(v.max()), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("n_envs", nargs="?", type=int, default=256)
    ap.add_argument("steps", nargs="?", type=int, default=2048)
    ap.add_argument("repeats", nargs="?", type=int, default=9)
    a = ap.parse_args()
    n, steps, repeats = a.n_envs, a.steps, max(5, a.repeats)
    rs = np.random.RandomState(0)
    speed, direction = rs.uniform(5.0, 15.0, size=(n, 1)), rs.uniform(0.0, 360.0, size=(n, 1))     # below half a pixel per frame
    this_lib = L.LIB_PATH
    envs = {"ceiling4": make_env(n, this_lib)}
    envs["ceiling4"].set_wind_ceiling(4)
    envs["ceiling1_A"] = make_env(n, a.parent_lib or this_lib)
    envs["ceiling1_B"] = make_env(n, a.parent_lib or this_lib)
    L._lib, L.LIB_PATH = None, this_lib
    t = {k: [] for k in ("ceiling1_A", "ceiling4", "ceiling1_B")}
    for rep in range(repeats + 1):
        for state in t:
            episode(envs[state], 100 + rep, speed, direction)
            ms = run_ms(envs[state], steps)
            if rep:                                                 # (the first round is the warm-up)
                t[state].append(ms)
    out = {"n_envs": n, "steps": steps, "repeats": repeats, "fused_step": bool(envs["ceiling4"].fused_step),
           "ceiling1_library": "parent commit" if a.parent_lib else "this build"}
    slow = {k: summary(v, n, steps) for k, v in t.items()}
    a_a = abs(slow["ceiling1_A"]["median_ms"] - slow["ceiling1_B"]["median_ms"])
    ref = 0.5 * (slow["ceiling1_A"]["median_ms"] + slow["ceiling1_B"]["median_ms"])
    diff = slow["ceiling4"]["median_ms"] - ref
    same = all(torch.equal(envs["ceiling4"]._obs, envs[k]._obs) for k in ("ceiling1_A", "ceiling1_B"))
    slow.update(a_a_spread_ms=round(a_a, 3), ceiling4_minus_ceiling1_ms=round(diff, 3), within_a_a_spread=bool(abs(diff) <= a_a),
                same_observations=bool(same))
    out["slow_winds"] = slow
    for k in ("ceiling1_A", "ceiling1_B"):
        envs[k].close()
    # (b) env 0 faster and faster, the others as before
    env = envs["ceiling4"]
    cases = {"max_0.x": None, "max_1.x": 1.5, "max_2.x": 2.5, "max_3.x": 3.5}
    tb = {k: [] for k in cases}
    for rep in range(repeats + 1):
        for k, px in cases.items():
            s, d = speed.copy(), direction.copy()
            if px is not None:
                s[0, 0], d[0, 0] = px * PX_PER_FRAME, 0.0
            episode(env, 200 + rep, s, d)
            ms = run_ms(env, steps)
            if rep:
                tb[k].append(ms)
    fast = {k: summary(v, n, steps) for k, v in tb.items()}
    us = [fast[k]["us_per_step"] for k in cases]
    fast["us_per_extra_round"] = [round(us[i + 1] - us[i], 3) for i in range(3)]
    out["fastest_env"] = fast
    out["finite"] = bool(torch.isfinite(env._obs).all())
    env.close()
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
