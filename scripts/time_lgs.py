#!/usr/bin/env python3
"""What the laser-guide-star spots (aoenv_set_lgs_spots, k_sh_spots_lgs) cost, float32, at the headline shard: C2 (8 m, 20 x 20
Shack-Hartmann, R = 120, p = 6, 316 valid lenslets), 256 envs, photon-noise camera.
    python scripts/time_lgs.py [--out file.json] [--label text] [--parent a.json ...] [--bench-this b.json ...] [--bench-parent b.json ...]
                               [n_envs] [steps] [repeats]
One NGS-calibrated env; the table is set on and forgotten from its loop shard, so every arm runs the same calibration and screens:
  none         run_integrator with nothing set: the fused step kernel (the headline's path)
  batched      the same with AOENV_OPT_FUSED_STEP off: the batched kernels an LGS shard runs, WITHOUT a table -- k_sh_spots_p6
  lgs_boxed    a shared table with truncated kernels (a 6 km sodium layer, FWHM 0.08, launch (2, 0) m: 32 .. 45 non-zero taps a lenslet,
               whose union over the lenslets is a 9 x 9 box of the 12 x 12 taps) -- k_sh_spots_lgs
  lgs_dense    a shared table with every tap non-zero (the 20 km layer, FWHM 1.0, launch (4, 0) m)
  lgs_per_env  the boxed table once per env (46 MB: no longer L2-resident beside the frames)
  none_again   nothing set again (the A/A spread of the session)
Per arm: us per step of the loop (wall clock over `steps` steps, median [min .. max] over the rounds, the first round a warm-up) and
us per launch of the spots kernel in the AOENV_K_SH_SPOTS slot of aoenv_profile over the same steps (the fused arms have none).
--parent merges runs of this script on other libraries (AOENV_LIB=that library), each under its --label: the parent commit's (it has
no table, only none / batched / none_again are timed) and earlier forms of the kernel; --bench-this / --bench-parent merge result lines of plain `bench.py --steps 200 --warmup 20`.  One JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from rlao_amd import _lib as L  # noqa: E402
from rlao_amd import calib  # noqa: E402
from rlao_amd.env import BatchedAOEnv  # noqa: E402

GAIN = 0.5
C2 = dict(diameter=8.0, nSubaperture=20, nPixelPerSubap=6, r0=0.13, L0=30.0, windSpeed=[10.0], windDirection=[72.0],
          fractionalR0=[1.0], altitude=[0.0], nModes=50)


def _library_has_lgs():
    import ctypes
    return hasattr(ctypes.CDLL(L.LIB_PATH), "aoenv_set_lgs_spots")


HAVE = _library_has_lgs()


def na_profile(width=20e3):
    """11 samples over `width` around 90 km, a Gaussian density"""
    h = np.linspace(90e3 - width / 2, 90e3 + width / 2, 11)
    w = np.exp(-0.5 * ((h - 90e3) / (width / 4)) ** 2)
    return np.stack([h, w / w.sum()])


def episode(env, seed):
    env.generate_new_phase_screen(seed)
    env.dm.coefs = 0
    env.dm_prev = 0
    env.measure()
    env.SR = []
    return env.reset_soft()


def stats(v, per):
    return {"median": round(float(np.median(v)) / per, 3), "min": round(min(v) / per, 3), "max": round(max(v) / per, 3)}


def tables(env):
    out = {}
    for name, width, fwhm, launch in (("lgs_boxed", 6e3, 0.08, [2.0, 0.0]), ("lgs_dense", 20e3, 1.0, [4.0, 0.0])):
        K, _ = calib.lgs_spot_kernels(env.param, env._sh_tables, na_profile(width), fwhm, launch)
        taps, box = calib.lgs_binned_taps(K)
        out[name] = (taps, box, False)
    taps, box, _ = out["lgs_boxed"]
    out["lgs_per_env"] = (np.broadcast_to(taps, (env.n_envs,) + taps.shape).copy(), box, True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--label", default="the committed library")
    ap.add_argument("--parent", nargs="*", default=[])
    ap.add_argument("--bench-this", nargs="*", default=[])
    ap.add_argument("--bench-parent", nargs="*", default=[])
    ap.add_argument("n_envs", nargs="?", type=int, default=256)
    ap.add_argument("steps", nargs="?", type=int, default=256)
    ap.add_argument("repeats", nargs="?", type=int, default=5)
    a = ap.parse_args()
    n, steps = a.n_envs, a.steps
    env = BatchedAOEnv(n_envs=n, device=0, dtype="f32", return_frame=False)
    env.set_params(dict(C2, nLoop=steps), camera="papyrus", wfs_type="shackhartmann", gainCL=GAIN)
    sh = env._shard
    tabs = tables(env) if HAVE else {}
    arms = ("none", "batched") + tuple(tabs) + ("none_again",)
    t, k_us, fused, boxes = {k: [] for k in arms}, {k: [] for k in arms}, {}, {}
    for rep in range(a.repeats + 1):
        for arm in arms:
            if HAVE:
                sh.set_lgs_spots(None, stream=env._stream())
            L.check(sh.lib.aoenv_set_option(sh.h, L.OPT_FUSED_STEP, 0 if arm == "batched" else 1))
            if arm in tabs:
                taps, box, per_env = tabs[arm]
                sh.set_lgs_spots(taps, box, per_env=per_env, stream=env._stream())
                boxes[arm] = [int(v) for v in box]
            fused[arm] = bool(env.fused_step)
            episode(env, 100 + rep)
            env.run_integrator(0, 2, GAIN)                          # (untimed: the first launches after the allocation)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            env.run_integrator(0, steps, GAIN)
            torch.cuda.synchronize()
            if rep:
                t[arm].append(1e6 * (time.perf_counter() - t0))
            if not fused[arm]:                                      # the spots kernel over the same steps, by aoenv_profile
                episode(env, 100 + rep)
                sh.profile(True)
                env.run_integrator(0, steps, GAIN)
                ms, cnt = sh.profile_read(env._stream())["sh_spots"]
                sh.profile(False)
                if rep and cnt:
                    k_us[arm].append(1e3 * ms / cnt)
    if HAVE:
        sh.set_lgs_spots(None, stream=env._stream())
    L.check(sh.lib.aoenv_set_option(sh.h, L.OPT_FUSED_STEP, 1))
    out = {"script": "scripts/time_lgs.py", "library": a.label, "device": torch.cuda.get_device_name(0), "dtype": "float32",
           "geometry": "C2, one ground layer", "n_envs": n, "steps": steps, "repeats": a.repeats, "n_valid_lenslets": int(env._sh_tables.nValid),
           "fused_step": fused, "box_x0_y0_nx_ny": boxes,
           "loop_us_per_step": {k: stats(v, steps) for k, v in t.items()},
           "spots_kernel_us_per_launch": {k: stats(v, 1) for k, v in k_us.items() if v}}
    us = out["loop_us_per_step"]
    out["a_a_spread_us"] = round(abs(us["none"]["median"] - us["none_again"]["median"]), 3)
    env.close()
    if a.parent:
        out["other_libraries"] = []
        for path in a.parent:
            par = json.load(open(path))
            out["other_libraries"].append({k: par[k] for k in ("library", "loop_us_per_step", "spots_kernel_us_per_launch", "a_a_spread_us")})
    for key, paths in (("bench_this", a.bench_this), ("bench_parent", a.bench_parent)):
        if paths:
            out[key] = [json.loads([l for l in open(p).read().splitlines() if l.startswith("{")][-1]) for p in paths]
    print(json.dumps(out))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
