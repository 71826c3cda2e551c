#!/usr/bin/env python3
"""What the science camera (BatchedAOEnv.set_science / science_psf / start_long_exposure) costs, float32, at the C2 shard (8 m,
20 x 20 Shack-Hartmann, R = 120, 256 envs).
    python scripts/time_science.py [--out file.json] [--label text] [--skip-window] [--skip-loop] [--parent a.json [b.json ...]]
                                   [n_envs] [steps] [repeats]
Part 1, the window alone, zp = 4, W in {32, 64, 130, 480}: `calls` calls per timed run, arms interleaved inside every round so
that clock drift hits all alike, the first round a warm-up, torch.cuda.synchronize() on both sides; median [min .. max] over the
rounds in us per call:
  mfma, mfma_again   aoenv_science_psf on the matrix-core kernel (their difference is the A/A spread of the session)
  general            AOENV_PATH_SCI_GENERAL: the fma-chain kernel
  full_render        aoenv_compute_psf(4) on the same shard -- the only route before the window existed; it renders all 480 x 480
                     pixels whatever W is
With the flop count of the two products written as real products of doubled contraction length, 8 R^2 U + 8 R U^2 per env
(U = 2 W), and its share of the 157.3 TFLOP/s fp32 matrix peak at the matrix-core kernel's median.
Part 2, the loop: us per step of the C2 on-device integrator (run_integrator, photon-noise camera) with nothing set, with the
camera set but nothing attached, and with the long exposure attached (W = 130, first_frame = 0: every step accumulates).
--parent merges the `none` arms of runs of this script on the parent commit's library (AOENV_LIB=that library, --skip-window: it
has no science entry points, only `none` is timed).
One JSON line."""
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
from rlao_amd.env import BatchedAOEnv  # noqa: E402

GAIN = 0.5
FP32_MATRIX_PEAK = 157.3e12
C2 = dict(diameter=8.0, nSubaperture=20, nPixelPerSubap=6, r0=0.13, L0=30.0, windSpeed=[10.0], windDirection=[72.0],
          fractionalR0=[1.0], altitude=[0.0], nModes=50)
NEW = ("aoenv_set_science", "aoenv_science_psf", "aoenv_set_science_accumulator")


def _library_has_science():
    """False for the parent commit's library (AOENV_LIB): the binding then declares the entry points that library has"""
    import ctypes
    try:
        ctypes.CDLL(L.LIB_PATH).aoenv_set_science
        return True
    except AttributeError:
        for name in NEW:
            L.EXPORTS.pop(name, None)
        return False


HAVE_SCI = _library_has_science()


def make_env(n, n_loop, camera):
    env = BatchedAOEnv(n_envs=n, device=0, dtype="f32", return_frame=False)
    env.set_params(dict(C2, nLoop=n_loop), camera=camera, wfs_type="shackhartmann", gainCL=GAIN)
    return env


def episode(env, seed):
    env.generate_new_phase_screen(seed)
    env.dm.coefs = 0
    env.dm_prev = 0
    env.measure()
    env.SR = []
    return env.reset_soft()


def stats(v, per):
    return {"median": round(float(np.median(v)) / per, 3), "min": round(min(v) / per, 3), "max": round(max(v) / per, 3)}


def window_flops(R, W, n):
    U = 2 * W
    return n * (8 * R * R * U + 8 * R * U * U)


def window(n, ws, calls, repeats):
    env = make_env(n, 8, "ideal")
    obs = episode(env, 17)
    for i in range(3):
        obs = env.step(i, GAIN * obs)[0]
    rows = []
    for W in ws:
        env.set_science(zero_padding=4, window=W)
        arms = {"mfma": 0, "general": L.PATH_SCI_GENERAL, "full_render": None, "mfma_again": 0}
        t = {k: [] for k in arms}
        for rep in range(repeats + 1):
            for k, path in arms.items():
                if path is None:
                    call, m = (lambda: env.tel.computePSF(4)), max(1, calls // 20)
                else:
                    L.check(env._shard.lib.aoenv_set_option(env._shard.h, L.OPT_FORCE_PATH, path))
                    call, m = env.science_psf, (calls if k != "general" else max(1, calls // 10))
                call()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(m):
                    call()
                torch.cuda.synchronize()
                if rep:
                    t[k].append(1e6 * (time.perf_counter() - t0) / m)
        L.check(env._shard.lib.aoenv_set_option(env._shard.h, L.OPT_FORCE_PATH, 0))
        us = {k: stats(v, 1) for k, v in t.items()}
        flops = window_flops(env.R, W, n)
        rows.append({"W": W, "us_per_call": us, "a_a_spread_us": round(abs(us["mfma"]["median"] - us["mfma_again"]["median"]), 3),
                     "flop": flops, "mfma_tflops": round(flops / us["mfma"]["median"] / 1e6, 2),
                     "fraction_of_fp32_matrix_peak": round(flops / (us["mfma"]["median"] * 1e-6) / FP32_MATRIX_PEAK, 4),
                     "full_render_over_mfma": round(us["full_render"]["median"] / us["mfma"]["median"], 2)})
        print(f"[window] W={W}: {rows[-1]}", file=sys.stderr, flush=True)
    out = {"geometry": "C2", "n_envs": n, "R": env.R, "zero_padding": 4, "calls": calls, "repeats": repeats, "sweep": rows}
    env.close()
    return out


def loop(n, steps, repeats, arms):
    env = make_env(n, steps, "papyrus")

    def prepare(arm):
        if not HAVE_SCI:
            return
        env.clear_science()
        if arm.startswith("none"):
            return
        env.set_science(zero_padding=4, window=130, first_frame=0)
        if arm == "long_exposure":
            env.start_long_exposure()

    t = {k: [] for k in arms}
    sr = {}
    for rep in range(repeats + 1):
        for arm in arms:
            episode(env, 100 + rep)
            prepare(arm)
            env.run_integrator(0, 2, GAIN)                          # (untimed: the first launches after set_science's allocation)
            if arm == "long_exposure":
                env.zero_long_exposure()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            env.run_integrator(0, steps, GAIN)
            torch.cuda.synchronize()
            if rep:
                t[arm].append(1e6 * (time.perf_counter() - t0))
            if arm == "long_exposure":
                sr[arm] = float(env.long_exposure_strehl().mean())
                assert int(env.long_exposure()[1].min()) == steps
    if HAVE_SCI:
        env.clear_science()
    us = {k: stats(v, steps) for k, v in t.items()}
    out = {"geometry": "C2", "n_envs": n, "R": env.R, "steps": steps, "repeats": repeats, "window": 130, "camera": "papyrus",
           "fused_step": bool(env.fused_step), "us_per_step": us, "a_a_spread_us": round(abs(us["none"]["median"] - us["none_again"]["median"]), 3)}
    if "long_exposure" in us:
        base = 0.5 * (us["none"]["median"] + us["none_again"]["median"])
        out["long_exposure_minus_none_us"] = round(us["long_exposure"]["median"] - base, 3)
        out["mean_long_exposure_strehl"] = round(sr["long_exposure"], 4)
    env.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--label", default="the committed library")
    ap.add_argument("--skip-window", action="store_true")
    ap.add_argument("--skip-loop", action="store_true")
    ap.add_argument("--parent", nargs="*", default=[], help="records of the parent commit's library: their `none` arms are put beside this run's")
    ap.add_argument("n_envs", nargs="?", type=int, default=256)
    ap.add_argument("steps", nargs="?", type=int, default=512)
    ap.add_argument("repeats", nargs="?", type=int, default=5)
    a = ap.parse_args()
    out = {"script": "scripts/time_science.py", "library": a.label, "device": torch.cuda.get_device_name(0), "dtype": "float32"}
    if not a.skip_window and HAVE_SCI:
        out["window"] = window(a.n_envs, (32, 64, 130, 480), 100, a.repeats)
    if not a.skip_loop:
        arms = ("none", "camera_set", "long_exposure", "none_again") if HAVE_SCI else ("none", "none_again")
        out["loop"] = loop(a.n_envs, a.steps, a.repeats, arms)
    if a.parent:
        out["loop"]["parent_library"] = []
        for path in a.parent:
            par = json.load(open(path))
            out["loop"]["parent_library"].append({"label": par["library"], "us_per_step": par["loop"]["us_per_step"],
                                                  "a_a_spread_us": par["loop"]["a_a_spread_us"]})
    print(json.dumps(out))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
