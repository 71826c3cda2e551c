#!/usr/bin/env python3
"""What the off-axis science target (BatchedAOEnv.set_science_direction / science_residual / record_science_direction) costs,
float32, at the C2 shard (8 m, 20 x 20 Shack-Hartmann, R = 120, 256 envs) with two layers at 0 and 10 km under fov = 1 and
fov = 20 arcsec (grids 124 / 125 and 124 / 139: layers on grids of their own, the batched kernels).
    python scripts/time_offaxis.py [--out file.json] [--label text] [--parent a.json [b.json ...]] [n_envs] [steps] [repeats]
Per field of view, every env at zenith fov / 2 with azimuths spread over the circle (every env blends):
  residual    us per science_residual() launch: k_science_residual alone (AOENV_OPT_STORE_ATM_OPD is on for this arm, so the
              on-axis OPD is not re-derived in front of it), `calls` calls per timed run, torch.cuda.synchronize() on both sides
  phase       the yardstick, us per launch of the batched phase kernel (AOENV_K_PHASE) on the same shard, from aoenv_profile
              over the steps of the integrator: that kernel does this kernel's warp plus the mirror product, without the blend
  loop        us per step of run_integrator (photon-noise camera) with nothing attached, with a direction set but no record,
              with the record attached, and with nothing attached again (the A/A spread of the session); arms interleaved inside
              every round, the first round a warm-up; median [min .. max] over the rounds
--parent merges the `none` arms of runs of this script on the parent commit's library (AOENV_LIB=that library: it has no
science direction, only `none` is timed).  One JSON line."""
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
C2 = dict(diameter=8.0, nSubaperture=20, nPixelPerSubap=6, r0=0.13, L0=30.0, windSpeed=[10.0, 15.0], windDirection=[72.0, 200.0],
          fractionalR0=[0.65, 0.35], altitude=[0.0, 10000.0], nModes=50)


def _library_has_direction():
    import ctypes
    return hasattr(ctypes.CDLL(L.LIB_PATH), "aoenv_set_science_direction")


HAVE = _library_has_direction()


def make_env(n, n_loop, fov):
    env = BatchedAOEnv(n_envs=n, device=0, dtype="f32", return_frame=False)
    env.set_params(dict(C2, nLoop=n_loop, fov=fov), camera="papyrus", wfs_type="shackhartmann", gainCL=GAIN)
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


def directions(env, fov):
    n = env.n_envs
    env.set_science_direction(np.full(n, fov / 2), 360.0 * np.arange(n) / n + 7.0)


def one_field(n, steps, repeats, fov, calls):
    env = make_env(n, steps, fov)
    out = {"fov_arcsec": fov, "grids": list(env._atm_tables.layer_res), "fused_step": bool(env.fused_step)}
    arms = ("none", "direction_set", "record", "none_again") if HAVE else ("none", "none_again")
    t = {k: [] for k in arms}
    res, phase_us, sr = [], [], None
    for rep in range(repeats + 1):
        for arm in arms:
            episode(env, 100 + rep)
            if HAVE:
                env.clear_science_direction()
                if arm in ("direction_set", "record"):
                    directions(env, fov)
                if arm == "record":
                    env.record_science_direction(0, steps)
            env.run_integrator(0, 2, GAIN)                          # (untimed: the first launches after the allocation)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            env.run_integrator(0, steps, GAIN)
            torch.cuda.synchronize()
            if rep:
                t[arm].append(1e6 * (time.perf_counter() - t0))
            if arm == "record":
                sr = float(env._oa_rec[:, 1].mean())
        # the yardstick: the batched phase kernel over the same steps, by aoenv_profile
        if HAVE:
            env.clear_science_direction()
        episode(env, 100 + rep)
        env._shard.profile(True)
        env.run_integrator(0, steps, GAIN)
        ms, cnt = env._shard.profile_read(env._stream())["phase"]
        env._shard.profile(False)
        if rep and cnt:
            phase_us.append(1e3 * ms / cnt)
        # the kernel alone
        if HAVE:
            directions(env, fov)
            L.check(env._shard.lib.aoenv_set_option(env._shard.h, L.OPT_STORE_ATM_OPD, 1))
            env.step(0, GAIN * env._obs)
            env.science_residual()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(calls):
                env.science_residual()
            torch.cuda.synchronize()
            if rep:
                res.append(1e6 * (time.perf_counter() - t0) / calls)
            L.check(env._shard.lib.aoenv_set_option(env._shard.h, L.OPT_STORE_ATM_OPD, 0))
    us = {k: stats(v, steps) for k, v in t.items()}
    out["loop_us_per_step"] = us
    out["a_a_spread_us"] = round(abs(us["none"]["median"] - us["none_again"]["median"]), 3)
    if phase_us:
        out["phase_kernel_us_per_launch"] = stats(phase_us, 1)
    if HAVE:
        base = 0.5 * (us["none"]["median"] + us["none_again"]["median"])
        out["record_minus_none_us"] = round(us["record"]["median"] - base, 3)
        out["direction_set_minus_none_us"] = round(us["direction_set"]["median"] - base, 3)
        out["science_residual_us_per_call"] = stats(res, 1)
        out["mean_recorded_strehl"] = round(sr, 4)
    env.close()
    print(f"[fov {fov}] {out}", file=sys.stderr, flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--label", default="the committed library")
    ap.add_argument("--parent", nargs="*", default=[])
    ap.add_argument("n_envs", nargs="?", type=int, default=256)
    ap.add_argument("steps", nargs="?", type=int, default=256)
    ap.add_argument("repeats", nargs="?", type=int, default=5)
    a = ap.parse_args()
    out = {"script": "scripts/time_offaxis.py", "library": a.label, "device": torch.cuda.get_device_name(0), "dtype": "float32",
           "geometry": "C2, two layers at 0 / 10 km", "n_envs": a.n_envs, "steps": a.steps, "repeats": a.repeats, "calls": 100,
           "fields": [one_field(a.n_envs, a.steps, a.repeats, fov, 100) for fov in (1.0, 20.0)]}
    if a.parent:
        out["parent_library"] = []
        for path in a.parent:
            par = json.load(open(path))
            out["parent_library"].append({"label": par["library"], "fields": [
                {"fov_arcsec": f["fov_arcsec"], "loop_us_per_step": f["loop_us_per_step"], "a_a_spread_us": f["a_a_spread_us"],
                 "phase_kernel_us_per_launch": f.get("phase_kernel_us_per_launch")} for f in par["fields"]]})
    print(json.dumps(out))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
