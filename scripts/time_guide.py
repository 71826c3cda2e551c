#!/usr/bin/env python3
"""What the off-axis guide star (BatchedAOEnv.set_guide_direction, k_guide_opd) costs, float32, at the shard of
scripts/time_offaxis.py: C2 (8 m, 20 x 20 Shack-Hartmann, R = 120, 256 envs) with two layers at 0 and 10 km under fov = 1 and
fov = 20 arcsec (grids 124 / 125 and 124 / 139), photon-noise camera.
    python scripts/time_guide.py [--out file.json] [--label text] [--parent a.json [b.json ...]] [n_envs] [steps] [repeats]
Per field of view, every env at zenith fov / 2 with azimuths spread over the circle (every env blends):
  guide_opd   us per launch of k_guide_opd.  The kernel has no entry of its own and no AoKernel id; a guided step is the unguided
              step with k_guide_opd in front of the phase kernel and that kernel reading the OPD where it formed it, so
                  k_guide_opd = (loop, guide set) - (loop, nothing set) + (phase from the screens) - (phase on the given OPD)
              with both phase kernels from aoenv_profile over the integrator's steps in their own state.  One gap between two
              kernels is part of the figure.
  phase       yardstick 1, us per launch of the batched phase kernel (AOENV_K_PHASE) from the screens, no direction set, from
              aoenv_profile over the steps of the integrator; phase_given: the same kernel on the OPD k_guide_opd wrote
  science     yardstick 2, us per science_residual() launch at the same directions (k_science_residual alone:
              AOENV_OPT_STORE_ATM_OPD is on for this arm), by the same device events
  loop        us per step of run_integrator with nothing set, with a guide direction set (the batched kernels + k_guide_opd) and
              with nothing set again (the A/A spread of the session); arms interleaved inside every round, the first round a
              warm-up; median [min .. max] over the rounds
--parent merges the `none` arms of runs of this script on the parent commit's library (AOENV_LIB=that library: it has no guide
direction, only `none` is timed).  One JSON line."""
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

sys.path.insert(0, os.path.join(REPO, "scripts"))
from time_offaxis import GAIN, episode, make_env, stats  # noqa: E402


def _library_has_guide():
    import ctypes
    return hasattr(ctypes.CDLL(L.LIB_PATH), "aoenv_set_guide_direction")


HAVE = _library_has_guide()


def directions(env, fov):
    n = env.n_envs
    return np.full(n, fov / 2), 360.0 * np.arange(n) / n + 7.0


def device_us(fn, calls):
    """us per call of `calls` back-to-back calls, between two events on the env's stream"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    fn()
    torch.cuda.synchronize()
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    torch.cuda.synchronize()
    return 1e3 * a.elapsed_time(b) / calls


def profiled_phase_us(env, seed, steps):
    """us per launch of the phase kernel over the steps of the integrator, in the state the env is in"""
    episode(env, seed)
    env._shard.profile(True)
    env.run_integrator(0, steps, GAIN)
    ms, cnt = env._shard.profile_read(env._stream())["phase"]
    env._shard.profile(False)
    return 1e3 * ms / cnt if cnt else None


def one_field(n, steps, repeats, fov, calls):
    env = make_env(n, steps, fov)
    out = {"fov_arcsec": fov, "grids": list(env._atm_tables.layer_res), "fused_step": bool(env.fused_step)}
    arms = ("none", "guide_set", "none_again") if HAVE else ("none", "none_again")
    t = {k: [] for k in arms}
    phase_given, phase_us, sci, sr = [], [], [], {}
    for rep in range(repeats + 1):
        for arm in arms:
            if HAVE:
                env.clear_guide_direction()
                if arm == "guide_set":
                    env.set_guide_direction(*directions(env, fov))
            episode(env, 100 + rep)
            env.run_integrator(0, 2, GAIN)                          # (untimed: the first launches after the allocation)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            _, _, strehl = env.run_integrator(0, steps, GAIN)
            torch.cuda.synchronize()
            if rep:
                t[arm].append(1e6 * (time.perf_counter() - t0))
            sr[arm] = float(strehl.mean())
        # yardstick 1: the batched phase kernel from the screens over the same steps, by aoenv_profile
        if HAVE:
            env.clear_guide_direction()
        us = profiled_phase_us(env, 100 + rep, steps)
        if rep and us:
            phase_us.append(us)
        if not HAVE:
            continue
        # ... and the same kernel on the OPD k_guide_opd wrote
        zen, az = directions(env, fov)
        env.set_guide_direction(zen, az)
        us = profiled_phase_us(env, 100 + rep, steps)
        if rep and us:
            phase_given.append(us)
        # yardstick 2: k_science_residual alone at the same directions
        env.clear_guide_direction()
        env.set_science_direction(zen, az)
        L.check(env._shard.lib.aoenv_set_option(env._shard.h, L.OPT_STORE_ATM_OPD, 1))
        env.step(0, GAIN * env._obs)
        us = device_us(env.science_residual, calls)
        if rep:
            sci.append(us)
        L.check(env._shard.lib.aoenv_set_option(env._shard.h, L.OPT_STORE_ATM_OPD, 0))
        env.clear_science_direction()
    us = {k: stats(v, steps) for k, v in t.items()}
    out["loop_us_per_step"] = us
    out["a_a_spread_us"] = round(abs(us["none"]["median"] - us["none_again"]["median"]), 3)
    out["mean_final_strehl"] = {k: round(v, 4) for k, v in sr.items()}
    if phase_us:
        out["phase_kernel_us_per_launch"] = stats(phase_us, 1)
    if HAVE:
        base = 0.5 * (us["none"]["median"] + us["none_again"]["median"])
        out["guide_set_minus_none_us"] = round(us["guide_set"]["median"] - base, 3)
        out["phase_kernel_given_opd_us_per_launch"] = stats(phase_given, 1)
        out["guide_opd_us_per_launch"] = round(out["guide_set_minus_none_us"] + out["phase_kernel_us_per_launch"]["median"]
                                               - out["phase_kernel_given_opd_us_per_launch"]["median"], 3)
        out["science_residual_us_per_launch"] = stats(sci, 1)
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
    out = {"script": "scripts/time_guide.py", "library": a.label, "device": torch.cuda.get_device_name(0), "dtype": "float32",
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
