#!/usr/bin/env python3
"""What a static aberration map (BatchedAOEnv.set_static_aberration) costs, float32, on the C2 shard of bench.py (8 m, 20 x 20
Shack-Hartmann, R = 120, 256 envs, photon-noise camera, the on-device integrator).
    python scripts/time_static.py [--out file.json] [--label text] [--parent a.json ...] [n_envs] [steps] [repeats]
States, alternating inside every round of one process so that clock drift hits all alike (the first round is a warm-up):
    fused          the default path (the fused step kernel), no map
    batched        AOENV_OPT_FUSED_STEP = 0, no map: the kernels a shard with a sensor-arm map runs around its surface
    wfs_map        every env its own sensor-arm map: k_dm_rows + k_dm_static_mfma in front of k_phase<float>
    wfs_general    the same under AOENV_PATH_DM_STATIC_GENERAL: k_coefs_image + k_dm_static<float>
    science_map    every env its own science-arm map alone: the shard stays fused, nothing in the loop reads the map
    fused_again    the default path once more: the A/A spread of the session
Each loop figure is us per step of run_integrator: median [min .. max] over `repeats` timed runs of `steps` steps,
torch.cuda.synchronize() on both sides; the mean final Strehl and the episode return of every state go with it.
Kernels (device events around back-to-back calls, and aoenv_profile for the phase kernel over the integrator's steps):
    surface_us      us per refresh of the surface: one k_dm_rows + k_dm_static_mfma pair, timed as set_coefs calls
    phase_us        the phase kernel per launch: k_phase<float> reading the surface (wfs_map), the batched k_phase_mfma4 forming the
                    surface itself (batched)
    science_static  us per science_residual() launch with a science-arm map alone (k_science_static)
    science_window  yardstick: us per science_psf() launch of the same shard without maps (the science window's own launch)
--parent merges the fused / batched arms of runs of this script on the parent commit's library (AOENV_LIB=that library: it has no
static maps, only those arms are timed).  One JSON line."""
import argparse
import ctypes
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
from time_dm_env import GEOMETRY  # noqa: E402

HAVE = hasattr(ctypes.CDLL(L.LIB_PATH), "aoenv_set_static_opd")
GAIN = 0.5
STATES = ("fused", "batched", "wfs_map", "wfs_general", "science_map", "fused_again") if HAVE else ("fused", "batched", "fused_again")


def stats(v, per):
    v = np.asarray(v, dtype=np.float64) / per
    return {"median": round(float(np.median(v)), 3), "min": round(float(v.min()), 3), "max": round(float(v.max()), 3), "n": int(v.size)}


def device_us(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    fn()
    torch.cuda.synchronize()
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    torch.cuda.synchronize()
    return 1e3 * a.elapsed_time(b) / calls


def episode(env, seed):
    env.generate_new_phase_screen(seed)
    env.dm.coefs = 0
    env.dm_prev = 0
    env.measure()
    return env.reset_soft()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--label", default="the committed library")
    ap.add_argument("--parent", nargs="*", default=[])
    ap.add_argument("n_envs", nargs="?", type=int, default=256)
    ap.add_argument("steps", nargs="?", type=int, default=256)
    ap.add_argument("repeats", nargs="?", type=int, default=5)
    a = ap.parse_args()
    from rlao_amd.env import BatchedAOEnv
    env = BatchedAOEnv(n_envs=a.n_envs, device=0, dtype="f32", return_frame=False)
    env.set_params(dict(GEOMETRY["C2"][0], nLoop=max(a.steps, 64)), camera="papyrus", wfs_type="shackhartmann")
    opt = lambda k, v: L.check(env._shard.lib.aoenv_set_option(env._shard.h, k, v))
    n = a.n_envs
    if HAVE:                                                        # an amplitude sweep across the shard, 20 .. 150 nm rms
        base_w, base_s = env.ncpa_map(f2=[1.0, 2, 30, 1.0], seed=5), env.ncpa_map(f2=[1.0, 4, 40, 2.0], seed=11)
        amp = np.linspace(20e-9, 150e-9, n)[:, None, None]
        s_w, s_s = amp * base_w[None], 0.5 * amp * base_s[None]
    t = {s: [] for s in STATES}
    fused, strehl, ret, phase = {}, {}, {}, {s: [] for s in ("batched", "wfs_map")}
    for rep in range(a.repeats + 1):
        for state in STATES:
            if HAVE:
                env.clear_static_aberration()
            opt(L.OPT_FUSED_STEP, 0 if state == "batched" else 1)
            if HAVE:
                opt(L.OPT_FORCE_PATH, L.PATH_DM_STATIC_GENERAL if state == "wfs_general" else 0)
                if state.startswith("wfs"):
                    env.set_static_aberration(wfs=s_w)
                if state == "science_map":
                    env.set_static_aberration(science=s_s)
            fused[state] = bool(env.fused_step)
            episode(env, 100 + rep)
            env.run_integrator(0, 2, GAIN)                          # (untimed: the first launches after the allocation)
            episode(env, 100 + rep)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            _, rew, sr = env.run_integrator(0, a.steps, GAIN)
            torch.cuda.synchronize()
            if rep:
                t[state].append(1e6 * (time.perf_counter() - t0))
            strehl[state] = float(sr.double().mean())
            ret[state] = float(rew.double().mean())                 # (the last frame's reward: the states run the same episode)
            if state in phase:
                episode(env, 100 + rep)
                env._shard.profile(True)
                env.run_integrator(0, a.steps, GAIN)
                ms, cnt = env._shard.profile_read(env._stream())["phase"]
                env._shard.profile(False)
                if rep and cnt:
                    phase[state].append(1e3 * ms / cnt)
    out = {"script": "scripts/time_static.py", "library": a.label, "device": torch.cuda.get_device_name(0), "dtype": "float32",
           "geometry": "C2 (bench.py)", "n_envs": n, "steps": a.steps, "repeats": a.repeats, "fused_step": fused,
           "loop_us_per_step": {k: stats(v, a.steps) for k, v in t.items()}, "mean_final_strehl": strehl, "mean_final_reward": ret,
           "phase_kernel_us_per_launch": {k: stats(v, 1) for k, v in phase.items() if v}}
    us = out["loop_us_per_step"]
    out["a_a_spread_us"] = round(abs(us["fused"]["median"] - us["fused_again"]["median"]), 3)
    if HAVE:
        out["wfs_map_vs_batched"] = round(us["wfs_map"]["median"] / us["batched"]["median"], 4)
        out["wfs_map_vs_fused"] = round(us["wfs_map"]["median"] / us["fused"]["median"], 4)
        out["general_vs_mfma"] = round(us["wfs_general"]["median"] / us["wfs_map"]["median"], 4)
        # the surface's own launches: a command upload re-forms it (k_dm_rows + k_dm_static_mfma), against the same upload without a map
        coefs = np.zeros((n, env.nValidAct))
        opt(L.OPT_FORCE_PATH, 0)
        env.clear_static_aberration()
        bare = device_us(lambda: env._shard.set_coefs(coefs), 50)
        env.set_static_aberration(wfs=s_w)
        with_map = device_us(lambda: env._shard.set_coefs(coefs), 50)
        opt(L.OPT_FORCE_PATH, L.PATH_DM_STATIC_GENERAL)
        general = device_us(lambda: env._shard.set_coefs(coefs), 50)
        opt(L.OPT_FORCE_PATH, 0)
        out["surface_us"] = {"set_coefs_without_map": round(bare, 3), "set_coefs_with_map_mfma": round(with_map, 3),
                             "set_coefs_with_map_general": round(general, 3), "rows_plus_static_mfma": round(with_map - bare, 3),
                             "image_plus_static_general": round(general - bare, 3)}
        # the science arm's light kernel against the science window's own launch
        env.clear_static_aberration()
        env.set_science(zero_padding=4, window=130, first_frame=0)
        episode(env, 7)
        env.step(0, GAIN * env._obs)
        window = device_us(env.science_psf, 100)
        env.set_static_aberration(science=s_s)
        both = device_us(env.science_psf, 100)
        resid = device_us(env.science_residual, 100)
        out["science_us"] = {"science_window_per_launch": round(window, 3), "window_with_science_map": round(both, 3),
                             "science_static_per_launch": round(resid, 3)}
        env.clear_science()
        env.clear_static_aberration()
    if a.parent:
        out["parent_library"] = []
        for path in a.parent:
            par = json.load(open(path))
            out["parent_library"].append({k: par[k] for k in ("library", "loop_us_per_step", "a_a_spread_us", "mean_final_strehl",
                                                             "mean_final_reward", "phase_kernel_us_per_launch")})
    env.close()
    print(json.dumps(out))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
