#!/usr/bin/env python3
"""What the wavefront read-out (BatchedAOEnv.set_wavefront_basis / project_wavefront / record_wavefront) costs, float32.
    python scripts/time_wavefront.py [--out file.json] [--label text] [--skip-loops] [--skip-projection] [--c4] [--ab gemm.json]
                                     [--mfma mfma.json] [--parent parent.json] [n_envs] [steps] [repeats]
Part 1, the projection alone at the C2 geometry (8 m, 20 x 20 Shack-Hartmann, R = 120, 256 envs), K in {10, 30, 64, 100, 500} (64:
the library's switch between its two float32 routes): `calls`
calls of project_wavefront per timed run, arms interleaved inside every round so that clock drift hits all alike, the first
round a warm-up, torch.cuda.synchronize() on both sides; median [min .. max] over the rounds in us per call:
  residual, residual_again   the default path (their difference is the A/A spread of the session)
  atmosphere                 the same on AOENV_B_OPD_ATM (handed over with aoenv_set_atm_opd, so that nothing is re-derived first)
  general                    AOENV_PATH_WF_GENERAL: one fma chain per (env, mode, slice)
With the bytes a call moves (X + P + the slabs written and read + the result) and their share of the 8 TB/s HBM figure.
The committed library takes k_wf_project_mfma up to 64 modes and the route it had before above: launch_gemm_nt_mfma with split-K
slabs plus the slab sum of k_wf_finish.  Either route at EVERY K is timed on two A/B builds (make FLAGS_env=-D... into a library of
its own, AOENV_LIB=that library, --label): -DAOENV_WF_GEMM_ABOVE_MODES=0 the GEMM route always, =1024 the matrix-core tile always;
--ab gemm.json / --mfma mfma.json merge the `residual` column of those records into this run's.
One and both OPDs: aoenv_project_wavefront takes one bit, so the pass that shares the P registers between both operands is
reachable through the record alone; it is timed there, in part 2 (record_both against record_residual).
Part 2, the loop: the C2 on-device integrator (run_integrator, photon-noise camera) with no basis, with a basis but no record,
recording the residual, recording both, at K = 30; `basis_cleared` sets the basis and clears it again before the run -- the device
allocation and free of `basis` with the library state of `none`, to tell what the allocator does to the runs after it from what
the basis does (two untimed steps after the arm is set up, so that the first launches after an
allocation are not in the figure); --parent parent.json merges the `none` arms of a run of this script on the
parent commit's library (AOENV_LIB, --skip-projection: it has no wavefront entry points, only `none` is timed).  --c4 adds the
K = 30 residual record at the C4 size (39 m, 80 x 80, R = 480, 512 envs).
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
HBM_BYTES_PER_S = 8e12
C2 = dict(diameter=8.0, nSubaperture=20, nPixelPerSubap=6, r0=0.13, L0=30.0, windSpeed=[10.0], windDirection=[72.0],
          fractionalR0=[1.0], altitude=[0.0], nModes=50)
C4 = dict(diameter=39.0, nSubaperture=80, nPixelPerSubap=6, r0=0.13, L0=30.0, windSpeed=[10.0], windDirection=[72.0],
          fractionalR0=[1.0], altitude=[0.0], nModes=300)


def _library_has_wavefront():
    """False for the parent commit's library (AOENV_LIB): the binding then declares the entry points that library has"""
    import ctypes
    try:
        ctypes.CDLL(L.LIB_PATH).aoenv_set_wavefront_basis
        return True
    except AttributeError:
        for name in ("aoenv_set_wavefront_basis", "aoenv_project_wavefront", "aoenv_set_wavefront_record"):
            L.EXPORTS.pop(name, None)
        return False


HAVE_WF = _library_has_wavefront()


def make_env(geo, n, n_loop, camera):
    env = BatchedAOEnv(n_envs=n, device=0, dtype="f32", return_frame=False, env_seed_stride=0 if n > 256 else 1)
    env.set_params(dict(geo, nLoop=n_loop), camera=camera, wfs_type="shackhartmann", gainCL=GAIN)
    return env


def episode(env, seed):
    env.generate_new_phase_screen(seed)
    env.dm.coefs = 0
    env.dm_prev = 0
    env.measure()
    env.SR = []
    return env.reset_soft()


def basis(env, K):
    """a projector of the right shape: pinv would cost minutes at K = 500 and the timing does not depend on the values"""
    P = int(np.count_nonzero(env.pupil))
    return np.random.RandomState(K).normal(0.0, 1.0 / P, (K, P))


def stats(v, per):
    return {"median": round(float(np.median(v)) / per, 3), "min": round(min(v) / per, 3), "max": round(max(v) / per, 3)}


def plan(r2, K):
    want = min(max(r2 // (4 * K), 1), 64)
    length = -(-(-(-r2 // want)) // 16) * 16
    return -(-r2 // length), length


def projection(n, ks, calls, repeats):
    env = make_env(C2, n, 8, "ideal")
    episode(env, 17)
    atm = env._shard.download(L.B_OPD_ATM, (n, env.R * env.R), env._stream())
    env._shard.set_atm_opd(atm, env._stream())
    r2 = env.R * env.R
    rows = []
    for K in ks:
        env.set_wavefront_basis(opd2m=basis(env, K))
        arms = {"residual": (0, "residual"), "atmosphere": (0, "atmosphere"), "general": (L.PATH_WF_GENERAL, "residual"),
                "residual_again": (0, "residual")}
        t = {k: [] for k in arms}
        for rep in range(repeats + 1):
            for k, (path, what) in arms.items():
                L.check(env._shard.lib.aoenv_set_option(env._shard.h, L.OPT_FORCE_PATH, path))
                env.project_wavefront(what)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(calls):
                    env.project_wavefront(what)
                torch.cuda.synchronize()
                if rep:
                    t[k].append(1e6 * (time.perf_counter() - t0))
        L.check(env._shard.lib.aoenv_set_option(env._shard.h, L.OPT_FORCE_PATH, 0))
        slices, length = plan(r2, K)
        # X + P + the result, and the tile route's slabs written and read (above 64 modes the GEMM route's slab count is the
        # library's own: left out, the figure is then a lower bound)
        moved = 4 * (n * r2 + K * ((r2 + 3) // 4 * 4) + (2 * slices * n * K if K <= 64 else 0) + n * K)
        us = {k: stats(v, calls) for k, v in t.items()}
        rows.append({"K": K, "slices": slices, "slice_len": length, "us_per_call": us,
                     "a_a_spread_us": round(abs(us["residual"]["median"] - us["residual_again"]["median"]), 3),
                     "bytes_moved": moved, "hbm_floor_us": round(1e6 * moved / HBM_BYTES_PER_S, 3),
                     "fraction_of_8TBps": round(1e6 * moved / HBM_BYTES_PER_S / us["residual"]["median"], 4)})
        print(f"[projection] K={K}: {rows[-1]}", file=sys.stderr, flush=True)
    out = {"geometry": "C2", "n_envs": n, "R": env.R, "calls": calls, "repeats": repeats, "sweep": rows}
    env.close()
    return out


def loops(name, geo, n, steps, repeats, K, camera, arms):
    t0 = time.perf_counter()
    env = make_env(geo, n, steps, camera)
    init_s = time.perf_counter() - t0

    def prepare(arm):
        if not HAVE_WF:
            return
        env.clear_wavefront_basis()
        if arm.startswith("none"):
            return
        env.set_wavefront_basis(opd2m=basis(env, K))
        if arm == "basis_cleared":                                  # the allocation and the free of `basis`, the library state of `none`
            env.clear_wavefront_basis()
        if arm == "record_residual":
            env.record_wavefront(0, steps, ("residual",))
        elif arm == "record_both":
            env.record_wavefront(0, steps, ("residual", "atmosphere"))

    t = {k: [] for k in arms}
    resid = {}
    for rep in range(repeats + 1):
        for arm in arms:
            episode(env, 100 + rep)
            prepare(arm)
            env.run_integrator(0, 2, GAIN)                          # (untimed: the first launches after set_wavefront_basis's allocation)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            env.run_integrator(0, steps, GAIN)
            torch.cuda.synchronize()
            if rep:
                t[arm].append(1e6 * (time.perf_counter() - t0))
            resid[arm] = float(np.mean(env.residual[steps - 1]))
    if HAVE_WF:
        env.clear_wavefront_basis()
    us = {k: stats(v, steps) for k, v in t.items()}
    out = {"geometry": name, "n_envs": n, "R": env.R, "steps": steps, "repeats": repeats, "K": K, "camera": camera, "init_s": round(init_s, 1),
           "fused_step": bool(env.fused_step), "us_per_step": us, "mean_residual_nm_last_step": {k: round(v, 3) for k, v in resid.items()}}
    if "none_again" in us:
        out["a_a_spread_us"] = round(abs(us["none"]["median"] - us["none_again"]["median"]), 3)
    if "record_both" in us:
        base = 0.5 * (us["none"]["median"] + us["none_again"]["median"])
        out["record_residual_minus_none_us"] = round(us["record_residual"]["median"] - base, 3)
        out["record_both_minus_record_residual_us"] = round(us["record_both"]["median"] - us["record_residual"]["median"], 3)
    env.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--label", default="the committed library")
    ap.add_argument("--skip-loops", action="store_true")
    ap.add_argument("--skip-projection", action="store_true")
    ap.add_argument("--c4", action="store_true")
    ap.add_argument("--c4-envs", type=int, default=512)
    ap.add_argument("--ab", default=None, help="record of the -DAOENV_WF_GEMM_ABOVE_MODES=0 build: its residual arm becomes the gemm_route column")
    ap.add_argument("--mfma", default=None, help="record of the -DAOENV_WF_GEMM_ABOVE_MODES=1024 build: its residual arm becomes the mfma_tile column")
    ap.add_argument("--parent", default=None, help="record of the parent commit's library: its `none` arms are put beside this run's")
    ap.add_argument("n_envs", nargs="?", type=int, default=256)
    ap.add_argument("steps", nargs="?", type=int, default=512)
    ap.add_argument("repeats", nargs="?", type=int, default=7)
    a = ap.parse_args()
    out = {"script": "scripts/time_wavefront.py", "library": a.label, "device": torch.cuda.get_device_name(0), "dtype": "float32"}
    if not a.skip_projection and HAVE_WF:
        out["projection"] = projection(a.n_envs, (10, 30, 64, 100, 500), 200, a.repeats)
    if not a.skip_loops:
        arms = ("none", "basis", "basis_cleared", "record_residual", "record_both", "none_again") if HAVE_WF else ("none", "none_again")
        out["loop"] = loops("C2", C2, a.n_envs, a.steps, a.repeats, 30, "papyrus", arms)
        if a.c4 and HAVE_WF:
            out["loop_c4"] = loops("C4", C4, a.c4_envs, 32, 3, 30, "ideal", ("none", "record_residual", "none_again"))
    if a.ab:
        ab = json.load(open(a.ab))
        out["gemm_route_library"] = ab["library"]
        for row, other in zip(out["projection"]["sweep"], ab["projection"]["sweep"]):
            assert row["K"] == other["K"]
            row["gemm_route_us_per_call"] = other["us_per_call"]["residual"]
            row["gemm_route_a_a_spread_us"] = other["a_a_spread_us"]
    if a.mfma:
        ab = json.load(open(a.mfma))
        out["mfma_tile_library"] = ab["library"]
        for row, other in zip(out["projection"]["sweep"], ab["projection"]["sweep"]):
            assert row["K"] == other["K"]
            row["mfma_tile_us_per_call"] = other["us_per_call"]["residual"]
            row["mfma_tile_a_a_spread_us"] = other["a_a_spread_us"]
    if a.parent:
        par = json.load(open(a.parent))
        out["loop"]["parent_library"] = {"label": par["library"], "us_per_step": par["loop"]["us_per_step"], "a_a_spread_us": par["loop"].get("a_a_spread_us")}
    print(json.dumps(out))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
