#!/usr/bin/env python3
"""What a step costs behind the geometric Shack-Hartmann (set_params(..., is_geometric=True)) against the diffractive sensor, float32,
aoenv_run_integrator, ideal camera, at the C2 shard (8 m, 20 x 20 lenslets, R = 120, 256 envs) or with --shape c4 at the C4 shard
(39 m, 80 x 80, R = 480).
    python scripts/time_geometric.py [--shape c2|c4] [--out file.json] [--label text] [--parent a.json [b.json ...]]
                                     [--also a.json [b.json ...]] [n_envs] [steps] [repeats]
Arms, interleaved inside every round (the first round is a warm-up), us per step as median [min .. max] over the rounds, a host clock
around a call that ends in torch.cuda.synchronize():
  geometric            the geometric loop: the phase kernel, then slopes + reconstruction + integrator in one launch
  diffractive_batched  the diffractive loop with AOENV_OPT_FUSED_STEP 0: phase, spots, (camera,) centroid + tail
  diffractive_fused    the diffractive loop as it runs by default (the fused step kernel inside its envelope)
and once per arm the per-kernel split of aoenv_profile over the same steps (a run of its own: the events slow the host).
The slopes kernel alone (k_sh_geometric, through aoenv_measure's sensor half): us per launch from aoenv_profile, the bytes it must
move -- n_env R^2 elements of unmasked phase read once, the pupil from cache, 2 nValid slopes written -- and the rate that is of the
8 TB/s HBM3E roof of the MI355X.
A library without the geometric sensor (AOENV_LIB = the parent commit's) runs the two diffractive arms alone; --parent merges such
runs, so that the diffractive lines of this commit stand beside the parent's; --also merges earlier runs of THIS library
(`other_runs_of_this_library`), so that the file holds the run-to-run spread of both.  One JSON line."""
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
HBM_ROOF = 8.0e12                                                   # bytes / s (MI355X, HBM3E)
SHAPES = {
    "c2": dict(diameter=8.0, nSubaperture=20, nPixelPerSubap=6, r0=0.13, L0=30.0, windSpeed=[10.0], windDirection=[72.0],
               fractionalR0=[1.0], altitude=[0.0], nModes=50),
    "c4": dict(diameter=39.0, nSubaperture=80, nPixelPerSubap=6, r0=0.13, L0=30.0, windSpeed=[10.0], windDirection=[72.0],
               fractionalR0=[1.0], altitude=[0.0], nModes=300),
}


def _library_has_geometric():
    import ctypes
    return hasattr(ctypes.CDLL(L.LIB_PATH), "aoenv_get_phase_no_pupil")


HAVE = _library_has_geometric()


def make_env(shape, n, n_loop, geometric, fused):
    env = BatchedAOEnv(n_envs=n, device=0, dtype="f32", return_frame=False)
    kw = dict(is_geometric=True) if geometric else {}
    env.set_params(dict(SHAPES[shape], nLoop=n_loop), camera="ideal", wfs_type="shackhartmann", gainCL=GAIN, **kw)
    if not fused:
        L.check(env._shard.lib.aoenv_set_option(env._shard.h, L.OPT_FUSED_STEP, 0))
    return env


def episode(env, seed):
    env.generate_new_phase_screen(seed)
    env.dm.coefs = 0
    env.dm_prev = 0
    env.measure()
    env.SR = []
    return env.reset_soft()


def stats(v, per=1.0):
    return {"median": round(float(np.median(v)) / per, 3), "min": round(min(v) / per, 3), "max": round(max(v) / per, 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="c2", choices=sorted(SHAPES))
    ap.add_argument("--out", default=None)
    ap.add_argument("--label", default="the committed library")
    ap.add_argument("--parent", nargs="*", default=[])
    ap.add_argument("--also", nargs="*", default=[])
    ap.add_argument("n_envs", nargs="?", type=int, default=256)
    ap.add_argument("steps", nargs="?", type=int, default=256)
    ap.add_argument("repeats", nargs="?", type=int, default=5)
    a = ap.parse_args()
    arms = {"diffractive_batched": (False, False), "diffractive_fused": (False, True)}
    if HAVE:
        arms = dict(geometric=(True, True), **arms)
    envs = {k: make_env(a.shape, a.n_envs, a.steps, *v) for k, v in arms.items()}
    out = {"script": "scripts/time_geometric.py", "library": a.label, "device": torch.cuda.get_device_name(0), "dtype": "float32",
           "shape": a.shape, "n_envs": a.n_envs, "steps": a.steps, "repeats": a.repeats,
           "fused_step_active": {k: bool(e.fused_step) for k, e in envs.items()}}
    t = {k: [] for k in arms}
    for rep in range(a.repeats + 1):
        for arm, env in envs.items():
            episode(env, 100 + rep)
            env.run_integrator(0, 2, GAIN)                          # (untimed: the first launches after the episode's prologue)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            env.run_integrator(0, a.steps, GAIN)
            torch.cuda.synchronize()
            if rep:
                t[arm].append(1e6 * (time.perf_counter() - t0))
    out["loop_us_per_step"] = {k: stats(v, a.steps) for k, v in t.items()}
    # the per-kernel split, in a run of its own
    split = {}
    for arm, env in envs.items():
        episode(env, 99)
        env._shard.profile(True)
        env.run_integrator(0, a.steps, GAIN)
        prof = env._shard.profile_read(env._stream())
        env._shard.profile(False)
        split[arm] = {k: {"us_per_launch": round(1e3 * ms / n, 3), "launches": n} for k, (ms, n) in prof.items() if n}
    out["kernel_split"] = split
    if HAVE:
        env = envs["geometric"]
        us = []
        for rep in range(a.repeats + 1):
            env._shard.profile(True)
            for _ in range(50):
                env._shard.measure(env._stream())
            ms, n = env._shard.profile_read(env._stream())["sh_centroid"]
            env._shard.profile(False)
            if rep:
                us.append(1e3 * ms / n)
        R, nv = env.R, env.nSignal // 2
        nbytes = a.n_envs * (R * R * 4 + 2 * nv * 4) + R * R
        k = stats(us)
        out["slopes_kernel"] = {"us_per_launch": k, "bytes": nbytes, "achieved_bytes_per_s": round(nbytes / (k["median"] * 1e-6), 1),
                                "share_of_hbm_roof": round(nbytes / (k["median"] * 1e-6) / HBM_ROOF, 4), "hbm_roof_bytes_per_s": HBM_ROOF,
                                "bound": "memory: one read of the unmasked phase; 2 p^2 adds per lenslet are far below the vector rate"}
        g, b = out["loop_us_per_step"]["geometric"]["median"], out["loop_us_per_step"]["diffractive_batched"]["median"]
        out["geometric_over_diffractive_batched"] = round(g / b, 4)
    for env in envs.values():
        env.close()
    if a.parent:
        out["parent_library"] = []
        for path in a.parent:
            par = json.load(open(path))
            out["parent_library"].append({"label": par["library"], "loop_us_per_step": par["loop_us_per_step"],
                                          "kernel_split": par["kernel_split"]})
    if a.also:
        out["other_runs_of_this_library"] = [{"label": r["library"], "loop_us_per_step": r["loop_us_per_step"]}
                                             for r in (json.load(open(path)) for path in a.also)]
    print(json.dumps(out))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
