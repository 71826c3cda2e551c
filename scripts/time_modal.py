#!/usr/bin/env python3
"""What the modal control surface (BatchedAOEnv.set_modal) costs, one build, one session, float32.
    python scripts/time_modal.py [--out file.json] [--skip-loops] [--label text] [--ab lifted.json] [--merge raw.json] [n_envs] [steps] [repeats]
Part 1, the loops, at the C2 shard (8 m, 20 x 20 Shack-Hartmann, 256 envs, photon noise, K = all 50 modes), arms interleaved inside
every round so that clock drift hits all alike:
  step, step_again        env.step(k, g * obs) called from Python (their difference is the A/A spread of the session)
  step_modal              env.step_modal(k, g * obs): the two modal launches around the same step
  int, int_again          run_integrator, the fused-gain epilogue
  int_modal               run_integrator_modal
  int_d1, int_modal_d1    the same two under set_delay(1): the zonal loop then pays one k_delay_push per step, the modal loop none
                          (its expansion writes into the line)
Each figure is the median over `repeats` timed runs of `steps` steps after a warm-up round, torch.cuda.synchronize() on both sides.
Part 2, the projection paths, at the C2 shape (with a basis of 200 modes, so that the sweep can pass the shard's own 50) and at the C4 shape (39 m, 80 x 80 Shack-Hartmann, n_signal = 10048, the per-GPU shard
of 512 envs): for K in a sweep, `calls` calls of reset_soft_modal -- the zonal reconstruction plus the projection -- on the default
path and with AOENV_PATH_MODAL_GEMM, against the same number of reset_soft calls; the differences are the cost of the projection's
launches.  Above the library's threshold the default path IS the GEMM path: the per-env kernel is timed there by running this script
on an A/B build whose threshold is lifted (make FLAGS_env=-DAOENV_MODAL_GEMM_THRESHOLD=..., AOENV_LIB=that library, --label).
profiles/modal_timing.json is written in two runs of one session:
    AOENV_LIB=<lifted build> python scripts/time_modal.py --skip-loops --label "threshold lifted" --out lifted.json
    python scripts/time_modal.py --ab lifted.json --out profiles/modal_timing.json
--ab merges the per-env kernel's column of the lifted run into this run's record, next to the one-launch yardsticks of
profiles/disturbance_timing.json and profiles/delay_timing.json and the threshold as rlao_amd/csrc/env.hip defines it;
--merge raw.json does the same from a raw record of this script (written without --ab) instead of measuring, and needs no GPU.
One JSON line."""
import argparse
import json
import os
import re
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from rlao_amd import _lib as L  # noqa: E402
from rlao_amd.env import BatchedAOEnv  # noqa: E402

GAIN = 0.5
C2 = dict(diameter=8.0, nSubaperture=20, nPixelPerSubap=6, r0=0.13, L0=30.0, windSpeed=[10.0], windDirection=[72.0],
          fractionalR0=[1.0], altitude=[0.0], nModes=50)
C4 = dict(diameter=39.0, nSubaperture=80, nPixelPerSubap=6, r0=0.13, L0=30.0, windSpeed=[10.0], windDirection=[72.0],
          fractionalR0=[1.0], altitude=[0.0], nModes=300)


def make_env(geo, n, n_loop, camera):
    env = BatchedAOEnv(n_envs=n, device=0, dtype="f32", return_frame=False, env_seed_stride=0 if n > 256 else 1)
    env.set_params(dict(geo, nLoop=n_loop), camera=camera, wfs_type="shackhartmann", gainCL=GAIN)
    return env


def episode(env, seed, modal):
    env.generate_new_phase_screen(seed)
    env.dm.coefs = 0
    env.dm_prev = 0
    env.measure()
    env.SR = []
    return env.reset_soft_modal() if modal else env.reset_soft()


def stepped(env, steps, modal):
    obs = env._mobs if modal else env._obs
    step = env.step_modal if modal else env.step
    for k in range(steps):
        obs = step(k, GAIN * obs)[0]


def loops(n, steps, repeats):
    envs = {}
    for d in (0, 1):
        envs[d] = make_env(C2, n, steps, "papyrus")
        envs[d].set_modal()
        envs[d].set_modal_gain(GAIN)
        envs[d].set_delay(d)
    arms = {
        "step": (0, False, lambda e: stepped(e, steps, False)), "step_modal": (0, True, lambda e: stepped(e, steps, True)),
        "int": (0, False, lambda e: e.run_integrator(0, steps, GAIN)), "int_modal": (0, True, lambda e: e.run_integrator_modal(0, steps)),
        "int_d1": (1, False, lambda e: e.run_integrator(0, steps, GAIN)), "int_modal_d1": (1, True, lambda e: e.run_integrator_modal(0, steps)),
        "step_again": (0, False, lambda e: stepped(e, steps, False)), "int_again": (0, False, lambda e: e.run_integrator(0, steps, GAIN)),
    }
    t = {k: [] for k in arms}
    resid = {}
    for rep in range(repeats + 1):
        for k, (d, modal, run) in arms.items():
            episode(envs[d], 100 + rep, modal)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run(envs[d])
            torch.cuda.synchronize()
            if rep:                                                 # (the first round is the warm-up)
                t[k].append(1e3 * (time.perf_counter() - t0))
            resid[k] = float(np.mean(envs[d].residual[steps - 1]))
    us = {k: round(1e3 * float(np.median(v)) / steps, 3) for k, v in t.items()}
    out = {"geometry": "C2", "n_envs": n, "steps": steps, "repeats": repeats, "camera": "papyrus (photon noise)", "n_modes": envs[0].n_modal,
           "n_signal": envs[0].nSignal, "fused_step": bool(envs[0].fused_step), "us_per_step": us,
           "min_max_us_per_step": {k: [round(1e3 * min(v) / steps, 3), round(1e3 * max(v) / steps, 3)] for k, v in t.items()},
           "a_a_spread_us": {"step": round(abs(us["step"] - us["step_again"]), 3), "run_integrator": round(abs(us["int"] - us["int_again"]), 3)},
           "step_modal_minus_step_us": round(us["step_modal"] - 0.5 * (us["step"] + us["step_again"]), 3),
           "int_modal_minus_int_us": round(us["int_modal"] - 0.5 * (us["int"] + us["int_again"]), 3),
           "int_modal_d1_minus_int_d1_us": round(us["int_modal_d1"] - us["int_d1"], 3),
           "mean_residual_nm_last_step": {k: round(v, 3) for k, v in resid.items()}}
    for e in envs.values():
        e.close()
    return out


def projection(name, geo, n, ks, calls, repeats):
    t0 = time.perf_counter()
    env = make_env(geo, n, 8, "ideal")
    init_s = time.perf_counter() - t0
    episode(env, 17, False)
    rows = []
    for K in ks:
        env.set_modal(K)
        arms = {"reset_soft": (0, env.reset_soft), "default": (0, env.reset_soft_modal), "gemm": (L.PATH_MODAL_GEMM, env.reset_soft_modal),
                "reset_soft_again": (0, env.reset_soft)}
        t = {k: [] for k in arms}
        for rep in range(repeats + 1):
            for k, (path, call) in arms.items():
                L.check(env._shard.lib.aoenv_set_option(env._shard.h, L.OPT_FORCE_PATH, path))
                call()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(calls):
                    call()
                torch.cuda.synchronize()
                if rep:
                    t[k].append(1e6 * (time.perf_counter() - t0) / calls)
        L.check(env._shard.lib.aoenv_set_option(env._shard.h, L.OPT_FORCE_PATH, 0))
        us = {k: round(float(np.median(v)), 2) for k, v in t.items()}
        base = 0.5 * (us["reset_soft"] + us["reset_soft_again"])
        rows.append({"K": K, "K_x_n_signal": K * env.nSignal, "us_per_call": us, "a_a_spread_us": round(abs(us["reset_soft"] - us["reset_soft_again"]), 2),
                     "projection_default_us": round(us["default"] - base, 2), "projection_gemm_us": round(us["gemm"] - base, 2)})
        print(f"[{name}] K={K}: {rows[-1]}", file=sys.stderr, flush=True)
    out = {"geometry": name, "n_envs": n, "n_signal": env.nSignal, "n_valid_act": env.nValidAct, "calls": calls, "repeats": repeats,
           "init_s": round(init_s, 1), "sweep": rows}
    env.close()
    return out


def threshold_in_source():
    src = open(os.path.join(REPO, "rlao_amd", "csrc", "env.hip")).read()
    return int(re.search(r"#define AOENV_MODAL_GEMM_THRESHOLD \(\(size_t\)(\d+)\)", src).group(1))


def compose(own, lifted):
    """The committed record: the loops and the two arms of this library (`own`, a raw record), the per-env kernel at every K from
    the raw record of the A/B build (`lifted`), the yardsticks and the threshold."""
    thr = threshold_in_source()
    prof = lambda name: json.load(open(os.path.join(REPO, "profiles", name)))
    dist, delay = prof("disturbance_timing.json"), prof("delay_timing.json")
    out = {"script": "scripts/time_modal.py", "device": own["device"], "dtype": "float32", "loops": own.get("loops"),
           "one_launch_yardsticks_us": {
               "k_disturb_apply (profiles/disturbance_timing.json)": dist["disturb_launch_us"],
               "k_delay_push with the explicit-action step (profiles/delay_timing.json)": delay["integrator_d1_minus_fused_gain_integrator_us"]},
           "projection_paths": []}
    for po, pl in zip(own["projection"], lifted["projection"]):
        rows = []
        for a, b in zip(po["sweep"], pl["sweep"]):
            if a["K"] != b["K"] or po["n_signal"] != pl["n_signal"] or po["n_envs"] != pl["n_envs"]:
                raise SystemExit("--ab: the two records were not taken at the same shapes")
            rows.append({"K": a["K"], "K_x_n_signal": a["K_x_n_signal"],
                         "per_env_kernel_us": b["projection_default_us"], "gemm_plus_finish_us": b["projection_gemm_us"],
                         "committed_library": {"default_path_us": a["projection_default_us"], "gemm_path_us": a["projection_gemm_us"],
                                               "default_is": "per-env kernel" if a["K_x_n_signal"] <= thr else "GEMM"},
                         "reset_soft_us": b["us_per_call"]["reset_soft"], "a_a_spread_us": max(a["a_a_spread_us"], b["a_a_spread_us"])})
        out["projection_paths"].append({**{k: po[k] for k in ("geometry", "n_envs", "n_signal", "n_valid_act", "calls", "repeats")}, "sweep": rows})
    out["projection_paths_note"] = (
        "per_env_kernel_us / gemm_plus_finish_us: reset_soft_modal minus reset_soft, per call, from the A/B build whose threshold is lifted "
        f"(its label: '{lifted['library']}'); committed_library: the same two arms of the "
        "library as committed, whose default path changes at the threshold")
    out["threshold"] = {"K_x_n_signal": thr, "defined_in": "rlao_amd/csrc/env.hip: AOENV_MODAL_GEMM_THRESHOLD / kModalGemmThreshold",
                        "rule": "the GEMM path above it, and wherever the signal row and the observations do not fit 64 KB of LDS"}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--label", default="the committed library")
    ap.add_argument("--skip-loops", action="store_true")
    ap.add_argument("--ab", default=None, help="raw record of the A/B build with the threshold lifted: write the merged record")
    ap.add_argument("--merge", default=None, help="a raw record of this library: merge it with --ab instead of measuring")
    ap.add_argument("--c4-envs", type=int, default=512)
    ap.add_argument("n_envs", nargs="?", type=int, default=256)
    ap.add_argument("steps", nargs="?", type=int, default=512)
    ap.add_argument("repeats", nargs="?", type=int, default=9)
    a = ap.parse_args()
    if a.merge:
        if not a.ab:
            raise SystemExit("--merge needs --ab")
        out = json.load(open(a.merge))
    else:
        out = {"library": a.label, "device": torch.cuda.get_device_name(0)}
        if not a.skip_loops:
            out["loops"] = loops(a.n_envs, a.steps, max(5, a.repeats))
        out["projection"] = [projection("C2", dict(C2, nModes=200), a.n_envs, (1, 5, 20, 50, 100, 200), 200, 5),
                             projection("C4", C4, a.c4_envs, (1, 5, 20, 100, 300), 50, 5)]
    if a.ab:
        out = compose(out, json.load(open(a.ab)))
    print(json.dumps(out))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
