#!/usr/bin/env python3
"""What a control delay inside the library (BatchedAOEnv.set_delay) costs the on-device loops at the C2 geometry (8 m, 20 x 20
Shack-Hartmann, 256 envs, float32 fused step, ideal camera), one build, one session.
    python scripts/time_delay.py [--out file.json] [n_envs] [steps] [repeats]
Arms, all interleaved inside every round so that clock drift hits all alike:
  int_d0, int_d0_again   run_integrator with no delay, the fused-gain epilogue (their difference is the A/A spread of the session)
  int_d1                 run_integrator under delay 1: one k_delay_push launch per step plus the explicit-action step
  roll_s0_d0             rollout(sigma = 0) with no delay: one k_rollout_action launch per step plus the explicit-action step --
                         the yardstick of int_d1 (its action kernel does strictly more work than the push)
  roll_d0, roll_d0_again rollout(sigma = 0.05) with no delay (A/A of the recorded loop)
  roll_d2                rollout(sigma = 0.05) under delay 2: no launch per step is added, one k_delay_refill per call
Each figure is the median over `repeats` timed runs of `steps` steps after a warm-up round, torch.cuda.synchronize() on both
sides.  One JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rlao_amd.env import BatchedAOEnv  # noqa: E402

GAIN = 0.5
SIGMA = 0.05


def make_env(n, steps, delay):
    geo = dict(diameter=8.0, nSubaperture=20, nPixelPerSubap=6, r0=0.13, L0=30.0, windSpeed=[10.0], windDirection=[72.0],
               fractionalR0=[1.0], altitude=[0.0], nModes=50, nLoop=steps)
    env = BatchedAOEnv(n_envs=n, device=0, dtype="f32", return_frame=False)
    env.set_params(geo, camera="ideal", wfs_type="shackhartmann", gainCL=GAIN)
    env.set_delay(delay)
    return env


def episode(env, seed):
    env.generate_new_phase_screen(seed)
    env.dm.coefs = 0
    env.dm_prev = 0
    env.measure()
    env.SR = []
    return env.reset_soft()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("n_envs", nargs="?", type=int, default=256)
    ap.add_argument("steps", nargs="?", type=int, default=512)
    ap.add_argument("repeats", nargs="?", type=int, default=9)
    a = ap.parse_args()
    n, steps, repeats = a.n_envs, a.steps, max(9, a.repeats)
    envs = {d: make_env(n, steps, d) for d in (0, 1, 2)}            # the arms of one delay share an env: every run is a new episode
    integrate = lambda e: e.run_integrator(0, steps, GAIN)
    arms = {
        "int_d0": (0, integrate), "int_d1": (1, integrate), "roll_s0_d0": (0, lambda e: e.rollout(0, steps, 0.0, gain=GAIN, seed=7)),
        "roll_d0": (0, lambda e: e.rollout(0, steps, SIGMA, gain=GAIN, seed=7)), "roll_d2": (2, lambda e: e.rollout(0, steps, SIGMA, gain=GAIN, seed=7)),
        "int_d0_again": (0, integrate), "roll_d0_again": (0, lambda e: e.rollout(0, steps, SIGMA, gain=GAIN, seed=7)),
    }
    t = {k: [] for k in arms}
    last = {}
    for rep in range(repeats + 1):
        for k, (d, run) in arms.items():
            episode(envs[d], 100 + rep)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run(envs[d])
            torch.cuda.synchronize()
            if rep:                                                 # (the first round is the warm-up)
                t[k].append(1e3 * (time.perf_counter() - t0))
            last[k] = envs[d]._obs.clone()
    us = {k: round(1e3 * float(np.median(v)) / steps, 3) for k, v in t.items()}
    spread = {k: [round(1e3 * min(v) / steps, 3), round(1e3 * max(v) / steps, 3)] for k, v in t.items()}
    out = {"n_envs": n, "steps": steps, "repeats": repeats, "gain": GAIN, "sigma": SIGMA, "fused_step": bool(envs[1].fused_step),
           "us_per_step": us, "min_max_us_per_step": spread,
           "a_a_spread_us": {"run_integrator": round(abs(us["int_d0"] - us["int_d0_again"]), 3), "rollout": round(abs(us["roll_d0"] - us["roll_d0_again"]), 3)},
           "rollout_d2_minus_d0_us": round(us["roll_d2"] - 0.5 * (us["roll_d0"] + us["roll_d0_again"]), 3),
           "integrator_d1_minus_rollout_sigma0_d0_us": round(us["int_d1"] - us["roll_s0_d0"], 3),
           "integrator_d1_minus_fused_gain_integrator_us": round(us["int_d1"] - 0.5 * (us["int_d0"] + us["int_d0_again"]), 3),
           "env_steps_per_s": {k: round(n * 1e6 / v) for k, v in us.items()},
           # same screens, same loop: the delay alone moves the last observation; two runs of one arm do not
           "max_abs_obs_difference_um": {"int_d1_vs_d0": round(float((last["int_d1"] - last["int_d0"]).abs().max()), 6),
                                         "roll_d2_vs_d0": round(float((last["roll_d2"] - last["roll_d0"]).abs().max()), 6),
                                         "int_d0_vs_again": float((last["int_d0"] - last["int_d0_again"]).abs().max())},
           "finite": bool(all(torch.isfinite(v).all() for v in last.values()))}
    for e in envs.values():
        e.close()
    print(json.dumps(out))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
