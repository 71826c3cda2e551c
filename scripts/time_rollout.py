#!/usr/bin/env python3
"""What an exploration episode costs as one library call (BatchedAOEnv.rollout) at the C2 geometry (8 m, 20 x 20 Shack-Hartmann,
256 envs, float32, ideal camera), one build, one session.
    python scripts/time_rollout.py [--out file.json] [n_envs] [steps] [repeats]
(a) run_integrator: the closed loop on the device, nothing recorded, no noise (twice, as "a" and "a2": their difference is the
    A/A spread of the session);
(b) rollout with sigma > 0: the same loop plus one action launch per step, every obs / action / reward / strehl recorded;
(c) the loop the trainers run (MAIN/PO4AO/mbrl.py:64-89) in Python: action = gainCL * obs + env.sample_noise(sigma), env.step,
    the transition written into preallocated trajectory tensors.
Each figure is the median over `repeats` timed runs of `steps` steps after a warm-up round, torch.cuda.synchronize() on both
sides; the states alternate inside every round so that clock drift hits all alike.  One JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rlao_amd.env import BatchedAOEnv  # noqa: E402

SIGMA, GAIN = 0.05, 0.5


def make_env(n, steps):
    geo = dict(diameter=8.0, nSubaperture=20, nPixelPerSubap=6, r0=0.13, L0=30.0, windSpeed=[10.0], windDirection=[72.0],
               fractionalR0=[1.0], altitude=[0.0], nModes=50, nLoop=steps)
    env = BatchedAOEnv(n_envs=n, device=0, dtype="f32", return_frame=False)
    env.set_params(geo, camera="ideal", wfs_type="shackhartmann", gainCL=GAIN)
    return env


def episode(env, seed):
    env.generate_new_phase_screen(seed)
    env.dm.coefs = 0
    env.dm_prev = 0
    env.measure()
    env.SR = []
    return env.reset_soft()


def python_loop(env, steps, traj):
    t_obs, t_act, t_rew, t_sr = traj
    obs = env._obs
    for k in range(steps):
        t_obs[k] = obs
        action = GAIN * obs + env.sample_noise(SIGMA)
        obs, _, reward, strehl, _, _ = env.step(k, action)
        t_act[k], t_rew[k], t_sr[k] = action, reward, strehl
    t_obs[steps] = obs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("n_envs", nargs="?", type=int, default=256)
    ap.add_argument("steps", nargs="?", type=int, default=512)
    ap.add_argument("repeats", nargs="?", type=int, default=9)
    a = ap.parse_args()
    n, steps, repeats = a.n_envs, a.steps, max(9, a.repeats)
    states = ("a", "b", "c", "a2")
    envs = {k: make_env(n, steps) for k in states}
    A_ = envs["c"].nActuator
    dev, dt = envs["c"].device, envs["c"].tdtype
    traj = (torch.empty((steps + 1, n, A_, A_), device=dev, dtype=dt), torch.empty((steps, n, A_, A_), device=dev, dtype=dt),
            torch.empty((steps, n), device=dev, dtype=dt), torch.empty((steps, n), device=dev, dtype=dt))
    run = {"a": lambda e: e.run_integrator(0, steps, GAIN), "a2": lambda e: e.run_integrator(0, steps, GAIN),
           "b": lambda e: e.rollout(0, steps, SIGMA, gain=GAIN, seed=1), "c": lambda e: python_loop(e, steps, traj)}
    t = {k: [] for k in states}
    for rep in range(repeats + 1):
        for k in states:
            episode(envs[k], 100 + rep)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run[k](envs[k])
            torch.cuda.synchronize()
            if rep:                                                 # (the first round is the warm-up)
                t[k].append(1e3 * (time.perf_counter() - t0))
    us = {k: round(1e3 * float(np.median(v)) / steps, 3) for k, v in t.items()}
    spread = {k: [round(1e3 * min(v) / steps, 3), round(1e3 * max(v) / steps, 3)] for k, v in t.items()}
    a_a = round(abs(us["a"] - us["a2"]), 3)
    out = {"n_envs": n, "steps": steps, "repeats": repeats, "sigma": SIGMA, "gain": GAIN, "fused_step": bool(envs["b"].fused_step),
           "us_per_step": {"run_integrator": us["a"], "run_integrator_again": us["a2"], "rollout": us["b"], "python_loop": us["c"]},
           "min_max_us_per_step": spread, "a_a_spread_us": a_a, "action_launch_us": round(us["b"] - 0.5 * (us["a"] + us["a2"]), 3),
           "python_loop_minus_rollout_us": round(us["c"] - us["b"], 3),
           "rollout_faster_than_python_loop_beyond_a_a": bool(us["c"] - us["b"] > a_a),
           "finite": bool(all(torch.isfinite(e._obs).all() for e in envs.values()))}
    for e in envs.values():
        e.close()
    print(json.dumps(out))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
