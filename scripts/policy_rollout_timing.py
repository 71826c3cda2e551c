#!/usr/bin/env python3
"""What a policy episode of PO4AO (MAIN/PO4AO/mbrl.py:64-89 after the warm-up) costs per step, on one shard each of the C3 geometry
(8 m, 40 x 40 Pyramid, 1024 envs) and the C2 geometry (8 m, 20 x 20 Shack-Hartmann, 256 envs), float32, ideal camera, the policy
of bench.py (n_history 20, 64 filters, its seeded weights), one build, one session.
    python scripts/policy_rollout_timing.py [--out profiles/policy_rollout_timing.json] [--steps K] [--repeats R] [--configs C3,C2]
(a) the loop a caller writes today: env.step plus the stock-PyTorch ConvPolicy of bench.py with its device ring histories;
(b) BatchedAOEnv.policy_rollout: the same policy by the library's kernels, the trajectory recorded;
and the policy alone in both: K calls of the torch policy, K calls of policy_action (three launches each).
Every figure is the median over R timed regions of K steps after a warm-up round of every state, torch.cuda.synchronize() on
both sides; the states alternate inside every round so that clock drift hits all alike.  The step share of (a) and (b) is the
region time minus the policy-alone time.  Before anything is timed the two policies are compared on the same random windows at
the timed size (max |library - torch|).  Writes one JSON file and prints it."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import bench  # noqa: E402
from rlao_amd.env import BatchedAOEnv  # noqa: E402
from rlao_amd.wrappers import DeviceHistory  # noqa: E402

N_HISTORY, N_FILT = 20, 64
CONFIGS = {"C3": dict(geo=bench.CONFIGS["C3"]["geo"], wfs="pyramid", envs=1024),
           "C2": dict(geo=bench.GEOMETRY, wfs="shackhartmann", envs=256)}


def episode(env, seed):
    env.generate_new_phase_screen(seed)
    env.dm.coefs = 0
    env.dm_prev = 0
    env.measure()
    env.SR = []
    return env.reset_soft()


def flops_per_env(a, H, F):
    """multiply-adds x 2 of the three convolutions at every pixel (the last one at every pixel too: an upper bound)"""
    return 2 * a * a * 9 * ((2 * H - 1) * F + F * F + F)


def measure(name, steps, repeats):
    cfg = CONFIGS[name]
    n, K = cfg["envs"], steps
    env = BatchedAOEnv(n_envs=n, device=0, dtype="f32", return_frame=False)
    env.set_params(dict(cfg["geo"], nLoop=K + 8), camera="ideal", wfs_type=cfg["wfs"])
    a = env.nActuator
    policy = bench.ConvPolicy(env, N_HISTORY, N_FILT)
    env.set_policy(policy.net)
    # the same function: random windows at the timed size
    g = torch.Generator(device="cpu").manual_seed(3)
    x = [torch.randn(s, generator=g).to(env.device) for s in ((n, a, a), (n, N_HISTORY - 1, a, a), (n, N_HISTORY - 1, a, a))]
    diff = float((env.policy_action(*x) - policy(*x)).abs().max())
    hist_o, hist_a = DeviceHistory(n, N_HISTORY - 1, a, env.device), DeviceHistory(n, N_HISTORY - 1, a, env.device)
    st = {}

    def loop_today():
        obs = st["obs"]
        for t in range(K):
            action = policy(obs, hist_o.window(), hist_a.window())
            nxt = env.step(t, action)[0]
            hist_o.push(obs)
            hist_a.push(action)
            obs = nxt

    def library():
        st["tr"], st["past"] = env.policy_rollout(0, K, sigma=0.0, past=st.get("past"))

    def torch_policy_alone():
        for _ in range(K):
            policy(st["obs"], hist_o.window(), hist_a.window())

    def library_policy_alone():
        for _ in range(K):
            env.policy_action(st["obs"], x[1], x[2])

    states = {"loop_today": loop_today, "policy_rollout": library, "torch_policy_alone": torch_policy_alone,
              "library_policy_alone": library_policy_alone}
    t = {k: [] for k in states}
    for rep in range(repeats + 1):
        for k, run in states.items():
            st["obs"] = episode(env, 100 + rep)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run()
            torch.cuda.synchronize()
            if rep:                                                 # (the first round is the warm-up)
                t[k].append(1e3 * (time.perf_counter() - t0) / K)
    ms = {k: round(float(np.median(v)), 4) for k, v in t.items()}
    spread = {k: [round(min(v), 4), round(max(v), 4)] for k, v in t.items()}
    fl = flops_per_env(a, N_HISTORY, N_FILT) * n
    out = {"geometry": name, "wfs": cfg["wfs"], "n_envs": n, "n_act": a, "steps": K, "repeats": repeats, "n_history": N_HISTORY, "n_filt": N_FILT,
           "fused_step": bool(env.fused_step), "max_abs_library_minus_torch": diff,
           "ms_per_step": ms, "min_max_ms_per_step": spread,
           "policy_share": {"loop_today": round(ms["torch_policy_alone"] / ms["loop_today"], 4),
                            "policy_rollout": round(ms["library_policy_alone"] / ms["policy_rollout"], 4)},
           "policy_gflop_per_step": round(fl / 1e9, 3),
           "policy_tflops": {"torch": round(fl / ms["torch_policy_alone"] / 1e9, 2), "library": round(fl / ms["library_policy_alone"] / 1e9, 2)},
           "finite": bool(torch.isfinite(st["tr"].obs).all())}
    env.set_policy(None)
    env.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "policy_rollout_timing.json"))
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--configs", default="C3,C2")
    a = ap.parse_args()
    out = {"note": "ms per step, median of `repeats` regions of `steps` steps after a warm-up round; policy share = policy alone / loop",
           "configs": [measure(c, a.steps, max(3, a.repeats)) for c in a.configs.split(",")]}
    print(json.dumps(out))
    with open(a.out, "w") as f:
        f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
