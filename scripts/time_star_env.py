#!/usr/bin/env python3
"""Cost of the per-env guide stars (aoenv_set_flux_env / aoenv_set_threshold_env) on the hot path, and the proof that the default
path does not pay for them.
    python scripts/time_star_env.py C2 [n_envs] [steps] [repeats]          one library (AOENV_LIB), one line "measure() <json>"
    bash scripts/ab_libs.sh "scripts/time_star_env.py C2" parent new | tee c2.txt      the two libraries in turn, twice, one session
    cat c2.txt | python scripts/time_star_env.py --collect profiles/star_env_timing.json
C2: the bench geometry (BASELINE configs[1]: 8 m, 20 x 20 Shack-Hartmann, 256 envs, float32, photon noise; the fused step kernel).
Each figure is ms per step of the on-device integrator (run_integrator), the median over `repeats` >= 5 timed runs of `steps`
steps after a warm-up round, torch.cuda.synchronize() on both sides.  The states alternate inside a process and the libraries
alternate between processes, so that clock drift hits all alike:
    off         no per-env star (the specialised instantiation of the step kernel: STEP_PHOTON)
    calibrated  every env at the calibrated magnitude and threshold THROUGH the API (factors of exactly 1; STEP_STAR)
    per_env     256 different magnitudes (m_cal - 2 .. m_cal + 4) and thresholds (0 .. 0.2)
    fainter     256 different magnitudes, none brighter than the calibrated star (m_cal .. m_cal + 4), the same thresholds: no env
                has more pixels above the camera's hand-over to the rejection sampler (alias_lmax) than the calibrated shard, so
                this state carries the cost of the per-env values alone and `per_env` minus it is the photon draw of brighter stars
A library without the entry points (the parent commit's, build/ab/libaoenv_parent.so) is measured in the off state only.
--collect pools the repeats of both passes per (library, state): median, min, max, and the condition the default path is held to
-- the new library's off median no slower than the parent's by more than the parent's own spread (max - min of its repeats); it
exits non-zero where that does not hold.  The states with the feature on are reported, not bounded."""
import ctypes
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

GEOMETRY = {
    "C2": (dict(diameter=8.0, nSubaperture=20, nPixelPerSubap=6, r0=0.13, L0=30.0, windSpeed=[10.0], windDirection=[72.0],
                fractionalR0=[1.0], altitude=[0.0], nModes=50, nLoop=64), 256, 1024),
}
NEW_EXPORTS = ("aoenv_set_flux_env", "aoenv_get_flux_env", "aoenv_set_threshold_env", "aoenv_get_threshold_env")


def run_ms(env, steps):
    import torch
    n_loop = int(env.param.nLoop)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    done = 0
    while done < steps:
        k = min(n_loop, steps - done)
        env.run_integrator(0, k, 0.5)
        done += k
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0)


def measure(which, n, steps, repeats):
    import torch
    from rlao_amd import _lib as L
    has = all(hasattr(ctypes.CDLL(L.LIB_PATH), name) for name in NEW_EXPORTS)
    if not has:                                                     # the parent commit's library: bind what it has
        for name in NEW_EXPORTS:
            L.EXPORTS.pop(name)
    from rlao_amd.env import BatchedAOEnv
    geo = GEOMETRY[which][0]
    env = BatchedAOEnv(n_envs=n, device=0, dtype="f32", return_frame=False)
    env.set_params(geo, camera="papyrus", wfs_type="shackhartmann")
    m_cal, t_cal = float(env.param.magnitude), float(env.param.threshold_cog)
    states = ["off", "calibrated", "per_env", "fainter"] if has else ["off"]
    t = {s: [] for s in states}
    for rep in range(repeats + 1):
        for state in states:
            if state in ("per_env", "fainter"):
                env.set_magnitude_per_env(m_cal + np.linspace(-2.0 if state == "per_env" else 0.0, 4.0, n))
                env.set_threshold_per_env(np.linspace(0.0, 0.2, n))
            elif state == "calibrated":
                env.set_magnitude_per_env(m_cal)
                env.set_threshold_per_env(t_cal)
            elif has:
                env.clear_star_per_env()
            env.generate_new_phase_screen(100 + rep)
            env.dm.coefs = 0
            env.dm_prev = 0
            env.measure()
            env.reset_soft()
            ms = run_ms(env, steps)
            if rep:                                                 # (the first round is the warm-up)
                t[state].append(round(ms / steps, 6))
    out = {"geometry": which, "n_envs": n, "steps": steps, "repeats": repeats, "fused_step": bool(env.fused_step),
           "lib": os.path.basename(L.LIB_PATH), "ms_per_step": t, "finite": bool(torch.isfinite(env._obs).all())}
    env.close()
    print("measure() " + json.dumps(out))


def collect(path):
    pooled = {}
    meta = {}
    for line in sys.stdin:
        if "measure()" not in line:
            continue
        name, rest = line.split("measure()", 1)
        rec = json.loads(rest)
        assert rec["finite"], line
        g = rec["geometry"]
        meta[g] = {k: rec[k] for k in ("n_envs", "steps", "repeats", "fused_step")}
        for state, v in rec["ms_per_step"].items():
            pooled.setdefault(g, {}).setdefault(f"{name.strip()}:{state}", []).extend(v)
    out = {"unit": "ms per step of the on-device integrator, median / min / max over the pooled repeats of two alternating passes",
           "command": "bash scripts/ab_libs.sh 'scripts/time_star_env.py <geometry>' parent new | python scripts/time_star_env.py --collect <file>"}
    for g, d in pooled.items():
        rows = {k: {"median": round(float(np.median(v)), 5), "min": round(min(v), 5), "max": round(max(v), 5), "n": len(v)} for k, v in d.items()}
        res = dict(meta[g], **rows)
        p, s = rows.get("parent:off"), rows.get("new:off")
        if p and s:
            spread = p["max"] - p["min"]
            res["parent_spread"] = round(spread, 5)
            res["off_vs_parent"] = round(s["median"] / p["median"], 4)
            res["default_path_holds"] = bool(s["median"] <= p["median"] + spread)
        for on in ("calibrated", "per_env", "fainter"):
            if s and rows.get("new:" + on):
                res[on + "_vs_off"] = round(rows["new:" + on]["median"] / s["median"], 4)
        out[g] = res
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))
    slower = [g for g in pooled if out[g].get("default_path_holds") is False]
    if slower:                                                      # a re-measurement must not record a regression silently
        sys.exit(f"the default path is slower than the parent's by more than the parent's spread at {', '.join(slower)}")


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--collect":
        collect(sys.argv[2])
    else:
        which = sys.argv[1] if len(sys.argv) > 1 else "C2"
        _, n0, s0 = GEOMETRY[which]
        measure(which, int(sys.argv[2]) if len(sys.argv) > 2 else n0, int(sys.argv[3]) if len(sys.argv) > 3 else s0,
                max(5, int(sys.argv[4]) if len(sys.argv) > 4 else 7))
