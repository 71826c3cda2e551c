"""GPU: every per-env and loop feature of the library AT ONCE -- per-env wind (one env above a pixel per frame), per-env r0, per-env
mis-registered mirrors, per-env guide stars and centroid thresholds, per-env vibration lines, a control delay, the modal surface, a
wavefront record, a running long exposure and a partial reset -- held to the float64 oracle that composes them per env
(tests/_compose_ref.ComposedOracle, pinned on the CPU by tests/test_compose_host.py) and to bitwise twins.  The features were
added one by one and tested one by one; env.hip threads their state through one another (the command the sensor sees, the delay
line's slots, the deferred ring with the env's innovation scale, the per-env tap rows and mirror tables, the choice of the step
kernel's instantiation), and this module is where a wrong interaction shows.

CASE_MIXED (tests/_compose_ref.py): 4 envs, 12 frames, delay 1, wind ceiling 2.  Shack-Hartmann: SMALL of tests/test_gpu_star_env.py
(R = 48, the fused step kernel in float32: with a per-env star it runs its STEP_STAR instantiation, rlao_amd/csrc/step_kernel.hip);
Pyramid: TINY_PYR (R = 24), the same case without thresholds.  Shards are built once per module.

a / b  oracle anchors: the float64 and the float32 shard (the fused step, then OPT_FUSED_STEP = 0, then also OPT_FUSED_TAIL = 0)
       replay the oracle's recorded float32 actions through step, and through step_modal with K = 2 and K = all modes; signal,
       observation, reward, Strehl and frame of every step and env, then the screens, both OPDs and the telemetry.  The oracle is
       handed the env's own ring operators, mode-to-command matrix and command matrices (build_base of the geometry and Pyramid
       sweeps; their _replay does not fit: it knows no modal step and stops comparing the end state beyond six frames).
c      every loop (run_integrator, rollout, policy_rollout, run_integrator_modal; calls of 1, 5 and 10 frames, so that the delay
       line's refill crosses call boundaries) equals the same frames driven one step at a time on a second shard, bit for bit, with
       photon and read-out noise, a wavefront record and a long exposure attached.
d      mixture independence: row e of the mixed shard equals row e of a twin shard whose envs all carry env e's values.
e      the two-step launch (OPT_STEP_PAIRS) under per-env mirrors and per-env r0, with and without the long exposure.
f      reset_envs([1, 3]) at frame 6, a checkpoint at frame 9 and its resume on another shard.
g      after every feature's clear call the shard runs like one that never had them.

Tolerances: float64 F64_SAME_OPERATOR_TOL_FULL of tests/test_gpu_parity.py, float32 F32_TOL, both unchanged: no quantity needed a
wider bound (measured on MI355X: every float64 maximum at or below 26 % of its bound -- the separable gy C gx^T product against the
dense Gaussian and the sine of the disturbance stay inside the re-ordering noise --, every float32 maximum at or below 21 %;
AO_PARITY_REPORT=<file> with this module alone rewrites profiles/compose_parity_maxima.json, the launch counts of every float32
path beside the maxima).  Nothing is measured against the code under test.

That the module bites was checked once with three scratch builds of the host layer, each wrong in one interaction: step_modal_t
running its step with the disturbance switched off -> every modal anchor (a, b) fails and every zonal one passes; the draw-ahead of
the deferred ring handed no innovation scale -> both step-pair tests fail, at the oracle's screens (the two runs still agree bit
for bit: why (e) carries an oracle anchor of its own); the tail kernel handed no per-env threshold -> the float64 Shack-Hartmann
anchors and the float32 tail anchors fail, the fused step, the centroid path and the Pyramid pass."""
import json
import os

import numpy as np
import pytest

import _compose_ref as CR
import _policy_ref as P
from test_gpu_parity import F32_TOL, F64_SAME_OPERATOR_TOL_FULL, _OBSERVED

pytestmark = pytest.mark.gpu

SMALL = dict(diameter=3.2, nSubaperture=8, nPixelPerSubap=6, r0=0.13, L0=30.0, windSpeed=[10.0], windDirection=[72.0],
             fractionalR0=[1.0], altitude=[0.0], nModes=20, nLoop=64)                      # tests/test_gpu_star_env.py
TINY_PYR = dict(diameter=1.6, nSubaperture=4, nPixelPerSubap=6, r0=0.13, L0=30.0, windSpeed=[10.0], windDirection=[72.0],
                fractionalR0=[1.0], altitude=[0.0], nModes=8, nLoop=64, modulation=0.0, psfCentering=True)
GEO = {"sh": SMALL, "pyr": TINY_PYR}
CASE = CR.CASE_MIXED
N, STEPS, SEED = CASE["n_envs"], CASE["steps"], CASE["seed"]
PITCH = 0.4                                                         # both geometries: diameter / nSubaperture [m]
MIN_CUT_GAP = 1e-7                                                  # tests/test_gpu_geometry_sweep.py
GAIN = 0.5
# the gain of the recorded modal runs, chosen on the CPU from the oracle alone among 0.3 .. 0.6 for the distance of every pixel from
# every env's centroid cut in both modal runs (K = 2: 8.9e-7, K = 20: 6.6e-7 of the brightest pixel; at 0.5 the K = 20 run comes
# within 2.6e-8 of a cut, under MIN_CUT_GAP)
MODAL_GAIN = 0.4
CALLS = (1, 5, 10)                                                  # frames per call of a device loop: 16 in all
ALL = ("r0", "wind", "star", "mirror", "disturbance", "delay")

# ---- shards: built once per module --------------------------------------------------------------------------------------------------
_SHARDS = {}


@pytest.fixture(scope="module", autouse=True)
def _close_shards():
    yield
    for env in _SHARDS.values():
        env.close()
    _SHARDS.clear()


def _new_shard(kind, dtype, camera="ideal", opts=None):
    from rlao_amd import _lib as L
    from rlao_amd.env import BatchedAOEnv
    env = BatchedAOEnv(n_envs=N, device=0, dtype=dtype, env_seed_stride=CASE["seed_stride"])
    try:
        env.set_params(dict(GEO[kind]), camera="ideal" if camera == "ideal" else camera.split("+")[0],
                       wfs_type="shackhartmann" if kind == "sh" else "pyramid", gainCL=GAIN)
        if camera == "papyrus+readout":
            env.wfs.cam.configure(readoutNoise=1.0)
        for k, v in (opts or {}).items():
            L.check(env._shard.lib.aoenv_set_option(env._shard.h, getattr(L, k), v))
        env._counters0 = env._shard.download(L.B_COUNTERS, (4,), env._stream(), dtype=np.uint32).copy()
        env._kind = kind
    except Exception:
        env.close()
        raise
    return env


def _shard(kind, dtype, camera="ideal", opts=None, tag="a"):
    key = (kind, dtype, camera, tuple(sorted((opts or {}).items())), tag)
    if key not in _SHARDS:
        _SHARDS[key] = _new_shard(kind, dtype, camera, opts)
    env = _SHARDS[key]
    _clear(env)
    return env


def _clear(env):
    """every feature off, through the calls a user makes (a cached shard starts each test from here)"""
    env.clear_disturbance()
    env.set_delay(0)
    env.clear_dm_per_env()
    env.clear_star_per_env()
    if env.n_modal:
        env.clear_modal()
    if env.n_wavefront_modes:
        env.clear_wavefront_basis()
    if env.science is not None:
        env.clear_science()
    if env.policy_n_history is not None:
        env.set_policy(None)


def _apply(env, envs=None, features=ALL):
    """CASE_MIXED through the public per-env calls.  ``envs``: which case env each env of the shard is (a twin: [e] * 4)."""
    rows = list(range(N)) if envs is None else list(envs)
    col = lambda key: np.array([CASE[key][e] for e in rows], dtype=np.float64)
    if "r0" in features:
        env.set_r0_per_env(col("r0"))
    else:
        env.atm.r0 = float(GEO[env._kind]["r0"])
    if "star" in features:
        env.set_magnitude_per_env(col("magnitude"))
        if env._kind == "sh":
            env.set_threshold_per_env(col("threshold"))
    if "mirror" in features:
        m = [CR.mixed_misreg(e, PITCH) for e in rows]
        env.set_dm_misregistration(**{k: np.array([x.get(k, 0.0) for x in m]) for k in CR.MISREG_KEYS})
    if "disturbance" in features:
        dt = env.param.samplingTime
        freq = np.array([0.0 if CASE["dist_period"][e] is None else 1.0 / (CASE["dist_period"][e] * dt) for e in rows])
        env.set_disturbance(1, col("dist_amp").reshape(N, 1, 1), freq.reshape(N, 1, 1), t0=CASE["t0"])
    if "delay" in features:
        env.set_delay(CASE["delay"])
    env._case_rows, env._case_wind = rows, "wind" in features


def _start(env, modal=False, seed=SEED):
    """the episode prologue of the trainers, every episode from the same camera frame number"""
    from rlao_amd import _lib as L
    env._shard.upload_state(L.B_COUNTERS, env._counters0, env._stream(), dtype=np.uint32)
    env.generate_new_phase_screen(seed)
    rows = env._case_rows
    if env._case_wind:
        env.set_wind_per_env(np.array([[CASE["wind_speed"][e]] for e in rows]), np.array([[CASE["wind_dir"][e]] for e in rows]),
                             reset=True, max_pixels=CASE["wind_ceiling"])
    env.dm.coefs = 0
    env.dm_prev = 0
    env.measure()
    return env.reset_soft_modal() if modal else env.reset_soft()


# ---- the oracle side: one base per geometry, one record per (geometry, surface) --------------------------------------------------------
_BASES, _RECORDS = {}, {}


def _base(env):
    kind = env._kind
    if kind not in _BASES:
        from test_gpu_geometry_sweep import build_base as build_sh
        from test_gpu_pyramid_sweep import build_base as build_pyr
        at = env._atm_tables
        base = (build_sh if kind == "sh" else build_pyr)(dict(GEO[kind], nLoop=16), env.M2C_CL, at.A, at.B)
        assert np.array_equal(env.dm_mask.astype(bool), base.dm_mask) and env.nSignal == base.wfs.nSignal
        geom = base.atm.layers[0].g
        _OBSERVED["compose-scaled-B-" + kind] = dict(
            CR.scaled_B_error(geom, np.asarray(at.A, dtype=np.float64), np.asarray(at.B, dtype=np.float64), GEO[kind]["r0"], CASE["r0"]),
            bound=CR.SCALED_B_BOUND, unit="max |B (r0_cal / r0_e)^(5/6) - chol at r0_e| / max |B_e|, formed on the test host's CPU from the env's tables")
        _BASES[kind] = base
    return _BASES[kind]


def _record(env, K=None, events=None):
    """The oracle's run of CASE_MIXED for this geometry: zonal (K None) or through the modal surface of K modes (the env must
    carry it: its command matrix is handed over).  From the oracle alone: the case's conditions."""
    key = (env._kind, K, None if events is None else "events")
    if key not in _RECORDS:
        base = _base(env)
        cm_K = None if K is None else np.asarray(env._modal["cm"], dtype=np.float64)
        orc = CR.mixed_oracle(base, PITCH, m2c=env.M2C_CL, modal_cm=env.modal_CM, modal=K, modal_cm_K=cm_K)
        rec = CR.drive(orc, STEPS, modal_gain=None if K is None else MODAL_GAIN, events=events)
        rec["modal_cm"], rec["cm_K"] = np.asarray(env.modal_CM, dtype=np.float64).copy(), cm_K
        if np.isfinite(rec["min_gap"]):
            seen = _OBSERVED.setdefault(f"compose-{env._kind}-oracle", {})
            seen["threshold_gap_min"] = min(seen.get("threshold_gap_min", np.inf), rec["min_gap"])
        _RECORDS[key] = rec
    rec = _RECORDS[key]
    # every env calibrates on the GPU in float64 whatever its dtype: a later shard must have come to the same controller
    np.testing.assert_allclose(env.modal_CM, rec["modal_cm"], rtol=0, atol=1e-12 * float(np.abs(rec["modal_cm"]).max()))
    if K is not None:
        np.testing.assert_allclose(env._modal["cm"], rec["cm_K"], rtol=0, atol=1e-12 * float(np.abs(rec["cm_K"]).max()))
    assert rec["min_gap"] >= MIN_CUT_GAP, rec["gap"]
    assert (rec["crossings"] >= 2).all(), rec["crossings"]
    rounds = rec["rounds"][:, :, 0]
    assert ((rounds[:, 3] >= 1) & (rounds[:, 0] == 0)).any() and rounds.max() < CASE["wind_ceiling"]
    return rec


class _Check:
    """Collects every comparison of a test, records the largest error per quantity (AO_PARITY_REPORT) and fails at the end with
    all of them: one run on the GPU shows every figure."""

    def __init__(self, tol, label):
        self.tol, self.label, self.bad = tol, label, []

    def close(self, got, want, key, what, scale=1.0, atol=None, rtol=0.0):
        got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
        assert got.shape == want.shape, (what, got.shape, want.shape)
        err = np.abs(got - want)
        rec = _OBSERVED.setdefault(self.label, {})
        rec[key] = max(rec.get(key, 0.0), float(err.max()) / scale if np.isfinite(err).all() else np.inf)
        bound = (self.tol[key] * scale if atol is None else atol) + rtol * np.abs(want)
        if not (err <= bound).all():
            self.bad.append(f"{what}: {key} off by {float(err.max()) / scale:.3e} (bound {float(np.max(bound)) / scale:.3e})")

    def done(self):
        path = os.environ.get("AO_PARITY_REPORT")
        if path:
            with open(path, "w") as f:
                json.dump(_OBSERVED, f, indent=1, sort_keys=True)
        print(self.label, json.dumps(_OBSERVED.get(self.label, {}), sort_keys=True))
        assert not self.bad, (self.label, len(self.bad), self.bad[:12])


def _launches(env, fn):
    env._shard.profile(True)
    out = fn()
    prof = env._shard.profile_read(env._stream())
    env._shard.profile(False)
    return out, {k: n for k, (ms, n) in prof.items()}


def _replay(env, rec, tol, label, K=None, rows=range(N), steps=STEPS, events=None, first_telemetry=None):
    """A fresh episode of the (configured) shard driven by the oracle's recorded float32 actions; every quantity of every step and
    of the listed rows, then the end state.  Returns what the shard gave per step."""
    import torch
    from rlao_amd import _lib as L
    chk = _Check(tol, label)
    obs0 = _start(env, modal=K is not None).cpu().numpy()
    out = [obs0]
    for e in rows:
        chk.close(obs0[e], rec["obs0"][e], "obs", f"obs after reset, env {e}")
    scr = env._download_screens()
    for e in rows:
        chk.close(scr[0][e], rec["screen0"][e][0], "screen", f"screen after reset, env {e}")
    for i in range(steps):
        if events and i in events:
            ids = [e for e, _, _ in events[i]]
            got = env.reset_envs(ids, seed=np.array([s for _, s, _ in events[i]]), r0=[r for _, _, r in events[i]]).cpu().numpy()
            for k, e in enumerate(ids):
                chk.close(got[k], rec["reset_obs"][i][k], "obs", f"obs of reset_envs at frame {i}, env {e}")
        act = torch.as_tensor(rec["actions"][i])
        obs, frame, rew, sr, _, _ = env.step_modal(i, act) if K is not None else env.step(i, act)
        obs, frame, rew, sr = obs.cpu().numpy(), frame.cpu().numpy(), rew.cpu().numpy(), sr.cpu().numpy()
        sig = env._shard.download(L.B_SIGNAL, (N, env.nSignal), env._stream())
        out.append((obs, frame, rew, sr, sig))
        for e in rows:
            at = f"step {i} env {e}"
            chk.close(sig[e], rec["signal"][i][e], "signal", at)
            chk.close(obs[e], rec["obs"][i][e], "obs", at)
            want_obs = rec["obs"][i][e]
            # zonal: -||obs||; modal: -sum obs^2, whose error is at most sum 2 |obs| d + d^2 for an error d of each coefficient
            slack = tol["obs"] if K is None else 2 * np.abs(want_obs).sum() * tol["obs"] + want_obs.size * tol["obs"] ** 2
            chk.close(rew[e], rec["reward"][i][e], "reward_rel", at, atol=slack, rtol=tol["reward_rel"])
            chk.close(sr[e], rec["strehl"][i][e], "strehl", at)
            chk.close(frame[e], rec["frame"][i][e], "frame_rel", at, scale=float(rec["frame"][i][e].max()))
    if steps == STEPS:
        scr = env._download_screens()
        opd_atm = env._shard.download(L.B_OPD_ATM, (N, env.R, env.R), env._stream())
        phase = env._shard.download(L.B_PHASE, (N, env.R, env.R), env._stream())
        tot, res = env.total[:steps], env.residual[:steps]
        for e in rows:
            f0 = 0 if first_telemetry is None else first_telemetry.get(e, 0)
            chk.close(scr[0][e], rec["screen"][e][0], "screen", f"screen env {e}")
            chk.close(opd_atm[e] * env.pupil, rec["opd_atm"][e], "opd_m", f"atm.OPD env {e}")
            chk.close(phase[e] * env.src_wavelength / (2 * np.pi), rec["opd_res"][e], "opd_m", f"residual OPD env {e}")
            chk.close(tot[f0:, e], rec["total"][f0:, e], "rms_nm", f"total env {e}")
            chk.close(res[f0:, e], rec["residual"][f0:, e], "rms_nm", f"residual env {e}")
    chk.done()
    return out


def _surface(env, K):
    if K is not None:
        env.set_modal(K)
        env.set_modal_gain(GAIN)


SURFACES = {"sh": [None, 2, 20], "pyr": [None, 2, 8]}
ANCHORS = [(k, K) for k in ("sh", "pyr") for K in SURFACES[k]]
_ids = lambda runs: ["-".join("zonal" if x is None else (f"K{x}" if isinstance(x, int) else str(x)) for x in r) for r in runs]


# ---- a. the float64 shard against the oracle ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,K", ANCHORS, ids=_ids(ANCHORS))
def test_float64_shard_matches_the_composed_oracle(kind, K):
    """float64, the ideal camera, every feature through the public per-env calls: re-ordering noise against the oracle that shares
    its operators."""
    env = _shard(kind, "f64")
    _surface(env, K)
    _apply(env)
    assert not env.fused_step and env.delay == CASE["delay"]
    _replay(env, _record(env, K), F64_SAME_OPERATOR_TOL_FULL, f"compose-{kind}-{'zonal' if K is None else f'K{K}'}-f64", K=K)


# ---- b. the float32 shard against the oracle --------------------------------------------------------------------------------------------
F32_RUNS = ([("sh", K, "fused") for K in SURFACES["sh"]] + [("sh", None, "tail"), ("sh", None, "centroid"), ("sh", 20, "tail")]
            + [("pyr", K, "pyramid") for K in SURFACES["pyr"]])
F32_OPTS = {"fused": {}, "tail": {"OPT_FUSED_STEP": 0}, "centroid": {"OPT_FUSED_STEP": 0, "OPT_FUSED_TAIL": 0}, "pyramid": {}}


@pytest.mark.parametrize("kind,K,path", F32_RUNS, ids=_ids(F32_RUNS))
def test_float32_shard_matches_the_composed_oracle(kind, K, path):
    """float32: the fused step kernel (with per-env stars its STEP_STAR instantiation: the arrays are present, the shard stays
    fused and every step is one env_step launch), the spots + tail kernels, the spots + centroid + reconstruction kernels, the
    Pyramid -- each held to the oracle, not to one another."""
    env = _shard(kind, "f32", opts=F32_OPTS[path])
    _surface(env, K)
    _apply(env)
    assert env.fused_step == (path == "fused")
    assert env._shard.get_flux_env(env._stream()).shape == (N,)     # the per-env star is in force: STEP_STAR (step_kernel.hip)
    label = f"compose-{kind}-{'zonal' if K is None else f'K{K}'}-f32-{path}"
    _, launches = _launches(env, lambda: _replay(env, _record(env, K), F32_TOL, label, K=K))
    _OBSERVED[label]["launches"] = {k: v for k, v in launches.items() if v}
    if path == "fused":
        assert launches["env_step"] == STEPS and launches["sh_tail"] == 0, launches
    elif path == "tail":
        assert launches["env_step"] == 0 and launches["sh_tail"] >= STEPS, launches
    elif path == "centroid":
        assert launches["env_step"] == 0 and launches["sh_tail"] == 0 and launches["sh_centroid"] >= STEPS, launches
    else:
        assert launches["pyramid"] >= STEPS, launches
    assert launches["gemm_ring"] > 0                                # the crossings and env 3's whole-pixel rounds


# ---- c. every loop equals stepping -------------------------------------------------------------------------------------------------------
LOOPS = ("run_integrator", "rollout", "policy_rollout", "run_integrator_modal")
K_LOOP, K_WF, W_LE, FIRST_LE = 5, 6, 32, 2


def _attach(env):
    """the modal surface, a policy, the wavefront basis and the science camera (configuration; the record and the exposure are
    attached per run)"""
    n_pix = int(np.count_nonzero(env.pupil))
    env.set_modal(K_LOOP)
    env.set_modal_gain(GAIN)
    env.set_policy(P.make_weights(3, 16, seed=5, scale=(20.0, 1.5, 2.0)))
    env.set_wavefront_basis(opd2m=np.random.RandomState(4).normal(0, 1, (K_WF, n_pix)) / n_pix)
    env.set_science(zero_padding=4, window=W_LE, first_frame=FIRST_LE, log10=True)


def _np(t):
    return t.detach().cpu().numpy()


def _end_of_call(env, handed):
    """what a caller can see after a call: the tensors handed out, the device buffers, the delay line and the checkpoint"""
    from rlao_amd import _lib as L
    out = {f"out[{j}]": _np(t) for j, t in enumerate(handed)}
    out["phase"] = env._shard.download(L.B_PHASE, (N, env.R, env.R), env._stream())
    out["frame"] = env._shard.download(L.B_FRAME, (N, env.cam_res, env.cam_res), env._stream())
    out["delay_line"] = _np(env.delay_line())
    for k, v in env.get_state().items():
        out["state." + k] = v
    return out


def _run_loop(env, loop, stepping=False, actions=None):
    """CALLS frames through the loop, or (``stepping``) the same frames one step / step_modal at a time -- the integrators' actions
    formed here as gain * obs, the rollouts' ``actions`` those the loop issued.  Returns per call what is visible at its end, per
    frame (obs, reward, strehl) where the loop hands them out, the issued actions, the record and the long exposure."""
    import torch
    modal = loop == "run_integrator_modal"
    obs = _start(env, modal=modal)
    n = sum(CALLS)
    rec = env.record_wavefront(0, n, ("residual", "atmosphere"))
    env.start_long_exposure()
    ends, frames, issued, past, i = [], [], [], None, 0
    for c in CALLS:
        if not stepping and loop == "run_integrator":
            obs, rew, sr = env.run_integrator(i, c)
            handed = [obs, rew, sr]
        elif not stepping and loop == "run_integrator_modal":
            obs, rew, sr = env.run_integrator_modal(i, c)
            handed = [obs, rew, sr]
        elif not stepping:
            if loop == "rollout":
                tr = env.rollout(i, c, sigma=0.05, gain=GAIN, seed=9 if i == 0 else None)
            else:
                tr, past = env.policy_rollout(i, c, sigma=0.02, past=past, seed=9 if i == 0 else None)
            issued += list(tr.action.unbind(0))
            frames += [(tr.obs[k + 1], tr.reward[k], tr.strehl[k]) for k in range(c)]
            handed = [tr.obs[c], tr.reward[c - 1], tr.strehl[c - 1]]
        else:
            for k in range(i, i + c):
                if loop in ("run_integrator", "run_integrator_modal"):
                    a = GAIN * obs
                else:
                    a = actions[k]
                obs, _, rew, sr, _, _ = env.step_modal(k, a) if modal else env.step(k, a)
                frames.append((obs, rew, sr))
            handed = [obs, rew, sr]
        i += c
        torch.cuda.synchronize()
        ends.append(_end_of_call(env, handed))
    le = [None if t is None else _np(t).copy() for t in env._le]
    env.stop_long_exposure()
    env.stop_wavefront_record()
    return dict(ends=ends, frames=[tuple(_np(t) for t in f) for f in frames], issued=issued, record=_np(rec).copy(), le=le)


def _same_runs(got, want, loop, rows=range(N), what=""):
    """bit for bit, over the listed rows (of per-env arrays)"""
    rows = list(rows)
    skip = {"state.explore_seed", "state.wind_env", "state.windSpeed", "state.windDirection", "state.wind_pixels", "state.delay"}
    if loop == "run_integrator_modal":
        skip.add("state.obs")                                       # (a modal loop keeps its observation apart)
    per_env_axis = {"delay_line": 1, "state.delay_line": 1, "state.screen": 1, "state.mt": 1, "state.clock_env": 1}
    for c, (a, b) in enumerate(zip(got["ends"], want["ends"])):
        assert a.keys() == b.keys()
        for k in a:
            if k in skip or a[k] is None:
                continue
            x, y = np.asarray(a[k]), np.asarray(b[k])
            if k == "state.counters":                               # word 1 counts the exploration stream's draws: a rollout's own
                x, y = x[[0, 2, 3]], y[[0, 2, 3]]
            elif len(rows) < N:
                x, y = np.take(x, rows, axis=per_env_axis.get(k, 0)), np.take(y, rows, axis=per_env_axis.get(k, 0))
            assert x.dtype == y.dtype and np.array_equal(x, y, equal_nan=True), (what, loop, "call", c, k)
    if got["frames"] and want["frames"]:
        assert len(got["frames"]) == len(want["frames"])
        for i, (a, b) in enumerate(zip(got["frames"], want["frames"])):
            for q, (x, y) in enumerate(zip(a, b)):
                assert np.array_equal(x[rows], y[rows], equal_nan=True), (what, loop, "frame", i, "quantity", q)
    assert np.array_equal(got["record"][:, :, rows], want["record"][:, :, rows], equal_nan=True), (what, loop, "wavefront record")
    for j, (x, y) in enumerate(zip(got["le"], want["le"])):
        assert (x is None) == (y is None) and (x is None or np.array_equal(x[rows], y[rows], equal_nan=True)), (what, loop, "long exposure", j)


def _loop_pair(dtype, camera):
    envs = [_shard("sh", dtype, camera, tag=t) for t in "ab"]
    for e in envs:
        _attach(e)
    return envs


LOOP_RUNS = [(d, l) for d in ("f32", "f64") for l in LOOPS]


@pytest.mark.parametrize("dtype,loop", LOOP_RUNS, ids=_ids(LOOP_RUNS))
def test_every_loop_equals_stepping_with_everything_on(dtype, loop):
    """CASE_MIXED, photon and read-out noise, the record of residual and atmosphere, the long exposure (window 32): the loop in
    calls of 1, 5 and 10 frames against the same frames through step / step_modal on a second shard -- observations, actions,
    rewards, Strehl, frames, the record, the exposure, the delay line and get_state(), bit for bit."""
    env, twin = _loop_pair(dtype, "papyrus+readout")
    for e in (env, twin):
        _apply(e)
    assert env.fused_step == (dtype == "f32")
    got = _run_loop(env, loop)
    want = _run_loop(twin, loop, stepping=True, actions=got["issued"])
    assert len(got["issued"]) == (sum(CALLS) if "rollout" in loop else 0)
    _same_runs(got, want, loop, what="loop against stepping")
    n = sum(CALLS)
    assert np.array_equal(got["le"][2], np.full(N, n - FIRST_LE, dtype=np.int32)) and got["le"][0].min() >= 0
    assert np.isfinite(got["record"]).all() and all(np.abs(got["record"][k]).max() > 0 for k in range(n))
    fr = got["ends"][-1]["frame"]
    assert (fr == np.round(fr)).all() and fr.max() > 0              # counts
    assert np.abs(got["ends"][-1]["delay_line"]).max() > 0
    assert not np.array_equal(got["ends"][-1]["out[0]"][1], got["ends"][-1]["out[0]"][3])


# ---- d. mixture independence ------------------------------------------------------------------------------------------------------------
MIX_RUNS = [("f32", "papyrus+readout"), ("f32", "razor"), ("f64", "papyrus+readout")]


@pytest.mark.parametrize("dtype,camera", MIX_RUNS, ids=_ids(MIX_RUNS))
def test_each_env_of_the_mixture_equals_its_uniform_twin(dtype, camera):
    """Row e of the mixed shard == row e of a twin shard in which every env carries env e's values, set through the same calls
    (row e has the same seed): over all four loops, with the record and the exposure attached."""
    env, twin = _loop_pair(dtype, camera)
    _apply(env)
    got = {loop: _run_loop(env, loop) for loop in LOOPS}
    for e in range(N):
        _apply(twin, envs=[e] * N)
        for loop in LOOPS:
            _same_runs(got[loop], _run_loop(twin, loop), loop, rows=[e], what=f"env {e} against its twin, {camera}")
    last = got["run_integrator"]["ends"][-1]["frame"]
    assert all(not np.array_equal(last[0], last[e]) for e in range(1, N))


# ---- e. the two-step launch under per-env tables ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("exposure", [False, True], ids=["plain", "long-exposure"])
def test_step_pairs_under_per_env_mirrors_and_r0(exposure):
    """float32, photon noise, per-env mirrors and per-env r0, the shared wind, no star, no disturbance, no delay (each of those
    makes a loop ineligible): run_integrator with OPT_STEP_PAIRS = 1 launches pairs, with 0 none, and everything a caller can see
    is the same bit for bit.  Two runs that agree could both have lost the env's innovation scale in the draw-ahead, so the
    atmosphere of the paired run -- the screens after 12 frames and the `total` telemetry, which no camera noise and no action
    reaches -- is held to the oracle with these r0 as well."""
    import torch
    from rlao_amd import _lib as L
    runs, counters = [], []
    for pairs in (1, 0):
        env = _shard("sh", "f32", "papyrus", opts={"OPT_STEP_PAIRS": pairs}, tag=f"pairs{pairs}")
        _apply(env, features=("r0", "mirror"))
        assert env.fused_step and not env._per_env_clock
        if exposure:
            env.set_science(zero_padding=4, window=W_LE, first_frame=FIRST_LE)
        _start(env)
        if exposure:
            env.start_long_exposure()
        env._shard.profile(True)
        ends, i = [], 0
        for c in (7, 4, 1):
            handed = list(env.run_integrator(i, c))
            i += c
            torch.cuda.synchronize()
            ends.append(_end_of_call(env, handed))
        counters.append(env._shard.step_counters())
        env._shard.profile(False)
        le = [None if t is None else _np(t).copy() for t in env._le] if exposure else []
        if exposure:
            env.stop_long_exposure()
        ends.append(dict(total=np.array(env.total[:i]), residual=np.array(env.residual[:i])))
        runs.append((ends, le))
    print("step counters (launches, steps): pairs on", counters[0], "off", counters[1])
    assert counters[1] == (12, 12), counters
    assert counters[0][1] == 12 and counters[0][0] < 12, counters    # pairs were launched
    (a, le_a), (b, le_b) = runs
    for c, (x, y) in enumerate(zip(a, b)):
        assert x.keys() == y.keys()
        for k in x:
            if x[k] is not None and k not in ("state.windSpeed", "state.windDirection"):
                assert np.array_equal(np.asarray(x[k]), np.asarray(y[k])), ("call", c, k)
    for x, y in zip(le_a, le_b):
        assert (x is None) == (y is None) and (x is None or np.array_equal(x, y))
    if exposure:
        assert np.array_equal(le_a[2], np.full(N, 12 - FIRST_LE, dtype=np.int32))
    fr = a[-2]["frame"]
    assert (fr == np.round(fr)).all() and not np.array_equal(fr[0], fr[1])
    orc = CR.ComposedOracle(_base(env), CR.mixed_specs(PITCH, off=("wind", "threshold", "magnitude", "disturbance")),
                            m2c=env.M2C_CL, modal_cm=env.modal_CM)
    rec = CR.drive(orc, 12, actions=[np.zeros((N, env.nActuator, env.nActuator), dtype=np.float32)] * 12)
    assert (rec["crossings"] >= 2).all() and len({s["r0"] for s in orc.specs}) == N
    chk = _Check(F32_TOL, "compose-sh-pairs-f32" + ("-long-exposure" if exposure else ""))
    for e in range(N):
        chk.close(a[-2]["state.screen"][0][e], rec["screen"][e][0], "screen", f"screen env {e}")
        chk.close(a[-1]["total"][:, e], rec["total"][:, e], "rms_nm", f"total env {e}")
    chk.done()


# ---- f. events in mid-episode -------------------------------------------------------------------------------------------------------------
EVENT_FRAME, CHECKPOINT_FRAME = 6, 9
EVENTS = {EVENT_FRAME: [(1, 177, 0.12), (3, 377, 0.15)]}          # reset_envs([1, 3], seed=77, r0=[0.12, 0.15]): seeds 77 + 100 e


def test_partial_reset_and_checkpoint_in_mid_episode():
    """float64, the ideal camera.  reset_envs([1, 3], seed=77, r0=...) in front of frame 6: the untouched rows are bit-identical to
    a run of the same actions without the event, the reset rows match the oracle restarted at that frame (new screens at the new
    r0, a flat mirror, the env's pending actions dropped; the disturbance's clock, the env's wind, star and mirror stay).  A
    checkpoint in front of frame 9, resumed on a fresh shard after the settings get_state() does not carry were applied again,
    continues bit for bit."""
    import torch
    env = _shard("sh", "f64")
    _apply(env)
    rec = _record(env, events=EVENTS)
    label = "compose-sh-zonal-f64-events"
    with_event = _replay(env, rec, F64_SAME_OPERATOR_TOL_FULL, label, events=EVENTS, first_telemetry={1: EVENT_FRAME, 3: EVENT_FRAME})
    scr_event = env._download_screens()
    plain = _shard("sh", "f64", tag="b")
    _apply(plain)
    _start(plain)
    for i in range(STEPS):
        obs, frame, rew, sr, _, _ = plain.step(i, torch.as_tensor(rec["actions"][i]))
        for x, y in zip((obs, frame, rew, sr), with_event[i + 1]):
            assert np.array_equal(_np(x)[[0, 2]], y[[0, 2]]), ("untouched rows, frame", i)
            assert i < EVENT_FRAME or not np.array_equal(_np(x)[1], y[1])
    assert np.array_equal(plain._download_screens()[0][[0, 2]], scr_event[0][[0, 2]])
    # the checkpoint: the same episode again up to frame 9 on `plain`, then the rest on a fresh shard
    _clear(plain)
    _apply(plain)
    _start(plain)
    for i in range(CHECKPOINT_FRAME):
        if i == EVENT_FRAME:
            plain.reset_envs([1, 3], seed=77, r0=[0.12, 0.15])
        plain.step(i, torch.as_tensor(rec["actions"][i]))
    snap = plain.get_state()
    assert snap["delay"] == CASE["delay"] and np.array_equal(snap["r0_env"], [0.13, 0.12, 0.16, 0.15]) and snap["wind_pixels"] == 2
    fresh = _new_shard("sh", "f64")
    try:
        _apply(fresh, features=("star", "mirror", "disturbance"))    # configuration; r0, the clocks and the delay line come with the state
        fresh.generate_new_phase_screen(1)                          # some other state first
        fresh.set_state(snap)
        for i in range(CHECKPOINT_FRAME, STEPS):
            out = fresh.step(i, torch.as_tensor(rec["actions"][i]))
            for x, y in zip((out[0], out[1], out[2], out[3]), with_event[i + 1]):
                assert np.array_equal(_np(x), y), ("resumed, frame", i)
        assert np.array_equal(fresh._download_screens(), scr_event)
    finally:
        fresh.close()


# ---- g. clearing ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_cleared_features_leave_no_trace(dtype):
    """Six frames with everything on, then clear_disturbance / clear_dm_per_env / clear_star_per_env / set_delay(0) / clear_modal /
    clear_wavefront_basis / clear_science / set_policy(None): the next 4 frames (two steps, then run_integrator) are bit-identical
    to those of a shard that never had them and was handed the checkpoint (screens, clocks, r0, commands: loop state)."""
    import torch
    env = _shard("sh", dtype, "papyrus+readout")
    _attach(env)
    _apply(env)
    obs = _start(env)
    rec = env.record_wavefront(0, 6, ("residual", "atmosphere"))
    env.start_long_exposure()
    tr = env.rollout(0, 6, sigma=0.05, gain=GAIN, seed=3)
    torch.cuda.synchronize()
    assert np.abs(_np(env.delay_line())).max() > 0 and np.abs(_np(rec)).max() > 0
    env.stop_long_exposure()
    env.stop_wavefront_record()
    _clear(env)
    assert env.delay == 0 and env.fused_step == (dtype == "f32")
    snap = env.get_state()
    assert "delay" not in snap
    never = _new_shard("sh", dtype, "papyrus+readout")
    try:
        never.set_state(snap)
        outs = []
        for e in (env, never):
            obs = torch.as_tensor(snap["obs"]).to(e.device, e.tdtype)
            got = []
            for i in (6, 7):
                obs, frame, rew, sr, _, _ = e.step(i, GAIN * obs)
                got += [_np(obs), _np(frame), _np(rew), _np(sr)]
            got += [_np(t) for t in e.run_integrator(8, 2)]
            torch.cuda.synchronize()
            state = e.get_state()
            got += [np.asarray(state[k]) for k in ("screen", "clock_env", "mt", "coefs", "dm_prev", "signal", "counters", "obs", "r0_env")]
            outs.append(got)
        for j, (x, y) in enumerate(zip(*outs)):
            assert np.array_equal(x, y, equal_nan=True), ("quantity", j)
        assert not np.array_equal(outs[0][0][0], outs[0][0][1])
    finally:
        never.close()
