"""GPU: every env of a shard its own ROTATED mirror, as actuator factor pairs (aoenv_set_dm_pairs / BatchedAOEnv.set_dm_rotation /
set_dm_pairs_per_env; kernels k_dm_pairs_mfma and k_dm_pairs<T> of rlao_amd/csrc/dm_pairs_kernels.hip).

* exact data: small-integer tables and commands, every summation order exact -- the matrix-core kernel, the general kernel on a
  float32 shard and a float64 shard all give the NumPy integer surface bit for bit, every pixel, at every geometry (a wrong lane
  map, a missed K tail, a padding row that is read);
* real mirrors: the surface against ``dense_e @ coefs_e`` of tests/_dm_rot_ref.py (float64) and within the bound of any summation
  order (float32, both kernels);
* the closed loop against one float64 oracle per env whose ``dm_modes`` is the rotated mirror's and whose reconstructor is the
  calibrated one (tests/_dm_rot_ref.rotated_oracle): Shack-Hartmann and Pyramid, float64 and float32, ``step`` and ``step_modal``,
  at the tolerances of tests/test_gpu_parity.py;
* twins: row e of the mixed shard against row e of a shard whose every env carries mirror e, bit for bit, over stepping,
  ``run_integrator``, ``rollout``, a disturbance behind a delay, ``reset_envs``, photon noise, the wavefront record and the long
  exposure;
* rotation 0 against the separable per-env path; off is off; the round trip of the tables.

The geometries are those of tests/test_gpu_dm_env.py; the loop harness is that of tests/test_gpu_compose.py.  The largest errors
seen go to the file AO_PARITY_REPORT names (profiles/dm_pairs_parity_maxima.json is such a run)."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import _dm_rot_ref as REF
import test_gpu_compose as TC
from test_gpu_dm_env import ODD, SMALL, WIDE, _episode, _same_row, _start
from test_gpu_dm_env import _make as _make_dm_env
from test_gpu_parity import F32_TOL, F64_SAME_OPERATOR_TOL, _OBSERVED

pytestmark = pytest.mark.gpu

TINY_PYR = dict(TC.TINY_PYR)                                        # R = 24 (tests/test_gpu_dm_env.py's, psfCentering spelled out)
GAIN = TC.GAIN
N, STEPS, SEED, STRIDE = TC.N, TC.STEPS, TC.SEED, TC.CASE["seed_stride"]
# case: (geometry, set_params keywords, n_envs)
CASES = {
    "tiny_pyr": (TINY_PYR, dict(wfs_type="pyramid"), 4),           # less than one 32-tile; the Pyramid behind it
    "odd": (ODD, {}, 4),                                            # R = 30: not a multiple of 4 or 16 (dword stores), A = 32
    "small": (SMALL, {}, 4),                                        # R = 48, 9 across, A = 69: a K tail
    "wide": (WIDE, {}, 2),                                          # R = 144 > 128, 37 across, A > 1000: two LDS chunks of the command
    "two_dm": (SMALL, dict(second_dm=dict(nSubaperture=4)), 4),    # the composite mirror: through set_dm_pairs_per_env only
}
MODES = ("mfma", "general", "f64")                                  # k_dm_pairs_mfma; k_dm_pairs<float> (forced); k_dm_pairs<double>
_ENVS = {}


@pytest.fixture(scope="module", autouse=True)
def _close_all():
    yield
    for env in _ENVS.values():
        env.close()
    _ENVS.clear()


def _dump():
    path = os.environ.get("AO_PARITY_REPORT")
    if path:
        with open(path, "w") as f:
            json.dump(_OBSERVED, f, indent=1, sort_keys=True)


def _seen(label, key, value):
    rec = _OBSERVED.setdefault(label, {})
    rec[key] = max(rec.get(key, 0.0), float(value))
    _dump()


def _path(env, general):
    from rlao_amd import _lib as L
    L.check(env._shard.lib.aoenv_set_option(env._shard.h, L.OPT_FORCE_PATH, L.PATH_DM_PAIRS_GENERAL if general else 0))


def _env(case, mode, tag="a"):
    """one shard per (case, dtype, tag) for the module, handed out with no per-env mirror and a flat command"""
    from rlao_amd.env import BatchedAOEnv
    geo, kw, n = CASES[case]
    dtype = "f64" if mode == "f64" else "f32"
    key = (case, dtype, tag)
    if key not in _ENVS:
        env = BatchedAOEnv(n_envs=n, device=0, dtype=dtype, env_seed_stride=STRIDE)
        env.set_params(dict(geo), **dict(dict(camera="ideal", wfs_type="shackhartmann", gainCL=GAIN), **kw))
        _ENVS[key] = env
    env = _ENVS[key]
    env.clear_dm_per_env()
    _path(env, mode == "general")
    env.dm.coefs = 0
    return env


def _parts(env):
    dmt = env._dm_tables
    return [dmt.dm1, dmt.dm2] if hasattr(dmt, "dm2") else [dmt]


def _mirror_rows(env):
    return list(range(4))[-env.n_envs:]                             # a 2-env shard (WIDE) carries mirrors 2 and 3


def _pairs(env, rows=None):
    """(PY, PX) float64 [n_envs, R, A]: row r carries mirror rows[r] of tests/_dm_rot_ref.mirrors (a two-DM env: both mirrors
    moved alike, the composite's columns side by side); mirror 3 has one actuator dead."""
    from rlao_amd import calib
    p = env.param
    rows = _mirror_rows(env) if rows is None else rows
    sets = REF.mirrors(p.diameter / p.nSubaperture)
    out = []
    for e in rows:
        per = [calib.dm_actuator_pairs(p, n_subap=d.nAct - 1, **sets[e]) for d in _parts(env)]
        py, px = np.hstack([q[0] for q in per]), np.hstack([q[1] for q in per])
        if e == 3:
            k = REF.dead_actuator(py.shape[1])
            py[:, k] = 0.0
            px[:, k] = 0.0
        out.append((py, px))
    return np.stack([q[0] for q in out]), np.stack([q[1] for q in out])


def _dense(env, e):
    """dm.modes [R^2, A] of mirror e from the restatement of the reference alone"""
    p = env.param
    sets = REF.mirrors(p.diameter / p.nSubaperture)
    m = np.hstack([REF.dense_modes(p.resolution, p.diameter, d.nAct - 1, p.mechanicalCoupling, d.act_idx, **sets[e]) for d in _parts(env)])
    if e == 3:
        m[:, REF.dead_actuator(m.shape[1])] = 0.0
    return m


# ---- exact data ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", list(CASES))
def test_integer_tables_give_the_integer_surface_bit_for_bit(case, mode):
    """py, px integers in [-3, 3], the command integers in [-4, 4]: every term and every partial sum is an integer below
    36 A < 2^24, exact in float32 in any order.  dm.surface() == the NumPy integer result at every pixel of every env; the tables
    are random, hence asymmetric: a transposed or permuted product cannot pass."""
    env = _env(case, mode)
    n, R, A = env.n_envs, env.R, env.nValidAct
    assert 36 * A < 2 ** 24
    rs = np.random.RandomState(7)
    PY, PX = rs.randint(-3, 4, (n, R, A)).astype(np.float64), rs.randint(-3, 4, (n, R, A)).astype(np.float64)
    c = rs.randint(-4, 5, (n, A)).astype(np.float64)
    env.set_dm_pairs_per_env(PY, PX)
    assert not env.fused_step
    env.dm.coefs = c
    got = env.dm.surface()
    want = np.einsum("eyk,exk->eyx", PY * c[:, None, :], PX)
    assert got.shape == want.shape == (n, R, R) and np.abs(want).max() > 36
    bad = np.argwhere(got != want)
    assert bad.size == 0, (case, mode, len(bad), bad[:5], got[tuple(bad[0])], want[tuple(bad[0])])
    # a second command on the same tables, through the other way a command arrives (the upload of AOENV_B_COEFS)
    from rlao_amd import _lib as L
    c2 = rs.randint(-4, 5, (n, A)).astype(np.float64)
    env._shard.upload_state(L.B_COEFS, c2.astype(np.float32 if env.dtype == "f32" else np.float64), env._stream(),
                            dtype=np.float32 if env.dtype == "f32" else np.float64)
    assert np.array_equal(env.dm.surface(), np.einsum("eyk,exk->eyx", PY * c2[:, None, :], PX))
    env.clear_dm_per_env()


# ---- real mirrors: the surface ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", list(CASES))
def test_surface_of_the_real_mirrors(case, mode):
    """float64: dm.surface() against dense_e @ coefs_e of the restatement, within F64_SAME_OPERATOR_TOL["opd_m"].  float32, both
    kernels: against the float64 sum of the values AS HELD (tables and command rounded to float32), per pixel within
    (A + 2) 2^-24 sum_k |c_k py px| -- one rounding of c py, and A roundings of the running sum, each of a partial sum that the
    sum of the magnitudes bounds: the bound of ANY summation order, derived, not measured.  The maxima are recorded."""
    env = _env(case, mode)
    n, R, A = env.n_envs, env.R, env.nValidAct
    rows = _mirror_rows(env)
    PY, PX = _pairs(env)
    if case == "two_dm":
        env.set_dm_pairs_per_env(PY, PX)
    else:
        sets = REF.mirrors(env.param.diameter / env.param.nSubaperture)
        env.set_dm_rotation(**{k: np.array([sets[e].get(k, 0.0) for e in rows]) for k in ("rotation_angle", "shift_x", "shift_y", "radial_scaling", "tangential_scaling")})
        assert np.array_equal(env.dm_rotation["rotation_angle"], [sets[e].get("rotation_angle", 0.0) for e in rows])
        env.set_dm_pairs_per_env(PY[-1:], PX[-1:], env_ids=[n - 1])   # mirror 3's dead actuator
    coefs = np.random.RandomState(3).normal(0, 2e-7, (n, A))
    env.dm.coefs = coefs
    got = env.dm.surface()
    label = f"dm-pairs-surface-{case}-{mode}"
    for r, e in enumerate(rows):
        if mode == "f64":
            want = (_dense(env, e) @ coefs[r]).reshape(R, R)
            err = float(np.abs(got[r] - want).max())
            _seen(label, "opd_m", err)
            assert err <= F64_SAME_OPERATOR_TOL["opd_m"], (case, e, err)
        else:
            hy, hx = (t[r].astype(np.float32).astype(np.float64) for t in (PY, PX))
            c = coefs[r].astype(np.float32).astype(np.float64)
            want = np.einsum("yk,xk->yx", hy * c[None, :], hx)
            bound = (A + 2) * 2.0 ** -24 * np.einsum("yk,xk->yx", np.abs(hy * c[None, :]), np.abs(hx))
            err = np.abs(got[r] - want)
            _seen(label, "opd_m", err.max())
            _seen(label, "fraction_of_the_bound", (err / bound).max())
            assert (err <= bound).all(), (case, mode, e, float((err / bound).max()))
            # ... which is the right mirror: far closer to its dense surface than the mirrors are to one another
            assert np.abs(got[r] - (_dense(env, e) @ coefs[r]).reshape(R, R)).max() < 1e-3 * np.abs(want).max()
    assert all(np.abs(got[r] - got[0]).max() > 1e-2 * np.abs(got[0]).max() for r in range(1, n))
    print(label, json.dumps(_OBSERVED[label], sort_keys=True))
    env.clear_dm_per_env()


# ---- round trip ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,mode", [("small", "mfma"), ("small", "f64"), ("wide", "mfma"), ("odd", "f64")])
def test_get_returns_the_pairs_rounded_to_the_env_dtype(case, mode):
    env = _env(case, mode)
    assert env.dm.pairs_per_env() is None
    PY, PX = _pairs(env)
    env.set_dm_pairs_per_env(PY, PX)
    py, px = env.dm.pairs_per_env()
    dt = np.float32 if env.dtype == "f32" else np.float64
    assert py.dtype == px.dtype == np.float64 and py.shape == PY.shape
    assert np.array_equal(py, PY.astype(dt).astype(np.float64)) and np.array_equal(px, PX.astype(dt).astype(np.float64))
    env.clear_dm_per_env()
    assert env.dm.pairs_per_env() is None


# ---- the closed loop against the oracle -----------------------------------------------------------------------------------------------------
_BASES, _RECORDS = {}, {}
# the stream of the oracle's action noise (zonal) and the gain of its modal run, chosen on the CPU from the oracle alone for the
# distance of every pixel of every frame from the centroid cut (RandomState(13): 2.1e-7 of the brightest pixel, gain 0.35 at K = 20:
# 2.1e-7; the streams 9 .. 11 and the gains 0.3, 0.4 and 0.5 come within 2e-8 .. 8e-8 of a cut, under MIN_CUT_GAP)
ACTION_SEED, MODAL_GAIN = 13, 0.35
ORACLE_RUNS = [("sh", "f64", None), ("sh", "f64", 20), ("pyr", "f64", None), ("sh", "mfma", None), ("sh", "general", None), ("sh", "mfma", 20),
               ("pyr", "mfma", None), ("pyr", "general", None)]
KIND_CASE = {"sh": "small", "pyr": "tiny_pyr"}


def _oracle_record(env, kind, K):
    """One oracle per env with the rotated mirror's dm_modes and the calibrated reconstructor, driven by its own observations; the
    float32 actions it issued are what the shard is replayed with.  Conditions from the oracle alone: every measurement clear of
    the centroid cut, every env's layer crossing a pixel."""
    if kind not in _BASES:
        from test_gpu_geometry_sweep import build_base as build_sh
        from test_gpu_pyramid_sweep import build_base as build_pyr
        at = env._atm_tables
        _BASES[kind] = (build_sh if kind == "sh" else build_pyr)(dict(TC.GEO[kind], nLoop=16), env.M2C_CL, at.A, at.B)
    base = _BASES[kind]
    assert np.array_equal(env.dm_mask.astype(bool), base.dm_mask) and env.nSignal == base.wfs.nSignal
    key = (kind, K)
    if key not in _RECORDS:
        cm_K = None if K is None else np.asarray(env._modal["cm"], dtype=np.float64)
        orc = REF.rotated_oracle(base, range(N), SEED, STRIDE, n_subap=env.param.nSubaperture, mech_coupling=env.param.mechanicalCoupling,
                                 m2c=env.M2C_CL, modal_cm=env.modal_CM, modal=K, modal_cm_K=cm_K)
        for e in range(N):
            assert np.array_equal(orc.envs[e].dm_modes, _dense(env, e))
        rec = TC.CR.drive(orc, STEPS, modal_gain=None if K is None else MODAL_GAIN, rs_seed=ACTION_SEED)
        rec["modal_cm"] = np.asarray(env.modal_CM, dtype=np.float64).copy()
        _RECORDS[key] = rec
    rec = _RECORDS[key]
    np.testing.assert_allclose(env.modal_CM, rec["modal_cm"], rtol=0, atol=1e-12 * float(np.abs(rec["modal_cm"]).max()))
    assert rec["min_gap"] >= TC.MIN_CUT_GAP, rec["gap"]
    assert (rec["crossings"] >= 1).all(), rec["crossings"]
    # the mirrors matter to the loop: the envs' residuals differ by far more than any tolerance below
    assert all(np.abs(rec["opd_res"][e] - rec["opd_res"][0]).max() > 100 * F32_TOL["opd_m"] for e in range(1, N))
    return rec


@pytest.mark.parametrize("kind,mode,K", ORACLE_RUNS, ids=TC._ids(ORACLE_RUNS))
def test_closed_loop_matches_the_oracle_with_the_rotated_mirrors(kind, mode, K):
    """The oracle's actions replayed through step (K None) or step_modal: signal, obs, reward, Strehl, frame of every step, then
    the screens, atm.OPD, the residual OPD and the telemetry -- F64_SAME_OPERATOR_TOL (float64) / F32_TOL (float32) of
    tests/test_gpu_parity.py, unchanged."""
    env = _env(KIND_CASE[kind], mode)
    env._kind, env._case_rows, env._case_wind = kind, list(range(N)), False
    from rlao_amd import _lib as L
    if not hasattr(env, "_counters0"):
        env._counters0 = env._shard.download(L.B_COUNTERS, (4,), env._stream(), dtype=np.uint32).copy()
    try:
        if K is not None:
            env.set_modal(K)
            env.set_modal_gain(GAIN)
        sets = REF.mirrors(env.param.diameter / env.param.nSubaperture)
        env.set_dm_rotation(**{k: np.array([s.get(k, 0.0) for s in sets]) for k in ("rotation_angle", "shift_x", "shift_y", "radial_scaling", "tangential_scaling")})
        PY, PX = _pairs(env)
        env.set_dm_pairs_per_env(PY[3:], PX[3:], env_ids=[3])
        assert not env.fused_step
        rec = _oracle_record(env, kind, K)
        tol = F64_SAME_OPERATOR_TOL if mode == "f64" else F32_TOL
        TC._replay(env, rec, tol, f"dm-pairs-{kind}-{'zonal' if K is None else f'K{K}'}-{mode}", K=K)
    finally:
        if K is not None:
            env.clear_modal()
        env.clear_dm_per_env()


def test_unrotated_float32_shard_on_the_plain_phase_kernel_for_comparison():
    """The yardstick beside the float32 figures above: the same quantities for the UNROTATED shard with OPT_MFMA_GEMM = 0
    (k_phase<float>, the separable mirror formed inside the phase kernel) against its oracle -- recorded under
    "dm-pairs-sh-zonal-unrotated-no_mfma", held to F32_TOL like every float32 shard."""
    from rlao_amd import _lib as L
    env = _env("small", "mfma", tag="plain")
    env._kind, env._case_rows, env._case_wind = "sh", list(range(N)), False
    if not hasattr(env, "_counters0"):
        env._counters0 = env._shard.download(L.B_COUNTERS, (4,), env._stream(), dtype=np.uint32).copy()
    L.check(env._shard.lib.aoenv_set_option(env._shard.h, L.OPT_MFMA_GEMM, 0))
    try:
        assert not env.fused_step
        _oracle_record(env, "sh", None)                             # (builds the base)
        orc = TC.CR.ComposedOracle(_BASES["sh"], [TC.CR.env_spec(seed=SEED + STRIDE * r) for r in range(N)], m2c=env.M2C_CL, modal_cm=env.modal_CM)
        rec = TC.CR.drive(orc, STEPS, rs_seed=ACTION_SEED)
        assert rec["min_gap"] >= TC.MIN_CUT_GAP
        TC._replay(env, rec, F32_TOL, "dm-pairs-sh-zonal-unrotated-no_mfma")
    finally:
        L.check(env._shard.lib.aoenv_set_option(env._shard.h, L.OPT_MFMA_GEMM, 1))


# ---- twins -----------------------------------------------------------------------------------------------------------------------------
TWIN_LOOPS = ("run_integrator", "rollout")
_TWINS = {}


def _twin_shard(dtype, camera, tag):
    key = (dtype, camera, tag)
    if key not in _TWINS:
        env = TC._new_shard("sh", dtype, camera)
        TC._attach(env)                                             # the wavefront basis and the science camera (and a modal surface, a policy)
        amp = (2e-7 * (1 + np.arange(N))).reshape(N, 1, 1)          # a disturbance per ROW (the twins' rows carry the same) behind a delay
        env.set_disturbance(1, amp, np.full((N, 1, 1), 1.0 / (17.0 * env.param.samplingTime)), t0=0)
        env.set_delay(1)
        env._case_rows, env._case_wind = list(range(N)), False
        _TWINS[key] = _ENVS[("twin",) + key] = env
    return _TWINS[key]


def _same_rows(got, want, loop, e, what):
    """TC._same_runs for ONE row of a shard on the shared clock: what get_state() holds per shard (the clock, the counters) is
    compared whole, everything with an env axis by its row e"""
    skip = {"state.explore_seed", "state.wind_env", "state.windSpeed", "state.windDirection", "state.wind_pixels", "state.delay"}
    per_env_axis = {"delay_line": 1, "state.delay_line": 1, "state.screen": 1, "state.mt": 1, "state.clock_env": 1}
    for c, (a, b) in enumerate(zip(got["ends"], want["ends"])):
        assert a.keys() == b.keys()
        for k in a:
            if k in skip or a[k] is None:
                continue
            x, y = np.asarray(a[k]), np.asarray(b[k])
            ax = per_env_axis.get(k, 0)
            if k == "state.counters":                               # word 1 counts the exploration stream's draws: a rollout's own
                x, y = x[[0, 2, 3]], y[[0, 2, 3]]
            elif x.ndim > ax and x.shape[ax] == N:
                x, y = np.take(x, [e], axis=ax), np.take(y, [e], axis=ax)
            assert x.dtype == y.dtype and np.array_equal(x, y, equal_nan=True), (what, loop, "call", c, k)
    assert len(got["frames"]) == len(want["frames"])
    for i, (a, b) in enumerate(zip(got["frames"], want["frames"])):
        for q, (x, y) in enumerate(zip(a, b)):
            assert np.array_equal(x[e], y[e], equal_nan=True), (what, loop, "frame", i, "quantity", q)
    assert np.array_equal(got["record"][:, :, e], want["record"][:, :, e], equal_nan=True), (what, loop, "wavefront record")
    for j, (x, y) in enumerate(zip(got["le"], want["le"])):
        assert (x is None) == (y is None) and (x is None or np.array_equal(x[e], y[e], equal_nan=True)), (what, loop, "long exposure", j)


def _reset_run(env):
    """reset_envs([1, 3]) in mid-episode: 5 frames, the partial reset, 6 more.  (A partial reset puts a shard on per-env clocks for
    good: a throwaway one in front makes every run of this sequence start there, the first like the later ones.)"""
    import torch
    env.reset_envs([0], seed=np.array([1]))
    TC._start(env)
    a = env.run_integrator(0, 5)
    obs = env.reset_envs([1, 3], seed=np.array([900, 901]))
    b = env.run_integrator(5, 6)
    torch.cuda.synchronize()
    return [TC._np(t) for t in (*a, *b)], TC._np(obs), TC._end_of_call(env, b)


@pytest.mark.parametrize("dtype,camera", [("f32", "papyrus+readout"), ("f64", "ideal"), ("f32", "ideal")], ids=["f32-photon", "f64-ideal", "f32-ideal"])
def test_each_env_of_the_mixed_shard_equals_its_uniform_twin(dtype, camera):
    """Row e of the mixed shard == row e of a shard whose every env carries mirror e (the same seeds, row by row): the frames of
    step (stepping), run_integrator and rollout in calls of 1, 5 and 10 with the wavefront record and the long exposure attached, a
    per-env disturbance behind a delay of one frame, reset_envs([1, 3]) in mid-episode -- observations, actions, rewards, Strehl,
    the phase and frame buffers, the delay line, the record, the exposure and get_state(), bit for bit."""
    env, twin = _twin_shard(dtype, camera, "a"), _twin_shard(dtype, camera, "b")
    PY, PX = _pairs(env)
    env.set_dm_pairs_per_env(PY, PX)
    try:
        assert not env.fused_step and env.delay == 1
        got = {loop: TC._run_loop(env, loop) for loop in TWIN_LOOPS}
        got["step"] = TC._run_loop(env, "run_integrator", stepping=True)
        got_reset = _reset_run(env)
        for e in range(N):
            twin.set_dm_pairs_per_env(np.tile(PY[e], (N, 1, 1)), np.tile(PX[e], (N, 1, 1)))
            for loop in TWIN_LOOPS:
                _same_rows(got[loop], TC._run_loop(twin, loop), loop, e, f"env {e} against its twin")
            _same_rows(got["step"], TC._run_loop(twin, "run_integrator", stepping=True), "run_integrator", e, f"env {e}, stepping")
        for e in range(N):                                          # (behind every loop on the shared clock: see _reset_run)
            twin.set_dm_pairs_per_env(np.tile(PY[e], (N, 1, 1)), np.tile(PX[e], (N, 1, 1)))
            want_reset = _reset_run(twin)
            for q, (x, y) in enumerate(zip(got_reset[0], want_reset[0])):
                assert np.array_equal(x[e], y[e]), ("reset_envs", e, q)
            if e in (1, 3):
                assert np.array_equal(got_reset[1][[1, 3].index(e)], want_reset[1][[1, 3].index(e)])
            for k in ("phase", "frame", "out[0]"):
                assert np.array_equal(got_reset[2][k][e], want_reset[2][k][e]), ("reset_envs", e, k)
        # stepping and the device loop agree with each other on the mixed shard too
        TC._same_runs(got["run_integrator"], got["step"], "run_integrator", what="loop against stepping")
        last = got["run_integrator"]["ends"][-1]["phase"]
        assert all(not np.array_equal(last[0], last[e]) for e in range(1, N))
        assert np.isfinite(got["rollout"]["record"]).all() and got["rollout"]["le"][0].max() > 0
    finally:
        env.clear_dm_per_env()
        twin.clear_dm_per_env()


# ---- rotation 0 against the separable per-env path -----------------------------------------------------------------------------------------
def test_rotation_zero_equals_the_separable_per_env_mirrors_float64():
    """A pairs shard with rotation 0 and env e's shifts and scalings against set_dm_misregistration with the same values
    (k_phase<double> forming gy C gx^T itself): the same operator, another summation order -- F64_SAME_OPERATOR_TOL, over a
    closed-loop episode driven by the same actions."""
    import torch
    from rlao_amd import _lib as L
    env = _env("small", "f64")
    L.check(env._shard.lib.aoenv_set_option(env._shard.h, L.OPT_FUSED_STEP, 0))
    pitch = env.param.diameter / env.param.nSubaperture
    m = dict(shift_x=np.array([0.0, 0.3, 0.0, 0.3]) * pitch, shift_y=np.array([0.0, 0.0, -0.5, -0.5]) * pitch,
             radial_scaling=np.array([0.0, 0.0, 0.02, 0.0]), tangential_scaling=np.array([0.0, 0.0, 0.0, -0.03]))
    tol = F64_SAME_OPERATOR_TOL

    def start(e):
        e.generate_new_phase_screen(SEED)
        e.dm.coefs = 0
        e.dm_prev = 0
        e.measure()
        return e.reset_soft()

    def run(actions):
        obs = start(env)
        out, acts = [], []
        for i in range(STEPS):
            a = (GAIN * obs) if actions is None else actions[i]
            acts.append(a)
            obs, frame, rew, sr, _, _ = env.step(i, a)
            sig = env._shard.download(L.B_SIGNAL, (N, env.nSignal), env._stream())
            ph = env._shard.download(L.B_PHASE, (N, env.R, env.R), env._stream())
            out.append(dict(obs=obs.cpu().numpy(), frame=frame.cpu().numpy(), reward=rew.cpu().numpy(), strehl=sr.cpu().numpy(), signal=sig,
                            opd=ph * env.src_wavelength / (2 * np.pi)))
        torch.cuda.synchronize()
        return out, acts

    env.set_dm_misregistration(**m)
    want, acts = run(None)
    env.clear_dm_per_env()
    env.set_dm_rotation(0.0, **m)
    got, _ = run(acts)
    env.clear_dm_per_env()
    label = "dm-pairs-rotation0-f64"
    for g, w in zip(got, want):
        for key, q, scale in (("obs", "obs", 1.0), ("signal", "signal", 1.0), ("strehl", "strehl", 1.0), ("opd_m", "opd", 1.0),
                              ("frame_rel", "frame", float(w["frame"].max()))):
            err = float(np.abs(g[q] - w[q]).max()) / scale
            _seen(label, key, err)
            assert err <= tol[key], (key, err)
        rel = float(np.abs(g["reward"] - w["reward"]).max() / np.abs(w["reward"]).max())
        _seen(label, "reward_rel", rel)
        assert rel <= tol["reward_rel"] + tol["obs"]
    assert not np.array_equal(want[-1]["obs"][0], want[-1]["obs"][3])
    print(label, json.dumps(_OBSERVED[label], sort_keys=True))


# ---- off is off ----------------------------------------------------------------------------------------------------------------------------
def test_off_is_off_and_refused_calls_change_nothing():
    """A shard that set and cleared pairs (twice: the block is allocated, freed and allocated again), and a loop around every
    refused call, run bit-identical to an untouched shard -- the fused step included; env.fused_step is False while pairs are on
    and True after the clear.  The pairs set a second time run like a shard that set them once."""
    steps, seed = 8, 5
    ref = _make_dm_env("fused")
    want, _ = _episode(ref, steps, seed)
    PY, PX = _pairs(ref)
    ref.set_dm_pairs_per_env(PY, PX)
    once, _ = _episode(ref, steps, seed)
    ref.close()
    env = _make_dm_env("fused")
    n = env.n_envs
    lib, h, st = env._shard.lib, env._shard.h, C.c_void_p(env._stream())
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    z = np.zeros_like(PY)
    surf = np.zeros((n, env.R * env.R))
    assert env.fused_step and env.dm_rotation is None and env.dm.pairs_per_env() is None
    assert lib.aoenv_get_dm_pairs(h, p(z), p(z), st) != 0 and b"no actuator factor pairs" in lib.aoenv_last_error()
    assert lib.aoenv_get_dm_surface(h, p(surf), st) != 0 and b"no surface buffer" in lib.aoenv_last_error()
    env.set_dm_rotation([0.0, 1.5, -3.0, 2.0])
    assert not env.fused_step and env.dm.pairs_per_env() is not None
    moved, _ = _episode(env, 2, seed)
    env.clear_dm_per_env()
    assert env.fused_step and env.dm.pairs_per_env() is None
    again, _ = _episode(env, steps, seed)
    env.set_dm_pairs_per_env(PY, PX)                                # set -> use -> clear -> set: like set once
    second, _ = _episode(env, steps, seed)
    # refused calls while pairs are in force: nothing changes
    bad = PY.copy()
    bad[1, 3, 2] = np.nan
    GX = np.tile(env._dm_tables.gx, (n, 1, 1))
    assert lib.aoenv_set_dm_pairs(h, p(PY), None, st) != 0 and b"null" in lib.aoenv_last_error()
    assert lib.aoenv_set_dm_pairs(h, None, p(PX), st) != 0
    assert lib.aoenv_set_dm_pairs(h, p(bad), p(PX), st) != 0 and b"py[%d] is not finite" % ((1 * env.R + 3) * env.nValidAct + 2) in lib.aoenv_last_error()
    assert lib.aoenv_set_dm_pairs(h, p(PY), p(bad), st) != 0 and b"px[" in lib.aoenv_last_error()
    assert lib.aoenv_set_dm_env(h, p(GX), p(GX), st) != 0 and b"pairs are in force" in lib.aoenv_last_error()
    with pytest.raises(ValueError, match=r"clear_dm_per_env\(\)"):
        env.set_dm_misregistration(shift_x=0.01)
    third, _ = _episode(env, steps, seed)
    env.clear_dm_per_env()
    # ... and the reverse, in the middle of a running loop of the untouched shard
    obs = _start(env, seed)
    part1, obs = _episode(env, 4, seed, obs=obs)
    assert lib.aoenv_set_dm_pairs(h, p(PY), None, st) != 0
    assert lib.aoenv_set_dm_pairs(h, p(bad), p(PX), st) != 0
    part2, _ = _episode(env, 4, seed, obs=obs, i0=4)
    env.set_dm_misregistration(shift_x=0.01)
    assert lib.aoenv_set_dm_pairs(h, p(PY), p(PX), st) != 0 and b"aoenv_set_dm_env" in lib.aoenv_last_error()
    with pytest.raises(ValueError, match=r"clear_dm_per_env\(\)"):
        env.set_dm_rotation(1.0)
    env.clear_dm_per_env()
    final, _ = _episode(env, steps, seed)
    assert env.fused_step
    env.close()
    for e in range(n):
        _same_row(again, want, e, what="after clear")
        _same_row(part1[:-1] + part2[1:], want, e, what="refused calls")
        _same_row(final, want, e, what="after the refused reverse")
        _same_row(second, once, e, what="set, cleared, set again")
        _same_row(third, once, e, what="refused calls while pairs are on")
    assert not np.array_equal(moved[2][0][1], want[2][0][1]) and not np.array_equal(once[-2][0][1], want[-2][0][1])


def test_dense_dm_shard_refuses_pairs_and_hands_out_its_surface():
    """aoenv_set_dm_pairs on a shard with dm_separable == 0: refused; aoenv_get_dm_surface there returns modes @ coefs, the GEMM of
    before (F64_SAME_OPERATOR_TOL["opd_m"])."""
    from rlao_amd import _lib as L
    from rlao_amd.env import BatchedAOEnv
    env = BatchedAOEnv(n_envs=2, device=0, dtype="f64")
    env.set_params(TINY_PYR, camera="ideal", wfs_type="shackhartmann")
    env._dm_separable = 0
    sh = env._make_shard(2, "f64", n_layer=0, max_group=1)
    try:
        sh.upload(L.C_SH_REF, np.zeros(env.nSignal))
        sh.upload(L.C_WFS_UNITS, np.array([1.0]))
        coefs = np.random.RandomState(0).normal(0, 1e-7, (2, env.nValidAct))
        sh.set_coefs(coefs)
        sh.measure()
        before = sh.download(L.B_PHASE, (2, env.R, env.R))
        g = np.ones((2, env.R, env.nValidAct))
        with pytest.raises(L.AoEnvError, match="dense"):
            sh.set_dm_pairs(g, g)
        sh.set_dm_pairs(None, None)                                # (nothing to clear: accepted)
        surf = sh.get_dm_surface()
        assert np.abs(surf - coefs @ env._dm_tables.dense_modes().T).max() <= F64_SAME_OPERATOR_TOL["opd_m"] and np.abs(surf).max() > 0
        sh.measure()
        assert np.array_equal(sh.download(L.B_PHASE, (2, env.R, env.R)), before)
    finally:
        sh.close()
        env.close()
