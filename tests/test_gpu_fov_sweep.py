"""GPU: layers on grids of their own.  Under a telescope with a field of view (the reference env's: fov = 1 arcsec, always) a layer at
altitude h has N = ceil(R / D (D + 2 tan(fov / 2) h)) + 4 pixels across, its own ring operators [A | B], index tables, screen
generator and footprint offset foot = N // 2 - R // 2 + 1 (calib.AtmosphereTables -> Layer::N/S, PhaseArgs::S_l/foot_l,
aoenv_upload_layer).  The cases of tests/_fov_cases.py put unequal grids behind every phase kernel: k_phase_mfma (R % 4 == 2: `two`),
k_phase_mfma4 (`three`, `top_first`: the larger grid first), the generic spots / centroid / tail kernels (`p5_shared`, two layers of
one grid size that own their device tables), the Pyramid (`pyr`); and ONE elevated grid -- a uniform shard with S != R + 6 and
foot > 1 -- behind the fused step kernel and k_phase_mfma4<BAND> (`up70`, `up71x2`).  Every case asserts its grids, offsets and
ring sizes (a change of the grid rule must not move it off its branch) and aoenv_fused_step_active.

Every comparison is against oracle.ao_oracle.OracleEnv (float64 NumPy) built with fov_arcsec and handed the env's OWN operators, one
(geometry, A, B) per layer: what is left is the device arithmetic.  One oracle run per case is recorded, as in
tests/test_gpu_geometry_sweep.py (three envs with seeds seed + 100 k, six closed-loop steps, gain 0.5 plus a bounded perturbation,
float32 actions from the oracle's own observations), and the float64 shard, the float32 shard and every float32 switch (MFMA_GEMM=0,
COEFS_IMAGE=1, DEFER_RING=0, RING_LOOKAHEAD=0, FAST_WFS=0; the up* cases also FUSED_STEP=0) replay it: the observation and EVERY
layer's whole screen after the reset, every step's signal, observation, reward, Strehl and frame, the final screens, atm.OPD, residual
OPD and the total / residual telemetry under F64_SAME_OPERATOR_TOL_FULL / F32_TOL, the calibration under CAL_TOL -- the tolerances
of tests/test_gpu_parity.py, unchanged; no env, step, layer or element is left out.  Winds of 0.40 .. 0.48 pixel per frame along
72 / 200 / 320 / 144 deg (both signs of both axes); from the oracle's clocks every layer of every env crosses a pixel in the six
steps (asserted).  The maxima measured on MI355X are in profiles/fov_sweep_parity_maxima.json (AO_PARITY_REPORT=<file> with this
module alone rewrites it).  The reference tree is never read here.

Centroid cut: as in the geometry sweep, the seed of every case was chosen on the CPU from the oracle alone, among 1 .. 8, for the
largest distance of any pixel from the 1 % cut over the three envs and all compared frames (two 5: 1.3e-6, three 6: 9.5e-7,
top_first 3: 3.8e-7, p5_shared 6: 2.4e-6, up70 5: 1.5e-6, up71x2 3: 6.5e-7), and every recorded run asserts MIN_CUT_GAP = 1e-7.

Behaviour on these shards (`three` unless said): a second episode and host-made screens per layer against ft_sh_phase_screen;
checkpoint / restore after a crossing (float32, float64, `up70`: the fused kernel); env e of the shard == a one-env shard of its seed;
run_integrator == stepping; per-env r0 (`two`); per-env winds, partial resets and a single operator pair are refused and leave the
shard as it was -- all bit for bit.

That the sweep bites was checked once with the kernels weakened in a scratch build, one change at a time (each variant reads
differently, always in bounds), the whole module run against each:
  foot_l[l] read as foot_l[0] in k_phase / k_phase_mfma / k_phase_mfma4    -> every float64, float32 and switch run of two, three,
                                                                             top_first and p5_shared, both Pyramid runs and the
                                                                             batch-position test fail; the up* cases pass, and so
                                                                             does the tiny_3layer_fov1 golden (its offsets are all 3)
  the torus wrapped at S_l[0] in front of the layer's own S_l[l]           -> the same runs fail, and the two `three` checkpoints
  the fused step kernel's k.pa.foot forced to 1                            -> the default float32 shards of up70 and up71x2 and their
                                                                             COEFS_IMAGE / DEFER_RING / RING_LOOKAHEAD runs fail (the
                                                                             other switches leave the fused kernel)
Unperturbed, every float32 maximum lies below 23 % of its tolerance (the screens, `three` with MFMA_GEMM=0: 1.2e-4 rad; every
other quantity below 4 %), every float64 one below 18 % (Strehl 3.5e-16, screens 2.7e-13 rad), the calibration below 1 %.
"""
import copy

import numpy as np
import pytest

import _fov_cases as F
import test_gpu_geometry_sweep as G
import test_gpu_pyramid_sweep as P
from test_gpu_geometry_sweep import MIN_CUT_GAP, N_ENVS, SEED_STRIDE, STEPS, _replay, _same_controller
from test_gpu_parity import CAL_TOL, F32_TOL, F64_SAME_OPERATOR_TOL_FULL, _OBSERVED, _close

pytestmark = pytest.mark.gpu

CASES = F.CASES
UNIFORM = [n for n, c in CASES.items() if c["uniform"]]


def _make_env(name, dtype, n_envs=N_ENVS, stride=SEED_STRIDE, opts=None, atm_AB=None, **geo_kw):
    from rlao_amd import _lib as L
    from rlao_amd.env import BatchedAOEnv
    env = BatchedAOEnv(n_envs=n_envs, device=0, dtype=dtype, env_seed_stride=stride)
    try:
        env.set_params(F.geo(name, **geo_kw), camera="ideal", wfs_type="shackhartmann", atm_AB=atm_AB)
        for k, v in (opts or {}).items():
            L.check(env._shard.lib.aoenv_set_option(env._shard.h, getattr(L, k), v))
    except Exception:
        env.close()
        raise
    return env


def _operators(env):
    return [(t.A, t.B) for t in env._atm_tables.layers]


# ---- the oracle side: built once per case, run once per case --------------------------------------------------------------------
_BASES = {}
_RECORDS = {}


def _base(name, env):
    if name not in _BASES:
        _BASES[name] = F.build_oracle(F.geo(name), env.M2C_CL, _operators(env))
    return _BASES[name]


def _record(name, env):
    if name not in _RECORDS:
        rec = G.run_oracle(_base(name, env), env.M2C_CL, env.modal_CM, CASES[name]["seed"])
        _OBSERVED.setdefault(name + "-oracle", {})["threshold_gap_min"] = rec["min_gap"]
        _RECORDS[name] = rec
    rec = _RECORDS[name]
    _same_controller(env, rec)
    # from the oracle alone: every measurement clear of the centroid cut, every layer of every env crossed a pixel
    assert rec["min_gap"] >= MIN_CUT_GAP, (name, rec["gap"])
    assert len(rec["gap"]) == N_ENVS * (STEPS + 1)
    assert rec["crossings"].shape == (N_ENVS, len(CASES[name]["grids"])) and (rec["crossings"] >= 1).all(), rec["crossings"]
    return rec


def _assert_grids(name, env, base=None):
    """The table of cases, from the env's host tables, from what the library was configured with and from the oracle."""
    c, at = CASES[name], env._atm_tables
    R = c["n_sub"] * c["ppx"]
    assert env.R == R and env.param.nLayer == len(c["grids"])
    assert at.layer_res == c["grids"] and at.uniform == c["uniform"]
    assert [t.S for t in at.layers] == [n + 2 for n in c["grids"]]
    assert [n // 2 - R // 2 + 1 for n in at.layer_res] == c["foot"] == [t.foot + 1 for t in at.layers]
    assert [t.n_inner + t.n_outer for t in at.layers] == c["K"]
    cfg = env._shard.cfg
    assert cfg.layer_res == c["grids"][0] and cfg.n_inner + cfg.n_outer == c["K"][0]
    assert list(cfg.layer_res_l)[:len(c["grids"])] == ([0] * len(c["grids"]) if c["uniform"] else c["grids"])
    scr = env._download_screens()
    assert [scr[l].shape for l in range(len(c["grids"]))] == [(env.n_envs, n + 2, n + 2) for n in c["grids"]]
    if base is not None:
        assert [lay.g.resolution for lay in base.atm.layers] == c["grids"]
        assert [lay.g.foot[0].start + 1 for lay in base.atm.layers] == c["foot"]
        assert [lay.A.shape[1] + lay.B.shape[1] for lay in base.atm.layers] == c["K"]
        assert np.array_equal(env._sh_tables.valid_2d, base.wfs.valid_2d) and np.array_equal(env.dm_mask.astype(bool), base.dm_mask)


def _fused_active(env):
    return int(env._shard.lib.aoenv_fused_step_active(env._shard.h))


# ---- the sweep --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_path_and_calibration_match_oracle(name):
    """The float32 shard of every case has the grids of the table and sits on the path it is here for: the fused step kernel for one
    elevated grid, the batched kernels for unequal ones.  The calibration (float64 on the GPU) gives the oracle's."""
    c = CASES[name]
    env = _make_env(name, "f32")
    try:
        base = _base(name, env)
        _assert_grids(name, env, base)
        assert _fused_active(env) == int(c["uniform"]) and env.fused_step == c["uniform"]
        label = name + "-cal"
        ns, nv = c["n_sub"], base.wfs.nValid
        assert env._sh_tables.nValid == nv
        ref2d, valid = base.wfs.reference_slopes_maps, base.wfs.valid_2d
        _close(env.reference_centroids[:nv], ref2d[:ns][valid], "ref", CAL_TOL, label)
        _close(env.reference_centroids[nv:], ref2d[ns:][valid], "ref", CAL_TOL, label)
        np.testing.assert_allclose(env.slopes_units, base.wfs.slopes_units, rtol=1e-9)
        assert env.imat.shape == base.imat.shape
        _close(env.imat, base.imat, "imat_rel", CAL_TOL, label, scale=float(np.abs(base.imat).max()))
    finally:
        env.close()


@pytest.mark.parametrize("name", list(CASES))
def test_float64_shard_matches_oracle(name):
    """float64 shard (the batched kernels, the generic phase kernel) against the oracle that shares its per-layer operators."""
    env = _make_env(name, "f64")
    try:
        assert _fused_active(env) == 0
        _assert_grids(name, env, _base(name, env))
        _replay(env, _record(name, env), F64_SAME_OPERATOR_TOL_FULL, name + "-f64", screens0=True)
    finally:
        env.close()


@pytest.mark.parametrize("name", list(CASES))
def test_float32_shard_matches_oracle(name):
    """float32 shard, default switches (the production path of the case), against the same oracle run."""
    env = _make_env(name, "f32")
    try:
        assert _fused_active(env) == int(CASES[name]["uniform"])
        _assert_grids(name, env)
        _replay(env, _record(name, env), F32_TOL, name + "-f32", screens0=True)
    finally:
        env.close()


SWITCHES = [{"OPT_MFMA_GEMM": 0}, {"OPT_COEFS_IMAGE": 1}, {"OPT_DEFER_RING": 0}, {"OPT_RING_LOOKAHEAD": 0}, {"OPT_FAST_WFS": 0}]
SWITCH_RUNS = [(n, o) for n in CASES for o in SWITCHES] + [(n, {"OPT_FUSED_STEP": 0}) for n in UNIFORM]


def _tag(opts):
    return "+".join(f"{k[4:]}={v}" for k, v in opts.items())


@pytest.mark.parametrize("name,opts", SWITCH_RUNS, ids=[n + "-" + _tag(o) for n, o in SWITCH_RUNS])
def test_float32_switches_match_oracle(name, opts):
    """The other float32 kernels behind these grids (VALU ring product and contractions, command images, the ring scattered by a
    launch of its own, operands gathered and drawn in front of the GEMM, generic spots; the elevated grid outside the fused step
    kernel: k_phase_mfma4<BAND>), one switch at a time: each run held to the oracle, not to the default run."""
    env = _make_env(name, "f32", opts=opts)
    try:
        if not CASES[name]["uniform"] or "OPT_FUSED_STEP" in opts:
            assert _fused_active(env) == 0
        _replay(env, _record(name, env), F32_TOL, f"{name}-f32-{_tag(opts)}", screens0=True)
    finally:
        env.close()


# ---- the Pyramid behind unequal layers ------------------------------------------------------------------------------------------------
def _pyr_geo():
    return P._geo(F.PYR["base"], **F.atmosphere(F.PYR, P.CASES[F.PYR["base"]]["ppx"]))


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_pyramid_behind_unequal_layers(dtype):
    """The smallest Pyramid geometry of tests/test_gpu_pyramid_sweep.py (pow64) with a second layer at 10 km under 20 arcsec:
    calibration, float64 and float32 replay of one oracle run, with that module's helpers and its valid-pixel cut condition."""
    from rlao_amd.env import BatchedAOEnv
    name, g = F.PYR["base"], _pyr_geo()
    c = P.CASES[name]
    env = BatchedAOEnv(n_envs=N_ENVS, device=0, dtype=dtype, env_seed_stride=SEED_STRIDE)
    try:
        env.set_params(g, camera="ideal", wfs_type="pyramid")
        at = env._atm_tables
        R = c["n_sub"] * c["ppx"]
        assert not at.uniform and at.layer_res[0] == R + 4 and at.layer_res[1] > at.layer_res[0] and not env.fused_step
        if "pyr" not in _BASES:
            _BASES["pyr"] = F.build_oracle(g, env.M2C_CL, _operators(env), wfs_type="pyramid", modulation=g["modulation"],
                                           psf_centering=g["psfCentering"])
            _OBSERVED.setdefault("pyr-oracle", {})["valid_cut_gap"] = P.valid_cut_gap(_BASES["pyr"])
        base = _BASES["pyr"]
        assert [lay.g.resolution for lay in base.atm.layers] == at.layer_res
        assert [lay.g.foot[0].start + 1 for lay in base.atm.layers] == [n // 2 - R // 2 + 1 for n in at.layer_res]
        assert P.valid_cut_gap(base) >= P.MIN_CUT_GAP
        assert base.wfs.nSignal == c["n_signal"] == env.nSignal and base.nValidAct == c["n_valid_act"] == env.nValidAct
        assert np.array_equal(env.validI4Q, base.wfs.validI4Q) and np.array_equal(env.dm_mask.astype(bool), base.dm_mask)
        label, ns, nv = "pyr-cal", c["n_sub"], c["n_signal"] // 2
        ref2d, valid = base.wfs.referenceSignal_2D, base.wfs.validI4Q
        _close(env.reference_centroids[:nv], ref2d[:ns][valid], "ref", CAL_TOL, label)
        _close(env.reference_centroids[nv:], ref2d[ns:][valid], "ref", CAL_TOL, label)
        _close(env.imat, base.imat, "imat_rel", CAL_TOL, label, scale=float(np.abs(base.imat).max()))
        if "pyr" not in _RECORDS:
            _RECORDS["pyr"] = P.run_oracle(base, env.M2C_CL, env.modal_CM, P.SEED)
        rec = _RECORDS["pyr"]
        _same_controller(env, rec)
        assert rec["crossings"].shape == (N_ENVS, 2) and (rec["crossings"] >= 1).all(), rec["crossings"]
        _replay(env, rec, F64_SAME_OPERATOR_TOL_FULL if dtype == "f64" else F32_TOL, "pyr-" + dtype, screens0=True)
    finally:
        env.close()


# ---- behaviour on shards whose layers have grids of their own ----------------------------------------------------------------------
def _prologue(env, seed, screens=None):
    env.generate_new_phase_screen(seed, screens=screens)
    env.dm.coefs = 0
    env.dm_prev = 0
    env.measure()
    return env.reset_soft()


def _steps(env, obs, i0, n, log):
    """n closed-loop steps with action = 0.5 obs (exact in both precisions); appends (obs, frame, reward, Strehl, signal)."""
    from rlao_amd import _lib as L
    for i in range(i0, i0 + n):
        obs, frame, rew, sr, _, _ = env.step(i, 0.5 * obs)
        log.append(tuple(x.cpu().numpy().copy() for x in (obs, frame, rew, sr)) + (env._shard.download(L.B_SIGNAL, (env.n_envs, env.nSignal)),))
    return obs


def _final(env):
    from rlao_amd import _lib as L
    p = env.param
    return [env._flat_screens(env._download_screens()).copy(), env._shard.get_buff(p.nLayer).copy(),
            env._shard.download(L.B_MT_STATE, (p.nLayer, env.n_envs, 625), dtype=np.uint32),
            env._shard.download(L.B_DM_PREV, (env.n_envs, env.nValidAct)), np.array(env.total[:12]), np.array(env.residual[:12])]


def _same_log(a, b, envs_a=slice(None), envs_b=slice(None)):
    assert len(a) == len(b)
    for i, (x, y) in enumerate(zip(a, b)):
        for q, (u, v) in enumerate(zip(x, y)):
            assert np.array_equal(u[envs_a], v[envs_b]), (i, q)


def _same_final(a, b):
    for q, (u, v) in enumerate(zip(a, b)):
        assert np.array_equal(u, v), q


def _oracle_screens(env, seed):
    """ft_sh_phase_screen of every env and layer, on the layer's own grid: a list of [n_envs, N_l, N_l]."""
    from oracle import ao_oracle as O
    p, at = env.param, env._atm_tables
    return [np.stack([O.ft_sh_phase_screen(p.r0, p.L0, t.N, t.layer_D / t.N, int(s) + l) for s in env.env_seeds(seed)])
            for l, t in enumerate(at.layers)]


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_second_episode_and_host_screens(dtype):
    """`three`: the per-layer screen generators are rebuilt as N changes from layer to layer; the screens of two episodes in a row,
    with a step between them, are the oracle's ft_sh_phase_screen on each layer's own grid (atol as in
    test_gpu_behaviour.py::test_device_phase_screens_match_oracle), and the same screens made on the host and uploaded as a
    per-layer list give the same loop (that test's tolerances: screens 10 x, observations 1e-6 / 3e-5)."""
    tol = 1e-9 if dtype == "f64" else 2e-5
    obs_tol = 1e-6 if dtype == "f64" else 3e-5
    env = _make_env("three", dtype)
    try:
        _assert_grids("three", env)
        for episode, seed in enumerate((21, 4)):
            obs = _prologue(env, seed)
            dev = env._download_screens()
            want = _oracle_screens(env, seed)
            for l, w in enumerate(want):
                assert dev[l][:, 1:-1, 1:-1].shape == w.shape
                np.testing.assert_allclose(dev[l][:, 1:-1, 1:-1], w, rtol=0, atol=tol, err_msg=f"episode {episode} layer {l}")
            if episode == 0:
                _steps(env, obs, 0, 1, [])
        log_dev = []
        _steps(env, obs, 0, 3, log_dev)
        obs_host = _prologue(env, 4, screens=want)
        up = env._download_screens()
        for l in range(len(want)):
            np.testing.assert_allclose(up[l], dev[l], rtol=0, atol=10 * tol)
        np.testing.assert_allclose(obs_host.cpu().numpy(), obs.cpu().numpy(), rtol=0, atol=obs_tol)
        log_host = []
        _steps(env, obs_host, 0, 3, log_host)
        for x, y in zip(log_dev, log_host):
            np.testing.assert_allclose(y[0], x[0], rtol=0, atol=obs_tol)
        with pytest.raises(ValueError, match="per-layer arrays"):
            env.generate_new_phase_screen(4, screens=[want[0], want[0], want[2]])
    finally:
        env.close()


@pytest.mark.parametrize("name,dtype", [("three", "f32"), ("three", "f64"), ("up70", "f32")])
def test_checkpoint_after_a_crossing(name, dtype):
    """State taken right after a step in which a layer crossed a pixel (its ring extruded; float32: scattered late, the next
    operand gathered ahead), restored into a fresh shard: the following steps and the final state are the same bit for bit."""
    a = _make_env(name, dtype)
    b = _make_env(name, dtype)
    try:
        assert _fused_active(a) == int(name == "up70" and dtype == "f32")
        nl = a.param.nLayer
        obs = _prologue(a, 11)
        _prologue(b, 12)                                            # (another episode: everything must come from the state)
        crossed, i = False, 0
        while not crossed:
            b0 = a._shard.get_buff(nl).copy()
            obs = _steps(a, obs, i, 1, [])
            crossed = bool((np.abs(a._shard.get_buff(nl)) < np.abs(b0)).any())
            i += 1
            assert i <= 4
        state = copy.deepcopy(a.get_state())
        b.set_state(state)
        la, lb = [], []
        _steps(a, obs, i, 4, la)
        _steps(b, b._obs, i, 4, lb)
        _same_log(la, lb)
        fa, fb = _final(a), _final(b)
        _same_final(fa[:4], fb[:4])
        assert np.array_equal(fa[4][i:i + 4], fb[4][i:i + 4]) and np.array_equal(fa[5][i:i + 4], fb[5][i:i + 4])
    finally:
        a.close()
        b.close()


def test_batch_position():
    """`three`, float32: env e of the three-env shard == a one-env shard with its seed, bit for bit (the ring GEMM's split count
    does not depend on the number of envs, at three different K); both are held to the oracle run."""
    env = _make_env("three", "f32")
    try:
        rec = _record("three", env)
        whole = _replay(env, rec, F32_TOL, "three-f32")
    finally:
        env.close()
    for e in range(N_ENVS):
        one = _make_env("three", "f32", n_envs=1)
        try:
            shifted = dict(rec, seed=rec["seed"] + SEED_STRIDE * e)
            got = _replay(one, shifted, F32_TOL, "three-f32-one-env", envs=[e])
        finally:
            one.close()
        assert np.array_equal(got[0][0], whole[0][e])
        for x, y in zip(got[1:], whole[1:]):
            for u, v in zip(x, y):
                assert np.array_equal(u[0], v[e])


@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_run_integrator_equals_stepping(dtype):
    """`three`: six steps of the on-device integrator (gain 0.5) == six step() calls with action = 0.5 obs, bit for bit."""
    a = _make_env("three", dtype)
    b = _make_env("three", dtype)
    try:
        log = []
        obs_a = _steps(a, _prologue(a, 7), 0, STEPS, log)
        _prologue(b, 7)
        obs_b, rew_b, sr_b = b.run_integrator(0, STEPS, gain=0.5)
        assert np.array_equal(obs_a.cpu().numpy(), obs_b.cpu().numpy())
        assert np.array_equal(log[-1][2], rew_b.cpu().numpy()) and np.array_equal(log[-1][3], sr_b.cpu().numpy())
        fa, fb = _final(a), _final(b)
        _same_final(fa[:4], fb[:4])
        assert np.array_equal(fa[4][:STEPS], fb[4][:STEPS]) and np.array_equal(fa[5][:STEPS], fb[5][:STEPS])
    finally:
        a.close()
        b.close()


def test_per_env_r0_sigma_one_env_is_the_plain_shard():
    """`two`, float32: with a Fried parameter per env, the envs whose r0 is the tables' (sigma = 1) are bit-identical to the shard
    without the feature; the other env's second layer (the larger grid) is not."""
    r0 = np.array([F.R0, 0.08, F.R0])
    runs = []
    for on in (False, True):
        env = _make_env("two", "f32")
        try:
            if on:
                env.set_r0_per_env(r0)
            log = []
            _steps(env, _prologue(env, 9), 0, STEPS, log)
            runs.append((log, env._download_screens()))
        finally:
            env.close()
    (off, scr_off), (on, scr_on) = runs
    _same_log(on, off, [0, 2], [0, 2])
    for l in range(2):
        assert np.array_equal(scr_on[l][[0, 2]], scr_off[l][[0, 2]])
        assert not np.array_equal(scr_on[l][1], scr_off[l][1])


def test_refusals_leave_the_shard_alone():
    """`three`, float32: per-env winds, a partial reset and a single pair of operators are refused on layers with grids of their own;
    after each refusal the shard steps on bit-identical to a twin that was never asked."""
    from rlao_amd import _lib as L
    env = _make_env("three", "f32")
    twin = _make_env("three", "f32")
    try:
        p, at = env.param, env._atm_tables
        oe, ot = _prologue(env, 13), _prologue(twin, 13)
        le, lt = [], []
        oe, ot = _steps(env, oe, 0, 2, le), _steps(twin, ot, 0, 2, lt)
        speed = np.tile(np.asarray(p.windSpeed) * 0.9, (N_ENVS, 1))
        i = 2
        for what in ("wind", "reset", "operators"):
            if what == "wind":
                with pytest.raises(L.AoEnvError, match="grids of their own"):
                    env.set_wind_per_env(speed=speed)
            elif what == "reset":
                with pytest.raises(L.AoEnvError, match="grids of their own"):
                    env.reset_envs([1], seed=3)
            else:
                with pytest.raises(ValueError, match="one pair per layer"):
                    env.set_params(F.geo("three"), camera="ideal", wfs_type="shackhartmann", atm_AB=(at.A, at.B))
                assert env._atm_tables is at and env.param is p
            assert not env._per_env_clock and env._wind_env is None
            oe, ot = _steps(env, oe, i, 2, le), _steps(twin, ot, i, 2, lt)
            i += 2
            _same_log(le, lt)
        _same_final(_final(env), _final(twin))
    finally:
        env.close()
        twin.close()
    # one pair per layer is what such a shard takes: the env's own operators handed back give the same loop, bit for bit
    own = _make_env("three", "f32", atm_AB=[(t.A.copy(), t.B.copy()) for t in at.layers])
    try:
        assert len({id(t) for t in own._atm_tables.layers}) == 3
        lo = []
        _steps(own, _prologue(own, 13), 0, 4, lo)
        _same_log(lo, lt[:4])
    finally:
        own.close()
