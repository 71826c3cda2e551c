"""GPU: the off-axis science target per env (aoenv_set_science_direction, rlao_amd/csrc/offaxis.hpp, k_science_residual).

Geometries from tests/_fov_cases.py: `two` (R = 42, grids 46 / 61: the batched float32 kernels), `p5_shared` (R = 30, generic
kernels), `up70` (one elevated grid: the fused step kernel) and the Pyramid behind unequal layers.  Four envs per shard, every env
its own direction; over the cases: fov / 2 at azimuth 0, 90, 180 and 270 (`up70`), diagonals with both fractions non-zero, negative
offsets (180, 225, 270), zenith 0, and in every case an offset whose fraction is above a half (where rounding is not truncating).

Parity: six closed-loop steps, the oracle's actions replayed (as tests/test_gpu_geometry_sweep.py records them); after every step
opd_atm_sci, phase_sci, rms_nm and strehl against tests/_offaxis_ref.py on the oracle's layers plus the oracle's mirror surface
of that step, under the unchanged opd_m / rms_nm / strehl entries of F32_TOL and F64_SAME_OPERATOR_TOL of tests/test_gpu_parity.py:
the same quantity, formed by the same arithmetic plus one blend and one difference.  AO_PARITY_REPORT=<file> with this module alone
writes the measured maxima (profiles/offaxis_parity_maxima.json).  tests/test_offaxis_host.py shows on the CPU, on these very
inputs, that dropping or flipping the fractions, swapping rows and columns or rounding in place of truncating moves opd_atm_sci by
more than 100 of these tolerances.

Everything else is bit for bit: zenith 0 against AOENV_B_PHASE / AOENV_B_OPD_ATM on the fused, the batched float32 and the float64
shard; an env of a mixed shard against a one-env shard of its seed and direction; every loop's record against a twin that steps and
calls science_residual(), with camera noise, a wavefront record and a long exposure attached, the loop's outputs against a run
without the record; the science camera, the long exposure and project_wavefront("science") against an upload of phase_sci; the
refusals and clear_science_direction().  Composition: `up70` with per-env winds (one above a pixel per frame), per-env r0 and a
mis-registered mirror per env against one oracle per env (tests/_compose_ref.py), same tolerances.  No test provokes a fault: the
refusals are host-side checks that return before a launch.
"""
import numpy as np
import pytest

import _fov_cases as F
import _offaxis_ref as X
import test_gpu_fov_sweep as V
import test_gpu_geometry_sweep as G
import test_gpu_pyramid_sweep as P
import test_gpu_science as S
from test_gpu_parity import F32_TOL, F64_SAME_OPERATOR_TOL, _close

pytestmark = pytest.mark.gpu

N = 4
STEPS = G.STEPS
STRIDE = G.SEED_STRIDE
GAIN = 0.5

# [zenith arcsec, azimuth deg] of the four envs of every case (fov: two 20, p5_shared 15, up70 10, pyr 20)
DIRS = {
    "two": [(10.0, 225.0), (7.6, 30.0), (0.0, 0.0), (10.0, 90.0)],
    "p5_shared": [(7.5, 225.0), (3.7, 30.0), (7.5, 180.0), (7.5, 0.0)],
    "up70": [(5.0, 0.0), (5.0, 90.0), (5.0, 180.0), (5.0, 270.0)],
    "pyr": [(10.0, 0.0), (10.0, 225.0), (7.6, 30.0), (0.0, 0.0)],
}
SEEDS = {"two": 5, "p5_shared": 6, "up70": 5, "pyr": P.SEED}


def _np(t):
    return t.detach().cpu().numpy()


def _geo(name, **kw):
    if name == "pyr":
        g = V._pyr_geo()
        g.update(kw)
        return g
    return F.geo(name, **kw)


def _make(name, dtype, n=N, **kw):
    from rlao_amd.env import BatchedAOEnv
    env = BatchedAOEnv(n_envs=n, device=0, dtype=dtype, env_seed_stride=STRIDE)
    try:
        env.set_params(_geo(name, **kw), camera="ideal", wfs_type="pyramid" if name == "pyr" else "shackhartmann")
    except Exception:
        env.close()
        raise
    return env


def _direct(env, name, ids=range(N)):
    d = np.array([DIRS[name][k] for k in ids])
    env.set_science_direction(d[:, 0], d[:, 1])
    return d


def _prologue(env, seed):
    env.generate_new_phase_screen(seed)
    env.dm.coefs = 0
    env.dm_prev = 0
    env.measure()
    env.SR = []
    return env.reset_soft()


def _buf(env, which):
    return env._shard.download(which, (env.n_envs, env.R, env.R), env._stream())


# ---- 1. parity ------------------------------------------------------------------------------------------------------------------------
_BASES, _RUNS = {}, {}


def _base(name, env):
    if name not in _BASES:
        g = _geo(name)
        kw = dict(wfs_type="pyramid", modulation=g["modulation"], psf_centering=g["psfCentering"]) if name == "pyr" else {}
        _BASES[name] = F.build_oracle(g, env.M2C_CL, V._operators(env), **kw)
    return _BASES[name]


def _oracle_run(name, env):
    """N envs (seeds seed + 100 k) of the case's oracle, one closed-loop episode with float32 actions from the oracle's own
    observations; after every step the science quantities of env k toward DIRS[name][k], behind the surface that step showed."""
    import copy
    if name in _RUNS:
        return _RUNS[name]
    base, g = _base(name, env), _geo(name)
    orcs, rec = [], dict(seed=SEEDS[name], actions=[], opd_sci=[], opd_res=[], rms=[], strehl=[], modal_cm=np.array(env.modal_CM))
    for k in range(N):
        o = copy.deepcopy(base, memo={id(x): x for x in (base.dm_modes, base.imat) if x is not None})
        o.M2C = np.asarray(env.M2C_CL, dtype=np.float64)
        o.modal_cm = np.asarray(env.modal_CM, dtype=np.float64)
        o.reconstructor = o.M2C @ o.modal_cm
        o.new_episode(SEEDS[name] + STRIDE * k)
        orcs.append(o)
    obs = np.stack([o.reset_soft() for o in orcs])
    rs = np.random.RandomState(9)
    for i in range(STEPS):
        act = (GAIN * obs + 0.05 * rs.randn(*obs.shape)).astype(np.float32) * orcs[0].dm_mask[None].astype(np.float32)
        row = dict(opd_sci=[], opd_res=[], rms=[], strehl=[])
        nxt = []
        for k, o in enumerate(orcs):
            dm = o.dm_opd(o.coefs)                                 # the surface this step's measurement sees
            nxt.append(o.step(i, act[k])[0])
            zen, az = DIRS[name][k]
            sci = X.science_opd(o.atm, g["altitude"], zen, az)
            opd, _, rms, sr = X.science_residual(sci, dm, o.pupil, o.wavelength)
            if zen == 0:                                           # (the restatement on axis is the oracle itself)
                assert np.array_equal(sci, o.atm.OPD_no_pupil) and np.array_equal(opd, o.tel_OPD)
            for q, v in zip(("opd_sci", "opd_res", "rms", "strehl"), (sci, opd, rms, sr)):
                row[q].append(v)
        for q, v in row.items():
            rec[q].append(np.stack(v))
        rec["actions"].append(act)
        obs = np.stack(nxt)
    _RUNS[name] = rec
    return rec


PARITY = [(n, d) for n in ("two", "p5_shared", "up70", "pyr") for d in ("f32", "f64")]


@pytest.mark.parametrize("name,dtype", PARITY, ids=[f"{n}-{d}" for n, d in PARITY])
def test_science_residual_matches_the_restatement(name, dtype):
    import torch
    tol = F32_TOL if dtype == "f32" else F64_SAME_OPERATOR_TOL
    label = f"offaxis-{name}-{dtype}"
    env = _make(name, dtype)
    try:
        rec = _oracle_run(name, env)
        G._same_controller(env, rec)
        assert env.fused_step == (name == "up70" and dtype == "f32")
        d = _direct(env, name)
        assert np.array_equal(env.science_direction, d) and np.array_equal(env.src.coordinates, d)
        _prologue(env, rec["seed"])
        k_opd = env.src_wavelength / (2 * np.pi)
        for i in range(STEPS):
            env.step(i, torch.as_tensor(rec["actions"][i]))
            phase, rms, sr = (_np(t) for t in env.science_residual())
            opd = _np(env.science_atmosphere())
            for k in range(N):
                _close(opd[k], rec["opd_sci"][i][k], "opd_m", tol, label, err_msg=f"opd_atm_sci step {i} env {k}")
                _close(phase[k] * k_opd, rec["opd_res"][i][k], "opd_m", tol, label, err_msg=f"phase_sci step {i} env {k}")
                _close(rms[k], rec["rms"][i][k], "rms_nm", tol, label, err_msg=f"rms step {i} env {k}")
                _close(sr[k], rec["strehl"][i][k], "strehl", tol, label, err_msg=f"strehl step {i} env {k}")
            assert (phase[:, ~np.asarray(env.pupil, dtype=bool)] == 0).all()
    finally:
        env.close()


# ---- 2. zenith 0 ----------------------------------------------------------------------------------------------------------------------
ZERO = [("up70", "f32", True), ("two", "f32", False), ("two", "f64", False)]


@pytest.mark.parametrize("name,dtype,fused", ZERO, ids=[f"{n}-{d}" for n, d, _ in ZERO])
def test_zenith_zero_is_the_guide_star_bit_for_bit(name, dtype, fused):
    """Every env at zenith 0 (any azimuth): the kernel computes the footprint, skips the blend as the reference does, and
    phase_sci / opd_atm_sci are the step's own AOENV_B_PHASE / AOENV_B_OPD_ATM.  The Strehl ratio is the step's to rounding."""
    from rlao_amd import _lib as L
    env = _make(name, dtype)
    try:
        assert env.fused_step == fused
        env.set_science_direction(0.0, np.array([0.0, 90.0, 225.0, 30.0]))
        obs = _prologue(env, 7)
        for i in range(3):
            obs, _, _, sr_step, _, _ = env.step(i, GAIN * obs)
            phase, rms, sr = (_np(t) for t in env.science_residual())
            opd = _np(env.science_atmosphere())
            assert np.abs(phase).max() > 0
            assert np.array_equal(phase, _buf(env, L.B_PHASE)), i
            assert np.array_equal(opd, _buf(env, L.B_OPD_ATM)), i
            np.testing.assert_allclose(sr, _np(sr_step), rtol=0, atol=(F32_TOL if dtype == "f32" else F64_SAME_OPERATOR_TOL)["strehl"])
    finally:
        env.close()


# ---- 3. twins and position ---------------------------------------------------------------------------------------------------------------
def _walk(env, seed, steps=4):
    out = []
    obs = _prologue(env, seed)
    for i in range(steps):
        obs = env.step(i, GAIN * obs)[0]
        out.append([_np(t).copy() for t in env.science_residual()] + [_np(env.science_atmosphere()).copy()])
    return out


@pytest.mark.parametrize("name", ["two", "up70"])
def test_an_env_has_the_same_bits_in_any_shard_and_at_any_place(name):
    """float32: env k of the mixed shard == the only env of a one-env shard with its seed and its direction, and == env 0 of a shard
    in which every env has that direction."""
    env = _make(name, "f32")
    try:
        _direct(env, name)
        whole = _walk(env, 11)
    finally:
        env.close()
    for k in (1, 3):
        one = _make(name, "f32", n=1)
        try:
            _direct(one, name, [k])
            got = _walk(one, 11 + STRIDE * k)
        finally:
            one.close()
        for a, b in zip(got, whole):
            for u, v in zip(a, b):
                assert np.array_equal(u[0], v[k]), k
    allk = _make(name, "f32", n=2)
    try:
        _direct(allk, name, [0, 0])
        got = _walk(allk, 11)
        for a, b in zip(got, whole):
            for u, v in zip(a, b):
                assert np.array_equal(u[0], v[0])
    finally:
        allk.close()


# ---- 4. every loop records what a per-call twin reads --------------------------------------------------------------------------------
LOOPS = ("step", "step_modal", "run_integrator", "run_integrator_delay", "rollout", "policy_rollout")
LOOP_CASES = [(d, l) for d in ("f32", "f64") for l in LOOPS]
_LOOP_ENVS = {}


def _loop_env(dtype, tag):
    if (dtype, tag) not in _LOOP_ENVS:
        env = _make("up70", dtype, gainCL=GAIN)
        env.wfs.cam.photonNoise = True
        _LOOP_ENVS[(dtype, tag)] = env
    env = _LOOP_ENVS[(dtype, tag)]
    env.set_delay(0)
    env.clear_modal()
    env._surface = "zonal"
    return env


@pytest.fixture(scope="module", autouse=True)
def _close_loop_envs():
    yield
    for env in _LOOP_ENVS.values():
        env.close()
    _LOOP_ENVS.clear()


def _attach(env, loop, record):
    """what every shard of the comparison carries: camera noise, a wavefront record, a long exposure, the direction"""
    S._configure(env, loop)
    if loop == "run_integrator_delay":
        env.set_delay(1)
    _direct(env, "up70")
    env.set_wavefront_basis(opd2m=np.linalg.pinv(_m2opd(env)))
    env.set_science(zero_padding=2, window=8, first_frame=2)
    obs = S._start(env, "step_modal" if loop == "step_modal" else "step")
    env.record_wavefront(0, S.STEPS)
    env.start_long_exposure()
    rec = env.record_science_direction(0, S.STEPS) if record else None
    return obs, rec


def _m2opd(env):
    """five smooth modes on the pupil, [n_pix, 5]"""
    yy, xx = np.nonzero(np.asarray(env.pupil))
    x, y = (xx - env.R / 2) / env.R, (yy - env.R / 2) / env.R
    return np.stack([x, y, x * y, x * x - y * y, x * x + y * y], axis=1) * 1e-7


def _loop_name(loop):
    return "run_integrator" if loop == "run_integrator_delay" else loop


@pytest.mark.parametrize("dtype,loop", LOOP_CASES, ids=[f"{d}-{l}" for d, l in LOOP_CASES])
def test_every_loop_records_what_a_per_call_twin_reads(dtype, loop):
    """8 frames of `up70` (float32: the fused step kernel) with photon noise, a wavefront record and a long exposure attached: the
    science-direction record bit for bit (rms, Strehl) what a twin gives that steps through the per-call API and calls
    science_residual() after every step; the loop's outputs, buffers, wavefront record, long exposure and get_state() bit for bit
    those of a third shard without the record; the fused shard stays fused."""
    import torch
    env, twin, plain = (_loop_env(dtype, t) for t in "abc")
    obs, rec = _attach(env, loop, True)
    assert env.fused_step == (dtype == "f32")
    handed, actions = S._run_loop(env, _loop_name(loop), obs)
    torch.cuda.synchronize()
    assert env.fused_step == (dtype == "f32")
    got_rec = _np(rec).copy()
    got = S._everything(env, handed)
    got["wf"], got["le"] = _np(env._wf_rec).copy(), [_np(t).copy() for t in env._le if t is not None]
    # the twin: the per-call API and science_residual()
    obs_t, _ = _attach(twin, loop, False)
    want = np.zeros_like(got_rec)
    for k in range(S.STEPS):
        if loop in ("run_integrator", "run_integrator_delay", "step"):
            obs_t = twin.step(k, GAIN * obs_t)[0]
        elif loop in ("rollout", "policy_rollout"):
            obs_t = twin.step(k, actions[k])[0]
        else:
            obs_t = twin.step_modal(k, S._modal_actions(twin, obs_t, k))[0]
        _, rms, sr = twin.science_residual()
        want[k, 0], want[k, 1] = _np(rms), _np(sr)
    # (the untrained policy drives the loop away: a Strehl ratio may underflow to 0 in float32)
    assert np.isfinite(got_rec).all() and (got_rec[:, 0] > 0).all() and (got_rec[:, 1] >= 0).all() and (got_rec[:, 1] < 1).all()
    assert np.array_equal(got_rec, want), np.abs(got_rec - want).max()
    assert not np.array_equal(got_rec[:, :, 0], got_rec[:, :, 1])
    # without the record
    obs_p, _ = _attach(plain, loop, False)
    handed_p, _ = S._run_loop(plain, _loop_name(loop), obs_p)
    torch.cuda.synchronize()
    ref = S._everything(plain, handed_p)
    ref["wf"], ref["le"] = _np(plain._wf_rec).copy(), [_np(t).copy() for t in plain._le if t is not None]
    assert got.keys() == ref.keys()
    for k in ref:
        if not (k == "state.obs" and loop == "step_modal"):
            S._same(got[k], ref[k], k)
    # a call that leaves the window is refused before anything is launched
    from rlao_amd import _lib as L
    with pytest.raises(L.AoEnvError, match="science-direction record"):
        (env.run_integrator_modal if loop == "step_modal" else env.run_integrator)(S.STEPS - 1, 2)
    for e in (env, twin, plain):
        e.stop_science_direction_record()
        e.stop_wavefront_record()
        e.stop_long_exposure()
        e.clear_science_direction()
        e.clear_science()
        e.clear_wavefront_basis()
        if loop == "policy_rollout":
            e.set_policy(None)


def test_launch_counts_without_a_direction():
    """float32 `up70`: 8 steps of run_integrator cost the launches they cost before a direction ever existed -- counted, not timed --
    with no direction, and after one was set and cleared; under a record the fused kernel covers one step per launch (the step
    pairs stand down) and nothing else changes."""
    a, b = _loop_env("f32", "a"), _loop_env("f32", "b")
    counts = []
    for env, mode in ((a, "never"), (b, "cleared"), (b, "record")):
        if mode == "cleared":
            _direct(env, "up70")
            env.clear_science_direction()
        _prologue(env, 5)
        if mode == "record":
            _direct(env, "up70")
            env.record_science_direction(0, 8)
        env._shard.profile(True)
        env.run_integrator(0, 8)
        prof = env._shard.profile_read(env._stream())
        counts.append(({k: v[1] for k, v in prof.items()}, env._shard.step_counters()))
        env._shard.profile(False)
    env.clear_science_direction()
    assert counts[0] == counts[1]
    assert counts[0][1][1] == 8                                       # steps covered, in however many launches
    assert counts[2][1] == (8, 8)
    assert {k: v for k, v in counts[2][0].items() if k != "env_step"} == {k: v for k, v in counts[0][0].items() if k != "env_step"}


# ---- 5. consumers ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_the_science_camera_and_the_projection_look_at_the_target(dtype):
    """`two`: science_psf(), the long exposure and project_wavefront("science") under a direction == the same read-outs of a
    twin without a direction whose AOENV_B_PHASE was uploaded with phase_sci, bit for bit."""
    import torch
    from rlao_amd import _lib as L
    env, twin = _make("two", dtype), _make("two", dtype)
    try:
        for e in (env, twin):
            e.set_science(zero_padding=2, window=8, first_frame=0)
            e.set_wavefront_basis(opd2m=np.linalg.pinv(_m2opd(e)))
        _direct(env, "two")
        obs = _prologue(env, 3)
        _prologue(twin, 3)
        env.start_long_exposure()
        twin_sum = torch.zeros((N, 8, 8), device=twin.device, dtype=twin.tdtype)
        for i in range(3):
            obs = env.step(i, GAIN * obs)[0]
            phase = env.science_residual()[0]
            twin._shard.upload_state(L.B_PHASE, _np(phase).reshape(N, -1), twin._stream())
            want_psf, want_wf = twin.science_psf(), twin.project_wavefront("residual")
            twin_sum = twin_sum + want_psf
            assert np.array_equal(_np(env.science_psf()), _np(want_psf)), i
            assert np.array_equal(_np(env.project_wavefront("science")), _np(want_wf)), i
            assert not np.array_equal(_np(env.project_wavefront("residual")), _np(want_wf))
            assert np.array_equal(_np(env.science_psf(flat=True)), _np(twin.science_psf(flat=True)))
        torch.cuda.synchronize()
        assert np.array_equal(_np(env._le[0]), _np(twin_sum)) and np.array_equal(_np(env._le[2]), np.full(N, 3, dtype=np.int32))
        with pytest.raises(L.AoEnvError, match="on demand only"):
            env.record_wavefront(0, 4, what=("science",))
    finally:
        env.close()
        twin.close()


# ---- 5b. composition ----------------------------------------------------------------------------------------------------------------------
COMPOSED = dict(r0=[0.13, 0.09, 0.16, 0.11], wind_speed=[10.0, 30.0, 22.0, 50.0], wind_dir=[72.0, 200.0, 144.0, 310.0],
                misreg=[dict(), dict(shift_x=0.2 * 0.4), dict(shift_y=-0.1 * 0.4, tangential_scaling=0.01), dict(radial_scaling=0.02)])


@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_composed_with_per_env_winds_r0_and_mirrors(dtype):
    """`up70` with every env its own wind (env 3: 1.5 pixels per frame, a whole-pixel ring round in every step), its own Fried
    parameter and its own mis-registered mirror, and its own direction: against one oracle per env (tests/_compose_ref.py) with the
    restatement on that oracle's layers and that oracle's mirror surface, under the same tolerances."""
    import torch
    import _compose_ref as CR
    tol = F32_TOL if dtype == "f32" else F64_SAME_OPERATOR_TOL
    label = f"offaxis-composed-{dtype}"
    env = _make("up70", dtype)
    try:
        g = _geo("up70")
        assert g["diameter"] / g["nSubaperture"] == pytest.approx(0.4)
        specs = [CR.env_spec(seed=9 + STRIDE * e, r0=COMPOSED["r0"][e], wind_speed=[COMPOSED["wind_speed"][e]],
                             wind_dir=[COMPOSED["wind_dir"][e]], misreg=COMPOSED["misreg"][e] or None) for e in range(N)]
        orc = CR.ComposedOracle(_base("up70", env), specs, m2c=env.M2C_CL, modal_cm=env.modal_CM)
        env.set_r0_per_env(np.array(COMPOSED["r0"]))
        env.set_dm_misregistration(**{k: np.array([m.get(k, 0.0) for m in COMPOSED["misreg"]]) for k in CR.MISREG_KEYS})
        _direct(env, "up70")
        env.generate_new_phase_screen(9)
        env.set_wind_per_env(np.array(COMPOSED["wind_speed"])[:, None], np.array(COMPOSED["wind_dir"])[:, None], reset=True, max_pixels=2)
        env.dm.coefs = 0
        env.dm_prev = 0
        env.measure()
        env.reset_soft()
        orc.new_episode()
        obs = orc.reset_soft()
        rs = np.random.RandomState(4)
        k_opd = env.src_wavelength / (2 * np.pi)
        for i in range(STEPS):
            act = (GAIN * obs + 0.05 * rs.randn(*obs.shape)).astype(np.float32) * orc.envs[0].dm_mask[None].astype(np.float32)
            dms = [o.dm_opd(o.coefs) for o in orc.envs]
            obs = orc.step(i, act)["obs"]
            env.step(i, torch.as_tensor(act))
            phase, rms, sr = (_np(t) for t in env.science_residual())
            opd = _np(env.science_atmosphere())
            for e, o in enumerate(orc.envs):
                zen, az = DIRS["up70"][e]
                sci = X.science_opd(o.atm, g["altitude"], zen, az)
                want, _, want_rms, want_sr = X.science_residual(sci, dms[e], o.pupil, o.wavelength)
                _close(opd[e], sci, "opd_m", tol, label, err_msg=f"opd_atm_sci step {i} env {e}")
                _close(phase[e] * k_opd, want, "opd_m", tol, label, err_msg=f"phase_sci step {i} env {e}")
                _close(rms[e], want_rms, "rms_nm", tol, label, err_msg=f"rms step {i} env {e}")
                _close(sr[e], want_sr, "strehl", tol, label, err_msg=f"strehl step {i} env {e}")
        assert orc.whole_rounds[3].max() >= 1                       # env 3 made whole-pixel rounds
    finally:
        env.close()


# ---- 6. refusals and lifecycle ----------------------------------------------------------------------------------------------------------
def test_refusals_and_a_cleared_direction_leave_no_trace():
    """`two`, float32: what is refused is refused before a launch and changes nothing; after clear_science_direction() the shard
    steps on bit-identical to a twin that never had a direction."""
    from rlao_amd import _lib as L
    from rlao_amd.env import BatchedAOEnv
    env, twin = _make("two", "f32"), _make("two", "f32")
    try:
        with pytest.raises(L.AoEnvError, match="no science direction"):
            env.science_residual()
        with pytest.raises(L.AoEnvError, match="no science direction"):
            env.record_science_direction(0, 4)
        d = _direct(env, "two")
        for bad in (10.0001, -0.1, np.inf):
            with pytest.raises(ValueError, match="zenith"):
                env.set_science_direction(bad, 0.0, env_ids=[1])
        zen = np.array([10.0, 10.0, 10.5, 10.0])                     # past the Python layer: the library's own check
        with pytest.raises(L.AoEnvError, match="above fov / 2"):
            L.call(env._shard, "aoenv_set_science_direction", zen, np.zeros(4), env._stream())
        assert np.array_equal(env.science_direction, d)
        oe, ot = _prologue(env, 13), _prologue(twin, 13)
        env._shard.set_atm_opd(np.zeros((N, env.R * env.R)))
        with pytest.raises(L.AoEnvError, match="user-defined"):
            env.science_residual()
        oe, ot = _prologue(env, 13), _prologue(twin, 13)
        rec = env.record_science_direction(2, 2)
        with pytest.raises(L.AoEnvError, match="science-direction record"):
            env.step(0, GAIN * oe)
        with pytest.raises(L.AoEnvError, match="science-direction record"):
            env.run_integrator(2, 3)
        assert not _np(rec).any()
        env.clear_science_direction()
        assert env.science_direction is None and not env.src.coordinates.any()
        la, lb = [], []
        V._steps(env, oe, 0, 4, la)
        V._steps(twin, ot, 0, 4, lb)
        V._same_log(la, lb)
        V._same_final(V._final(env), V._final(twin))
    finally:
        env.close()
        twin.close()
    flat = BatchedAOEnv(n_envs=2, device=0, dtype="f32")                # no layers above the ground and no field of view: zenith 0 alone
    try:
        flat.set_params(S.R24, camera="ideal", wfs_type="shackhartmann")
        with pytest.raises(ValueError, match="zenith"):
            flat.set_science_direction(0.4)
        flat.set_science_direction(0.0, 45.0)
        cal = flat._make_shard(1, "f32", n_layer=0, max_group=1)      # a shard without layers
        try:
            with pytest.raises(L.AoEnvError, match="no layers"):
                L.call(cal, "aoenv_set_science_direction", np.zeros(1), np.zeros(1), 0)
        finally:
            cal.close()
    finally:
        flat.close()
