"""GPU: the off-axis guide star per env (aoenv_set_guide_direction, rlao_amd/csrc/offaxis.hpp, k_guide_opd): the SENSOR's line of sight.

Cases, four envs per shard, every env its own direction (tests/_fov_cases.py; DIRS below are tests/test_gpu_offaxis.py's where the
case is shared: fov / 2 at azimuth 0 / 90 / 180 / 270, diagonals with both fractions non-zero, negative offsets, a fraction above
one half, zenith 0):
  two        R = 42, grids 46 / 61, the batched float32 kernels (k_phase_mfma)
  p5_shared  R = 30, the generic kernels
  top_first  R = 66, the elevated layer first
  up70       R = 60, one elevated grid: fused without a direction, so the case also shows the shard leaving the fused path
  pyr        the Pyramid of tests/test_gpu_fov_sweep.py
  geo        `two` behind the geometric Shack-Hartmann sensor
Tile edges of k_guide_opd's 16-row x 64-column tiles: `top_first` (R = 66) crosses both -- four full row tiles plus 2 rows, one full
column tile plus 2 columns; `two` (42 = 2 x 16 + 10), `p5_shared` (30 = 16 + 14) and `up70` (60 = 3 x 16 + 12) end in a partial row
tile and have one partial column tile.

1 parity: STEPS closed-loop steps replaying the guided oracle's float32 actions (tests/_guide_ref.py on the case's OracleEnv, one
  per env); after every step, per env, AOENV_B_OPD_ATM, the phase, the WFS signal, obs, reward, Strehl and the residual rms under
  the unchanged opd_m / strehl / rms_nm entries of F32_TOL / F64_SAME_OPERATOR_TOL of tests/test_gpu_parity.py and the signal / obs /
  reward entries tests/test_gpu_fov_sweep.py holds these very cases to (F32_TOL / F64_SAME_OPERATOR_TOL_FULL); the geometric sensor's
  signal under tests/test_gpu_geometric.py's bound.  AO_PARITY_REPORT=<file> with this module alone writes the measured maxima
  (profiles/guide_parity_maxima.json).  tests/test_guide_host.py shows on the CPU that an oracle which ignores the direction misses
  these inputs by more than 100 tolerances.
2 zenith 0 is the axis: every output buffer over several steps == a twin with no direction and AOENV_OPT_FUSED_STEP off.
3 the two kernels agree: science direction == guide direction -> science_atmosphere() == AOENV_B_OPD_ATM, phase_sci == AOENV_B_PHASE.
4 off-axis sensor, on-axis target: science_atmosphere() == the AOENV_B_OPD_ATM of an unguided twin; science_residual() against
  the restatement.
5 place invariance, 6 every loop == per-call stepping, 7 composition with per-env winds, r0 and mirrors, 8 off is off.
Everything but 1, 7 and the second half of 4 is bit for bit.  No test provokes a fault: the refusals are host-side checks that
return before a launch."""
import copy

import numpy as np
import pytest

import _fov_cases as F
import _guide_ref as R
import _offaxis_ref as X
import test_gpu_fov_sweep as V
import test_gpu_geometric as GEOT
import test_gpu_geometry_sweep as G
import test_gpu_offaxis as OA
import test_gpu_science as S
from test_gpu_parity import F32_TOL, F64_SAME_OPERATOR_TOL, F64_SAME_OPERATOR_TOL_FULL, _close

pytestmark = pytest.mark.gpu

N = 4
STEPS = 4
STRIDE = G.SEED_STRIDE
GAIN = 0.5

CASES = ("two", "p5_shared", "top_first", "up70", "pyr", "geo")
# [zenith arcsec, azimuth deg] of the four envs (fov: two 20, p5_shared 15, top_first 30, up70 10, pyr 20)
DIRS = dict(OA.DIRS, top_first=[(15.0, 0.0), (15.0, 225.0), (12.5, 20.0), (0.0, 0.0)], geo=OA.DIRS["two"])
SEEDS = dict(OA.SEEDS, top_first=3, geo=5)
# opd_m, strehl, rms_nm: tests/test_gpu_parity.py; signal, obs, reward: what tests/test_gpu_fov_sweep.py holds these cases to
TOL = {"f32": dict(F32_TOL),
       "f64": dict(F64_SAME_OPERATOR_TOL, **{k: F64_SAME_OPERATOR_TOL_FULL[k] for k in ("signal", "obs", "reward_rel")})}


def _np(t):
    return t.detach().cpu().numpy()


def _geo(name, **kw):
    if name == "pyr":
        g = V._pyr_geo()
        g.update(kw)
        return g
    return F.geo("two" if name == "geo" else name, **kw)


def _make(name, dtype, n=N, opts=None, **kw):
    from rlao_amd import _lib as L
    from rlao_amd.env import BatchedAOEnv
    env = BatchedAOEnv(n_envs=n, device=0, dtype=dtype, env_seed_stride=STRIDE)
    try:
        extra = dict(is_geometric=True) if name == "geo" else {}
        env.set_params(_geo(name, **kw), camera="ideal", wfs_type="pyramid" if name == "pyr" else "shackhartmann", **extra)
        for k, v in (opts or {}).items():
            L.check(env._shard.lib.aoenv_set_option(env._shard.h, getattr(L, k), v))
    except Exception:
        env.close()
        raise
    return env


def _direct(env, name, ids=range(N)):
    d = np.array([DIRS[name][k] for k in ids])
    env.set_guide_direction(d[:, 0], d[:, 1])
    return d


_prologue, _buf = OA._prologue, OA._buf


def _signal(env):
    from rlao_amd import _lib as L
    return env._shard.download(L.B_SIGNAL, (env.n_envs, env.nSignal), env._stream())


# ---- 1. parity ------------------------------------------------------------------------------------------------------------------------
_BASES, _RUNS = {}, {}


def _base(name, env):
    if name not in _BASES:
        g = _geo(name)
        if name == "geo":
            _BASES[name] = GEOT._oracle_for(env, g)
        else:
            kw = dict(wfs_type="pyramid", modulation=g["modulation"], psf_centering=g["psfCentering"]) if name == "pyr" else {}
            _BASES[name] = F.build_oracle(g, env.M2C_CL, V._operators(env), **kw)
    return _BASES[name]


def guided_copies(base, name, g, m2c, modal_cm, variant=None):
    """One deep copy of `base` per env of the case with the controller (m2c, modal_cm) and the env's guide star (the closure of
    tests/_guide_ref.py is bound to the copy: it is attached after the copy is made)."""
    out = []
    for k in range(N):
        o = copy.deepcopy(base, memo={id(x): x for x in (base.dm_modes, base.imat) if x is not None})
        if m2c is not None:
            o.M2C = np.asarray(m2c, dtype=np.float64)
            o.modal_cm = np.asarray(modal_cm, dtype=np.float64)
            o.reconstructor = o.M2C @ o.modal_cm
        R.guide(o, g["altitude"], *DIRS[name][k], variant=variant)
        out.append(o)
    return out


def _oracle_run(name, env):
    """N guided oracles (seeds seed + 100 k), one closed-loop episode with float32 actions from their own observations; per step
    what the sensor's line of sight gives, and the residual toward an on-axis target behind the same mirror (test 4)."""
    if name in _RUNS:
        return _RUNS[name]
    g = _geo(name)
    orcs = guided_copies(_base(name, env), name, g, env.M2C_CL, env.modal_CM)
    keys = ("opd_atm", "opd_res", "signal", "obs", "reward", "strehl", "rms", "axis_atm", "axis_res", "axis_rms", "axis_strehl")
    rec = dict(seed=SEEDS[name], actions=[], modal_cm=np.array(env.modal_CM), **{q: [] for q in keys})
    for k, o in enumerate(orcs):
        o.new_episode(SEEDS[name] + STRIDE * k)
    obs = np.stack([o.reset_soft() for o in orcs])
    rec["obs0"] = obs
    rs = np.random.RandomState(9)
    for i in range(STEPS):
        act = (GAIN * obs + 0.05 * rs.randn(*obs.shape)).astype(np.float32) * orcs[0].dm_mask[None].astype(np.float32)
        row = {q: [] for q in keys}
        for k, o in enumerate(orcs):
            dm = o.dm_opd(o.coefs)                                 # the surface this step's measurement sees
            oo, _, orw, osr, _, _ = o.step(i, act[k])
            axis = X.science_opd(o.atm, g["altitude"], 0.0, 0.0)
            a_opd, _, a_rms, a_sr = X.science_residual(axis, dm, o.pupil, o.wavelength)
            for q, v in zip(keys, (o.atm.OPD_no_pupil, o.tel_OPD, o.wfs.signal, oo, orw, osr, o.residual[i], axis, a_opd, a_rms, a_sr)):
                row[q].append(np.array(v, dtype=np.float64, copy=True))
        for q, v in row.items():
            rec[q].append(np.stack(v))
        rec["actions"].append(act)
        obs = rec["obs"][-1]
    _RUNS[name] = rec
    return rec


PARITY = [(n, d) for n in CASES for d in ("f32", "f64")]


@pytest.mark.parametrize("name,dtype", PARITY, ids=[f"{n}-{d}" for n, d in PARITY])
def test_the_loop_sees_the_guide_stars_line_of_sight(name, dtype):
    import torch
    from rlao_amd import _lib as L
    tol, label = dict(TOL[dtype]), f"guide-{name}-{dtype}"
    env = _make(name, dtype)
    try:
        rec = _oracle_run(name, env)
        G._same_controller(env, rec)
        if name == "geo":                                           # (tests/test_gpu_geometric.py: the slopes' bound from the OPD's)
            tol["signal"] = GEOT._sig_bound(env, dtype)
            tol["obs"] = float(np.abs(np.asarray(env.reconstructor)).sum(axis=1).max() * 1e6 * tol["signal"])
        assert env.fused_step == (name == "up70" and dtype == "f32")
        d = _direct(env, name)
        assert not env.fused_step
        assert np.array_equal(env.guide_direction, d) and np.array_equal(env.ngs.coordinates, d) and env.source is env.ngs
        obs0 = _np(_prologue(env, rec["seed"]))
        k_opd = env.src_wavelength / (2 * np.pi)
        for k in range(N):
            _close(obs0[k], rec["obs0"][k], "obs", tol, label, err_msg=f"obs after reset env {k}")
        for i in range(STEPS):
            obs, _, rew, sr = (_np(t) for t in env.step(i, torch.as_tensor(rec["actions"][i]))[:4])
            sig, phase, atm = _signal(env), _buf(env, L.B_PHASE), _buf(env, L.B_OPD_ATM)
            res = np.asarray(env.residual)[i]
            for k in range(N):
                what = f"step {i} env {k}"
                _close(atm[k], rec["opd_atm"][i][k], "opd_m", tol, label, err_msg="AOENV_B_OPD_ATM " + what)
                _close(phase[k] * k_opd, rec["opd_res"][i][k], "opd_m", tol, label, err_msg="phase " + what)
                _close(sig[k], rec["signal"][i][k], "signal", tol, label, err_msg="signal " + what)
                _close(obs[k], rec["obs"][i][k], "obs", tol, label, err_msg="obs " + what)
                G._reward(rew[k], rec["reward"][i][k], tol, label)
                _close(sr[k], rec["strehl"][i][k], "strehl", tol, label, err_msg="strehl " + what)
                _close(res[k], rec["rms"][i][k], "rms_nm", tol, label, err_msg="residual rms " + what)
    finally:
        env.close()


# ---- 2. zenith 0 ----------------------------------------------------------------------------------------------------------------------
ZERO = [("up70", "f32"), ("two", "f32"), ("p5_shared", "f32"), ("two", "f64")]


def _walk(env, seed, steps=4, actions=None):
    """steps closed-loop steps (action = 0.5 obs, or the given ones); per step the log of V._steps plus the phase and atmosphere
    buffers, then V._final"""
    from rlao_amd import _lib as L
    log, obs = [], _prologue(env, seed)
    for i in range(steps):
        row = []
        if actions is None:
            obs = V._steps(env, obs, i, 1, row)
        else:
            env.step(i, actions[i])
            row.append((_signal(env),))
        log.append(row[0] + (_buf(env, L.B_PHASE), _buf(env, L.B_OPD_ATM)))
    return log, V._final(env)


@pytest.mark.parametrize("name,dtype", ZERO, ids=[f"{n}-{d}" for n, d in ZERO])
def test_zenith_zero_is_the_axis_bit_for_bit(name, dtype):
    """Every env at zenith 0 (any azimuth): k_guide_opd computes the footprint, skips the blend, and the phase kernel on its OPD
    gives what the batched kernels give from the screens -- every step output, buffer, screen, clock and telemetry row."""
    env, twin = _make(name, dtype), _make(name, dtype, opts=dict(OPT_FUSED_STEP=0))
    try:
        env.set_guide_direction(0.0, np.array([0.0, 90.0, 225.0, 30.0]))
        assert not env.fused_step and not twin.fused_step
        (la, fa), (lb, fb) = _walk(env, 7), _walk(twin, 7)
        assert np.abs(la[-1][-1]).max() > 0
        V._same_log(la, lb)
        V._same_final(fa, fb)
    finally:
        env.close()
        twin.close()


# ---- 3. the two kernels agree -----------------------------------------------------------------------------------------------------------
AGREE = [("two", "f32"), ("two", "f64"), ("top_first", "f32"), ("up70", "f32")]


@pytest.mark.parametrize("name,dtype", AGREE, ids=[f"{n}-{d}" for n, d in AGREE])
def test_science_and_guide_kernels_agree_bit_for_bit(name, dtype):
    """The science direction set equal to the guide direction (blending envs included): k_science_residual's opd_atm_sci is
    k_guide_opd's AOENV_B_OPD_ATM, and phase_sci is AOENV_B_PHASE."""
    from rlao_amd import _lib as L
    env = _make(name, dtype)
    try:
        d = _direct(env, name)
        env.set_science_direction(d[:, 0], d[:, 1])
        obs = _prologue(env, 7)
        for i in range(3):
            obs = env.step(i, GAIN * obs)[0]
            phase = _np(env.science_residual()[0])
            opd = _np(env.science_atmosphere())
            assert np.abs(opd).max() > 0 and np.abs(phase).max() > 0
            assert np.array_equal(opd, _buf(env, L.B_OPD_ATM)), i
            assert np.array_equal(phase, _buf(env, L.B_PHASE)), i
    finally:
        env.close()


# ---- 4. off-axis sensor, on-axis target ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_off_axis_sensor_on_axis_target(dtype):
    """`two`: guide direction off axis, science direction zenith 0 -- classical anisoplanatism.  science_atmosphere() is bit for bit
    the AOENV_B_OPD_ATM of an unguided twin with the same seed and actions on the batched path; science_residual() against the
    restatement on the guided oracle's layers and mirror."""
    import torch
    from rlao_amd import _lib as L
    tol, label = TOL[dtype], f"guide-axis-target-{dtype}"
    env, twin = _make("two", dtype), _make("two", dtype, opts=dict(OPT_FUSED_STEP=0))
    try:
        rec = _oracle_run("two", env)
        G._same_controller(env, rec)
        _direct(env, "two")
        env.set_science_direction(0.0, 0.0)
        _prologue(env, rec["seed"])
        _prologue(twin, rec["seed"])
        k_opd = env.src_wavelength / (2 * np.pi)
        for i in range(STEPS):
            act = torch.as_tensor(rec["actions"][i])
            env.step(i, act)
            twin.step(i, act)
            phase, rms, sr = (_np(t) for t in env.science_residual())
            opd = _np(env.science_atmosphere())
            assert np.array_equal(opd, _buf(twin, L.B_OPD_ATM)), i
            assert not np.array_equal(opd[0], _buf(env, L.B_OPD_ATM)[0])
            for k in range(N):
                what = f"step {i} env {k}"
                _close(opd[k], rec["axis_atm"][i][k], "opd_m", tol, label, err_msg="opd_atm_sci " + what)
                _close(phase[k] * k_opd, rec["axis_res"][i][k], "opd_m", tol, label, err_msg="phase_sci " + what)
                _close(rms[k], rec["axis_rms"][i][k], "rms_nm", tol, label, err_msg="rms " + what)
                _close(sr[k], rec["axis_strehl"][i][k], "strehl", tol, label, err_msg="strehl " + what)
    finally:
        env.close()
        twin.close()


# ---- 5. place invariance ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["two", "up70"])
def test_an_env_has_the_same_bits_in_any_shard_and_at_any_place(name):
    """float32: env k of the mixed shard == the only env of a one-env shard with its seed and direction, and env 0 == env 0 of a
    two-env shard in which both envs have its direction."""
    env = _make(name, "f32")
    try:
        _direct(env, name)
        whole, _ = _walk(env, 11)
    finally:
        env.close()
    for k in (1, 3):
        one = _make(name, "f32", n=1)
        try:
            _direct(one, name, [k])
            got, _ = _walk(one, 11 + STRIDE * k)
        finally:
            one.close()
        V._same_log(got, whole, [0], [k])
    both = _make(name, "f32", n=2)
    try:
        _direct(both, name, [0, 0])
        got, _ = _walk(both, 11)
        V._same_log(got, whole, [0], [0])
    finally:
        both.close()


# ---- 6. every loop equals per-call stepping ------------------------------------------------------------------------------------------------
LOOPS = ("run_integrator", "run_integrator_delay", "rollout", "policy_rollout", "run_integrator_modal")
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


def _attach(env, loop):
    """what both shards of the comparison carry: photon noise, the direction, a wavefront record of the atmosphere, a long exposure"""
    name = "run_integrator" if loop == "run_integrator_delay" else loop
    S._configure(env, name)
    if loop == "run_integrator_delay":
        env.set_delay(1)
    _direct(env, "up70")
    env.set_wavefront_basis(opd2m=np.linalg.pinv(OA._m2opd(env)))
    env.set_science(zero_padding=2, window=8, first_frame=2)
    obs = S._start(env, name)
    env.record_wavefront(0, S.STEPS, what=("residual", "atmosphere"))
    env.start_long_exposure()
    return obs


def _loop_state(env):
    out = S._everything(env, [])
    # (what a loop and the per-call API keep differently: the retained observation, the exploration noise's seed and counter)
    for k in ("state.obs", "state.counters", "state.explore_seed"):
        out.pop(k)
    out["wf"], out["le"] = _np(env._wf_rec).copy(), [_np(t).copy() for t in env._le if t is not None]
    return out


@pytest.mark.parametrize("dtype,loop", LOOP_CASES, ids=[f"{d}-{l}" for d, l in LOOP_CASES])
def test_every_loop_equals_per_call_stepping(dtype, loop):
    """8 frames of `up70` under four guide directions with photon noise, a wavefront record (residual and atmosphere) and a long
    exposure attached: the on-device loop's final outputs, buffers, get_state(), record and long exposure are bit for bit those of
    a twin that takes the same frames through the per-call API."""
    import torch
    name = "run_integrator" if loop == "run_integrator_delay" else loop
    modal = loop == "run_integrator_modal"
    env, twin = _loop_env(dtype, "a"), _loop_env(dtype, "b")
    try:
        obs = _attach(env, loop)
        assert not env.fused_step
        handed, actions = S._run_loop(env, name, obs)
        torch.cuda.synchronize()
        got = _loop_state(env)
        obs_t = _attach(twin, loop)
        for k in range(S.STEPS):
            if modal:
                last = twin.step_modal(k, GAIN * obs_t)
            elif actions is not None:
                last = twin.step(k, actions[k])
            else:
                last = twin.step(k, GAIN * obs_t)
            obs_t = last[0]
        torch.cuda.synchronize()
        want = _loop_state(twin)
        assert got.keys() == want.keys()
        for k in want:
            S._same(got[k], want[k], k)
        assert np.abs(got["wf"]).max() > 0 and not np.array_equal(got["wf"][:, 0], got["wf"][:, 1])
        if not modal and actions is None:                           # run_integrator: (obs, reward, Strehl) of the last frame
            for a, b in zip(handed, (last[0], last[2], last[3])):
                assert np.array_equal(_np(a), _np(b))
    finally:
        for e in (env, twin):
            e.stop_wavefront_record()
            e.stop_long_exposure()
            e.clear_guide_direction()
            e.clear_science()
            e.clear_wavefront_basis()
            if loop == "policy_rollout":
                e.set_policy(None)


# ---- 7. composition ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_composed_with_per_env_winds_r0_and_mirrors(dtype):
    """`up70` with every env its own wind (env 3: 1.5 pixels per frame, a whole-pixel ring round in every step), Fried parameter,
    mis-registered mirror and guide direction: against one guided oracle per env (tests/_compose_ref.py plus tests/_guide_ref.py)."""
    import torch
    import _compose_ref as CR
    from rlao_amd import _lib as L
    C = OA.COMPOSED
    tol, label = TOL[dtype], f"guide-composed-{dtype}"
    env = _make("up70", dtype)
    try:
        g = _geo("up70")
        specs = [CR.env_spec(seed=9 + STRIDE * e, r0=C["r0"][e], wind_speed=[C["wind_speed"][e]], wind_dir=[C["wind_dir"][e]],
                             misreg=C["misreg"][e] or None) for e in range(N)]
        orc = CR.ComposedOracle(_base("up70", env), specs, m2c=env.M2C_CL, modal_cm=env.modal_CM)
        for e, o in enumerate(orc.envs):
            R.guide(o, g["altitude"], *DIRS["up70"][e])
        env.set_r0_per_env(np.array(C["r0"]))
        env.set_dm_misregistration(**{k: np.array([m.get(k, 0.0) for m in C["misreg"]]) for k in CR.MISREG_KEYS})
        _direct(env, "up70")
        env.generate_new_phase_screen(9)
        env.set_wind_per_env(np.array(C["wind_speed"])[:, None], np.array(C["wind_dir"])[:, None], reset=True, max_pixels=2)
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
            want = orc.step(i, act)
            obs = want["obs"]
            got_obs, _, _, got_sr, _, _ = env.step(i, torch.as_tensor(act))
            sig, phase, atm = _signal(env), _buf(env, L.B_PHASE), _buf(env, L.B_OPD_ATM)
            for e, o in enumerate(orc.envs):
                what = f"step {i} env {e}"
                _close(atm[e], o.atm.OPD_no_pupil, "opd_m", tol, label, err_msg="AOENV_B_OPD_ATM " + what)
                _close(phase[e] * k_opd, o.tel_OPD, "opd_m", tol, label, err_msg="phase " + what)
                _close(sig[e], want["signal"][e], "signal", tol, label, err_msg="signal " + what)
                _close(_np(got_obs)[e], want["obs"][e], "obs", tol, label, err_msg="obs " + what)
                _close(_np(got_sr)[e], want["strehl"][e], "strehl", tol, label, err_msg="strehl " + what)
        assert orc.whole_rounds[3].max() >= 1                       # env 3 made whole-pixel rounds
    finally:
        env.close()


# ---- 8. off is off ------------------------------------------------------------------------------------------------------------------------
def test_launch_counts_and_the_fused_path():
    """float32 `up70`: without a direction -- never set, or set and cleared -- 8 steps of run_integrator launch the same kernels
    (counted, not timed) on the fused path; under a direction the fused kernel is not launched and the phase kernel runs once per
    step."""
    a, b = _loop_env("f32", "a"), _loop_env("f32", "b")
    counts = []
    for env, mode in ((a, "never"), (b, "cleared"), (b, "set")):
        assert env.fused_step
        if mode != "never":
            _direct(env, "up70")
            assert not env.fused_step
        if mode == "cleared":
            env.clear_guide_direction()
            assert env.fused_step and env.guide_direction is None and not env.ngs.coordinates.any()
        _prologue(env, 5)
        env._shard.profile(True)
        env.run_integrator(0, 8)
        prof = env._shard.profile_read(env._stream())
        counts.append(({k: v[1] for k, v in prof.items()}, env._shard.step_counters()))
        env._shard.profile(False)
        env.clear_guide_direction()
    assert counts[0] == counts[1]
    assert counts[0][1][1] == 8 and counts[0][0]["env_step"] >= 1
    assert counts[2][0].get("env_step", 0) == 0 and counts[2][0]["phase"] == 8 and tuple(counts[2][1]) == (0, 0)


def test_refusals_and_a_cleared_direction_leave_no_trace():
    """`up70`, float32 (fused): what is refused is refused before a launch and changes nothing; a cleared shard and a shard that
    only saw refused calls step on bit-identical to an untouched one, on the fused path."""
    from rlao_amd import _lib as L
    from rlao_amd.env import BatchedAOEnv
    cleared, refused, plain = (_make("up70", "f32") for _ in range(3))
    try:
        d = _direct(cleared, "up70")
        for env, had in ((cleared, True), (refused, False)):
            for bad in (5.0001, -0.1, np.inf, np.nan):
                with pytest.raises(ValueError):
                    env.set_guide_direction(bad, 0.0, env_ids=[1])
            zen = np.array([5.0, 5.0, 5.5, 5.0])                     # past the Python layer: the library's own checks
            with pytest.raises(L.AoEnvError, match="above fov / 2"):
                L.call(env._shard, "aoenv_set_guide_direction", zen, np.zeros(4), env._stream())
            with pytest.raises(L.AoEnvError, match="not finite"):
                L.call(env._shard, "aoenv_set_guide_direction", np.array([1.0, np.nan, 1.0, 1.0]), np.zeros(4), env._stream())
            with pytest.raises(L.AoEnvError, match="not finite"):
                L.call(env._shard, "aoenv_set_guide_direction", np.ones(4), np.array([0.0, 0.0, np.nan, 0.0]), env._stream())
            with pytest.raises(L.AoEnvError, match="one of the two arrays is null"):
                L.call(env._shard, "aoenv_set_guide_direction", np.ones(4), None, env._stream())
            if had:
                assert np.array_equal(env.guide_direction, d) and not env.fused_step
                p = env.param
                with pytest.raises(L.AoEnvError, match="a guide direction is set"):
                    L.call(env._shard, "aoenv_set_field", float(p.diameter), float(p.fov), np.ascontiguousarray(p.altitude, dtype=np.float64))
                with pytest.raises(L.AoEnvError, match="no guide direction"):
                    L.call(refused._shard, "aoenv_get_guide_direction", np.zeros(4), np.zeros(4))
            else:
                assert env.guide_direction is None and env.fused_step
        cleared.clear_guide_direction()
        assert cleared.guide_direction is None and cleared.fused_step
        logs = []
        for env in (cleared, refused, plain):
            log = []
            V._steps(env, _prologue(env, 13), 0, 4, log)
            logs.append((log, V._final(env)))
        for log, fin in logs[:2]:
            V._same_log(log, logs[2][0])
            V._same_final(fin, logs[2][1])
    finally:
        for env in (cleared, refused, plain):
            env.close()
    flat = BatchedAOEnv(n_envs=2, device=0, dtype="f32")                # no layers above the ground and no field of view: zenith 0 alone
    try:
        flat.set_params(S.R24, camera="ideal", wfs_type="shackhartmann")
        with pytest.raises(ValueError, match="zenith"):
            flat.set_guide_direction(0.4)
        flat.set_guide_direction(0.0, 45.0)
        assert not flat.fused_step
        cal = flat._make_shard(1, "f32", n_layer=0, max_group=1)      # a shard without layers
        try:
            with pytest.raises(L.AoEnvError, match="no layers"):
                L.call(cal, "aoenv_set_guide_direction", np.zeros(1), np.zeros(1), 0)
        finally:
            cal.close()
    finally:
        flat.close()


def test_a_user_defined_opd_wins_until_the_atmosphere_advances():
    """`two`, float32: after set_atm_opd the measurement sees the given OPD, not the guide star's; the next step looks through the
    layers toward the star again."""
    from rlao_amd import _lib as L
    env, twin = _make("two", "f32"), _make("two", "f32")
    try:
        _direct(env, "two")
        oe, ot = _prologue(env, 3), _prologue(twin, 3)
        given = np.zeros((N, env.R * env.R))
        for e in (env, twin):
            e._shard.set_atm_opd(given)
            e.measure()
        assert np.array_equal(_signal(env), _signal(twin)) and np.array_equal(_buf(env, L.B_PHASE), _buf(twin, L.B_PHASE))
        env.step(0, GAIN * oe)
        twin.step(0, GAIN * ot)
        assert not np.array_equal(_buf(env, L.B_OPD_ATM)[0], _buf(twin, L.B_OPD_ATM)[0])      # env 0: 10 arcsec off axis
        assert np.array_equal(_buf(env, L.B_OPD_ATM)[2], _buf(twin, L.B_OPD_ATM)[2])          # env 2: zenith 0
    finally:
        env.close()
        twin.close()
