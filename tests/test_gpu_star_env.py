"""GPU: every env of a shard its own guide star and centroid threshold (aoenv_set_flux_env / aoenv_set_threshold_env;
BatchedAOEnv.set_magnitude_per_env / set_threshold_per_env).

The checker of the flux is the path of before the feature: a TWIN shard of the same size, seeds and calibration whose SHARED
amplitude table was replaced, after set_params, through shard.upload(C_WFS_AMP, T(amp) * T(a_e)) -- the product formed in NumPy in
the env dtype, a_e = sqrt(flux_scale(m_e, m_cal)) rounded once.  The kernels multiply the loaded amplitude by the env's factor in a
statement of its own, so row e of the mixed shard must be BIT-IDENTICAL to row e of twin e on every kernel that loads the amplitude.
The threshold has no table to replace: a mixed shard is compared with uniform shards set through the same call (bit-identical), and
its slopes with the oracle's centroiding run on the device's own frame at thr_e (tests/test_gpu_camera_streams.py).  Beside that:
off is off, a shard built at the env's magnitude, the camera count for count, the loops and the refusals.

The envs: magnitudes m_cal, m_cal - 2.5, m_cal + 1, m_cal + 4; thresholds cfg, 0, 0.05, 0.2."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import _camera_ref as R
from test_gpu_camera_streams import _oracle_sh_signal
from test_gpu_parity import F32_TOL, F64_SAME_OPERATOR_TOL_FULL

pytestmark = pytest.mark.gpu

SMALL = dict(diameter=3.2, nSubaperture=8, nPixelPerSubap=6, r0=0.13, L0=30.0, windSpeed=[10.0], windDirection=[72.0],
             fractionalR0=[1.0], altitude=[0.0], nModes=20, nLoop=64)                      # tests/test_gpu_dm_env.py
PX4 = dict(SMALL, nPixelPerSubap=4)
PX8 = dict(SMALL, nPixelPerSubap=8)
TINY_PYR = dict(diameter=1.6, nSubaperture=4, nPixelPerSubap=6, r0=0.13, L0=30.0, windSpeed=[10.0], windDirection=[72.0],
                fractionalR0=[1.0], altitude=[0.0], nModes=8, nLoop=64, modulation=0.0)    # the 4 x 4 geometry
GAIN = 0.5
STEPS = 14
D_MAG = np.array([0.0, -2.5, 1.0, 4.0])
THR = [None, 0.0, 0.05, 0.2]                                       # None: param.threshold_cog


def _pyr_geo(name):
    from test_gpu_pyramid_sweep import _geo                        # the smallest cases of the sweep that reach nRes 288 / 528
    return _geo(name)


# case: (geometry, dtype, options, wfs, n_envs, steps, fused step expected)
CASES = {
    "fused": (lambda: SMALL, "f32", {}, "shackhartmann", 4, STEPS, True),
    "sh6_f64": (lambda: SMALL, "f64", {}, "shackhartmann", 4, STEPS, False),
    "p6_tail": (lambda: SMALL, "f32", {"OPT_FUSED_STEP": 0}, "shackhartmann", 4, STEPS, False),
    "p6_centroid": (lambda: SMALL, "f32", {"OPT_FUSED_STEP": 0, "OPT_FUSED_TAIL": 0}, "shackhartmann", 4, STEPS, False),
    "px4": (lambda: PX4, "f32", {}, "shackhartmann", 4, STEPS, False),
    "px8": (lambda: PX8, "f32", {}, "shackhartmann", 4, STEPS, False),
    "px4_f64": (lambda: PX4, "f64", {}, "shackhartmann", 4, STEPS, False),
    "pyramid": (lambda: TINY_PYR, "f32", {}, "pyramid", 4, STEPS, False),
    "pyramid_f64": (lambda: TINY_PYR, "f64", {}, "pyramid", 4, STEPS, False),
    "pyr288": (lambda: _pyr_geo("f288a"), "f32", {}, "pyramid", 4, 3, False),
    "pyr528": (lambda: _pyr_geo("f528a"), "f32", {}, "pyramid", 4, 3, False),
}
KERNELS = {
    "fused": "k_env_step_sh6<.., STEP_STAR> (the amplitude behind the pupil test, the cut)",
    "sh6_f64": "k_sh_spots_p6<double> and k_sh_tail<double>",
    "p6_tail": "k_sh_spots_p6<float> (register pairs) and k_sh_tail<float>",
    "p6_centroid": "k_sh_spots_p6<float> and k_sh_centroid<float> (FUSED_TAIL = 0)",
    "px4": "k_sh_spots<float> at 4 px per lenslet, k_sh_tail",
    "px8": "k_sh_spots<float> at 8 px per lenslet, k_sh_tail",
    "px4_f64": "k_sh_spots<double>, k_sh_tail<double>",
    "pyramid": "k_pyr_rows<float> (the generic Pyramid, nRes 96)",
    "pyramid_f64": "k_pyr_rows<double>",
    "pyr288": "k_pyr528_rows at nRes 288",
    "pyr528": "k_pyr528_rows at nRes 528",
}


def _make(case, n_envs=None, **geo_kw):
    from rlao_amd import _lib as L
    from rlao_amd.env import BatchedAOEnv
    geo, dtype, opts, wfs, n, _, fused = CASES[case]
    env = BatchedAOEnv(n_envs=n_envs or n, device=0, dtype=dtype)
    try:
        env.set_params(dict(geo(), **geo_kw), camera="ideal", wfs_type=wfs)
        for k, v in opts.items():
            L.check(env._shard.lib.aoenv_set_option(env._shard.h, getattr(L, k), v))
        assert env.fused_step == fused, case
        env._counters0 = env._shard.download(L.B_COUNTERS, (4,), env._stream(), dtype=np.uint32).copy()
    except Exception:
        env.close()
        raise
    return env


def _dt(env):
    return np.float32 if env.dtype == "f32" else np.float64


def _mags(env):
    return float(env.param.magnitude) + D_MAG[:env.n_envs]


def _thrs(env):
    return np.array([float(env.param.threshold_cog) if t is None else t for t in THR[:env.n_envs]])


def _factors(env, mags):
    """a_e in the env dtype, formed here from the magnitudes alone"""
    from rlao_amd import calib
    return np.sqrt(calib.flux_scale(mags, env.param.magnitude)).astype(_dt(env))


def _calibrated_amp(env):
    return np.asarray(env._sh_tables.amp if env.wfs_type == "sh" else env._pyr_tables.amplitude(env._wfs_n_theta), dtype=np.float64)


def _as_twin(env, a_e):
    """the path of before the feature: ONE amplitude table for the shard, through aoenv_upload"""
    from rlao_amd import _lib as L
    dt = _dt(env)
    table = _calibrated_amp(env).astype(dt) * dt(a_e)
    assert table.dtype == dt
    env._shard.upload(L.C_WFS_AMP, table.astype(np.float64))


def _start(env, seed):
    from rlao_amd import _lib as L
    env._shard.upload_state(L.B_COUNTERS, env._counters0, env._stream(), dtype=np.uint32)   # the camera's frame number: every episode from one
    env.generate_new_phase_screen(seed)
    env.dm.coefs = 0
    env.dm_prev = 0
    env.measure()
    return env.reset_soft()


def _buffers(env):
    from rlao_amd import _lib as L
    sh, n, st = env._shard, env.n_envs, env._stream()
    return [sh.download(L.B_PHASE, (n, env.R, env.R), st), sh.download(L.B_FRAME, (n, env.cam_res, env.cam_res), st),
            sh.download(L.B_WFS_MAX, (n,), st), sh.download(L.B_SIGNAL, (n, env.nSignal), st)]


def _episode(env, steps, seed, obs=None, i0=0):
    """closed-loop integrator steps; per step obs, reward, strehl, frame and the phase / frame / wfs_max / signal buffers"""
    if obs is None:
        obs = _start(env, seed)
    out = [[obs.cpu().numpy()]]
    for i in range(i0, i0 + steps):
        obs, frame, rew, sr, _, _ = env.step(i, GAIN * obs)
        out.append([obs.cpu().numpy(), rew.cpu().numpy(), sr.cpu().numpy(), frame.cpu().numpy()] + _buffers(env))
    out.append([np.asarray(env.residual).reshape(-1, env.n_envs)[:i0 + steps], np.asarray(env.total).reshape(-1, env.n_envs)[:i0 + steps]])
    return out, obs


def _same_row(got, want, e, what=""):
    assert len(got) == len(want)
    for k, (a, b) in enumerate(zip(got, want)):
        last = k == len(got) - 1
        for q, (x, y) in enumerate(zip(a, b)):
            x, y = (x[:, e], y[:, e]) if last else (x[e], y[e])      # (the telemetry is [step, env])
            assert x.dtype == y.dtype and np.array_equal(x, y), (what, "env", e, "record", k, "quantity", q, float(np.abs(x.astype(np.float64) - y).max()))


# ---- 1. twins ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("camera", ["ideal", "photon"])
@pytest.mark.parametrize("case", list(CASES))
def test_each_env_equals_the_twin_with_its_amplitude_table(case, camera):
    """Row e of obs, reward, strehl, the frame, AOENV_B_PHASE, _FRAME, _WFS_MAX, _SIGNAL and the telemetry of the mixed shard == row
    e of twin e, every step, bit for bit.  The kernel of each case: KERNELS[case]."""
    steps, seed = CASES[case][5], 31
    env = _make(case)
    try:
        mags = _mags(env)
        a = _factors(env, mags)
        assert a[0] == 1 and len(set(a.tolist())) == env.n_envs
        env.wfs.cam.photonNoise = camera == "photon"
        env.set_magnitude_per_env(mags)
        held = env._shard.get_flux_env(env._stream())
        assert np.array_equal(held, a.astype(np.float64))           # the host's factors are the ones formed here
        assert env.fused_step == CASES[case][6]
        got, _ = _episode(env, steps, seed)
    finally:
        env.close()
    twin = _make(case)
    try:
        twin.wfs.cam.photonNoise = camera == "photon"
        for e in range(twin.n_envs):
            _as_twin(twin, a[e])
            want, _ = _episode(twin, steps, seed)
            _same_row(got, want, e, what=KERNELS[case])
            if e == 0:
                calibrated = want[-2][5]                            # every env at the calibrated star
    finally:
        twin.close()
    frames = got[-2][5]                                             # AOENV_B_FRAME of the last step
    assert all(not np.array_equal(frames[e], calibrated[e]) for e in range(1, len(a)))     # the stars really differ
    assert all(np.isfinite(r[0]).all() for r in got[:-1])
    if camera == "photon":
        assert (frames == np.floor(frames)).all()


# ---- 2. threshold -----------------------------------------------------------------------------------------------------------------
THRESHOLD_CASES = ["fused", "p6_tail", "p6_centroid", "sh6_f64"]


@pytest.mark.parametrize("case", THRESHOLD_CASES)
def test_mixed_thresholds_equal_uniform_shards_and_the_oracle(case):
    """A mixed shard against the same shard set to ONE value through the same call: row e bit-identical.  And the slopes of env e
    == the oracle's centroiding (oracle.ao_oracle.OracleSH.measure, as tests/test_gpu_camera_streams.py runs it) on the device's own
    frame with thr_e, within the signal bound that file uses.  Precondition, from the frame and the oracle's arithmetic alone: no
    pixel within 1e-6 relative of any env's cut."""
    from rlao_amd import _lib as L
    steps, seed = 6, 31
    env = _make(case)
    try:
        thr = _thrs(env)
        mags = _mags(env)
        env.set_magnitude_per_env(mags)
        env.set_threshold_per_env(thr)
        assert np.array_equal(env._shard.get_threshold_env(env._stream()), thr.astype(_dt(env)).astype(np.float64))
        assert env.fused_step == CASES[case][6]
        got, _ = _episode(env, steps, seed)
        tol = F32_TOL if env.dtype == "f32" else F64_SAME_OPERATOR_TOL_FULL
        frame = got[-2][5].astype(np.float64)
        signal = got[-2][7].astype(np.float64)
        worst = 0.0
        for e in range(env.n_envs):
            env.param.threshold_cog, keep = float(thr[e]), env.param.threshold_cog
            try:
                want, mx = _oracle_sh_signal(env, frame[e])
            finally:
                env.param.threshold_cog = keep
            for t in thr:                                           # the precondition: the oracle's frame alone
                cut = t * mx
                lit = frame[e][frame[e] > 0]
                assert cut == 0 or np.abs(lit - cut).min() > 1e-6 * cut, (e, t)
            err = float(np.abs(signal[e] - want).max())
            worst = max(worst, err)
            print(f"{case} env {e} thr {thr[e]}: max |signal - oracle| = {err:.3e} (bound {tol['signal']:.1e})")
            np.testing.assert_allclose(signal[e], want, rtol=0, atol=tol["signal"], err_msg=f"{case} env {e}")
        # the thresholds bite: env 3 (0.2) drops pixels env 1 (0) keeps
        assert ((frame[3] > 0) & (frame[3] < thr[3] * frame[3].max())).sum() >= 8
        for e in range(env.n_envs):
            env.set_threshold_per_env(float(thr[e]))                # uniform, through the same call
            want_u, _ = _episode(env, steps, seed)
            _same_row(got, want_u, e, what="uniform " + KERNELS[case])
        sig_u = want_u[-2][7]
        assert not np.array_equal(sig_u[0], got[-2][7][0])          # (env 0 at 0.2 is not env 0 at cfg)
    finally:
        env.close()


# ---- 3. off is off ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["fused", "p6_tail", "pyramid"])
def test_off_is_off(case):
    """Every env at the calibrated star and the cfg threshold through the API, a cleared shard, and a loop around refused calls all
    run bit-identical to an untouched shard; aoenv_fused_step_active keeps its value with the feature on."""
    steps, seed = 8, 5
    sh = CASES[case][3] == "shackhartmann"
    ref = _make(case)
    try:
        want, _ = _episode(ref, steps, seed)
    finally:
        ref.close()
    env = _make(case)
    try:
        n = env.n_envs
        env.set_magnitude_per_env(env.param.magnitude)
        if sh:
            env.set_threshold_per_env(np.full(n, env.param.threshold_cog))
        assert (env._shard.get_flux_env(env._stream()) == 1).all() and env.fused_step == CASES[case][6]
        got, _ = _episode(env, steps, seed)
        env.set_magnitude_per_env(_mags(env))
        moved, _ = _episode(env, 2, seed)
        env.clear_star_per_env()
        assert np.array_equal(env.magnitude, np.full(n, env.param.magnitude))
        lib, h, st = env._shard.lib, env._shard.h, C.c_void_p(env._stream())
        z = np.zeros(n)
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        assert lib.aoenv_get_flux_env(h, p(z), st) != 0 and b"one star" in lib.aoenv_last_error()      # absent, not ones
        assert lib.aoenv_get_threshold_env(h, p(z), st) != 0
        again, _ = _episode(env, steps, seed)
        obs = _start(env, seed)
        part1, obs = _episode(env, 4, seed, obs=obs)
        for bad, word in ((np.array([1.0, np.nan, 1, 1]), b"not finite"), (np.array([1.0, 0.0, 1, 1]), b"not above 0"),
                          (np.array([1.0, -2.0, 1, 1]), b"not above 0"), (np.array([np.inf, 1.0, 1, 1]), b"not finite")):
            assert lib.aoenv_set_flux_env(h, p(bad), st) != 0 and word in lib.aoenv_last_error()
        for bad, word in ((np.array([0.01, np.nan, 0, 0]), b"not finite"), (np.array([0.01, -0.1, 0, 0]), b"below 0")):
            assert lib.aoenv_set_threshold_env(h, p(bad), st) != 0 and (word in lib.aoenv_last_error() or not sh)
        if not sh:
            assert lib.aoenv_set_threshold_env(h, p(np.full(n, 0.01)), st) != 0 and b"Pyramid" in lib.aoenv_last_error()
        assert lib.aoenv_get_flux_env(h, p(z), st) != 0             # still absent
        part2, _ = _episode(env, 4, seed, obs=obs, i0=4)
    finally:
        env.close()
    for e in range(n):
        _same_row(got, want, e, what="calibrated star through the API")
        _same_row(again, want, e, what="after clear")
        _same_row(part1[:-1] + part2[1:], want, e, what="refused calls")
    assert not np.array_equal(moved[2][3][1], want[2][3][1]) and np.array_equal(moved[2][3][0], want[2][3][0])


def test_refusals_leave_the_arrays_in_force():
    """A refused call on a shard WITH per-env stars leaves them as they are (the getters return what was set); a shard with
    max_group > 1 refuses a per-env threshold and takes a per-env flux."""
    from rlao_amd import _lib as L
    env = _make("p6_tail")
    try:
        mags, thr = _mags(env), _thrs(env)
        env.set_magnitude_per_env(mags)
        env.set_threshold_per_env(thr)
        a0, t0 = env._shard.get_flux_env(), env._shard.get_threshold_env()
        with pytest.raises(L.AoEnvError, match="not above 0"):
            env._shard.set_flux_env(np.array([1.0, 2.0, 0.0, 1.0]))
        with pytest.raises(L.AoEnvError, match="below 0"):
            env._shard.set_threshold_env(np.array([0.0, 0.1, 0.2, -1e-9]))
        with pytest.raises(ValueError):
            env.set_magnitude_per_env([1.0, 2.0])
        assert np.array_equal(env._shard.get_flux_env(), a0) and np.array_equal(env._shard.get_threshold_env(), t0)
        assert np.array_equal(env.magnitude, mags) and np.array_equal(env.threshold_cog, thr)
        # partial calls: listed envs replaced, the others keep theirs
        env.set_magnitude_per_env([mags[0] + 2], env_ids=[2])
        env.wfs.threshold_cog = 0.03
        assert np.array_equal(env.magnitude, [mags[0], mags[1], mags[0] + 2, mags[3]]) and (env.wfs.threshold_cog == 0.03).all()
        assert env._shard.get_flux_env()[1] == a0[1] and env._shard.get_flux_env()[2] != a0[2]
        group = env._make_shard(4, "f32", n_layer=0, max_group=2)
        try:
            with pytest.raises(L.AoEnvError, match="max_group"):
                group.set_threshold_env(thr)
            group.set_flux_env(np.array([1.0, 2.0, 3.0, 4.0]))
            assert np.array_equal(group.get_flux_env(), np.sqrt([1.0, 2.0, 3.0, 4.0]).astype(np.float32).astype(np.float64))
            group.set_flux_env(None)
            with pytest.raises(L.AoEnvError, match="one star"):
                group.get_flux_env()
        finally:
            group.close()
    finally:
        env.close()


# ---- 4. against a shard built at that magnitude -----------------------------------------------------------------------------------
def test_frame_equals_a_shard_built_at_the_envs_magnitude():
    """float64, ideal camera, one measurement of the same screens: env e against set_params(magnitude = m_e).  The calibrated
    amplitude there is sqrt(fluxMap(m_e)) formed in one go, here sqrt(fluxMap(m_cal)) * a_e: a few units of 2^-52 apart, squared
    by the intensity -- the frames differ by less than 1e-13 of the peak."""
    from rlao_amd import _lib as L
    seed = 31
    env = _make("sh6_f64")
    try:
        mags = _mags(env)
        env.set_magnitude_per_env(mags)
        _start(env, seed)
        got = env._shard.download(L.B_FRAME, (env.n_envs, env.cam_res, env.cam_res), env._stream())
    finally:
        env.close()
    worst = 0.0
    for e in range(1, len(mags)):
        built = _make("sh6_f64", magnitude=float(mags[e]))
        try:
            _start(built, seed)
            want = built._shard.download(L.B_FRAME, (built.n_envs, built.cam_res, built.cam_res), built._stream())[e]
        finally:
            built.close()
        rel = float(np.abs(got[e] - want).max() / want.max())
        worst = max(worst, rel)
        print(f"env {e} magnitude {mags[e]}: max |frame - built| / peak = {rel:.3e}")
        assert rel < 1e-13, (e, rel)
        assert want.max() > 0
    out = os.environ.get("AO_PARITY_REPORT")
    if out:
        with open(out, "w") as f:
            f.write(json.dumps({"unit": "max |frame(env e of the mixed shard) - frame(shard built at magnitude m_e)| / peak, float64, 8 x 8 x 6 px",
                                "bound": 1e-13, "largest": worst}, indent=1) + "\n")


# ---- 5. the camera, count for count ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def table():
    from rlao_amd import _lib as L
    lib = L.load()
    n = C.c_size_t()
    L.check(lib.aoenv_test_poisson_table(None, 0, C.byref(n)))
    t = np.zeros(n.value, dtype=np.uint32)
    L.check(lib.aoenv_test_poisson_table(t.ctypes.data_as(C.c_void_p), t.size, C.byref(n)))
    return t


@pytest.mark.parametrize("case", ["fused", "p6_tail"])
def test_photon_frames_equal_their_restatement_per_env(case, table):
    """tests/_camera_ref.noisy_frame on the mixed shard's own ideal frames (a twin mixed shard with the ideal camera, driven by the
    same actions), per env index, against the noisy shard's frames: assert_flips at the cap that module grants the device.  Env 3
    (m_cal + 4) lies below the env's hand-over to PTRS (alias_lmax), env 1 (m_cal - 2.5, ten times the flux) has pixels above it:
    those are PTRS pixels and are held to the Poisson law.  fused: the camera block of k_env_step_sh6; p6_tail: k_detector_sh6."""
    import torch
    from scipy import stats
    from rlao_amd import _lib as L
    noisy_env, ideal_env = _make(case), _make(case)
    try:
        mags = _mags(noisy_env)
        cfg = R.CameraCfg.from_fields(noisy_env.param.samplingTime, seed=noisy_env.detector_seed, **R.SETTINGS["photon"])
        layout = R.layout_for(noisy_env.cam_res, noisy_env.param.nSubaperture, True)
        lmax = R.env_lmax(table, True, 6, noisy_env.R, noisy_env.nActuator)
        valid2d = noisy_env._sh_tables.valid_2d
        rs = np.random.RandomState(21)
        actions = [torch.as_tensor((0.05 * rs.randn(4, noisy_env.nActuator, noisy_env.nActuator) * noisy_env.dm_mask[None]).astype(np.float32)) for _ in range(2)]
        noisy_env.wfs.cam.configure(**R.SETTINGS["photon"])
        for e in (noisy_env, ideal_env):
            e.set_magnitude_per_env(mags)
            _start(e, 7)
        x, lam = [], []
        for i, a in enumerate(actions):
            _, ideal, _, _, _, _ = ideal_env.step(i, a)
            _, noisy, _, _, _, _ = noisy_env.step(i, a)
            number = int(noisy_env._shard.download(L.B_COUNTERS, (4,), noisy_env._stream(), dtype=np.uint32)[0])
            ideal32 = np.ascontiguousarray(ideal.cpu().numpy(), dtype=np.float32)
            got = noisy.cpu().numpy().astype(np.float64)
            assert ideal32[3].max() < lmax < ideal32[1].max(), (ideal32[3].max(), lmax, ideal32[1].max())
            want, ptrs = R.noisy_frame(ideal32, cfg, layout, np.arange(4), number, table, valid2d=valid2d, lmax=lmax)
            assert not ptrs[3].any() and ptrs[1].sum() >= 8
            R.assert_flips(got, want, ptrs, cfg, R.DEVICE_FLIP_CAP, f"{case} star frame {i}")
            for e in range(4):                                      # every env draws from ITS ideal frame: the totals follow the flux
                assert abs(got[e].sum() - ideal32[e].astype(np.float64).sum()) < 6 * np.sqrt(ideal32[e].sum()), e
            x.append(got[ptrs])
            lam.append(ideal32[ptrs].astype(np.float64))
        u = R.pit(np.concatenate(x), np.concatenate(lam), np.random.RandomState(12))
        assert u.size >= 16 and float(stats.kstest(u, "uniform").statistic) * np.sqrt(u.size) < 2.2
    finally:
        noisy_env.close()
        ideal_env.close()


# ---- 6. the loops -------------------------------------------------------------------------------------------------------------------
def _loop_run(env, disturbed):
    """rollout -> run_integrator -> reset_envs([1, 3]) -> rollout, recorded (SMALL f32, the fused step)"""
    import torch
    n = env.n_envs
    if disturbed:
        amp = np.full((n, 2, 1), 4e-8) * (1 + np.arange(n))[:, None, None]
        env.set_disturbance(2, amp, np.full((2, 1), 37.0), phase=np.full((2, 1), 0.1), t0=100)
        env.set_delay(2)
    _start(env, 11)
    a = env.rollout(0, 6, sigma=2e-3, gain=GAIN, seed=77)
    o, r, s = env.run_integrator(6, 3, GAIN)
    reset_obs = env.reset_envs([1, 3], seed=900)
    b = env.rollout(9, 5, sigma=2e-3, gain=GAIN, seed=78)
    torch.cuda.synchronize()
    rec = [a.obs, a.action, a.reward.unsqueeze(-1), a.strehl.unsqueeze(-1), o[None], r[None, :, None], s[None, :, None],
           b.obs, b.action, b.reward.unsqueeze(-1), b.strehl.unsqueeze(-1)]
    return [t.cpu().numpy() for t in rec], reset_obs.cpu().numpy()


@pytest.mark.parametrize("disturbed", [False, True])
def test_loops_and_resets_keep_the_envs_star(disturbed):
    """rollout, run_integrator and reset_envs([1, 3]) on the mixed shard (magnitudes; one threshold for the shard, so that the twins
    hold it too), `disturbed`: with per-env vibration lines and set_delay(2): obs, action, reward and Strehl of env e are
    bit-identical to twin e's, and the stars are still there afterwards."""
    env = _make("fused")
    try:
        mags = _mags(env)
        a = _factors(env, mags)
        env.set_magnitude_per_env(mags)
        env.set_threshold_per_env(0.05)
        got, got_reset = _loop_run(env, disturbed)
        assert np.array_equal(env._shard.get_flux_env(env._stream()), a.astype(np.float64))     # still there after reset_envs
        assert (env._shard.get_threshold_env(env._stream()) == np.float64(np.float32(0.05))).all() and env.fused_step
    finally:
        env.close()
    twin = _make("fused")
    try:
        twin.set_threshold_per_env(0.05)
        for e in range(twin.n_envs):
            _as_twin(twin, a[e])
            want, want_reset = _loop_run(twin, disturbed)
            for q, (x, y) in enumerate(zip(got, want)):
                assert np.array_equal(x[:, e], y[:, e]), (e, q)
            if e in (1, 3):
                k = [1, 3].index(e)
                assert np.array_equal(got_reset[k], want_reset[k]), e
    finally:
        twin.close()
    assert not np.array_equal(got[0][-1, 0], got[0][-1, 1]) and np.abs(got[1]).max() > 0
