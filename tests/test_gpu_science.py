"""GPU: the science camera on the device (aoenv_set_science / aoenv_science_psf / aoenv_set_science_accumulator;
BatchedAOEnv.set_science, science_psf, start_long_exposure, long_exposure*): the windowed short-exposure PSF of
``tel.computePSF(zp)`` from two small complex products per env, and its long exposure behind every stepped loop
(MAIN_CODE/predictiveControl/POL_error_CL.py, integrator_network.py:134-138, OOPAOEnv.py:473-482).

Checkers.  The reference's render: ``oracle.telescope_psf`` of the downloaded phase, cropped, within the project's tolerance for the
PSF (2e-7 / 2e-5 of the full PSF's peak, tests/test_gpu_behaviour.py), and the crop of ``tel.computePSF`` within the sum of the
two.  Exact data: a table of sparse integers and an integer amplitude, for which every float32 sum is exact, so every pixel is the
integer product's -- a wrong pixel in the wings, a swapped row / column or a k mapping that differs between the operands cannot
hide under a tolerance relative to the peak.  The loops: a twin stepped through the per-call API that adds ``science_psf()`` in
frame order, bit for bit; a third shard with nothing attached, bit for bit.  The parity maxima measured on MI355X are in
profiles/science_parity_maxima.json (AO_SCIENCE_REPORT=<file> with this module alone rewrites it).

Shards, built once per module: 4 lenslets x 6 px (R = 24, fused on float32), 6 x 5 (R = 30, the geometry sweep's p5) and 7 x 5
(R = 35: R % 4 != 0 and odd, the reference then transforms at 2 M + 1, and so do the window and the full render), float32 and float64, and the tiny Pyramid."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import _policy_ref as P
import _science_ref as S

pytestmark = pytest.mark.gpu

R24 = dict(diameter=1.6, nSubaperture=4, nPixelPerSubap=6, r0=0.13, L0=30.0, windSpeed=[10.0], windDirection=[72.0],
           fractionalR0=[1.0], altitude=[0.0], nModes=8, nLoop=64)
KINDS = {
    "r24": dict(geo=R24, wfs="shackhartmann"),
    "r30": dict(geo=dict(R24, diameter=2.4, nSubaperture=6, nPixelPerSubap=5), wfs="shackhartmann"),
    "r35": dict(geo=dict(R24, diameter=2.8, nSubaperture=7, nPixelPerSubap=5, nModes=10), wfs="shackhartmann"),
    "pyr": dict(geo=dict(R24, modulation=0.0), wfs="pyramid"),                                   # tests/golden/tiny_pyr.npz
}
ZPS = {"r24": (2, 3, 4), "r30": (2, 4), "r35": (2, 4), "pyr": (2, 4)}
TOL = {"f64": 2e-7, "f32": 2e-5}                                    # of the full PSF's peak: tests/test_gpu_behaviour.py:359
GAIN = 0.5                                                          # (gain * obs is then the same float in the kernel and in torch)
PARITY = [(k, d) for k in ("r24", "r30", "r35") for d in ("f32", "f64")] + [("pyr", "f32")]
PARITY_IDS = [f"{k}-{d}" for k, d in PARITY]
_ENVS = {}
_OBSERVED = {}


def _env(kind, dtype, n=3, tag="a"):
    from rlao_amd.env import BatchedAOEnv
    key = (kind, dtype, n, tag)
    if key not in _ENVS:
        env = BatchedAOEnv(n_envs=n, device=0, dtype=dtype)
        env.set_params(KINDS[kind]["geo"], camera="ideal", wfs_type=KINDS[kind]["wfs"], gainCL=GAIN)
        _ENVS[key] = env
    env = _ENVS[key]
    _path(env, False)
    env.set_delay(0)
    env.clear_modal()
    env.clear_science()
    env._surface = "zonal"
    return env


def _path(env, general):
    from rlao_amd import _lib as L
    L.check(env._shard.lib.aoenv_set_option(env._shard.h, L.OPT_FORCE_PATH, L.PATH_SCI_GENERAL if general else 0))


def _paths(dtype):
    """float32 shards: the matrix-core kernel, then the general one; float64 shards have the general one alone"""
    return (False, True) if dtype == "f32" else (False,)


@pytest.fixture(scope="module", autouse=True)
def _close_all():
    yield
    for env in _ENVS.values():
        env.close()
    _ENVS.clear()
    report = os.environ.get("AO_SCIENCE_REPORT")
    if report and _OBSERVED:
        with open(report, "w") as f:
            json.dump(dict(sorted(_OBSERVED.items())), f, indent=1)
            f.write("\n")


def _np(t):
    return t.detach().cpu().numpy()


def _prologue(env, seed=5):
    env.generate_new_phase_screen(seed)
    env.dm.coefs = 0
    env.dm_prev = 0
    env.measure()
    env.SR = []


def _phase(env):
    from rlao_amd import _lib as L
    return env._shard.download(L.B_PHASE, (env.n_envs, env.R, env.R), env._stream())


def _flux(env):
    return env._sh_tables.flux_map if env.wfs_type == "sh" else env._pyr_tables.flux_map


# ---- 1. against the reference's render --------------------------------------------------------------------------------------------
_RENDERS = {}


def _stepped(kind, dtype):
    """the shard after 4 closed-loop frames, its phase and the oracle's full PSFs {zp: [n, M, M]} of it (and of a flat wavefront)"""
    from oracle import ao_oracle as O                       # checker only
    env = _env(kind, dtype)
    if (kind, dtype) not in _RENDERS:
        _prologue(env, seed=9)
        obs = env.reset_soft()
        for i in range(4):
            obs = env.step(i, GAIN * obs)[0]
        phase = _phase(env).astype(np.float64)
        assert np.abs(phase).max() > 0
        pupil, flux = np.asarray(env.pupil).astype(float), _flux(env)
        full = {zp: np.stack([O.telescope_psf(pupil, flux, phase[e], zp) for e in range(env.n_envs)]) for zp in ZPS[kind]}
        flat = {zp: O.telescope_psf(pupil, flux, np.zeros_like(phase[0]), zp) for zp in ZPS[kind]}
        _RENDERS[(kind, dtype)] = (phase, full, flat)
    else:                                                           # (another test of the module may have moved the phase buffer)
        from rlao_amd import _lib as L
        env._shard.upload_state(L.B_PHASE, _RENDERS[(kind, dtype)][0].reshape(env.n_envs, -1), env._stream())
    return (env,) + _RENDERS[(kind, dtype)]


def _windows(kind, R):
    for zp in ZPS[kind]:
        for W in (2, 8, 18, zp * R):
            yield zp, W


@pytest.mark.parametrize("kind,dtype", PARITY, ids=PARITY_IDS)
def test_window_equals_the_crop_of_the_oracle_render(kind, dtype):
    """science_psf() against the crop of oracle.telescope_psf of the downloaded phase, for every zp and W in {2, 8, 18, zp R}, on
    both float32 kernels; flat=True against the window of the zero-phase oracle.  Tolerance: the project's own for the PSF."""
    env, phase, full, flat = _stepped(kind, dtype)
    worst = 0.0
    for zp, W in _windows(kind, env.R):
        env.set_science(zero_padding=zp, window=W)
        assert env.science["window"] == W and env.science["zero_padding"] == zp
        peak = full[zp].max(axis=(1, 2))
        for general in _paths(dtype):
            _path(env, general)
            got = _np(env.science_psf()).astype(np.float64)
            assert got.shape == (env.n_envs, W, W)
            err = np.abs(got - S.crop(full[zp], W)).max(axis=(1, 2)) / peak
            got_flat = _np(env.science_psf(flat=True)).astype(np.float64)
            err_flat = np.abs(got_flat - S.crop(flat[zp], W)[None]).max() / flat[zp].max()
            print(f"{kind} {dtype} zp={zp} W={W} {'general' if general else 'default'}: err / peak = {err.max():.3e}, flat {err_flat:.3e}")
            worst = max(worst, float(err.max()), float(err_flat))
            assert (err <= TOL[dtype]).all(), (zp, W, general, err)
            assert err_flat <= TOL[dtype], (zp, W, general, err_flat)
        _path(env, False)
    _OBSERVED[f"oracle-{kind}-{dtype}"] = {"max_err_over_peak": worst, "tolerance": TOL[dtype]}


@pytest.mark.parametrize("kind,dtype", PARITY, ids=PARITY_IDS)
def test_window_equals_the_crop_of_the_full_render(kind, dtype):
    """science_psf() against the crop of tel.computePSF(zp) (aoenv_compute_psf, the full transform) of the same phase, within the
    sum of the two tolerances.

    The full render itself is held to the oracle here too, at the project's tolerance: at r35 (odd R) the reference pads by
    ceil((2 M - R) / 2) on both sides and transforms at 2 M + 1 (OOPAO/Telescope.py:320-325), and aoenv_compute_psf then forms the
    image as the window with W = M.  (Its 2 M-point transform was 6.2e-3 to 3.65e-2 of the peak off the oracle at R = 35, measured
    on MI355X, which this check and the one above could not both pass.)"""
    import torch
    env, phase, full, flat = _stepped(kind, dtype)
    worst, missed = 0.0, []
    for zp in ZPS[kind]:
        render = env.tel.computePSF(zp)
        torch.cuda.synchronize()
        render = _np(render).astype(np.float64)
        peak = full[zp].max(axis=(1, 2))
        err_render = np.abs(render - full[zp]).max(axis=(1, 2)) / peak
        print(f"{kind} {dtype} zp={zp}: |computePSF - oracle| / peak = {err_render.max():.3e}")
        assert (err_render <= TOL[dtype]).all(), (zp, err_render)
        for W in (2, 8, 18, zp * env.R):
            env.set_science(zero_padding=zp, window=W)
            for general in _paths(dtype):
                _path(env, general)
                got = _np(env.science_psf()).astype(np.float64)
                err = np.abs(got - S.crop(render, W)).max(axis=(1, 2)) / peak
                print(f"{kind} {dtype} zp={zp} W={W} {'general' if general else 'default'}: |window - computePSF| / peak = {err.max():.3e}")
                worst = max(worst, float(err.max()))
                if not (err <= 2 * TOL[dtype]).all():               # (every figure is printed before the test fails)
                    missed.append((zp, W, general, float(err.max())))
            _path(env, False)
    _OBSERVED[f"render-{kind}-{dtype}"] = {"max_err_over_peak": worst, "tolerance": 2 * TOL[dtype]}
    assert not missed, missed


# ---- 2. exact data ------------------------------------------------------------------------------------------------------------------
# (kind, W, zp); the last three reach 6, 7 and 8 tile slots per wave of the matrix-core kernel, the last one two groups of row tiles
EXACT = [("r24", 8, 2), ("r30", 18, 2), ("r35", 18, 2), ("r35", 70, 2), ("r35", 176, 8), ("r35", 212, 8), ("r35", 280, 8)]


@pytest.mark.parametrize("kind,W,zp", EXACT, ids=[f"{k}-W{w}" for k, w, _ in EXACT])
def test_every_pixel_with_exact_data(kind, W, zp):
    """A table of sparse integers (re, im in {-1, 0, 1}, non-zero with probability 1/4), an amplitude in {0, 1, 2} on a disc
    uploaded as the WFS amplitude, zero phase: the matrix-core kernel, the general kernel and a float64 shard give
    T(bin) * T(1 / n_fft^2) of the int64 product, one rounding, in every pixel of every env."""
    from rlao_amd import _lib as L
    for dtype in ("f32", "f64"):
        env = _env(kind, dtype)
        R, t = env.R, S.DT[dtype]
        dft, amp = S.exact_case(R, W, seed=R + W)
        bins, partial, biggest = S.exact_window(dft, amp)
        assert partial <= 2 ** 11 and biggest < 2 ** 24 and biggest > 0, (partial, biggest)      # every float32 sum is then exact
        n_fft = S.geom(R, zp, W)["n_fft"]
        want = bins.astype(t) * t(1.0 / (float(n_fft) * float(n_fft)))
        assert len(np.unique(want)) > 8
        try:
            env._shard.upload(L.C_WFS_AMP, amp)
            env._sci = None                                         # (the upload dropped the configuration in the library)
            env.set_science(zero_padding=zp, window=W, dft=dft)
            env._shard.upload_state(L.B_PHASE, np.zeros((env.n_envs, R * R)), env._stream())
            for general in _paths(dtype):
                _path(env, general)
                got = _np(env.science_psf())
                assert got.dtype == t and got.shape == (env.n_envs, W, W)
                for e in range(env.n_envs):
                    assert np.array_equal(got[e], want), (dtype, general, e, np.argwhere(got[e] != want)[:4])
                assert np.array_equal(_np(env.science_psf(flat=True)), got)
        finally:
            _path(env, False)
            env._shard.upload(L.C_WFS_AMP, env._sh_tables.amp)
            env._sci = None


# ---- 3. every loop accumulates what a per-call twin does ------------------------------------------------------------------------------
LOOPS = ("step", "run_integrator", "rollout", "policy_rollout", "step_modal", "run_integrator_modal")
N_LOOP, STEPS, FIRST = 5, 8, 3


def _configure(env, loop):
    if loop in ("run_integrator_modal", "step_modal"):
        env.set_modal(5)
        env.set_modal_gain(0.5)
    if loop == "policy_rollout":
        env.set_policy(P.make_weights(3, 16, seed=5, scale=(20.0, 1.5, 2.0)))


def _start(env, loop):
    from rlao_amd import _lib as L
    _prologue(env)
    env._shard.upload_state(L.B_COUNTERS, np.zeros(4, dtype=np.uint32), env._stream(), dtype=np.uint32)
    return env.reset_soft_modal() if loop in ("run_integrator_modal", "step_modal") else env.reset_soft()


def _modal_actions(env, obs, k):
    import torch
    g = torch.Generator(device="cpu").manual_seed(100 + k)
    return GAIN * obs + 0.05 * torch.randn((env.n_envs, 5), generator=g, dtype=torch.float64).to(device=obs.device, dtype=obs.dtype)


def _run_loop(env, loop, obs):
    """frames [0, STEPS) through the loop under test: (what it hands out, the actions a twin replays)"""
    if loop == "run_integrator":
        return list(env.run_integrator(0, STEPS)), None
    if loop == "run_integrator_modal":
        return list(env.run_integrator_modal(0, STEPS)), None
    if loop == "rollout":
        tr = env.rollout(0, STEPS, sigma=0.05, gain=GAIN, seed=9)
        return list(tr), tr.action
    if loop == "policy_rollout":
        tr, past = env.policy_rollout(0, STEPS, seed=9)
        return list(tr) + list(past), tr.action
    out, actions = [], []
    for k in range(STEPS):
        if loop == "step":
            actions.append(GAIN * obs)
            obs, frame, rew, sr, _, _ = env.step(k, actions[-1])
        else:
            obs, frame, rew, sr, _, _ = env.step_modal(k, _modal_actions(env, obs, k))
        out += [obs, frame, rew, sr]
    return out, actions if loop == "step" else None


def _twin_sums(twin, loop, obs, actions):
    """the same frames on the per-call API, science_psf() added in frame order in the env dtype"""
    import torch
    W = twin.science["window"]
    acc = torch.zeros((twin.n_envs, W, W), device=twin.device, dtype=twin.tdtype)
    acc_log = torch.zeros_like(acc)
    for k in range(STEPS):
        if loop in ("run_integrator", "step"):
            obs = twin.step(k, GAIN * obs)[0]
        elif loop == "run_integrator_modal":
            obs = twin.step_modal(k, 0.5 * obs)[0]
        elif loop in ("rollout", "policy_rollout"):
            obs = twin.step(k, actions[k])[0]
        else:
            obs = twin.step_modal(k, _modal_actions(twin, obs, k))[0]
        if k >= FIRST:
            psf = twin.science_psf()
            acc = acc + psf
            acc_log = acc_log + torch.log10(psf)
    return _np(acc), _np(acc_log)


def _everything(env, handed):
    from rlao_amd import _lib as L
    out = {f"out[{j}]": _np(t) for j, t in enumerate(handed) if t is not None}
    out["phase"] = _phase(env)
    out["frame"] = env._shard.download(L.B_FRAME, (env.n_envs, env.cam_res, env.cam_res), env._stream())
    for k, v in env.get_state().items():
        out["state." + k] = v
    return out


def _same(a, b, what):
    if isinstance(a, (tuple, list)):
        assert isinstance(b, (tuple, list)) and len(a) == len(b), what
        for i, (x, y) in enumerate(zip(a, b)):
            _same(x, y, f"{what}[{i}]")
    elif a is None or b is None:
        assert a is None and b is None, what
    else:
        assert np.array_equal(np.asarray(a), np.asarray(b)), what


LOOP_CASES = [(d, l) for d in ("f32", "f64") for l in LOOPS]


@pytest.mark.parametrize("dtype,loop", LOOP_CASES, ids=[f"{d}-{l}" for d, l in LOOP_CASES])
def test_every_loop_accumulates_what_a_per_call_twin_does(dtype, loop):
    """8 frames with first_frame = 3, window 8, log10: sum, sum_log10 and count (5 per env) bit for bit those of a twin that steps
    through the per-call API and adds science_psf() in frame order; the loop's outputs, buffers and get_state() bit for bit those
    of a third shard with nothing attached; the fused shard stays fused; after stop_long_exposure() the buffers are left alone."""
    import torch
    env, twin, plain = (_env("r24", dtype, N_LOOP, tag) for tag in "abc")
    for e in (env, twin, plain):
        _configure(e, loop)
    for e in (env, twin):
        e.set_science(zero_padding=4, window=8, first_frame=FIRST, log10=True)
    obs = _start(env, loop)
    env.start_long_exposure()
    assert env.fused_step == (dtype == "f32")
    handed, actions = _run_loop(env, loop, obs)
    torch.cuda.synchronize()
    acc, acc_log, count = (_np(t).copy() for t in env._le)
    got = _everything(env, handed)
    assert env.fused_step == (dtype == "f32")
    # the twin
    want, want_log = _twin_sums(twin, loop, _start(twin, loop), actions)
    assert np.array_equal(count, np.full(N_LOOP, STEPS - FIRST, dtype=np.int32))
    assert np.isfinite(acc).all() and acc.min() > 0 and np.isfinite(acc_log).all()
    assert np.array_equal(acc, want), np.abs(acc - want).max()
    assert np.array_equal(acc_log, want_log), np.abs(acc_log - want_log).max()
    assert not np.array_equal(acc[0], acc[1])
    # nothing attached
    handed_plain, _ = _run_loop(plain, loop, _start(plain, loop))
    torch.cuda.synchronize()
    ref = _everything(plain, handed_plain)
    assert got.keys() == ref.keys()
    for k in ref:
        # (a modal loop keeps its observation apart; the retained zonal one is what an earlier zonal call of the shard left)
        if not (k == "state.obs" and loop in ("run_integrator_modal", "step_modal")):
            _same(got[k], ref[k], k)
    # detached: further steps leave the buffers alone
    env.stop_long_exposure()
    if loop in ("run_integrator_modal", "step_modal"):
        env.run_integrator_modal(STEPS, 2)
    else:
        env.run_integrator(STEPS, 2)
    torch.cuda.synchronize()
    assert np.array_equal(_np(env._le[0]), acc) and np.array_equal(_np(env._le[1]), acc_log) and np.array_equal(_np(env._le[2]), count)
    if loop == "policy_rollout":
        for e in (env, twin, plain):
            e.set_policy(None)


# ---- 4. batch position ----------------------------------------------------------------------------------------------------------------
def test_an_env_has_the_same_bits_anywhere_in_any_shard():
    """Env 0 of a 1-env shard and env 3 of a 5-env shard with the same phase give the same bits, in both float32 kernels."""
    from rlao_amd import _lib as L
    one, five = _env("r24", "f32", 1), _env("r24", "f32", N_LOOP)
    rng = np.random.RandomState(3)
    r2 = one.R * one.R
    phase = rng.normal(0, 1.5, (1, r2))
    big = rng.normal(0, 1.5, (N_LOOP, r2))
    big[3] = phase[0]
    one._shard.upload_state(L.B_PHASE, phase, one._stream())
    five._shard.upload_state(L.B_PHASE, big, five._stream())
    for zp, W in ((4, 8), (2, 18), (4, 96)):
        for e in (one, five):
            e.set_science(zero_padding=zp, window=W)
        for general in (False, True):
            _path(one, general)
            _path(five, general)
            a, b = _np(one.science_psf()), _np(five.science_psf())
            assert np.array_equal(a[0], b[3]), (zp, W, general)
            assert not np.array_equal(a[0], b[2])
    _path(one, False)
    _path(five, False)


# ---- 5. read-outs ---------------------------------------------------------------------------------------------------------------------
def test_read_outs():
    """long_exposure() is sum over count; zero_long_exposure([1, 3]) zeroes those envs alone; the count and the mean are 0 where
    nothing was added; the Strehl ratio of a loop held flat (zero screens, zero wind) is 1 within 4 float32 ulps."""
    import torch
    env = _env("r24", "f32", N_LOOP, "c")
    env.set_science(zero_padding=4, window=8, first_frame=2, log10=True)
    obs = _start(env, "step")
    env.start_long_exposure()
    le, count = env.long_exposure()
    assert float(le.abs().max()) == 0.0 and int(count.abs().max()) == 0 and float(env.long_exposure_log10().abs().max()) == 0.0
    env.run_integrator(0, 6)
    torch.cuda.synchronize()
    acc, acc_log, cnt = env._le
    le, count = env.long_exposure()
    assert np.array_equal(_np(count), np.full(N_LOOP, 4, dtype=np.int32))
    assert torch.equal(le, acc / 4) and torch.equal(env.long_exposure_log10(), acc_log / 4)
    sr = env.long_exposure_strehl()
    assert sr.shape == (N_LOOP,) and float(sr.min()) > 0 and float(sr.max()) < 1
    before = _np(acc).copy()
    env.zero_long_exposure([1, 3])
    le, count = env.long_exposure()
    assert _np(count).tolist() == [4, 0, 4, 0, 4]
    for e in range(N_LOOP):
        if e in (1, 3):
            assert float(acc[e].abs().max()) == 0.0 and float(acc_log[e].abs().max()) == 0.0 and float(le[e].abs().max()) == 0.0
        else:
            assert np.array_equal(_np(acc[e]), before[e])
    # a loop held flat
    env.stop_long_exposure()
    state = env.get_state()
    state["screen"] = [np.zeros_like(s) for s in state["screen"]] if isinstance(state["screen"], list) else np.zeros_like(state["screen"])
    speed = env.atm.windSpeed
    state["windSpeed"] = [0.0]
    try:
        env.set_state(state)
        env.dm.coefs = 0
        env.dm_prev = 0
        env.measure()
        env.reset_soft()
        env.set_science(zero_padding=4, window=8, first_frame=0)
        env.start_long_exposure()
        env.run_integrator(0, 6)
        torch.cuda.synchronize()
        # (flat to rounding: the integrator acts on slopes of 1e-7 of the reference centroids' size; 3e-6 rad measured)
        assert float(np.abs(_phase(env)).max()) < 1e-4
        sr = _np(env.long_exposure_strehl()).astype(np.float64)
        assert np.array_equal(_np(env.long_exposure()[1]), np.full(N_LOOP, 6, dtype=np.int32))
        assert (np.abs(sr - 1.0) <= 4 * 2.0 ** -23).all(), sr
    finally:
        env.stop_long_exposure()
        env.atm.windSpeed = speed


# ---- 6. refusals through the C ABI ----------------------------------------------------------------------------------------------------
def test_refusals_leave_the_configuration_as_it_was():
    import torch
    from rlao_amd import _lib as L
    env = _env("r35", "f32")
    lib, h, st = env._shard.lib, env._shard.h, C.c_void_p(env._stream())
    R, n = env.R, env.n_envs
    out = torch.zeros((n, 70, 70), device=env.device, dtype=env.tdtype)
    count = torch.zeros((n,), device=env.device, dtype=torch.int32)
    po, pc = C.c_void_p(out.data_ptr()), C.c_void_p(count.data_ptr())

    def refused(rc, text):
        assert rc != 0 and text in lib.aoenv_last_error().decode(), lib.aoenv_last_error()

    def science(zp, W, first=16, flags=0, dft=None):
        cfg = L.AoScience(zero_padding=zp, window=W, first_frame=first, flags=flags, h_dft=None if dft is None else dft.ctypes.data_as(C.c_void_p))
        return lib.aoenv_set_science(h, C.byref(cfg), st)

    refused(lib.aoenv_science_psf(h, 0, po, st), "no science camera")
    refused(lib.aoenv_set_science_accumulator(h, po, None, pc), "no science camera")
    with pytest.raises(L.AoEnvError, match="set_science"):
        env.science_psf()
    with pytest.raises(L.AoEnvError, match="start_long_exposure"):
        env.long_exposure()
    nan = np.zeros((16, R, 2))
    nan[15, R - 1, 1] = np.inf
    bad = (((2, 7), S.MESSAGES[S.WINDOW_ODD]), ((2, 72), S.MESSAGES[S.WINDOW_RANGE]), ((2, 0), S.MESSAGES[S.WINDOW_RANGE]),
           ((0, 8), S.MESSAGES[S.BAD_ZP]), ((9, 8), S.MESSAGES[S.BAD_ZP]), ((3, 8), S.MESSAGES[S.ODD_IMAGE]),
           ((2, 8, 16, 0, nan), S.MESSAGES[S.NOT_FINITE]), ((2, 8, -1), S.MESSAGES[S.FIRST_FRAME]), ((2, 8, 16, 2), S.MESSAGES[S.BAD_FLAGS]))
    for args, text in bad:
        refused(science(*args), text)
    refused(lib.aoenv_science_psf(h, 0, po, st), "no science camera")                # nothing was set
    env._shard.upload_state(L.B_PHASE, np.random.RandomState(2).normal(0, 1, (n, R * R)), env._stream())
    env.set_science(zero_padding=2, window=18, log10=True)
    first = _np(env.science_psf()).copy()
    for args, text in bad:
        refused(science(*args), text)
        assert np.array_equal(_np(env.science_psf()), first)        # a refused configuration changes nothing
    refused(lib.aoenv_science_psf(h, 0, None, st), "null output")
    refused(lib.aoenv_set_science_accumulator(h, po, None, pc), "d_sum_log10 is null")
    refused(lib.aoenv_set_science_accumulator(h, po, po, None), "null count")
    env.set_science(zero_padding=2, window=18)
    refused(lib.aoenv_set_science_accumulator(h, po, po, pc), "without AOENV_SCI_LOG10")
    assert np.array_equal(_np(env.science_psf()), first)
    assert lib.aoenv_set_science_accumulator(h, None, None, None) == 0
    env.clear_science()
    assert env.science is None
    refused(lib.aoenv_science_psf(h, 0, po, st), "no science camera")
