"""GPU: wavefront modes on the device (aoenv_set_wavefront_basis / aoenv_project_wavefront / aoenv_set_wavefront_record;
BatchedAOEnv.set_wavefront_basis, project_wavefront, record_wavefront): the reference's ``opd2m @ tel.OPD[xpupil, ypupil]`` with
``opd2m = pinv(M2OPD)`` (MAIN_CODE/OOPAOEnv/SinEnv.py:150-204, predictiveControl/EOF/EOF_POL.py:105-123) for the residual and the
atmosphere OPD, on demand and as a per-step record of every stepped loop.

Checkers.  Layout: small integers, for which every float32 sum is exact, so the coefficients are the integer product bit for bit
whatever the order -- a swapped row / column, a k mapping that differs between the operands or a wrong tail cannot hide.  Real
data: the float64 product on the downloaded buffers within the bound of ANY summation order,
    |c - c64| <= (R^2 + 4) u s sum_q |P[m][q]| |X[e][q]|,   u = 2^-24 (float32 shards) or 2^-53 (float64)
(tests/_wavefront_ref.projection_bound).  The maxima of err / bound measured on MI355X are in
profiles/wavefront_parity_maxima.json (AO_WAVEFRONT_REPORT=<file> with this module alone rewrites it).  The record: a twin stepped
with ``step`` that projects after every step, bit for bit; the loops with and without a record, bit for bit.

Shards, built once per module: SMALL of tests/test_gpu_modal.py (3.2 m, 8 x 6 px, R = 48) fused, batched (PATH_GENERIC) and as a
Pyramid, and a 7-lenslet x 5-pixel Shack-Hartmann (R = 35: R^2 is odd, env 1's row is not 16-byte aligned and the loads go element
by element), float32 and float64, 3 envs; SMALL float32 with 17 and 33 envs for the ragged env tile of the matrix-core kernel.
K in {1, 5, 16, 17, 33}: below, at and above one and two 16-mode blocks; the layout and the batch-position test add K = 80, above
the 64 modes up to which a float32 shard takes the matrix-core tile (beyond: the split-K GEMM of the reconstruction).  The basis is pinv of a seeded Gaussian [P][K]."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import _wavefront_ref as W

pytestmark = pytest.mark.gpu

SMALL = dict(diameter=3.2, nSubaperture=8, nPixelPerSubap=6, r0=0.13, L0=30.0, windSpeed=[10.0], windDirection=[72.0],
             fractionalR0=[1.0], altitude=[0.0], nModes=20, nLoop=64)
ODD35 = dict(SMALL, diameter=2.8, nSubaperture=7, nPixelPerSubap=5, nModes=10)
GAIN = 0.5                                                          # (gain * obs is then the same float in the kernel and in torch)
KINDS = {
    "sh_fused": dict(geo=SMALL, wfs="shackhartmann", path=0),
    "sh_batched": dict(geo=SMALL, wfs="shackhartmann", path="PATH_GENERIC"),
    "pyramid": dict(geo=dict(SMALL, modulation=0.0), wfs="pyramid", path=0),
    "odd35": dict(geo=ODD35, wfs="shackhartmann", path=0),
}
DTYPES = ("f32", "f64")
MODES = (1, 5, 16, 17, 33)
MODES_GEMM = MODES + (80,)                                          # ... and one above 64 modes: float32 shards then take the split-K GEMM
N = 3
SEED = 20261020
I0, STEPS = 3, 12
SHARDS = [(kind, dtype, N) for kind in KINDS for dtype in DTYPES] + [("sh_fused", "f32", 17), ("sh_fused", "f32", 33)]
SHARD_IDS = [f"{k}-{d}-n{n}" for k, d, n in SHARDS]
KD = [(kind, dtype) for kind in KINDS for dtype in DTYPES]
KD_IDS = [f"{k}-{d}" for k, d in KD]
_ENVS = {}
_OBSERVED = {}


def _env(kind, dtype, tag="a", n=N):
    """One shard per (kind, dtype, tag, n) for the whole module: building one costs more than any test here."""
    from rlao_amd.env import BatchedAOEnv
    key = (kind, dtype, tag, n)
    if key not in _ENVS:
        k = KINDS[kind]
        env = BatchedAOEnv(n_envs=n, device=0, dtype=dtype)
        env.set_params(k["geo"], camera="ideal", wfs_type=k["wfs"], gainCL=GAIN)
        _ENVS[key] = env
    env = _ENVS[key]
    _path(env, kind)
    env.set_delay(0)
    env.clear_disturbance()
    env.clear_modal()
    env.clear_wavefront_basis()
    assert env.fused_step == (kind == "sh_fused" and dtype == "f32")
    return env


def _path(env, kind, general=False):
    from rlao_amd import _lib as L
    base = KINDS[kind]["path"]
    L.check(env._shard.lib.aoenv_set_option(env._shard.h, L.OPT_FORCE_PATH, (getattr(L, base) if base else 0) | (L.PATH_WF_GENERAL if general else 0)))


def _paths(dtype):
    """float32 shards: the matrix-core kernel, then the general one; float64 shards have the general one alone"""
    return (False, True) if dtype == "f32" else (False,)


@pytest.fixture(scope="module", autouse=True)
def _close_all():
    yield
    for env in _ENVS.values():
        env.close()
    _ENVS.clear()
    report = os.environ.get("AO_WAVEFRONT_REPORT")
    if report and _OBSERVED:
        with open(report, "w") as f:
            json.dump(dict(sorted(_OBSERVED.items())), f, indent=1)
            f.write("\n")


def _prologue(env, seed=5):
    env.generate_new_phase_screen(seed)
    env.dm.coefs = 0
    env.dm_prev = 0
    env.measure()
    env.SR = []


def _np(t):
    return t.detach().cpu().numpy()


def _flat_pupil(env):
    return np.asarray(env.pupil).ravel() != 0


def _gauss_m2opd(env, K):
    P = int(_flat_pupil(env).sum())
    return np.random.RandomState(SEED + K).normal(0.0, 1.0, (P, K))


def _download(env, which):
    from rlao_amd import _lib as L
    return env._shard.download(getattr(L, which), (env.n_envs, env.R * env.R), env._stream())


# ---- 1. layout, exact data -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,dtype,n", SHARDS, ids=SHARD_IDS)
def test_layout_with_exact_data(kind, dtype, n):
    """Integers |x| <= 8 in AOENV_B_PHASE and through aoenv_set_atm_opd, an integer-valued asymmetric opd2m (|p| <= 8): every sum is
    exact in float32 (<= 2304 * 64 < 2^24).  The atmosphere coefficients ARE the integer product, the residual ones
    T(sum) * T(lambda / 2 pi), on the matrix-core and the general path, for every K and every shard size."""
    from rlao_amd import _lib as L
    env = _env(kind, dtype, n=n)
    t = W.DT[dtype]
    flat = _flat_pupil(env)
    P, r2 = int(flat.sum()), env.R * env.R
    rng = np.random.RandomState(SEED + n)
    x_res, x_atm = rng.randint(-8, 9, (n, r2)).astype(np.float64), rng.randint(-8, 9, (n, r2)).astype(np.float64)
    x_res[:, -1], x_atm[:, -1], x_res[:, 0] = 8, -8, 7             # the last element of every row: a tail that is dropped shows
    env._shard.upload_state(L.B_PHASE, x_res, env._stream())
    env._shard.set_atm_opd(x_atm, env._stream())
    s = t(env.src_wavelength / (2 * np.pi))
    for K in MODES_GEMM:
        opd2m = rng.randint(-8, 9, (K, P)).astype(np.float64)
        opd2m[:, -1] = np.arange(1, K + 1) % 9                      # (the last pupil pixel is seen by every mode, each differently)
        env.set_wavefront_basis(opd2m=opd2m)
        assert env.n_wavefront_modes == K
        want_res, want_atm = x_res[:, flat] @ opd2m.T, x_atm[:, flat] @ opd2m.T
        assert np.abs(want_atm).max() > 8 and not np.array_equal(want_res, want_atm)
        for general in _paths(dtype):
            _path(env, kind, general)
            got_atm, got_res = _np(env.project_wavefront("atmosphere")), _np(env.project_wavefront("residual"))
            assert got_atm.shape == (n, K) and got_atm.dtype == t
            assert np.array_equal(got_atm.astype(np.float64), want_atm), (K, general, "atmosphere")
            assert np.array_equal(got_res, want_res.astype(t) * s), (K, general, "residual")
    _path(env, kind)


# ---- 2. real data --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,dtype", KD, ids=KD_IDS)
def test_real_data_within_the_bound_of_any_order(kind, dtype):
    """After a new screen, a few closed-loop steps and measure(): project_wavefront against opd2m @ buffer[:, pupil] in float64 on the
    downloaded buffers, and the residual through the public surface, opd2m @ env.tel.OPD[e][pupil == 1]."""
    env = _env(kind, dtype)
    _prologue(env)
    obs = env.reset_soft()
    for i in range(3):
        obs = env.step(i, GAIN * obs)[0]
    env.measure()
    flat = _flat_pupil(env)
    phase, atm = _download(env, "B_PHASE").astype(np.float64), _download(env, "B_OPD_ATM").astype(np.float64)
    opd = np.asarray(env.tel.OPD, dtype=np.float64).reshape(N, -1)
    assert np.abs(phase).max() > 0 and np.abs(atm).max() > 0
    s = env.src_wavelength / (2 * np.pi)
    worst = 0.0
    for K in MODES:
        env.set_wavefront_basis(m2opd=_gauss_m2opd(env, K))
        opd2m = env._wf
        assert np.array_equal(opd2m, np.linalg.pinv(_gauss_m2opd(env, K)))
        table = W.scatter("f64", opd2m, flat)
        for general in _paths(dtype):
            _path(env, kind, general)
            for what, x, scale, c64 in (("residual", phase, s, s * (phase[:, flat] @ opd2m.T)), ("atmosphere", atm, 1.0, atm[:, flat] @ opd2m.T)):
                got = _np(env.project_wavefront(what)).astype(np.float64)
                bound = W.projection_bound(dtype, table, x, scale)
                err = np.abs(got - c64)
                ratio = float((err / np.maximum(bound, 1e-300)).max())
                print(f"{kind} {dtype} K={K} {'general' if general else 'default'} {what}: max err / bound = {ratio:.4f}")
                worst = max(worst, ratio)
                assert got.shape == (N, K) and (err <= bound).all() and (bound > 0).all(), (K, general, what, ratio)
                assert np.abs(c64).max() > bound.max()                # the coefficients are above what rounding could fake
                if what == "residual":
                    assert (np.abs(got - opd[:, flat] @ opd2m.T) <= bound).all(), (K, general, "tel.OPD")
    _OBSERVED[f"{kind}-{dtype}"] = {"max_err_over_bound": worst}
    _path(env, kind)


# ---- 3. batch position ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [17, 33])
def test_an_env_has_the_same_bits_anywhere_in_any_shard(n):
    """Env e of the 17- and 33-env shards with the buffers of a 1-env twin uploaded gives the twin's bits, on both paths; the two
    paths are each within the bound of test 2 of the float64 product."""
    from rlao_amd import _lib as L
    twin, env = _env("sh_fused", "f32", n=1), _env("sh_fused", "f32", n=n)
    _prologue(twin, seed=11)
    obs = twin.reset_soft()
    for i in range(2):
        obs = twin.step(i, GAIN * obs)[0]
    twin.measure()
    phase, atm = _download(twin, "B_PHASE"), _download(twin, "B_OPD_ATM")
    twin._shard.set_atm_opd(atm, twin._stream())                    # (both shards then project this very buffer)
    rng = np.random.RandomState(SEED)
    big_phase, big_atm = rng.normal(0, 1, (n, phase.shape[1])), rng.normal(0, 1e-7, (n, phase.shape[1]))
    places = sorted({0, 5, 15, 16, n - 1})
    big_phase[places], big_atm[places] = phase[0], atm[0]
    env._shard.upload_state(L.B_PHASE, big_phase, env._stream())
    env._shard.set_atm_opd(big_atm, env._stream())
    flat = _flat_pupil(env)
    for K in (5, 17, 33, 80):
        m2opd = _gauss_m2opd(env, K)
        twin.set_wavefront_basis(m2opd=m2opd)
        env.set_wavefront_basis(m2opd=m2opd)
        table = W.scatter("f64", env._wf, flat)
        for general in (False, True):
            _path(twin, "sh_fused", general)
            _path(env, "sh_fused", general)
            for what, x, scale in (("residual", phase, env.src_wavelength / (2 * np.pi)), ("atmosphere", atm, 1.0)):
                want, got = _np(twin.project_wavefront(what)), _np(env.project_wavefront(what))
                for e in places:
                    assert np.array_equal(got[e], want[0]), (K, general, what, e)
                assert not np.array_equal(got[1], want[0])
                x64 = x.astype(np.float64)
                c64 = scale * (x64[:, flat] @ env._wf.T)
                bound = W.projection_bound("f32", table, x64, scale)
                assert (np.abs(want.astype(np.float64) - c64) <= bound).all(), (K, general, what)     # the bound of test 2, each path
    _path(twin, "sh_fused")
    _path(env, "sh_fused")


# ---- 4. / 5. the record ----------------------------------------------------------------------------------------------------------
LOOPS = ("run_integrator", "run_integrator_modal", "rollout", "step_modal")
K_REC = 17


def _configure(env, loop, hard):
    env.set_wavefront_basis(m2opd=_gauss_m2opd(env, K_REC))
    if loop in ("run_integrator_modal", "step_modal"):
        env.set_modal(5)
        env.set_modal_gain(0.5)
    if hard:                                                        # a delay of two frames and a vibration line on mode 0
        env.set_delay(2)
        amp = np.zeros((2, 1))
        amp[0, 0] = 2e-7
        env.set_disturbance(2, amp, np.full((2, 1), (1.0 / 40.0) / env.param.samplingTime))


def _start(env, loop):
    from rlao_amd import _lib as L
    _prologue(env)
    # (the exploration stream goes on from call to call: back to its start, so that a repeated rollout draws the same noise)
    env._shard.upload_state(L.B_COUNTERS, np.zeros(4, dtype=np.uint32), env._stream(), dtype=np.uint32)
    return env.reset_soft_modal() if loop in ("run_integrator_modal", "step_modal") else env.reset_soft()


def _modal_actions(env, obs, k):
    import torch
    g = torch.Generator(device="cpu").manual_seed(100 + k)
    return GAIN * obs + 0.05 * torch.randn((env.n_envs, 5), generator=g, dtype=torch.float64).to(device=obs.device, dtype=obs.dtype)


def _run_loop(env, loop, obs):
    """frames [I0, I0 + STEPS) through the loop under test; returns (what the loop hands out, the actions a twin replays)"""
    import torch
    from rlao_amd import _lib as L
    if loop == "run_integrator":                                    # with a frame to copy the last step's into (d_frame)
        env._obs = env._obs.clone()
        rew = torch.empty(env.n_envs, device=env.device, dtype=env.tdtype)
        sr = torch.empty_like(rew)
        frame = torch.full((env.n_envs, env.cam_res, env.cam_res), float("nan"), device=env.device, dtype=env.tdtype)
        L.check(env._shard.lib.aoenv_run_integrator(env._shard.h, I0, STEPS, GAIN, C.c_void_p(env._obs.data_ptr()), C.c_void_p(frame.data_ptr()),
                                                    C.c_void_p(rew.data_ptr()), C.c_void_p(sr.data_ptr()), C.c_void_p(env._stream())))
        return [env._obs, frame, rew, sr], None
    if loop == "run_integrator_modal":
        return list(env.run_integrator_modal(I0, STEPS)), None
    if loop == "rollout":
        tr = env.rollout(I0, STEPS, sigma=0.05, gain=GAIN, seed=9)
        return list(tr), tr.action
    out = []
    for k in range(STEPS):
        obs, frame, rew, sr, _, _ = env.step_modal(I0 + k, _modal_actions(env, obs, k))
        out += [obs, frame, rew, sr]
    return out, None


def _twin_steps(twin, loop, obs, actions):
    """the same frames on the per-call API, projecting after every step: [STEPS, 2, n, K]"""
    rows = []
    for k in range(STEPS):
        if loop == "run_integrator":
            obs = twin.step(I0 + k, GAIN * obs)[0]
        elif loop == "run_integrator_modal":
            obs = twin.step_modal(I0 + k, 0.5 * obs)[0]
        elif loop == "rollout":
            obs = twin.step(I0 + k, actions[k])[0]
        else:
            obs = twin.step_modal(I0 + k, _modal_actions(twin, obs, k))[0]
        rows.append(np.stack([_np(twin.project_wavefront("residual")), _np(twin.project_wavefront("atmosphere"))]))
    return np.stack(rows)


RECORD_CASES = [(kind, dtype, loop, False) for kind, dtype in KD for loop in LOOPS] + \
    [("sh_fused", "f32", "run_integrator", True), ("pyramid", "f64", "run_integrator", True), ("sh_batched", "f32", "rollout", True)]
RECORD_IDS = [f"{k}-{d}-{l}{'-delay2-line' if h else ''}" for k, d, l, h in RECORD_CASES]


@pytest.mark.parametrize("kind,dtype,loop,hard", RECORD_CASES, ids=RECORD_IDS)
def test_record_equals_projection_on_demand(kind, dtype, loop, hard):
    """12 frames from i_base = i0 = 3 with both bits recorded against a twin stepped by step / step_modal that calls
    project_wavefront after every step: bit for bit.  The recorded residual is the one the sensor saw in that step."""
    import torch
    env, twin = _env(kind, dtype), _env(kind, dtype, "b")
    for e in (env, twin):
        _configure(e, loop, hard)
    obs = _start(env, loop)
    rec = env.record_wavefront(I0, STEPS, ("residual", "atmosphere"))
    assert rec.shape == (STEPS, 2, N, K_REC) and rec.dtype == env.tdtype
    _, actions = _run_loop(env, loop, obs)
    torch.cuda.synchronize()
    got = _np(rec)
    env.stop_wavefront_record()
    want = _twin_steps(twin, loop, _start(twin, loop), actions)
    assert np.isfinite(got).all() and np.abs(got[:, 0]).max() > 0 and np.abs(got[:, 1]).max() > 0
    for k in range(STEPS):
        assert np.array_equal(got[k, 0], want[k, 0]), (k, "residual")
        assert np.array_equal(got[k, 1], want[k, 1]), (k, "atmosphere")
    assert not np.array_equal(got[0], got[1])
    for e in (env, twin):
        e.set_delay(0)
        e.clear_disturbance()


def _everything(env, handed_out):
    from rlao_amd import _lib as L
    out = {f"out[{j}]": _np(t) for j, t in enumerate(handed_out) if t is not None}
    out["phase"], out["frame"] = _download(env, "B_PHASE"), env._shard.download(L.B_FRAME, (env.n_envs, env.cam_res, env.cam_res), env._stream())
    out["total"], out["residual"] = np.array(env.total[I0:I0 + STEPS]), np.array(env.residual[I0:I0 + STEPS])
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


@pytest.mark.parametrize("kind,dtype,loop,hard", RECORD_CASES, ids=RECORD_IDS)
def test_the_loop_is_not_disturbed(kind, dtype, loop, hard):
    """The same 12-frame loops with and without a record attached: obs, reward, Strehl, the frame handed out for the last step, the
    library's phase and frame buffers, total / residual and get_state() are bit-identical."""
    import torch
    env = _env(kind, dtype)
    _configure(env, loop, hard)
    runs = []
    for recorded in (False, True, False):
        obs = _start(env, loop)
        if recorded:
            rec = env.record_wavefront(I0, STEPS, ("residual", "atmosphere"))
        handed, _ = _run_loop(env, loop, obs)
        torch.cuda.synchronize()
        runs.append(_everything(env, handed))
        if recorded:
            assert np.abs(_np(rec)).max() > 0
            env.stop_wavefront_record()
    plain, recorded, again = runs
    assert plain.keys() == recorded.keys() == again.keys()
    for k in plain:
        _same(recorded[k], plain[k], k)
        _same(again[k], plain[k], k + " (after the record)")
    assert np.abs(plain["phase"]).max() > 0 and plain["frame"].max() > 0
    env.set_delay(0)
    env.clear_disturbance()


# ---- 6. refusals ---------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_shard_usable():
    import torch
    from rlao_amd import _lib as L
    env, twin = _env("sh_fused", "f32"), _env("sh_fused", "f32", "b")
    lib, h = env._shard.lib, env._shard.h
    flat = _flat_pupil(env)
    P = int(flat.sum())
    out = torch.zeros((N, 8), device=env.device, dtype=env.tdtype)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    st = C.c_void_p(env._stream())

    def refused(rc, text):
        assert rc != 0 and text in lib.aoenv_last_error().decode(), lib.aoenv_last_error()

    # projection and record without a basis
    refused(lib.aoenv_project_wavefront(h, L.WF_RESIDUAL, C.c_void_p(out.data_ptr()), st), "no wavefront basis")
    refused(lib.aoenv_set_wavefront_record(h, L.WF_RESIDUAL, C.c_void_p(out.data_ptr()), 0, 1), "no wavefront basis")
    with pytest.raises(L.AoEnvError, match="set_wavefront_basis"):
        env.project_wavefront()
    good = np.random.RandomState(1).normal(0, 1, (4, P))

    def basis(K, n_pix, table):
        cfg = L.AoWavefrontBasis(n_modes=K, n_pix=n_pix, h_opd2m=None if table is None else ptr(table))
        return lib.aoenv_set_wavefront_basis(h, C.byref(cfg), st)

    nan = good.copy()
    nan[3, P - 1] = np.nan
    for args, text in (((4, P - 1, good), "the pupil has"), ((4, P + 1, np.zeros((4, P + 1))), "the pupil has"),
                       ((0, P, good), "n_modes 0 outside"), ((P + 1, P, np.zeros((P + 1, P))), "outside"),
                       ((L.MAX_WF_MODES + 1, P, np.zeros((L.MAX_WF_MODES + 1, P))), "outside"),
                       ((4, P, nan), "not finite"), ((4, P, None), "null opd2m")):
        refused(basis(*args), text)
    refused(lib.aoenv_project_wavefront(h, L.WF_RESIDUAL, C.c_void_p(out.data_ptr()), st), "no wavefront basis")      # nothing was set
    assert basis(4, P, good) == 0
    env._wf = good                                                  # (the Python layer's view of what the library now holds)
    first = _np(env.project_wavefront("residual")).copy()
    for args, text in (((4, P - 1, good), "the pupil has"), ((4, P, nan), "not finite")):
        refused(basis(*args), text)
    assert np.array_equal(_np(env.project_wavefront("residual")), first)          # a refused basis changes nothing
    # what: exactly one bit for the projection, one or two known bits for the record
    for what in (0, 3, 4):
        refused(lib.aoenv_project_wavefront(h, what, C.c_void_p(out.data_ptr()), st), "exactly one")
    refused(lib.aoenv_project_wavefront(h, L.WF_RESIDUAL, None, st), "null output")
    for what in (0, 4, 7):
        refused(lib.aoenv_set_wavefront_record(h, what, C.c_void_p(out.data_ptr()), 0, 1), "no combination")
    refused(lib.aoenv_set_wavefront_record(h, 3, C.c_void_p(out.data_ptr()), -1, 1), "window")
    refused(lib.aoenv_set_wavefront_record(h, 3, C.c_void_p(out.data_ptr()), 0, 0), "window")
    with pytest.raises(ValueError, match="one of"):
        env.project_wavefront(("residual", "atmosphere"))
    # a loop whose frames leave the record's window is refused before anything is launched: the state does not move
    for e in (env, twin):
        _prologue(e)
        e.set_modal(5)
        e.set_modal_gain(0.5)
    obs, mobs = env.reset_soft(), env.reset_soft_modal()
    env._surface = "zonal"
    rec = env.record_wavefront(4, 3)
    before = env.get_state()
    for call in (lambda: env.step(3, GAIN * obs), lambda: env.step(7, GAIN * obs), lambda: env.run_integrator(3, 2),
                 lambda: env.run_integrator(5, 3), lambda: env.rollout(2, 3, sigma=0.0), lambda: env.step_modal(8, 0.5 * mobs)):
        with pytest.raises(L.AoEnvError, match="wavefront record"):
            call()
    env._surface = "modal"
    with pytest.raises(L.AoEnvError, match="wavefront record"):
        env.run_integrator_modal(6, 2)
    env._surface = "zonal"
    torch.cuda.synchronize()
    _same(list(env.get_state().values()), list(before.values()), "state after the refused loops")
    assert float(rec.abs().max()) == 0.0
    # clear_wavefront_basis() detaches the record, and the next loop runs as on a shard that never had one
    env.clear_wavefront_basis()
    assert env.n_wavefront_modes == 0 and env._wf_rec is None
    twin.reset_soft()
    got, want = env.run_integrator(2, 6), twin.run_integrator(2, 6)
    torch.cuda.synchronize()
    for a, b in zip(got, want):
        assert torch.equal(a, b)
    assert float(rec.abs().max()) == 0.0
    a, b = env.get_state(), twin.get_state()                        # (the loop state; the shards' rollout seeds have their own histories)
    for key in ("screen", "coefs", "dm_prev", "mt", "signal"):
        _same(a[key], b[key], "state after the loop: " + key)
