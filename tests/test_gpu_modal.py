"""GPU: the modal control surface (aoenv_set_modal / BatchedAOEnv.set_modal): step_modal, reset_soft_modal and
run_integrator_modal take and return [n_envs, K] modal coefficients, as the reference's modal envs do
(MAIN/OOPAOEnv/modalAOEnv.py:150-171, 190), around the unchanged explicit-action step of ``step``.

Checkers.  The expansion: the host model of rlao_amd/csrc/modal.hpp restated in exact integer arithmetic with one rounding per fma
(tests/_modal_ref.py, pinned against the host driver in tests/test_modal_host.py), bit for bit.  The step: a twin shard stepped
with ``step`` on the expanded images, bit for bit.  The projection: the float64 NumPy product of the handed-over ``cm`` and the
downloaded AOENV_B_SIGNAL, within the bound of ANY summation order,
    |o - o64| <= 1e6 (n_signal + 4) u sum_j |cm[m][j]| |signal[j]|,   u = 2^-24 (float32 shards) or 2^-53 (float64),
the +4 for rounding ``cm`` to the env dtype and for the scale; the reward through 2 |o| |delta o| summed, with delta o the bound
above and its square added: (o + d)^2 - o^2 = 2 o d + d^2 exactly, and the first-order term alone is no bound.  On the default
per-env path o and the reward are moreover the fixed order of modal.hpp bit for bit: ``_modal_ref.exact_project``, the order
restated in Python and pinned against the host driver in tests/test_modal_host.py, on the downloaded slopes.

Geometry: the 3.2 m / 8-lenslet SMALL of tests/test_gpu_delay.py (9 x 9 actuators, 69 valid, 104 slopes: with 3 envs the image row
of env 1 is not 16-byte aligned and the last element of env 0's goes on its own), fused, batched (a path bit set) and as a
Pyramid, float32 and float64, 3 envs, K in {1, 5, 20 = the whole basis}: every test runs that whole product (CASES), except
where its docstring names the one K the issue fixes for it; the 2 m / 5-lenslet ODD (42 slopes, K = 7: no multiples of 4) is
run in addition for the GEMM path.  Shards are built once per module and reset by the prologue of every test."""
import ctypes as C

import numpy as np
import pytest

import _modal_ref as R

pytestmark = pytest.mark.gpu

SMALL = dict(diameter=3.2, nSubaperture=8, nPixelPerSubap=6, r0=0.13, L0=30.0, windSpeed=[10.0], windDirection=[72.0],
             fractionalR0=[1.0], altitude=[0.0], nModes=20, nLoop=64)
ODD = dict(SMALL, diameter=2.0, nSubaperture=5, nModes=10)
GAIN = 0.4
KINDS = {
    "sh_fused": dict(geo=SMALL, wfs="shackhartmann", path=0),
    "sh_batched": dict(geo=SMALL, wfs="shackhartmann", path="PATH_GENERIC"),
    "pyramid": dict(geo=dict(SMALL, modulation=0.0), wfs="pyramid", path=0),
    "odd": dict(geo=ODD, wfs="shackhartmann", path=0),
}
DTYPES = ("f32", "f64")
MODES = (1, 5, 20)
STATE_KEYS = ("screen", "coefs", "dm_prev", "mt", "signal")
N = 3
_ENVS = {}


def _env(kind, dtype, tag="a", n=N, offset=0):
    """One shard per (kind, dtype, tag) for the whole module: building one costs more than any test here."""
    from rlao_amd import _lib as L
    from rlao_amd.env import BatchedAOEnv
    key = (kind, dtype, tag, n, offset)
    if key not in _ENVS:
        k = KINDS[kind]
        env = BatchedAOEnv(n_envs=n, device=0, dtype=dtype, env_index_offset=offset)
        env.set_params(k["geo"], camera="ideal", wfs_type=k["wfs"], gainCL=GAIN)
        _ENVS[key] = env
    env = _ENVS[key]
    _path(env, kind)
    env.set_delay(0)
    env.clear_disturbance()
    env.clear_dm_per_env()
    env.clear_modal()
    env.accumulate_returns(None)
    return env


def _path(env, kind, extra=0):
    from rlao_amd import _lib as L
    base = KINDS[kind]["path"]
    L.check(env._shard.lib.aoenv_set_option(env._shard.h, L.OPT_FORCE_PATH, (getattr(L, base) if base else 0) | extra))


@pytest.fixture(scope="module", autouse=True)
def _close_all():
    yield
    for env in _ENVS.values():
        env.close()
    _ENVS.clear()


def _prologue(env, seed=5):
    env.generate_new_phase_screen(seed)
    env.dm.coefs = 0
    env.dm_prev = 0
    env.measure()
    env.SR = []


def _np(t):
    return t.detach().cpu().numpy()


def _actions(env, K, obs, k, seed=1):
    """random modal coefficients for every env: GAIN * obs plus 0.05 um of noise on every mode"""
    import torch
    g = torch.Generator(device="cpu").manual_seed(1000 * seed + k)
    return GAIN * obs + 0.05 * torch.randn((env.n_envs, K), generator=g, dtype=torch.float64).to(device=obs.device, dtype=obs.dtype)


def _host_image(env, a):
    """the action image of the host model for coefficients a [n, K] (a tensor of the env dtype)"""
    import torch
    v = R.exact_expand(env.dtype, env._modal["m2c"], _np(a))
    return torch.as_tensor(R.to_image(v, env._dm_tables.act_idx, env.nActuator)).to(env.device)


def _state(env):
    s = env.get_state()
    return {k: np.asarray(s[k]).copy() for k in STATE_KEYS}


def _same_state(a, b, what, n_steps=None):
    sa, sb = _state(a), _state(b)
    for key in STATE_KEYS:
        assert np.array_equal(sa[key], sb[key]), (what, key)
    if n_steps:
        assert np.array_equal(a.total[:n_steps], b.total[:n_steps]) and np.array_equal(a.residual[:n_steps], b.residual[:n_steps]), what


def _check_projection(env, obs, reward, what, exact=False):
    """o and the reward against the float64 product of the handed-over cm and the downloaded signal; exact: also bit for bit
    against the fixed order of modal.hpp restated on the host (the default per-env path only)"""
    from rlao_amd import _lib as L
    K = env.n_modal
    raw = env._shard.download(L.B_SIGNAL, (env.n_envs, env.nSignal))
    sig = raw.astype(np.float64)
    if exact:
        want_o, want_r = R.exact_project(env.dtype, env._modal["cm"], raw)
        assert np.array_equal(_np(obs), want_o), (what, "the order of modal.hpp")
        if reward is not None:
            assert np.array_equal(_np(reward), want_r.astype(want_o.dtype)), (what, "the reward's order")
    cm = env._modal["cm"]
    o64 = -1e6 * sig @ cm.T
    bound = R.projection_bound(env.dtype, cm, sig)
    o = _np(obs).astype(np.float64)
    err = np.abs(o - o64)
    print(f"{what}: max |o - o64| / bound = {float((err / np.maximum(bound, 1e-300)).max()):.3f}")
    assert o.shape == (env.n_envs, K) and (err <= bound).all(), (what, float(err.max()), float(bound.min()))
    if reward is not None:
        r64 = -(o64 ** 2).sum(axis=1)
        rb = (2 * np.abs(o64) * bound + bound ** 2).sum(axis=1)
        assert (np.abs(_np(reward).astype(np.float64) - r64) <= rb).all(), (what, _np(reward), r64, rb)
    return o64, bound


CASES = [(kind, dtype, K) for kind in ("sh_fused", "sh_batched", "pyramid") for dtype in DTYPES for K in MODES]


@pytest.mark.parametrize("kind,dtype,K", CASES, ids=[f"{k}-{d}-K{m}" for k, d, m in CASES])
def test_twin_and_projection(kind, dtype, K):
    """Under set_delay(1) the newest entry of the delay line is the expanded action: the host model bit for bit.  A twin stepped
    with ``step`` on those images gives the same frame and Strehl ratio at every step and ends with the same screens, streams,
    commands, slopes and telemetry, 6 steps with a pixel crossing.  The same at delay 0, on the images the first run verified.
    After every step o and the reward are within the bound of the float64 product, and equal to the fixed order of modal.hpp
    restated on the host bit for bit."""
    import torch
    env, twin = _env(kind, dtype), _env(kind, dtype, "b")
    assert env.fused_step == (kind == "sh_fused" and dtype == "f32") == twin.fused_step
    env.set_modal(K)
    assert env.n_modal == K and twin.n_modal == 0
    images, actions = [], []
    for d in (1, 0):
        env.set_delay(d)
        twin.set_delay(d)
        _prologue(env)
        _prologue(twin)
        screen0 = _state(env)["screen"]
        obs = env.reset_soft_modal()
        twin.reset_soft()
        assert tuple(obs.shape) == (N, K) and obs.dtype == env.tdtype
        _check_projection(env, obs, None, (kind, dtype, K, d, "reset"), exact=True)
        for k in range(6):
            if d == 1:
                actions.append(_actions(env, K, obs, k))
            a = actions[k].clone()
            r = env.step_modal(k, a)
            a.fill_(123.0)                                          # the caller's tensor may be reused at once
            if d == 1:
                img = env.delay_line()[-1]
                assert torch.equal(img, _host_image(env, actions[k])), (kind, dtype, K, k)
                images.append(img.clone())
            rt = twin.step(k, images[k])
            assert torch.equal(r[1], rt[1]) and torch.equal(r[3], rt[3]), (kind, dtype, K, d, k)
            obs = r[0]
            _check_projection(env, obs, r[2], (kind, dtype, K, d, k), exact=True)
        _same_state(env, twin, (kind, dtype, K, d), 6)
        assert not np.array_equal(_state(env)["screen"], screen0)   # a pixel crossing happened
        assert np.abs(_state(env)["coefs"]).max() > 1e-9
    assert not torch.equal(images[0], images[1])


PATH_CASES = CASES + [("odd", "f32", 7), ("odd", "f64", 7)]


@pytest.mark.parametrize("kind,dtype,K", PATH_CASES, ids=[f"{k}-{d}-K{m}" for k, d, m in PATH_CASES])
def test_gemm_path_against_the_default(kind, dtype, K):
    """AOENV_PATH_MODAL_GEMM: the projection as a batched product plus the finish kernel.  In a closed loop both paths stay within
    the bound of the float64 product at every step, and on the same slopes (the reset) they are within twice the bound of each
    other.  Stepped with the same actions the two leave an identical loop state: the bit touches nothing inside the step and
    leaves the shard on the fused step kernel.  K = 1: a product with one column and a finish kernel with one element of LDS.
    ODD: 42 slopes and 7 modes, no multiples of 64, 32 or 4."""
    import torch
    from rlao_amd import _lib as L
    env = _env(kind, dtype)
    env.set_modal(K)
    if kind == "odd":
        assert env.nSignal == 42 and K % 4 and env.nSignal % 4
    fused = env.fused_step
    first, states = [], []
    for extra in (0, L.PATH_MODAL_GEMM):
        _path(env, kind, extra)
        assert env.fused_step == fused
        _prologue(env)
        obs = env.reset_soft_modal()
        first.append((_np(obs).astype(np.float64), _check_projection(env, obs, None, (kind, dtype, extra, "reset"), exact=not extra)[1]))
        for k in range(6):                                          # closed loop: each path on its own observations
            obs, _, rew, _, _, _ = env.step_modal(k, GAIN * obs)
            _check_projection(env, obs, rew, (kind, dtype, extra, k))
        _prologue(env)
        obs = env.reset_soft_modal()
        for k in range(6):                                          # the same actions through both paths
            env.step_modal(k, _actions(env, K, torch.zeros_like(obs), k))
        states.append((_state(env), env.total[:6].copy(), env.residual[:6].copy()))
    _path(env, kind)
    assert (np.abs(first[0][0] - first[1][0]) <= 2 * first[0][1]).all()
    for key in STATE_KEYS:
        assert np.array_equal(states[0][0][key], states[1][0][key]), key
    assert np.array_equal(states[0][1], states[1][1]) and np.array_equal(states[0][2], states[1][2])
    assert np.abs(states[0][0]["coefs"]).max() > 1e-9


@pytest.mark.parametrize("kind,dtype,K", CASES, ids=[f"{k}-{d}-K{m}" for k, d, m in CASES])
def test_batch_independence(kind, dtype, K):
    """Env 1 of the 3-env shard and the same env alone (same seeds through env_index_offset): the same observations and rewards
    bit for bit on the default per-env path, every step of a closed loop.  K = 1: a launch of 4 waves of which one has a mode."""
    import torch
    env, one = _env(kind, dtype), _env(kind, dtype, "one", n=1, offset=1)
    for e in (env, one):
        e.set_modal(K)
        _prologue(e)
    o3, o1 = env.reset_soft_modal(), one.reset_soft_modal()
    assert torch.equal(o3[1:2], o1)
    for k in range(6):
        a = _actions(env, K, o3, k)
        r3, r1 = env.step_modal(k, a), one.step_modal(k, a[1:2])
        o3, o1 = r3[0], r1[0]
        assert torch.equal(o3[1:2], o1) and torch.equal(r3[2][1:2], r1[2]), (kind, dtype, K, k)
    assert o3[1].abs().max() > 0


@pytest.mark.parametrize("per_env", [False, True])
@pytest.mark.parametrize("kind,dtype,K", CASES, ids=[f"{k}-{d}-K{m}" for k, d, m in CASES])
def test_integrator_equals_stepping(kind, dtype, K, per_env):
    """run_integrator_modal for 8 steps is 8 calls of step_modal with a = g * o formed by the caller in the env dtype: the same
    observation, reward, Strehl ratio and loop state, with shared and with per-env gains.  Per-env gains: env 2 has g = 0 and
    stays open loop, its command exactly 0.  The control delay rides along with K (1: none, 5: two frames, 20: one), so that
    every kind and dtype runs the fused-gain expansion into the internal image and into the delay line."""
    import torch
    d = {1: 0, 5: 2, 20: 1}[K]
    env, twin = _env(kind, dtype), _env(kind, dtype, "b")
    rng = np.random.RandomState(4)
    g = rng.uniform(0.2, 0.6, (N, K)) if per_env else rng.uniform(0.2, 0.6, K)
    if per_env:
        g[2] = 0.0
    for e in (env, twin):
        e.set_modal(K)
        e.set_delay(d)
        _prologue(e)
    env.set_modal_gain(g)
    ret = torch.zeros(N, device=env.device, dtype=env.tdtype)
    env.accumulate_returns(ret)
    obs = env.reset_soft_modal()
    o = twin.reset_soft_modal()
    assert torch.equal(obs, o)
    gt = torch.as_tensor(np.broadcast_to(g, (N, K)).copy()).to(device=env.device, dtype=env.tdtype)
    want_ret = torch.zeros(N, device=env.device, dtype=env.tdtype)
    for k in range(8):
        o, _, rw, sr, _, _ = twin.step_modal(k, gt * o)
        want_ret += rw
    got = env.run_integrator_modal(0, 8)
    assert got[0] is not obs and torch.equal(got[0], o) and torch.equal(got[1], rw) and torch.equal(got[2], sr)
    assert torch.equal(ret, want_ret) and (ret < 0).all()           # the accumulator received the MODAL reward
    env.accumulate_returns(None)
    _same_state(env, twin, (kind, dtype, d, per_env), 8)
    coefs = _state(env)["coefs"]
    assert np.abs(coefs[0]).max() > 1e-9
    if per_env:
        assert (coefs[2] == 0).all()
    if d:
        assert torch.equal(env.delay_line(), twin.delay_line())


@pytest.mark.parametrize("kind", ["sh_fused", "sh_batched", "pyramid"])
def test_full_basis_is_the_zonal_integrator(kind):
    """K = the whole basis, every gain gainCL: cm is the modal command matrix the reconstructor is built from (R = M2C cm), so the
    modal integrator and run_integrator are one controller in two roundings.  Residual rms after 30 steps within the float32
    zonal-versus-oracle obs tolerance of tests/test_gpu_parity.py (micrometres); float32 shards, whose tolerance it is."""
    from test_gpu_parity import F32_TOL
    env, twin = _env(kind, "f32"), _env(kind, "f32", "b")
    env.set_modal()
    assert env.n_modal == SMALL["nModes"] and np.array_equal(env._modal["cm"], env.modal_CM)
    env.set_modal_gain(env.gainCL)
    _prologue(env)
    _prologue(twin)
    env.reset_soft_modal()
    twin.reset_soft()
    env.run_integrator_modal(0, 30)
    twin.run_integrator(0, 30)
    res_m, res_z = env.residual[:30], twin.residual[:30]           # nm rms
    print(f"residual rms at step 29: modal {res_m[29]} nm, zonal {res_z[29]} nm, open loop {env.total[29]} nm")
    if kind != "pyramid":                                           # (an unmodulated Pyramid on open-loop turbulence need not close)
        assert (res_z[29] < twin.total[29]).all()                   # the loop is closed
    assert (np.abs(res_m[29] - res_z[29]) * 1e-3 <= F32_TOL["obs"]).all()


@pytest.mark.parametrize("kind,dtype", [(k, d) for k in ("sh_fused", "sh_batched", "pyramid") for d in DTYPES])
def test_composition(kind, dtype):
    """K = 2 -- the one K the issue fixes for this case: tip and tilt, the reference's vibration envs -- on every kind and dtype.
    A disturbance on mode 0 with modal gains: visible in o[:, 0] in open loop (the run with the disturbance minus the run
    without), rejected below that amplitude in closed loop.  A mis-registered mirror on env 1 changes that env's observations
    only.  reset_envs on env 1 leaves the modal trajectory of the others bit-identical.
    The line: 0.2 um at 1 / 320 cycles per frame (w = 0.0196 rad per frame, phase 0: a rise that stays monotonic over the 60 frames
    run, to 0.18 um), gains 0.5, leak 0.99, a loop latency of two frames.  The open loop is L = G g e^{-jw} / (e^{jw} - 0.99) with
    G the sensor's gain on the mode: arg L = -(atan2(sin w, cos w - 0.99) + w) = -(1.11 + 0.02), cos(arg L) = 0.43 > 0, so
    |1 + L|^2 = 1 + 2 |L| cos + |L|^2 > 1 and the line is rejected for EVERY G > 0 -- for the Shack-Hartmann (G = 1, |L| = 23) and
    for the unmodulated Pyramid alike, which this atmosphere drives far into saturation (a faster line would be amplified at a
    small G: at 50 frames per cycle cos(arg L) = -0.17 and the rejection needs |L| > 0.34).  "Visible": above a hundred times the
    summation bound of the projection itself, i.e. nothing its rounding could fake (the camera is ideal: there is no other
    noise).  The cross-talk into mode 1 is bounded for the Shack-Hartmann only: a saturated Pyramid is not linear."""
    K, T = 2, 60
    env = _env(kind, dtype)
    amp = np.zeros((2, 1))
    amp[0, 0] = 2e-7                                                # 0.2 um of mode 0, 320 frames per cycle
    hz = np.full((2, 1), (1.0 / 320.0) / env.param.samplingTime)
    floor = [0.0]

    def run(gain, disturbed=True, misreg=False, reset_at=None):
        env.clear_dm_per_env()
        env.clear_disturbance()
        env.set_modal(K)
        env.set_modal_gain(gain)
        if disturbed:
            env.set_disturbance(2, amp, hz)
        if misreg:
            env.set_dm_misregistration(shift_x=0.2 * env.param.diameter / env.param.nSubaperture, env_ids=[1])
        _prologue(env)
        floor[0] = max(floor[0], float(_check_projection(env, env.reset_soft_modal(), None, (kind, dtype, "composition"))[1].max()))
        out = []
        for k in range(T):
            if reset_at == k:
                env.reset_envs([1], seed=77)
            out.append(_np(env.run_integrator_modal(k, 1)[0]).astype(np.float64))
        return np.stack(out)                                        # [T, N, K]

    seen = run(0.0) - run(0.0, disturbed=False)                     # the disturbance alone, as the modes measure it in open loop
    closed = run(0.5)
    left = closed - run(0.5, disturbed=False)                       # ... and what the integrator leaves of it
    print(f"mode 0: open loop {np.abs(seen[20:, :, 0]).max(axis=0)} um, closed loop {np.abs(left[20:, :, 0]).max(axis=0)} um, "
          f"projection bound {floor[0]:.2e} um")
    assert np.abs(seen[:, :, 0]).max() > 100 * floor[0] > 0
    if kind != "pyramid":
        assert np.abs(seen[:, :, 1]).max() < 0.2 * np.abs(seen[:, :, 0]).max()
    assert (np.abs(left[20:, :, 0]).max(axis=0) < np.abs(seen[20:, :, 0]).max(axis=0)).all()
    mis = run(0.5, misreg=True)
    assert np.array_equal(mis[:, [0, 2]], closed[:, [0, 2]]) and not np.array_equal(mis[:, 1], closed[:, 1])
    rst = run(0.5, reset_at=12)
    assert np.array_equal(rst[:, [0, 2]], closed[:, [0, 2]]) and np.array_equal(rst[:12, 1], closed[:12, 1])
    assert not np.array_equal(rst[12:, 1], closed[12:, 1])
    env.clear_dm_per_env()
    env.clear_disturbance()


def test_refusals_leave_the_shard_stepping():
    """step_modal without a basis, run_integrator_modal without gains, a wrong K, non-finite entries: each fails with a message,
    and the shard steps on as a twin that saw none of it."""
    import torch
    from rlao_amd import _lib as L
    env, twin = _env("sh_fused", "f32"), _env("sh_fused", "f32", "b")
    lib, h = env._shard.lib, env._shard.h
    _prologue(env)
    _prologue(twin)
    obs = env.reset_soft()
    twin.reset_soft()
    buf = torch.zeros((N, 20), device=env.device, dtype=env.tdtype)
    p = C.c_void_p(buf.data_ptr())
    assert lib.aoenv_step_modal(h, 0, p, p, None, None, None, None) != 0 and b"no modal basis" in lib.aoenv_last_error()
    assert lib.aoenv_reset_soft_modal(h, p, None) != 0 and b"no modal basis" in lib.aoenv_last_error()
    assert lib.aoenv_run_integrator_modal(h, 0, 1, p, None, None, None, None) != 0 and b"no modal basis" in lib.aoenv_last_error()
    assert lib.aoenv_set_modal_gain(h, p, 0, None) != 0 and b"no modal basis" in lib.aoenv_last_error()
    with pytest.raises(L.AoEnvError, match="set_modal"):
        env.step_modal(0, buf)
    m2c, cm = env.M2C_CL.copy(), env.modal_CM.copy()
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    for K, what in ((0, b"outside"), (env.nValidAct + 1, b"outside")):
        cfg = L.AoModal(n_modes=K, h_m2c=ptr(m2c), h_cm=ptr(cm))
        assert lib.aoenv_set_modal(h, C.byref(cfg), None) != 0 and what in lib.aoenv_last_error()
    cfg = L.AoModal(n_modes=5, h_m2c=None, h_cm=ptr(cm))
    assert lib.aoenv_set_modal(h, C.byref(cfg), None) != 0 and b"null" in lib.aoenv_last_error()
    bad = m2c[:, :5].copy()
    bad[3, 2] = np.nan
    cfg = L.AoModal(n_modes=5, h_m2c=ptr(bad), h_cm=ptr(cm))
    assert lib.aoenv_set_modal(h, C.byref(cfg), None) != 0 and b"not finite" in lib.aoenv_last_error()
    badc = cm[:5].copy()
    badc[4, -1] = np.inf
    cfg = L.AoModal(n_modes=5, h_m2c=ptr(np.ascontiguousarray(m2c[:, :5])), h_cm=ptr(badc))
    assert lib.aoenv_set_modal(h, C.byref(cfg), None) != 0 and b"not finite" in lib.aoenv_last_error()
    assert lib.aoenv_step_modal(h, 0, p, p, None, None, None, None) != 0      # none of them left a basis behind
    with pytest.raises(ValueError, match="outside"):
        env.set_modal(21)
    env.set_modal(5)
    with pytest.raises(L.AoEnvError, match="set_modal_gain"):
        env.run_integrator_modal(0, 1)
    assert lib.aoenv_run_integrator_modal(h, 0, 1, p, None, None, None, None) != 0 and b"no modal gains" in lib.aoenv_last_error()
    for g in (np.array([0.1, 0.2, np.nan, 0.1, 0.1]), np.array([0.1, -0.2, 0.1, 0.1, 0.1])):
        assert lib.aoenv_set_modal_gain(h, ptr(g), 0, None) != 0 and b"not finite or negative" in lib.aoenv_last_error()
    assert lib.aoenv_run_integrator_modal(h, 0, 1, p, None, None, None, None) != 0      # ... nor gains
    with pytest.raises(ValueError, match="shape"):
        env.step_modal(0, torch.zeros((N, 4)))                      # a wrong K
    assert lib.aoenv_step_modal(h, 64, p, p, None, None, None, None) != 0 and b"outside" in lib.aoenv_last_error()
    assert lib.aoenv_step_modal(h, 0, None, p, None, None, None, None) != 0 and b"null" in lib.aoenv_last_error()
    env.clear_modal()
    assert env.n_modal == 0
    for k in range(4):                                              # the zonal loop goes on as if nothing had been asked
        r, rt = env.step(k, GAIN * obs), twin.step(k, GAIN * obs)
        assert all(torch.equal(r[q], rt[q]) for q in (0, 1, 2, 3))
        obs = r[0]
    _same_state(env, twin, "after the refusals", 4)
