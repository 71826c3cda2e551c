"""GPU: the command-space disturbance (aoenv_set_disturbance / BatchedAOEnv.set_disturbance): per-env vibration lines that the
stepped loops -- step, run_integrator, rollout, policy_rollout -- see on top of dm.coefs, as the reference's vibration envs do with
``dm.coefs = vibration_state + correction_state`` (MAIN/OOPAOEnv/vibrationEnv.py:119-123, 146-167, 197-202).

Checkers: ``env.disturbance(i)``, the model of rlao_amd/csrc/disturb.hpp in NumPy float64 on the host (pinned against the host
driver in tests/test_disturb_host.py), and the env's own step: a twin with no disturbance whose dm.coefs is set to the side buffer
``dm.coefs_seen`` before each step must reproduce every bit, and so must a disturbed twin stepped with a rollout's recorded actions.

Tolerances of the side buffer (u = 2^-24 for float32 shards, 2^-53 for float64), per actuator a, with S = sum_m |B[a][m]| |v[m]|:
(M + 2) u (|coefs| + S): the roundings of B and v into the env dtype, the M fused multiply-adds, the one addition; float64 adds
sum_m |B[a][m]| sum_j amp[m][j] 2^-50 for the sines of two libraries."""
import ctypes as C

import numpy as np
import pytest

import _policy_ref as P

pytestmark = pytest.mark.gpu

SMALL = dict(diameter=3.2, nSubaperture=8, nPixelPerSubap=6, r0=0.13, L0=30.0, windSpeed=[10.0], windDirection=[72.0],
             fractionalR0=[1.0], altitude=[0.0], nModes=20, nLoop=64)
SMALL3 = dict(SMALL, windSpeed=[10.0, 25.0, 18.0], windDirection=[0.0, 72.0, 200.0], fractionalR0=[0.6, 0.25, 0.15],
              altitude=[0.0, 1000.0, 5000.0])
GAIN = 0.4
KINDS = {
    "f32_fused": dict(dtype="f32"),
    "f64_batched": dict(dtype="f64"),
    "pyramid": dict(dtype="f32", geo=dict(SMALL, modulation=0.0), wfs="pyramid"),
    "3layer_env_clocks": dict(dtype="f32", geo=SMALL3),
}
M, J = 3, 2


def _make(n, dtype="f32", geo=SMALL, wfs="shackhartmann", **kw):
    from rlao_amd.env import BatchedAOEnv
    env = BatchedAOEnv(n_envs=n, device=0, dtype=dtype, **kw)
    env.set_params(geo, camera="ideal", wfs_type=wfs, gainCL=GAIN)
    return env


def _winds(kind, n=4):
    if kind != "3layer_env_clocks":
        return None
    return (np.tile(SMALL3["windSpeed"], (n, 1)) + np.arange(n)[:, None], np.tile(SMALL3["windDirection"], (n, 1)) + 20.0 * np.arange(n)[:, None])


def _prologue(env, seed=5, winds=None):
    env.generate_new_phase_screen(seed)
    if winds is not None:
        env.set_wind_per_env(winds[0], winds[1], reset=True)
    env.dm.coefs = 0
    env.dm_prev = 0
    env.measure()
    env.SR = []
    return env.reset_soft()


def _lines(env, n=4, seed=3, m=M, j=J):
    """amp [n, m, j] in metres (the 1e-7 of vibrationEnv), freq in Hz (0.01 .. 0.45 cycles per frame, 53 random bits), phase in
    cycles: different for every env, mode and line"""
    rng = np.random.RandomState(seed)
    return (rng.uniform(0.2e-7, 1e-7, (n, m, j)), rng.uniform(0.01, 0.45, (n, m, j)) / env.param.samplingTime, rng.uniform(0.0, 1.0, (n, m, j)))


def _same(a, b):
    """obs, frame, reward, strehl of two step() results"""
    import torch
    return all(torch.equal(a[q], b[q]) for q in (0, 1, 2, 3))


@pytest.mark.parametrize("kind", list(KINDS))
def test_side_buffer_against_the_formula(kind):
    """coefs_seen minus the coefs read before the step equals disturbance(i), at frames 0, 1, 63 with t0 = 0 and t0 = 10^9."""
    from rlao_amd.env import disturbance_value
    env = _make(4, **KINDS[kind])
    if kind != "3layer_env_clocks":
        assert env.fused_step == (kind == "f32_fused")
    obs = _prologue(env, winds=_winds(kind))
    amp, hz, phase = _lines(env)
    B = env.M2C_CL[:, :M]
    u = 2.0 ** -24 if env.dtype == "f32" else 2.0 ** -53
    worst = 0.0
    for t0 in (0, 10 ** 9):
        env.set_disturbance(M, amp, hz, phase, t0=t0)
        for i in (0, 1, 63):
            c0 = np.asarray(env.dm.coefs, dtype=np.float64)
            obs = env.step(i, GAIN * obs)[0]
            seen = env.dm.coefs_seen
            assert tuple(seen.shape) == (4, env.nValidAct) and seen.dtype == env.tdtype and seen.is_cuda
            want = env.disturbance(i)
            v = disturbance_value(dict(env._disturb, modes=np.eye(M)), i)                       # [4, M]
            tol = (M + 2) * u * (np.abs(c0) + np.abs(v) @ np.abs(B).T)
            if env.dtype == "f64":
                tol = tol + (amp.sum(axis=2) @ np.abs(B).T) * 2.0 ** -50
            err = np.abs(seen.double().cpu().numpy() - c0 - want)
            worst = max(worst, float((err / tol).max()))
            print(f"{kind} t0={t0} i={i}: max err / tol = {(err / tol).max():.3f}, max |d| = {np.abs(want).max():.3e}, max |coefs| = {np.abs(c0).max():.3e}")
            assert (err <= tol).all(), (kind, t0, i)
            assert np.abs(want).max() > 1e-8 and (i == 0 or np.abs(c0).max() > 1e-8)
            # the step went on writing the pure command: dm.coefs = leak dm_prev + action is what dm_prev now holds
            assert np.array_equal(np.asarray(env.dm.coefs), np.asarray(env.dm_prev))
    env.close()


@pytest.mark.parametrize("kind", list(KINDS))
def test_the_step_sees_exactly_that_buffer(kind):
    """12 frames: a twin with NO disturbance, given dm.coefs = env.dm.coefs_seen before each step and the same action, returns the
    same bits; env's command and integrator state are those of a third env that never saw a disturbance."""
    import torch
    env, twin, third = (_make(4, **KINDS[kind]) for _ in range(3))
    w = _winds(kind)
    obs = _prologue(env, winds=w)
    _prologue(twin, winds=w)
    _prologue(third, winds=w)
    env.set_disturbance(M, *_lines(env))
    differs = False
    for k in range(12):
        a = GAIN * obs
        r = env.step(k, a)
        twin.dm.coefs = env.dm.coefs_seen
        rt = twin.step(k, a)
        assert _same(r, rt), (kind, k)
        plain = third.step(k, a)                                    # the same actions, no disturbance
        differs = differs or not torch.equal(r[0], plain[0])
        obs = r[0]
    assert differs                                                  # the disturbance was seen at all
    assert np.array_equal(env.residual[:12], twin.residual[:12]) and np.array_equal(env.total[:12], twin.total[:12])
    a, b = env.get_state(), third.get_state()
    for key in ("coefs", "dm_prev", "screen", "mt"):
        assert np.array_equal(np.asarray(a[key]), np.asarray(b[key])), (kind, key)
    for e in (env, twin, third):
        e.close()


@pytest.mark.parametrize("kind", ["f32_fused", "f64_batched"])
def test_every_loop(kind):
    """rollout, policy_rollout and run_integrator on a disturbed env against a twin with the same disturbance stepped frame by
    frame: the recorded rollouts bit for bit, the integrator within the 1e-6 that test_sigma_zero_is_the_integrator grants its
    fused gain * obs; an env with no disturbance gives other trajectories."""
    import torch
    env, twin, plain = (_make(4, **KINDS[kind]) for _ in range(3))
    assert env.fused_step == (kind == "f32_fused")
    lines = _lines(env)
    for e in (env, twin):
        e.set_disturbance(M, *lines, t0=7)
    pw = P.make_weights(3, 16, seed=5, scale=(20.0, 1.5, 2.0))
    for e in (env, plain):
        e.set_policy(pw)

    def check(run):
        obs0 = _prologue(env)
        tr = run(env)
        o = _prologue(twin)
        assert torch.equal(tr.obs[0], obs0) and torch.equal(o, obs0)
        for k in range(12):
            o, fr, r, s, _, _ = twin.step(k, tr.action[k])
            assert torch.equal(tr.obs[k + 1], o) and torch.equal(tr.reward[k], r) and torch.equal(tr.strehl[k], s), (kind, k)
        assert torch.equal(env._frame, fr)
        a, b = env.get_state(), twin.get_state()
        for key in ("screen", "coefs", "dm_prev", "mt", "signal"):
            assert np.array_equal(np.asarray(a[key]), np.asarray(b[key])), (kind, key)
        assert np.array_equal(env.dm.coefs_seen.cpu().numpy(), twin.dm.coefs_seen.cpu().numpy())
        _prologue(plain)
        other = run(plain)
        assert torch.equal(other.obs[0], obs0) and not torch.equal(other.obs[1], tr.obs[1]) and not torch.equal(other.obs[-1], tr.obs[-1])

    check(lambda e: e.rollout(0, 12, 0.05, seed=11))
    check(lambda e: e.policy_rollout(0, 12)[0])
    # the integrator: action = gain * obs fused into the step's epilogue
    _prologue(env)
    obs, rew, sr = env.run_integrator(0, 12)
    o = _prologue(twin)
    for k in range(12):
        o, _, r, s, _, _ = twin.step(k, GAIN * o)
    torch.cuda.synchronize()
    np.testing.assert_allclose(obs.cpu().numpy(), o.cpu().numpy(), atol=1e-6)
    np.testing.assert_allclose(sr.cpu().numpy(), s.cpu().numpy(), atol=1e-6)
    _prologue(plain)
    pobs, _, _ = plain.run_integrator(0, 12)
    assert float((pobs - obs).abs().max()) > 1e-3                   # micrometres: a thousand times the tolerance above
    for e in (env, twin, plain):
        e.close()


@pytest.mark.parametrize("kind", list(KINDS))
def test_off_means_off(kind):
    """12 steps and one rollout: an env that never set a disturbance, one that set and cleared one, one whose amplitudes are all
    zero -- the same bits (the zero-amplitude env: equal in value)."""
    import torch
    never, cleared, zero = (_make(4, **KINDS[kind]) for _ in range(3))
    amp, hz, phase = _lines(never)
    cleared.set_disturbance(M, amp, hz, phase)
    cleared.clear_disturbance()
    zero.set_disturbance(M, np.zeros_like(amp), hz, phase, t0=10 ** 9)
    assert (cleared.disturbance(3) == 0).all() and (zero.disturbance(3) == 0).all()
    w = _winds(kind)
    obs = [_prologue(e, winds=w) for e in (never, cleared, zero)]
    assert torch.equal(obs[0], obs[1]) and torch.equal(obs[0], obs[2])
    o = obs[0]
    for k in range(12):
        a = GAIN * o
        c0 = np.asarray(zero.dm.coefs)
        rs = [e.step(k, a) for e in (never, cleared, zero)]
        assert _same(rs[0], rs[1]) and _same(rs[0], rs[2]), (kind, k)
        o = rs[0][0]
    # the zero-amplitude env did write its side buffer: the command of before the step, in value
    assert np.array_equal(zero.dm.coefs_seen.cpu().numpy(), c0) and np.abs(c0).max() > 1e-8
    trs = [e.rollout(12, 6, 0.05, seed=3) for e in (never, cleared, zero)]
    for t in trs[1:]:
        assert all(torch.equal(x, y) for x, y in zip(trs[0], t)), kind
    states = [e.get_state() for e in (never, cleared, zero)]
    for s in states[1:]:
        for key in ("screen", "coefs", "dm_prev", "mt", "signal", "counters"):
            assert np.array_equal(np.asarray(states[0][key]), np.asarray(s[key])), (kind, key)
        assert np.array_equal(never.total[:18], cleared.total[:18]) and np.array_equal(never.total[:18], zero.total[:18])
    for e in (never, cleared, zero):
        e.close()


@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_batch_position_and_env_ids(dtype):
    """Env 3 of a 4-env shard against env 0 of a 1-env shard with env 3's lines and the same coefs: the same bits.  env_ids=[1, 3]
    changes rows 1 and 3 only."""
    env4, env1 = _make(4, dtype), _make(1, dtype)
    obs4, obs1 = _prologue(env4), _prologue(env1)
    amp, hz, phase = _lines(env4)
    A = env4.nValidAct
    c = np.random.RandomState(8).normal(0, 2e-7, (4, A)).astype(np.float32 if dtype == "f32" else np.float64).astype(np.float64)
    env4.set_disturbance(M, amp, hz, phase, t0=123456789)
    env1.set_disturbance(M, amp[3:], hz[3:], phase[3:], t0=123456789)

    def seen(env, coefs, i=5):
        env.dm.coefs = coefs
        env.step(i, 0 * (obs4 if env is env4 else obs1))
        return env.dm.coefs_seen.cpu().numpy().astype(np.float64)

    s4, s1 = seen(env4, c), seen(env1, c[3])
    assert np.array_equal(s4[3], s1[0]) and np.array_equal(s4[3] - c[3], s1[0] - c[3])
    assert np.abs(s4[3] - c[3]).max() > 1e-8 and not np.array_equal(s4[0] - c[0], s4[3] - c[3])
    amp2, hz2, ph2 = _lines(env4, n=2, seed=4)
    env4.set_disturbance(None, amp2, hz2, ph2, t0=123456789, env_ids=[1, 3])
    t4 = seen(env4, c)
    assert np.array_equal(t4[[0, 2]], s4[[0, 2]])
    assert not np.array_equal(t4[1], s4[1]) and not np.array_equal(t4[3], s4[3])
    env1.set_disturbance(M, amp2[1:], hz2[1:], ph2[1:], t0=123456789)              # the second listed env is env 3
    assert np.array_equal(seen(env1, c[3])[0], t4[3])
    env4.close()
    env1.close()


def test_it_is_a_vibration():
    """gain 0, zero actions, 64 frames, one tip line of 1e-7 m at 8 / 64 cycles per frame: the mode-0 projection of the difference
    between the disturbed and the undisturbed observations (identical screens) has its largest non-DC rfft bin at bin 8."""
    import torch
    dist, calm = _make(2), _make(2)
    o = _prologue(dist)
    _prologue(calm)
    dist.set_disturbance(1, [[1e-7]], [[(8.0 / 64.0) / dist.param.samplingTime]])
    zero = torch.zeros_like(o)
    idx = torch.as_tensor(np.asarray(dist._dm_tables.act_idx, dtype=np.int64), device=o.device)
    mode0 = torch.as_tensor(np.linalg.pinv(dist.M2C_CL)[0], device=o.device, dtype=torch.float64)
    proj = []
    for k in range(64):
        d = dist.step(k, zero)[0] - calm.step(k, zero)[0]
        proj.append((d.reshape(2, -1)[:, idx].double() @ mode0).cpu().numpy())
    assert (np.asarray(dist.dm.coefs) == 0).all()                   # nothing was corrected: the command stayed flat
    spec = np.abs(np.fft.rfft(np.array(proj), axis=0))              # [33, 2]
    print("spectrum of env 0:", np.round(spec[:, 0] / spec[1:, 0].max(), 3))
    assert (np.argmax(spec[1:], axis=0) + 1 == 8).all()
    dist.close()
    calm.close()


def test_refusals_through_the_abi_change_nothing():
    from rlao_amd import _lib as L
    env, twin = _make(2), _make(2)
    obs = _prologue(env)
    _prologue(twin)
    lib, h, A, N = env._shard.lib, env._shard.h, env.nValidAct, 2
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)

    def call(m, j, amp_fill=1e-7, null_modes=False, poke=None):
        B = np.ones((A, max(m, 1)))
        arrs = [np.full((N, max(m, 1), j), v) for v in (amp_fill, 0.1, 0.0)]
        if poke is not None:
            arrs[0][1, 0, 0] = poke
        cfg = L.AoDisturbance(n_modes=m, n_lines=j, t0=0, h_modes=None if null_modes else ptr(B), h_amp=ptr(arrs[0]), h_freq=ptr(arrs[1]),
                              h_phase=ptr(arrs[2]))
        return lib.aoenv_set_disturbance(h, C.byref(cfg), C.c_void_p(env._stream()))

    for kw in (dict(m=0, j=1), dict(m=65, j=1), dict(m=2, j=9), dict(m=2, j=0), dict(m=2, j=2, poke=np.nan), dict(m=2, j=2, poke=-1e-9),
               dict(m=2, j=2, poke=np.inf), dict(m=2, j=2, null_modes=True)):
        assert call(**kw) != 0, kw
        assert len(lib.aoenv_last_error()) > 0
        a = GAIN * obs
        r, rt = env.step(0, a), twin.step(0, a)
        assert _same(r, rt), kw
        obs = r[0]
    with pytest.raises(ValueError):
        env.set_disturbance(2, np.full((2, 2), -1.0), np.zeros((2, 2)))
    # a refused call leaves a disturbance in force as it was: the same command and frame give the same side buffer
    assert call(2, 2) == 0
    c0 = np.asarray(env.dm.coefs)
    env.step(1, 0 * obs)
    before = env.dm.coefs_seen.cpu().numpy()
    assert float(np.abs(before - c0).max()) > 1e-8
    assert call(2, 2, poke=np.nan) != 0 and call(3, 1, null_modes=True) != 0
    env.dm.coefs = c0
    env.step(1, 0 * obs)
    assert np.array_equal(env.dm.coefs_seen.cpu().numpy(), before)
    env.close()
    twin.close()
