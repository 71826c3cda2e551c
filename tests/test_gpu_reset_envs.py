"""GPU: partial reset (aoenv_reset_envs / BatchedAOEnv.reset_envs) -- a new episode for SOME envs of a shard.  The checker is the
full-reset path (generate_new_phase_screen, pinned to the reference by the golden replays): a listed env must afterwards be
BIT-IDENTICAL to the same env of a fresh shard of the same size reset with its seed, and every other env to the same env of a twin
shard that was never reset.  Every comparison is torch.equal / np.array_equal: there are no tolerances."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# 3.2 m, 8 x 8 lenslets of 6 px, R = 48; 25 m/s = 0.75 px per frame: pixel crossings on both sides of every reset
SMALL = dict(diameter=3.2, nSubaperture=8, nPixelPerSubap=6, r0=0.13, L0=30.0, windSpeed=[25.0], windDirection=[72.0],
             fractionalR0=[1.0], altitude=[0.0], nModes=20, nLoop=64)
SMALL3 = dict(SMALL, windSpeed=[10.0, 25.0, 18.0], windDirection=[0.0, 72.0, 200.0], fractionalR0=[0.6, 0.25, 0.15],
              altitude=[0.0, 1000.0, 5000.0])
SPEEDS = np.array([[0.0], [10.0], [17.0], [28.0], [12.0], [24.0]])
DIRS = np.array([[0.0], [72.0], [190.0], [270.0], [-45.0], [135.0]])


def _make(n, dtype="f32", geo=SMALL, wfs="shackhartmann", camera="ideal", stride=1):
    from rlao_amd.env import BatchedAOEnv
    env = BatchedAOEnv(n_envs=n, device=0, dtype=dtype, env_seed_stride=stride)
    env.set_params(geo, camera=camera, wfs_type=wfs)
    return env


def _prologue(env, seed, winds=None):
    """the full reset: new screens for every env, flat DM, one measurement -> reset_soft() observation"""
    env.generate_new_phase_screen(seed)
    if winds is not None:
        env.set_wind_per_env(winds[0], winds[1], reset=True)
    env.dm.coefs = 0
    env.dm_prev = 0
    env.measure()
    return env.reset_soft()


def _steps(env, obs, i0, i1, log, gain=0.5):
    for i in range(i0, i1):
        obs, frame, rew, sr, _, _ = env.step(i, gain * obs)
        log.append((obs.clone(), frame.clone(), rew.clone(), sr.clone()))
    return obs


def _partial(env, obs, ids, seed):
    """reset_envs, and the caller's observation with the rows of the listed envs replaced (the others' stay valid)"""
    import torch
    rows = env.reset_envs(ids, seed=seed)
    obs = obs.clone()
    obs[torch.as_tensor(list(ids), device=obs.device)] = rows
    return rows, obs


def _same(x, y, rows_x, rows_y=None):
    import torch
    rows_y = rows_x if rows_y is None else rows_y
    return all(torch.equal(p[rows_x], q[rows_y]) for p, q in zip(x, y))


def _final_state(env):
    """logical screens [nLayer, n, S, S] and clock accumulators [nLayer, n, 2] (shared clock: the layer's, for every env)"""
    from rlao_amd import _lib as L
    nl, n, S = env.param.nLayer, env.n_envs, env._atm_tables.S
    scr = env._shard.download(L.B_SCREEN, (nl, n, S, S), env._stream())
    if env._per_env_clock:
        buff = env._shard.get_clock_env(nl, n)[..., 2:]
    else:
        buff = np.repeat(env._shard.get_buff(nl)[:, None, :], n, axis=1)
    return scr, buff


def _check_partial(make, ids, k, n_steps, seed0=5, seed1=77, winds=None, seeds=None, others=None, make_fresh=None):
    """The two comparisons every scenario makes.  Shard A runs n_steps closed-loop steps with reset_envs(ids) after step k - 1;
    twin T is never reset; twin F is a fresh shard, fully reset with the new seed and stepped with i = k ...: A's listed envs == F's
    from step k on, the obs reset_envs returns == F's reset_soft() rows, A's other envs == T's over all steps; at the end screens
    and clock accumulators of every env equal its twin's."""
    import torch
    ids = list(ids)
    a, log_a = make(), []
    n = a.n_envs
    others = [e for e in range(n) if e not in ids] if others is None else others
    obs = _steps(a, _prologue(a, seed0, winds), 0, k, log_a)
    held = obs                                                      # what a caller holds across the reset
    held_copy = obs.clone()
    rows, obs = _partial(a, obs, ids, seed1 if seeds is None else np.asarray(seeds))
    assert a._per_env_clock and rows.shape == (len(ids), a.nActuator, a.nActuator) and rows.data_ptr() != a._obs.data_ptr()
    assert torch.equal(held, held_copy)                            # tensors handed out earlier are not written to
    assert torch.equal(a._obs[ids], rows) and torch.equal(a._obs[others], held[others])     # the retained obs (get_state) is coherent
    _steps(a, obs, k, n_steps, log_a)
    scr_a, buff_a = _final_state(a)
    a.close()
    t, log_t = make(), []
    _steps(t, _prologue(t, seed0, winds), 0, n_steps, log_t)
    scr_t, buff_t = _final_state(t)
    t.close()
    f, log_f = (make_fresh or make)(), []
    obs_f = _prologue(f, seed1, winds)
    _steps(f, obs_f, k, n_steps, log_f)
    scr_f, buff_f = _final_state(f)
    f.close()
    assert torch.equal(rows, obs_f[ids])
    for i in range(n_steps):
        assert _same(log_a[i], log_t[i], others), ("untouched envs", i)
        if i >= k:
            assert _same(log_a[i], log_f[i - k], ids), ("reset envs", i)
    assert not _same(log_a[-1], log_t[-1], ids)                     # the reset really changed the listed envs
    assert np.array_equal(scr_a[:, others], scr_t[:, others]) and np.array_equal(buff_a[:, others], buff_t[:, others])
    assert np.array_equal(scr_a[:, ids], scr_f[:, ids]) and np.array_equal(buff_a[:, ids], buff_f[:, ids])
    assert np.abs(buff_a).max() > 0


@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_partial_reset_in_mid_episode(dtype):
    """6 envs, 20 steps, envs 1 and 4 restarted after step 8: float32 runs the fused step kernel, float64 the batched kernels."""
    _check_partial(lambda: _make(6, dtype), [1, 4], 8, 20)


def test_reset_after_a_crossing_step_three_layers():
    """float32 fused kernel, 3 layers: the reset comes right after a step on which a layer crossed a pixel -- the ring pipeline
    then holds the operand of that layer's NEXT crossing (look-ahead) and the deferred-scatter machinery has just run; both must be
    flushed / forgotten before the clocks become per-env.  The crossing is read off the twin's host clock, not guessed."""
    probe = _make(1, "f32", SMALL3)
    obs = _prologue(probe, 5)
    ratio = probe._atm_tables.wind_ratio(probe.param.windSpeed, probe.param.windDirection, probe.param.samplingTime)
    k = None
    for i in range(12):
        before = probe._shard.get_buff(3).copy()
        obs = probe.step(i, 0.5 * obs)[0]
        crossed = (np.abs(before + ratio) >= 1).any(axis=1)
        after = probe._shard.get_buff(3)
        assert np.array_equal(crossed, (np.abs(after - (before + ratio)) > 0.5).any(axis=1))    # the accumulator wrapped there
        if i >= 3 and crossed.any():
            k = i + 1
            break
    assert probe.fused_step
    probe.close()
    assert k is not None, "no layer crossed a pixel in steps 3..11"
    _check_partial(lambda: _make(6, "f32", SMALL3), [1, 4], k, k + 10)


def test_per_env_winds_are_kept():
    """6 envs with 6 winds; env 3 (28 m/s along -y) restarted: its new episode == env 3 of a fresh per-env-wind shard."""
    _check_partial(lambda: _make(6, "f32"), [3], 6, 14, seed1=21, winds=(SPEEDS, DIRS))


def test_partial_reset_under_the_pyramid():
    """The Pyramid runs the batched kernels in float32."""
    geo = dict(SMALL, modulation=0.0)
    _check_partial(lambda: _make(4, "f32", geo, wfs="pyramid"), [0, 3], 5, 12)


@pytest.mark.parametrize("dtype,geo", [("f32", SMALL), ("f64", SMALL3)], ids=["f32-1layer", "f64-3layers"])
def test_resetting_every_env_equals_the_full_reset(dtype, geo):
    """The identity list against the null list: both resets run the same launches, so every env, step and final state is equal.
    float32 / one layer runs the fused step kernel, float64 / three layers the batched kernels."""
    import torch
    n = 5
    a, log_a = _make(n, dtype, geo), []
    obs = _steps(a, _prologue(a, 5), 0, 3, log_a)
    rows = a.reset_envs(range(n), seed=31)
    _steps(a, rows, 3, 9, log_a)
    scr_a, buff_a = _final_state(a)
    a.close()
    f, log_f = _make(n, dtype, geo), []
    obs_f = _prologue(f, 31)
    _steps(f, obs_f, 3, 9, log_f)
    scr_f, buff_f = _final_state(f)
    f.close()
    assert torch.equal(rows, obs_f)
    for x, y in zip(log_a[3:], log_f):
        assert _same(x, y, slice(None))
    assert np.array_equal(scr_a, scr_f) and np.array_equal(buff_a, buff_f)


def test_ragged_list_across_tile_boundaries_with_per_env_seeds():
    """67 envs (more than one 64-row tile of the ring GEMM), the list out of order and with one seed per listed env: env e gets
    40 + 3 e, which is what a fresh shard with env_seed_stride = 3 gives it.  A sample of the unlisted envs is undisturbed."""
    ids = [32, 0, 66, 1, 31]
    _check_partial(lambda: _make(67), ids, 4, 8, seed1=40, seeds=[40 + 3 * e for e in ids], others=[2, 30, 33, 65],
                   make_fresh=lambda: _make(67, stride=3))


def test_checkpoint_after_a_partial_reset():
    import torch
    a, log = _make(6), []
    obs = _steps(a, _prologue(a, 5), 0, 4, log)
    _, obs = _partial(a, obs, [1, 4], 77)
    obs = _steps(a, obs, 4, 6, log)
    snap = a.get_state()
    assert snap["clock_env"] is not None and snap["buff"] is None
    cont = []
    _steps(a, obs, 6, 10, cont)
    a.close()
    b, again = _make(6), []
    b.generate_new_phase_screen(1)                                  # some other state first
    b.set_state(snap)
    _steps(b, obs.clone(), 6, 10, again)
    b.close()
    for x, y in zip(cont, again):
        assert _same(x, y, slice(None))


def test_photon_noise():
    """camera = "papyrus" (photon noise).  reset_envs measures once: one camera frame number for the whole shard, so the untouched
    envs are bit-identical to a twin that called measure() at the reset step.  The reset envs ARE compared bit for bit with the
    fresh-shard twin: the two can share one frame-counter schedule -- the noise streams are indexed by (pixel, env, frame number), and
    the fresh twin makes the 7 measurements it is behind (6 steps and the first prologue's) before its own prologue; the counters
    are compared at the end to show the schedules agree."""
    import torch
    from rlao_amd import _lib as L
    ids, others, k, n_steps = [1, 4], [0, 2, 3, 5], 6, 12
    make = lambda: _make(6, camera="papyrus")                        # noqa: E731
    a, log_a = make(), []
    obs = _steps(a, _prologue(a, 5), 0, k, log_a)
    rows, obs = _partial(a, obs, ids, 77)
    _steps(a, obs, k, n_steps, log_a)
    cnt_a = a._shard.download(L.B_COUNTERS, (4,), a._stream(), dtype=np.uint32)
    a.close()
    t, log_t = make(), []
    obs = _steps(t, _prologue(t, 5), 0, k, log_t)
    t.measure()
    _steps(t, obs, k, n_steps, log_t)
    t.close()
    f, log_f = make(), []
    for _ in range(k + 1):
        f.measure()
    obs_f = _prologue(f, 77)
    _steps(f, obs_f, k, n_steps, log_f)
    cnt_f = f._shard.download(L.B_COUNTERS, (4,), f._stream(), dtype=np.uint32)
    f.close()
    assert np.array_equal(cnt_a, cnt_f) and cnt_a[0] > n_steps
    assert torch.equal(rows, obs_f[ids])
    for i in range(n_steps):
        assert _same(log_a[i], log_t[i], others), ("untouched envs", i)
        if i >= k:
            assert _same(log_a[i], log_f[i - k], ids), ("reset envs", i)
            fr = log_a[i][1][ids]
            assert torch.isfinite(fr).all() and not torch.equal(fr, log_t[i][1][ids])
    assert not torch.equal(log_a[-1][1][others], log_a[-2][1][others])         # (the frames are noisy: no two alike)


def test_refusals_leave_the_shard_alone():
    import torch
    from rlao_amd import _lib as L
    a, t = _make(4), _make(4)
    oa, ot = (_steps(e, _prologue(e, 5), 0, 2, []) for e in (a, t))
    sh, p, at = a._shard, a.param, a._atm_tables
    px = at.layer_D / at.N
    one = np.array([[7]], dtype=np.uint32)
    with pytest.raises(L.AoEnvError, match="outside"):
        sh.reset_envs([0, 4], np.tile(one, (2, 1)), np.tile(one, (2, 1)), p.r0, p.L0, px)
    with pytest.raises(L.AoEnvError, match="outside"):
        sh.reset_envs([-1], one, one, p.r0, p.L0, px)
    with pytest.raises(L.AoEnvError, match="twice"):
        sh.reset_envs([1, 1], np.tile(one, (2, 1)), np.tile(one, (2, 1)), p.r0, p.L0, px)
    for bad in ((0.0, p.L0, px), (p.r0, -1.0, px), (p.r0, p.L0, 0.0)):
        with pytest.raises(L.AoEnvError, match="positive"):
            sh.reset_envs([1], one, one, *bad)
    idx = np.array([1], dtype=np.int32)
    ptr = lambda x: x.ctypes.data_as(C.c_void_p)                     # noqa: E731
    assert sh.lib.aoenv_reset_envs(sh.h, None, 1, ptr(one), ptr(one), p.r0, p.L0, px, None) != 0
    assert sh.lib.aoenv_reset_envs(sh.h, ptr(idx), 1, None, ptr(one), p.r0, p.L0, px, None) != 0
    assert sh.lib.aoenv_reset_envs(sh.h, ptr(idx), 1, ptr(one), None, p.r0, p.L0, px, None) != 0
    assert b"null" in sh.lib.aoenv_last_error()
    assert sh.lib.aoenv_reset_envs(sh.h, ptr(idx), -1, ptr(one), ptr(one), p.r0, p.L0, px, None) != 0
    assert sh.lib.aoenv_reset_envs(None, ptr(idx), 1, ptr(one), ptr(one), p.r0, p.L0, px, None) != 0
    with pytest.raises(ValueError):
        a.reset_envs([4])
    with pytest.raises(ValueError):
        a.reset_envs([1, 1])
    with pytest.raises(ValueError):
        a.reset_envs([1, 2], seed=[3])
    # the empty list is a no-op: not even the clocks are switched
    assert a.reset_envs([]).shape == (0, a.nActuator, a.nActuator)
    assert sh.lib.aoenv_reset_envs(sh.h, None, 0, None, None, p.r0, p.L0, px, None) == 0
    assert not a._per_env_clock
    with pytest.raises(L.AoEnvError, match="shared clock"):
        sh.get_clock_env(1, 4)
    # nothing changed: one more step equals the twin's
    xa, xt = [], []
    _steps(a, oa, 2, 3, xa)
    _steps(t, ot, 2, 3, xt)
    assert _same(xa[0], xt[0], slice(None))
    sa, st = _final_state(a), _final_state(t)
    assert np.array_equal(sa[0], st[0]) and np.array_equal(sa[1], st[1])
    # a shard without atmosphere; one whose ring tables were never uploaded
    for n_layer, msg in ((0, "no atmosphere"), (1, "not been uploaded")):
        raw = a._make_shard(2, "f32", n_layer=n_layer, max_group=1)
        with pytest.raises(L.AoEnvError, match=msg):
            raw.reset_envs([0], one, one, p.r0, p.L0, px)
        raw.close()
    a.close()
    t.close()
    # layers on grids of their own (fov = 1 arcsec with layers at altitude): no per-env clocks
    g = _make(2, geo=dict(SMALL3, fov=1.0))
    assert not g._atm_tables.uniform
    with pytest.raises(L.AoEnvError, match="grids of their own"):
        g.reset_envs([0], seed=3)
    assert not g._per_env_clock
    g.close()
