"""GPU: per-env winds of a pixel per frame and more (AOENV_OPT_ENV_WIND_PIXELS; env.set_wind_ceiling, set_wind_per_env(max_pixels=)).
A per-env clock then makes whole-pixel ring rounds (k_ring_round_env) in front of its sub-pixel crossing, in the order of the shared
host clock, which has served such winds all along and is pinned to the reference above one pixel per frame by
tests/golden/tiny_fastwind.npz.  That clock is the checker: an env stepped by its own clock must be BIT-IDENTICAL to a shard of the
same size stepped with that wind on the shared clock (the same n_envs: the ring GEMM's split count is the same on both sides).  Every
comparison but the oracle's is torch.equal / np.array_equal.

Geometry: 3.2 m, 8 x 8 lenslets of 6 px, R = 48 (the smallest at which the fused step kernel runs): a pixel is 6.67 cm, at 500 Hz one
pixel per frame is 33.3 m/s."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SMALL = dict(diameter=3.2, nSubaperture=8, nPixelPerSubap=6, r0=0.13, L0=30.0, windSpeed=[10.0], windDirection=[72.0],
             fractionalR0=[1.0], altitude=[0.0], nModes=20, nLoop=64)
SMALL3 = dict(SMALL, windSpeed=[10.0, 25.0, 18.0], windDirection=[0.0, 72.0, 200.0], fractionalR0=[0.6, 0.25, 0.15],
              altitude=[0.0, 1000.0, 5000.0])
TINY_PYR = dict(diameter=1.6, nSubaperture=4, nPixelPerSubap=6, r0=0.13, L0=30.0, windSpeed=[10.0], windDirection=[72.0],
                fractionalR0=[1.0], altitude=[0.0], nModes=8, nLoop=64, modulation=0.0)
# floors of |ratio| per axis: (0,0) (0,0) (1,0) (0,1) (1,1) (2,2) (2,1): no round, one axis, diagonal, diagonal then single-axis,
# negative signs, and envs that sit out rounds others take
FAST_SPEEDS = np.array([[0.0], [28.0], [40.0], [50.0], [75.0], [110.0], [95.0]])
FAST_DIRS = np.array([[0.0], [72.0], [190.0], [270.0], [-45.0], [135.0], [30.0]])
FAST_FLOORS = [(0, 0), (0, 0), (1, 0), (0, 1), (1, 1), (2, 2), (2, 1)]
# the slow winds of tests/test_gpu_wind.py (all below one pixel per frame)
SPEEDS = np.array([[0.0], [10.0], [17.0], [28.0], [12.0], [24.0]])
DIRS = np.array([[0.0], [72.0], [190.0], [270.0], [-45.0], [135.0]])


def _make(n, dtype="f32", geo=SMALL, stride=0, wfs="shackhartmann"):
    from rlao_amd.env import BatchedAOEnv
    env = BatchedAOEnv(n_envs=n, device=0, dtype=dtype, env_seed_stride=stride)   # stride 0: the same screens in every env
    env.set_params(geo, camera="ideal", wfs_type=wfs)
    return env


def _prologue(env, seed, winds=None, ceiling=None, raw=None):
    """the full reset.  winds = (speed, direction) [n_envs, nLayer]: per-env clocks; raw = ratio [nLayer, n_envs, 2] straight into
    aoenv_set_wind_env, or [nLayer, 2] into aoenv_set_wind (the shared clock)"""
    env.generate_new_phase_screen(seed)
    if winds is not None:
        env.set_wind_per_env(winds[0], winds[1], reset=True, max_pixels=ceiling)
    elif ceiling is not None:
        env.set_wind_ceiling(ceiling)
    if raw is not None:
        raw = np.asarray(raw, dtype=np.float64)
        if raw.ndim == 3:
            env._shard.set_wind_env(raw, True, env._stream())
        else:
            env._shard.set_wind(raw, True)
    env.dm.coefs = 0
    env.dm_prev = 0
    env.measure()
    return env.reset_soft()


def _steps(env, obs, i0, i1, log, gain=0.5):
    import torch
    for i in range(i0, i1):
        obs, frame, rew, sr, _, _ = env.step(i, gain * obs)
        log.append((obs.clone(), frame.clone(), rew.clone(), sr.clone()))
    torch.cuda.synchronize()
    return obs


def _state(env, per_env):
    """logical screens [nLayer, n, S, S] and clock accumulators [nLayer, n, 2] (shared clock: the layer's, for every env)"""
    from rlao_amd import _lib as L
    nl, n, S = env.param.nLayer, env.n_envs, env._atm_tables.S
    scr = env._shard.download(L.B_SCREEN, (nl, n, S, S), env._stream())
    if per_env:
        buff = env._shard.get_clock_env(nl, n)[..., 2:]
    else:
        buff = np.repeat(env._shard.get_buff(nl)[:, None, :], n, axis=1)
    return scr, buff


def _same(x, y, rows_x, rows_y=None):
    import torch
    rows_y = rows_x if rows_y is None else rows_y
    return all(torch.equal(p[rows_x], q[rows_y]) for p, q in zip(x, y))


# ---- 1. each env equals a shard with its wind -------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_each_fast_env_equals_a_shard_with_its_wind(dtype):
    """7 envs, ceiling 4, winds up to 3.3 px per frame, 10 closed-loop steps: env e == env e of a shared-clock shard of 7 envs whose
    wind is wind e -- obs, frame, reward, Strehl on every step, the logical screen and the accumulator at the end.  float32 runs the
    fused step kernel (the sub-pixel ring deferred to it), float64 the batched kernels."""
    import torch
    n, steps = len(FAST_SPEEDS), 10
    env = _make(n, dtype)
    got = []
    _steps(env, _prologue(env, 9, winds=(FAST_SPEEDS, FAST_DIRS), ceiling=4), 0, steps, got)
    assert env.wind_pixels == 4 and env._per_env_clock and env.fused_step == (dtype == "f32")
    scr, buff = _state(env, True)
    clk = env._shard.get_clock_env(1, n)
    env.close()
    floors = [(int(abs(clk[0, e, 1])), int(abs(clk[0, e, 0]))) for e in range(n)]      # (y, x): direction 0 blows along y
    assert floors == FAST_FLOORS and np.abs(clk[0, :, :2]).max() > 2
    assert np.abs(buff).max() < 1
    for e in range(n):
        ref = _make(n, dtype)
        ref.atm.windSpeed = list(FAST_SPEEDS[e])
        ref.atm.windDirection = list(FAST_DIRS[e])
        want = []
        _steps(ref, _prologue(ref, 9), 0, steps, want)
        assert not ref._per_env_clock
        rs, rb = _state(ref, False)
        ref.close()
        for i in range(steps):
            assert _same(got[i], want[i], e), (e, i)
        assert np.array_equal(scr[0, e], rs[0, e]) and np.array_equal(buff[0, e], rb[0, e]), e
    assert not np.array_equal(scr[0, 5], scr[0, 1])                 # the fastest env's screen is not the 28 m/s env's
    assert not torch.equal(got[-1][0][5], got[-1][0][1])


# ---- 2. exact integers ------------------------------------------------------------------------------------------------------------
def test_whole_pixel_ratios_through_the_shard_api():
    """Raw ratios through aoenv_set_wind_env: (1, 0) and (-2, 1) have no fractional part (the sub-pixel clock never crosses: whole
    rounds alone), (0, 0) never moves, and the last env sits just under one pixel on x and just under the ceiling on y -- the
    largest ceiling, 8: seven rounds per step, the torus origin wraps.  Twins: the same ratio through aoenv_set_wind."""
    import torch
    ratios = [(1.0, 0.0), (-2.0, 1.0), (0.0, 0.0), (float(np.nextafter(1.0, 0.0)), float(np.nextafter(8.0, 0.0)))]
    n, steps = len(ratios), 8
    env = _make(n)
    got = []
    _steps(env, _prologue(env, 4, ceiling=8, raw=np.array(ratios)[None]), 0, steps, got)
    scr = _state(env, True)[0]
    clk = env._shard.get_clock_env(1, n)
    env.close()
    assert np.array_equal(clk[0, :3, 2:], np.zeros((3, 2)))          # no fractional part: the accumulators never left 0
    for e, r in enumerate(ratios):
        ref = _make(n)
        want = []
        _steps(ref, _prologue(ref, 4, raw=np.array([r])), 0, steps, want)
        rs, rb = _state(ref, False)
        ref.close()
        for i in range(steps):
            assert _same(got[i], want[i], e), (r, i)
        assert np.array_equal(scr[0, e], rs[0, e]) and np.array_equal(clk[0, e, 2:], rb[0, e]), r
    assert not torch.equal(got[-1][0][0], got[-1][0][2])


# ---- 3. three layers, launch counts -----------------------------------------------------------------------------------------------
def test_three_layers_with_a_fast_middle_layer_and_the_launch_count():
    """3 layers, only the middle one fast (75 m/s at 72 deg: ratio (0.70, 2.14), two rounds), 4 envs with seeds of their own: uniform
    winds through the per-env path == the shared clock.  With profiling on, the ring-prepare stage is launched steps x sum over
    the layers of (1 + rounds of the layer) times: a layer pays for its own rounds only."""
    geo = dict(SMALL3, windSpeed=[10.0, 75.0, 18.0])
    steps, outs = 10, []
    for per_env in (False, True):
        env = _make(4, geo=geo, stride=1)
        w = (np.tile(geo["windSpeed"], (4, 1)), np.tile(geo["windDirection"], (4, 1))) if per_env else None
        obs = _prologue(env, 3, winds=w, ceiling=3 if per_env else None)
        env._shard.profile(True)
        log = []
        _steps(env, obs, 0, steps, log)
        prof = env._shard.profile_read(env._stream())
        env._shard.profile(False)
        outs.append((log, _state(env, per_env)))
        if per_env:
            assert prof["ring_prepare"][1] == steps * ((1 + 0) + (1 + 2) + (1 + 0)), prof
            assert prof["gemm_ring"][1] == steps * 5, prof
        env.close()
    for i in range(steps):
        assert _same(outs[0][0][i], outs[1][0][i], slice(None)), i
    assert np.array_equal(outs[0][1][0], outs[1][1][0]) and np.array_equal(outs[0][1][1], outs[1][1][1])


# ---- 4. raising the ceiling is free for slow shards ------------------------------------------------------------------------------
def test_a_raised_ceiling_changes_nothing_for_slow_winds():
    """The winds of tests/test_gpu_wind.py (all below a pixel per frame) with ceiling 4 against ceiling 1: the same outputs bit for
    bit, and the same number of launches of every profiled kernel."""
    steps, runs = 12, []
    for ceiling in (None, 4):
        env = _make(len(SPEEDS))
        obs = _prologue(env, 9, winds=(SPEEDS, DIRS), ceiling=ceiling)
        assert env.wind_pixels == (ceiling or 1)
        env._shard.profile(True)
        log = []
        _steps(env, obs, 0, steps, log)
        prof = env._shard.profile_read(env._stream())
        env._shard.profile(False)
        runs.append((log, _state(env, True), {k: v[1] for k, v in prof.items()}))
        env.close()
    for i in range(steps):
        assert _same(runs[0][0][i], runs[1][0][i], slice(None)), i
    assert np.array_equal(runs[0][1][0], runs[1][1][0]) and np.array_equal(runs[0][1][1], runs[1][1][1])
    assert runs[0][2] == runs[1][2] and runs[0][2]["ring_prepare"] == steps, runs[0][2]


# ---- 5. Pyramid -------------------------------------------------------------------------------------------------------------------
def test_fast_per_env_winds_under_the_pyramid():
    """The Pyramid runs the batched kernels in float32: 3 envs, one of them at 2.85 px per frame, each equal to its twin."""
    sp, di = FAST_SPEEDS[[1, 6, 2]], FAST_DIRS[[1, 6, 2]]
    steps = 8
    env = _make(3, geo=TINY_PYR, wfs="pyramid")
    got = []
    _steps(env, _prologue(env, 5, winds=(sp, di), ceiling=3), 0, steps, got)
    scr = _state(env, True)[0]
    env.close()
    for e in range(3):
        ref = _make(3, geo=TINY_PYR, wfs="pyramid")
        ref.atm.windSpeed = list(sp[e])
        ref.atm.windDirection = list(di[e])
        want = []
        _steps(ref, _prologue(ref, 5), 0, steps, want)
        rs = _state(ref, False)[0]
        ref.close()
        for i in range(steps):
            assert _same(got[i], want[i], e), (e, i)
        assert np.array_equal(scr[0, e], rs[0, e]), e
    assert not np.array_equal(scr[0, 0], scr[0, 1])


# ---- 6. partial reset -------------------------------------------------------------------------------------------------------------
def _check_partial(make, prologue, ids, k, n_steps, before_reset, seed0=5, seed1=77):
    """Shard A runs n_steps closed-loop steps with reset_envs(ids) after step k - 1 (before_reset(A) is called in front of it); twin T
    is never reset; twin F is fully reset with the new seed and stepped with i = k ...: A's listed envs == F's from step k on, A's
    other envs == T's over all steps, and so the screens and accumulators at the end."""
    import torch
    a, log_a = make(), []
    n = a.n_envs
    others = [e for e in range(n) if e not in ids]
    obs = _steps(a, prologue(a, seed0), 0, k, log_a)
    before_reset(a)
    rows = a.reset_envs(ids, seed=seed1)
    assert a._per_env_clock
    obs = obs.clone()
    obs[torch.as_tensor(list(ids), device=obs.device)] = rows
    _steps(a, obs, k, n_steps, log_a)
    scr_a, buff_a = _state(a, True)
    a.close()
    t, log_t = make(), []
    _steps(t, prologue(t, seed0), 0, n_steps, log_t)
    scr_t, buff_t = _state(t, t._per_env_clock)
    t.close()
    f, log_f = make(), []
    obs_f = prologue(f, seed1)
    _steps(f, obs_f, k, n_steps, log_f)
    scr_f, buff_f = _state(f, f._per_env_clock)
    f.close()
    assert torch.equal(rows, obs_f[ids])
    for i in range(n_steps):
        assert _same(log_a[i], log_t[i], others), ("untouched envs", i)
        if i >= k:
            assert _same(log_a[i], log_f[i - k], ids), ("reset envs", i)
    assert not _same(log_a[-1], log_t[-1], ids)
    assert np.array_equal(scr_a[:, others], scr_t[:, others]) and np.array_equal(buff_a[:, others], buff_t[:, others])
    assert np.array_equal(scr_a[:, ids], scr_f[:, ids]) and np.array_equal(buff_a[:, ids], buff_f[:, ids])


def test_partial_reset_of_a_shared_clock_shard_with_a_fast_wind():
    """Shared clock at 50 m/s (1.5 px per frame, 4 envs with seeds of their own): reset_envs([1]) is refused at the default ceiling
    with the shard still on the shared clock; after set_wind_ceiling(2) it goes through -- the shared wind handed to every env's
    clock -- and both twins (shared clock, never switched) are matched over 6 more steps."""
    from rlao_amd import _lib as L
    geo = dict(SMALL, windSpeed=[50.0])

    def before_reset(a):
        with pytest.raises(L.AoEnvError, match="< 1"):
            a.reset_envs([1], seed=77)
        assert not a._per_env_clock and a.wind_pixels == 1
        a._shard.get_buff(1)                                        # (the library agrees: still the shared clock)
        a.set_wind_ceiling(2)
    _check_partial(lambda: _make(4, geo=geo, stride=1), lambda env, seed: _prologue(env, seed), [1], 5, 11, before_reset)


def test_partial_reset_inside_a_fast_per_env_shard():
    """Per-env winds up to 3.3 px per frame: envs 2 and 5 (a slow and the fastest one) restarted right after a step with whole
    rounds; the rounds of the next step start from origin 0 for them and from where they were for the others."""
    w = (FAST_SPEEDS, FAST_DIRS)
    _check_partial(lambda: _make(len(FAST_SPEEDS), stride=1), lambda env, seed: _prologue(env, seed, winds=w, ceiling=4), [5, 2], 4, 10,
                   lambda a: None)


# ---- 7. checkpoint ----------------------------------------------------------------------------------------------------------------
def test_checkpoint_carries_the_ceiling_and_the_fast_clocks():
    """get_state after 5 fast steps, set_state into a fresh env (default ceiling) that had another state: 5 more steps bit for bit.
    A state without the ceiling key loads as ceiling 1."""
    import torch
    n = len(FAST_SPEEDS)
    env = _make(n)
    log = []
    obs = _steps(env, _prologue(env, 9, winds=(FAST_SPEEDS, FAST_DIRS), ceiling=4), 0, 5, log)
    snap = env.get_state()
    assert snap["wind_pixels"] == 4
    cont = []
    _steps(env, obs, 5, 10, cont)
    env.close()
    env2 = _make(n)
    _prologue(env2, 1)                                              # some other state first
    assert env2.wind_pixels == 1
    env2.set_state(snap)
    assert env2.wind_pixels == 4 and env2._per_env_clock
    again = []
    _steps(env2, obs.clone(), 5, 10, again)
    for i in range(5):
        assert all(torch.equal(p, q) for p, q in zip(cont[i], again[i])), i
    # an old checkpoint: slow winds, no key -- the ceiling goes back to 1 (the fast clocks are replaced first)
    slow = _make(n)
    _steps(slow, _prologue(slow, 9, winds=(FAST_SPEEDS / 4, FAST_DIRS)), 0, 3, [])
    old = slow.get_state()
    slow.close()
    del old["wind_pixels"]
    env2.set_state(old)
    assert env2.wind_pixels == 1
    from rlao_amd import _lib as L
    with pytest.raises(L.AoEnvError, match="< 1"):
        env2.set_wind_per_env(FAST_SPEEDS, FAST_DIRS)
    env2.close()


# ---- 8. per-env r0 together with fast winds -------------------------------------------------------------------------------------------
def test_fast_per_env_winds_with_per_env_r0():
    """Env e with (wind e, r0 e) == env e of a shared-clock shard with wind e and the same set_r0_per_env: the innovations of the
    whole-pixel rounds carry sigma_e as every draw does."""
    sp, di = FAST_SPEEDS[[1, 3, 5, 6]], FAST_DIRS[[1, 3, 5, 6]]
    r0 = np.array([0.13, 0.09, 0.2, 0.11])
    steps = 8
    env = _make(4, stride=1)
    env.set_r0_per_env(r0)
    got = []
    _steps(env, _prologue(env, 6, winds=(sp, di), ceiling=4), 0, steps, got)
    scr = _state(env, True)[0]
    env.close()
    for e in range(4):
        ref = _make(4, stride=1)
        ref.set_r0_per_env(r0)
        ref.atm.windSpeed = list(sp[e])
        ref.atm.windDirection = list(di[e])
        want = []
        _steps(ref, _prologue(ref, 6), 0, steps, want)
        assert not ref._per_env_clock
        rs = _state(ref, False)[0]
        ref.close()
        for i in range(steps):
            assert _same(got[i], want[i], e), (e, i)
        assert np.array_equal(scr[0, e], rs[0, e]), e


# ---- 9. oracle --------------------------------------------------------------------------------------------------------------------
def test_a_fast_per_env_wind_matches_the_oracle():
    """The 95 m/s at 30 deg env (2.47, 1.43 px per frame: two rounds and a sub-pixel crossing on most steps) against the NumPy oracle
    with that wind, 10 steps, at the tolerances tests/test_gpu_wind.py uses for this geometry."""
    from oracle import ao_oracle as O                               # checker only
    env = _make(2)
    got = []
    _steps(env, _prologue(env, 9, winds=(FAST_SPEEDS[[1, 6]], FAST_DIRS[[1, 6]]), ceiling=3), 0, 10, got)
    orc = O.OracleEnv(resolution=48, diameter=3.2, n_subap=8, r0=0.13, L0=30.0, windSpeed=list(FAST_SPEEDS[6]),
                      windDirection=list(FAST_DIRS[6]), fractionalR0=[1.0], altitude=[0.0], m2c=env.M2C_CL, n_modes=20)
    env.close()
    orc.new_episode(9)
    obs_o = orc.reset_soft()
    for i in range(10):
        obs_o, fr_o, rw_o, sr_o, _, _ = orc.step(i, 0.5 * obs_o)
        np.testing.assert_allclose(got[i][0][1].cpu().numpy(), obs_o, atol=3e-5)
        np.testing.assert_allclose(float(got[i][3][1]), sr_o, atol=1e-5)


# ---- 10. refusals -----------------------------------------------------------------------------------------------------------------
def test_refusals_leave_everything_as_it_was():
    """Winds at or over the ceiling, option values outside 1 .. 8, a ceiling lowered under held winds, a raw clock at the ceiling:
    each refused, and the shard steps on exactly like a twin that was never asked."""
    from rlao_amd import _lib as L
    n = 4
    sp, di = FAST_SPEEDS[[1, 2, 6, 0]], FAST_DIRS[[1, 2, 6, 0]]       # up to 2.47 px per frame
    env, twin = _make(n), _make(n)
    log, log_t = [], []
    # default ceiling
    obs = _prologue(env, 9)
    with pytest.raises(L.AoEnvError, match="< 1"):
        env.set_wind_per_env(sp, di, reset=True)
    assert not env._per_env_clock and env.wind_pixels == 1
    env._shard.get_buff(1)                                          # the shard is still on the shared clock
    # option values
    for bad in (0, 9, -1):
        with pytest.raises(L.AoEnvError, match="AOENV_OPT_ENV_WIND_PIXELS"):
            env.set_wind_ceiling(bad)
        assert env.wind_pixels == 1
    obs = _prologue(env, 9, winds=(sp, di), ceiling=3)
    obs_t = _prologue(twin, 9, winds=(sp, di), ceiling=3)
    obs, obs_t = _steps(env, obs, 0, 3, log), _steps(twin, obs_t, 0, 3, log_t)
    clk = env._shard.get_clock_env(1, n)
    # ceiling 3, a 3.3 px per frame wind
    with pytest.raises(L.AoEnvError, match="< 3"):
        env.set_wind_per_env(np.array([[28.0], [40.0], [110.0], [0.0]]), np.array([[72.0], [190.0], [0.0], [0.0]]))
    # lowering the ceiling under held winds (env 2 holds 2.47 px per frame)
    with pytest.raises(L.AoEnvError, match="holds"):
        env.set_wind_ceiling(2)
    with pytest.raises(L.AoEnvError, match="holds"):
        env.set_wind_per_env(sp / 4, di, max_pixels=1)              # (the ceiling goes first: refused before the winds are touched)
    assert env.wind_pixels == 3
    # a raw clock with a ratio AT the ceiling
    bad = clk.copy()
    bad[0, 1, 1] = -3.0
    with pytest.raises(L.AoEnvError, match="< 3"):
        env._shard.set_clock_env(bad)
    assert np.array_equal(env._shard.get_clock_env(1, n), clk)
    # ... and everything is as it was
    _steps(env, obs, 3, 6, log)
    _steps(twin, obs_t, 3, 6, log_t)
    for i in range(6):
        assert _same(log[i], log_t[i], slice(None)), i
    a, b = _state(env, True), _state(twin, True)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    env.set_wind_ceiling(8)                                         # raising stays possible
    assert env.wind_pixels == 8
    env.close()
    twin.close()
