"""GPU: a pixel crossing served by the default library -- the ring pipeline: the ring GEMM with the next crossing's innovations
drawn beside it (k_ring_gemm_draw_ahead), the ring scattered, the next Z gathered and the screen's range rescanned inside the fused
step kernel -- against its two independent implementations:

    AOENV_OPT_DEFER_RING = 0       the ring scattered and the range taken by k_scatter_minmax, in front of the step kernel
    AOENV_OPT_RING_LOOKAHEAD = 0   Z gathered and xi drawn in place by k_ring_prepare, behind a kernel boundary

Everything a caller sees must be the same BIT FOR BIT (torch.equal): obs, frame, reward and Strehl of every step, and the
downloaded AOENV_B_SCREEN and AOENV_B_XI at the end.  The same Z, the same xi from the same stream (mt_normal_body in its in-place
and out-of-place forms, through k_ring_prepare, k_ring_prepare_env and the draw-ahead workgroups, at real ring sizes), the same
split-K slabs summed in the same order, the same min / max.

Confirmed on the parent first: with the library of the commit before the one-pass draw (the block-by-block walk), run in the same
GPU session, every comparison of every case below already held exactly, under AOENV_OPT_DEFER_RING = 0 as well as under
AOENV_OPT_RING_LOOKAHEAD = 0 (tests/test_gpu_behaviour.py::test_switches_agree_small asserts it for the look-ahead alone).  So all
comparisons are torch.equal and none is held to a tolerance.

Geometry: SMALL of tests/test_gpu_behaviour.py (3.2 m, 8 x 8 lenslets, R = 48, S = 54, 9 split-K slabs of 16: the z < splits
guards), 3 envs, 15 m/s = 0.45 pixels per frame, 24 steps -- at least 8 pixel crossings, counted on the host clock (at 45 and 225
degrees they come as 7 steps that cross both axes at once)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GAIN = 0.5
SMALL = dict(diameter=3.2, nSubaperture=8, nPixelPerSubap=6, r0=0.13, L0=30.0, windSpeed=[15.0], windDirection=[72.0],
             fractionalR0=[1.0], altitude=[0.0], nModes=20, nLoop=64)
C2 = dict(diameter=8.0, nSubaperture=20, nPixelPerSubap=6, r0=0.13, L0=30.0, windSpeed=[15.0], windDirection=[72.0],
          fractionalR0=[1.0], altitude=[0.0], nModes=50, nLoop=64)
THREE = dict(windSpeed=[10.0, 12.0, 11.0], windDirection=[0.0, 72.0, 144.0], fractionalR0=[0.5, 0.3, 0.2], altitude=[0.0, 0.0, 0.0])
SWITCHES = {"default": {}, "defer_ring_0": {"OPT_DEFER_RING": 0}, "lookahead_0": {"OPT_RING_LOOKAHEAD": 0}}


def _checkerboard(screen, a):
    i, j = np.indices(screen.shape[-2:])
    return np.broadcast_to(np.where((i + j) % 2 == 0, a, -a), screen.shape).astype(screen.dtype)


def _run(geo, opts, n_envs=3, steps=24, camera="ideal", winds=None, star=False, clip=None):
    """One shard: the record of everything compared, the number of steps in which 1, 2, ... layers crossed (shared clock: from the
    host clock's accumulators) and the launch counts."""
    import torch
    from rlao_amd import _lib as L
    from rlao_amd.env import BatchedAOEnv
    env = BatchedAOEnv(n_envs=n_envs, device=0, dtype="f32")
    try:
        env.set_params(geo, camera=camera, wfs_type="shackhartmann", gainCL=GAIN)
        sh = env._shard
        for k, v in opts.items():
            L.check(sh.lib.aoenv_set_option(sh.h, getattr(L, k), v))
        if clip is not None:
            L.check(sh.lib.aoenv_set_option(sh.h, L.OPT_STORE_ATM_OPD, 1))
        assert env.fused_step
        env.generate_new_phase_screen(29)
        if winds is not None:
            env.set_wind_per_env(winds[0], winds[1], reset=True)
        if star:
            env.set_magnitude_per_env(env.param.magnitude + np.linspace(0.0, 1.0, n_envs))
        env.dm.coefs = 0
        env.dm_prev = 0
        env.measure()
        obs = env.reset_soft()
        if clip is not None:                                        # a two-valued screen through the state interface
            state = env.get_state()
            state["screen"] = _checkerboard(state["screen"], clip)
            env.set_state(state)
            obs = env._obs
        n_layer = env.param.nLayer
        ratio = env._atm_tables.wind_ratio(env.param.windSpeed, env.param.windDirection, env.param.samplingTime)
        rec, crossed, pixels = [], [], 0
        sh.profile(True)
        for i in range(steps):
            before = None if winds is not None else sh.get_buff(n_layer)
            obs, frame, rew, sr, _, _ = env.step(i, GAIN * obs)
            rec += [(f"obs[{i}]", obs.clone()), (f"frame[{i}]", frame.clone()), (f"reward[{i}]", rew.clone()), (f"strehl[{i}]", sr.clone())]
            if clip is not None:
                rec.append((f"opd_atm[{i}]", torch.from_numpy(sh.download(L.B_OPD_ATM, (n_envs, env.R, env.R), env._stream()))))
            if before is not None:
                moved = np.abs(sh.get_buff(n_layer) - (before + ratio)) > 0.5         # [layer][axis]: a pixel was crossed
                crossed.append(int(moved.any(axis=1).sum()))
                pixels += int(moved.sum())
        torch.cuda.synchronize()
        prof = {k: v[1] for k, v in sh.profile_read(env._stream()).items()}
        sh.profile(False)
        at = env._atm_tables
        scr = env._download_screens()
        rec.append(("screen", torch.from_numpy(np.ascontiguousarray(scr))))
        rec.append(("xi", torch.from_numpy(sh.download(L.B_XI, (n_envs, at.n_inner + at.n_outer), env._stream()))))
        info = dict(crossed=crossed, pixels=pixels, prof=prof, n_outer=at.n_outer, S=at.S, R=env.R)
    finally:
        env.close()
    return rec, info


def _compare(geo, **kw):
    import torch
    runs = {name: _run(geo, opts, **kw) for name, opts in SWITCHES.items()}
    ref, info = runs["default"]
    for name in ("defer_ring_0", "lookahead_0"):
        got, _ = runs[name]
        assert len(got) == len(ref)
        for (what, a), (what_b, b) in zip(ref, got):
            assert what == what_b and a.shape == b.shape and a.dtype == b.dtype, (name, what)
            assert torch.equal(a, b), (name, what, float((a.double() - b.double()).abs().max()))
    last = dict(ref)
    assert all(torch.isfinite(v).all() for v in last.values())
    return runs


@pytest.mark.parametrize("direction", [0.0, 90.0, 45.0, 225.0, 72.0])
def test_wind_directions(direction):
    """one axis (0, 90), both axes on the same step (45), negative shifts -- the gather reads the opposite borders (225) -- and 72"""
    runs = _compare(dict(SMALL, windDirection=[direction]))
    info = runs["default"][1]
    assert info["S"] == 54 and info["R"] == 48
    # at least 8 pixel crossings on the host clock: 10 crossing steps at 0, 90 and 72 degrees, and at 45 / 225 degrees (0.32 pixels
    # per frame and axis) 7 steps on which BOTH axes cross = 14 pixels, one extrusion with a diagonal shift each
    steps_crossed = sum(1 for c in info["crossed"] if c)
    assert info["pixels"] >= 8 and steps_crossed >= 7, info
    assert (info["pixels"] == 2 * steps_crossed) == (direction in (45.0, 225.0)), info
    # the three runs took the three routes: operands prepared ahead (all but the first), prepared in place at every crossing,
    # and the ring scattered by k_scatter_minmax
    prof = {name: r[1]["prof"] for name, r in runs.items()}
    print(direction, {name: {k: p[k] for k in ("ring_prepare", "gemm_ring", "ring_scatter")} for name, p in prof.items()})
    assert all(p["gemm_ring"] == steps_crossed for p in prof.values()), prof
    assert prof["default"]["ring_prepare"] == 1 and prof["default"]["ring_scatter"] == 0, prof
    assert prof["lookahead_0"]["ring_prepare"] == steps_crossed and prof["defer_ring_0"]["ring_scatter"] == steps_crossed, prof


def test_three_layers_two_crossing_on_one_step():
    runs = _compare(dict(SMALL, **THREE))
    crossed = runs["default"][1]["crossed"]
    assert max(crossed) >= 2, crossed                               # (host clocks) two layers crossed in one step
    assert sum(crossed) >= 8, crossed


def test_per_env_winds():
    """the PE instantiation: env 0 is calm and never crosses, env 1 crosses on most steps (0.9 pixels per frame)"""
    speed = np.array([[0.0], [30.0], [15.0], [12.0], [7.0]])
    direction = np.array([[0.0], [0.0], [72.0], [225.0], [144.0]])
    _compare(SMALL, n_envs=5, winds=(speed, direction))


@pytest.mark.parametrize("kind", ["papyrus", "razor", "star"])
def test_instantiations(kind):
    """photon noise only, any camera (the Razor settings) and a guide star per env (STEP_STAR): each compiles its own copy"""
    if kind == "star":
        _compare(SMALL, camera="papyrus", star=True)
    else:
        _compare(SMALL, camera=kind)


def test_c2_geometry():
    runs = _compare(C2, n_envs=2, steps=12)
    info = runs["default"][1]
    assert info["n_outer"] == 500 and sum(1 for c in info["crossed"] if c) >= 3, info     # 16 slabs of 93 columns


@pytest.mark.parametrize("a", [1e-3, 1e3])
def test_clip_active(a):
    """A two-valued screen (+-a on alternate pixels): the Catmull-Rom interpolant overshoots the range on every pixel, so the clip
    to the screen's min / max acts everywhere and a wrong range changes every pixel of AOENV_B_OPD_ATM.  a = 1e-3: the new ring
    values set the range; a = 1e3: the interior does.  The first crossing after the upload prepares its operand in place, the
    later ones come through the pipeline."""
    runs = _compare(SMALL, steps=12, clip=a)
    info = runs["default"][1]
    assert sum(1 for c in info["crossed"] if c) >= 3, info["crossed"]
    assert info["prof"]["gemm_ring"] >= 3 and info["prof"]["ring_prepare"] == 1, info["prof"]
    opd = dict(runs["default"][0])
    assert float(opd["opd_atm[11]"].abs().max()) > 0
