"""GPU: the trainer's policy inside the library (aoenv_set_policy / aoenv_policy_forward / aoenv_run_policy_rollout;
BatchedAOEnv.set_policy / policy_action / policy_rollout): ConvPolicy of MAIN/PO4AO/conv_models_simple.py:56-111 on the matrix
cores and the policy episodes of MAIN/PO4AO/mbrl.py:64-89 as a recorded on-device rollout.

Checkers: the float64 restatement of tests/_policy_ref.py (pinned against a torch module of the reference's shape on the CPU,
tests/test_policy_host.py); the env's own step (a twin stepped with the recorded actions reproduces every bit); policy_action on
windows rebuilt from the returned trajectory (teacher forcing: every recorded action, bit for bit); rollout(gain = 0) on a twin
for the exploration noise.

Tolerances.  float32: 8 x the largest difference between the torch-CPU float32 evaluation of the same module and its float64
evaluation, computed by each test on its own inputs (the margin: the MFMA sums K in blocks of 4 in (ci, ky, kx) order, another
order than the CPU library).  float64: that tolerance times 2^-29, the ratio of the unit roundoffs.  The largest differences
measured on MI355X are in profiles/policy_parity_maxima.json (AO_PARITY_REPORT=<file> with this module alone rewrites it).

Weights are seeded normals scaled so that the float64 reference output has clamped and unclamped valid actuators; every parity
case asserts on the reference alone that 10 % - 90 % of them are unclamped before the device result is looked at."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import _policy_ref as P

pytestmark = pytest.mark.gpu

SMALL = dict(diameter=3.2, nSubaperture=8, nPixelPerSubap=6, r0=0.13, L0=30.0, windSpeed=[10.0], windDirection=[72.0],
             fractionalR0=[1.0], altitude=[0.0], nModes=20, nLoop=64)
# a = 21: two bands of image rows in the MFMA convolution (11 + 10), 441 = 27 tiles of 16 + 9 pixels
BIG = dict(diameter=8.0, nSubaperture=20, nPixelPerSubap=6, r0=0.13, L0=30.0, windSpeed=[10.0], windDirection=[72.0],
           fractionalR0=[1.0], altitude=[0.0], nModes=50, nLoop=64)
SCALE = (1.0, 1.5, 2.0)                                            # layer gains: the network output has a standard deviation near 1.5
MAXIMA = {}


def _make(n, dtype="f32", geo=SMALL, wfs="shackhartmann", **kw):
    from rlao_amd.env import BatchedAOEnv
    env = BatchedAOEnv(n_envs=n, device=0, dtype=dtype, **kw)
    env.set_params(geo, camera="ideal", wfs_type=wfs, gainCL=0.4)
    return env


def _prologue(env, seed=5):
    env.generate_new_phase_screen(seed)
    env.dm.coefs = 0
    env.dm_prev = 0
    env.measure()
    env.SR = []
    return env.reset_soft()


def _counters(env):
    from rlao_amd import _lib as L
    return env._shard.download(L.B_COUNTERS, (4,), env._stream(), dtype=np.uint32)


def _act_idx(env):
    return np.asarray(env._dm_tables.act_idx, dtype=np.int64)


def _np_dtype(env):
    return np.float32 if env.dtype == "f32" else np.float64


def _inputs(env, H, seed, n=None, scale=1.0):
    """obs [n, a, a], past_obs, past_act [n, H-1, a, a]: normals, exactly representable in the env dtype, as float64"""
    rng = np.random.RandomState(seed)
    n, a, dt = n or env.n_envs, env.nActuator, _np_dtype(env)
    return tuple((scale * rng.normal(0, 1, s)).astype(dt).astype(np.float64) for s in ((n, a, a), (n, H - 1, a, a), (n, H - 1, a, a)))


def _f_matrix(env):
    return env.M2C_CL @ np.linalg.pinv(env.M2C_CL)


def _reference(env, w, x, proj):
    """-> float64 restatement, float32 tolerance (8 x |torch f32 - torch f64|), that yardstick; asserts the input condition"""
    import torch
    idx = _act_idx(env)
    xv, yv = np.divmod(idx, env.nActuator)
    F = _f_matrix(env) if proj else None
    ref = P.policy(w, *x, idx, F)
    inner = np.abs(P.network(w, *x).reshape(x[0].shape[0], -1)[:, idx])
    unclamped = float((inner < 1).mean())
    assert 0.1 <= unclamped <= 0.9, unclamped                       # a condition on the inputs: clamped and unclamped actuators
    t64 = P.torch_eval(w, *x, xv, yv, F, dtype=torch.float64)
    t32 = P.torch_eval(w, *x, xv, yv, F, dtype=torch.float32)
    assert np.abs(t64 - ref).max() <= 1e-12
    yard = float(np.abs(t32 - t64).max())
    return ref, 8.0 * yard, yard


def _tol(env, tol32):
    return tol32 if env.dtype == "f32" else tol32 * 2.0 ** -29


def _action(env, x):
    return env.policy_action(*x).double().cpu().numpy()


@pytest.fixture(scope="module")
def shards():
    made = {}

    def get(kind):
        if kind not in made:
            n, dtype, geo = {"small32": (4, "f32", SMALL), "small64": (4, "f64", SMALL), "small32_1": (1, "f32", SMALL),
                             "big32": (3, "f32", BIG), "big32_1": (1, "f32", BIG)}[kind]
            made[kind] = _make(n, dtype, geo)
        return made[kind]

    yield get
    for e in made.values():
        e.close()
    out = os.environ.get("AO_PARITY_REPORT")
    if out and MAXIMA:
        with open(out, "w") as f:
            f.write(json.dumps(MAXIMA, indent=1, sort_keys=True) + "\n")


CASES = [(1, 16), (3, 16), (20, 64), (3, 24)]                       # (3, 24): n_filt % 16 != 0, the general kernel


@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("proj", [False, True], ids=["noproj", "proj"])
@pytest.mark.parametrize("H,n_filt", CASES)
def test_forward_parity(shards, H, n_filt, proj, dtype):
    env = shards("small32" if dtype == "f32" else "small64")
    w = P.make_weights(H, n_filt, seed=100 + H + n_filt, scale=SCALE)
    x = _inputs(env, H, seed=7 + H)
    ref, tol32, yard = _reference(env, w, x, proj)
    env.set_policy(w, F=True if proj else None)
    got = _action(env, x)
    err = float(np.abs(got - ref).max())
    MAXIMA[f"a9_H{H}_F{n_filt}_{'proj' if proj else 'noproj'}_{dtype}"] = {"gpu_vs_f64": err, "torch_f32_vs_f64": yard}
    print(f"H={H} F={n_filt} proj={proj} {dtype}: |gpu - f64| = {err:.3e}, |torch f32 - f64| = {yard:.3e}, tol = {_tol(env, tol32):.3e}")
    assert err <= _tol(env, tol32)
    mask = np.ones(env.nActuator ** 2, dtype=bool)
    mask[_act_idx(env)] = False
    assert (got.reshape(env.n_envs, -1)[:, mask] == 0).all()        # zero off the valid actuators
    env.set_policy(None)


@pytest.mark.parametrize("H,n_filt", [(3, 16), (20, 64), (2, 32), (3, 24)])
def test_forward_parity_two_bands(shards, H, n_filt):
    """a = 21: the image is two bands of rows and 28 tiles of pixels, the seam between the bands inside the pupil"""
    env = shards("big32")
    assert env.nActuator == 21
    w = P.make_weights(H, n_filt, seed=300 + H + n_filt, scale=SCALE)
    x = _inputs(env, H, seed=17 + H)
    ref, tol32, yard = _reference(env, w, x, True)
    env.set_policy(w)
    got = _action(env, x)
    err = float(np.abs(got - ref).max())
    MAXIMA[f"a21_H{H}_F{n_filt}_proj_f32"] = {"gpu_vs_f64": err, "torch_f32_vs_f64": yard}
    print(f"a=21 H={H} F={n_filt}: |gpu - f64| = {err:.3e}, |torch f32 - f64| = {yard:.3e}")
    assert err <= tol32
    env.set_policy(w, path=1)
    gen = _action(env, x)
    assert float(np.abs(gen - got).max()) <= tol32
    env.set_policy(None)


@pytest.mark.parametrize("H,n_filt", [(3, 16), (20, 64)])
def test_paths_agree(shards, H, n_filt):
    """path = 1 (the general kernel) against the default (MFMA) on a float32 shard, and the general kernel on a float32 shard
    against the general kernel on a float64 shard, both within the float32 tolerance of the case"""
    e32, e64 = shards("small32"), shards("small64")
    w = P.make_weights(H, n_filt, seed=100 + H + n_filt, scale=SCALE)
    x = _inputs(e32, H, seed=7 + H)
    _, tol32, _ = _reference(e32, w, x, True)
    e32.set_policy(w)
    default = _action(e32, x)
    e32.set_policy(w, path=1)
    general = _action(e32, x)
    e64.set_policy(w, path=1)
    general64 = _action(e64, x)
    print(f"H={H} F={n_filt}: |general - default| = {np.abs(general - default).max():.3e}, |general f32 - f64| = {np.abs(general - general64).max():.3e}")
    assert np.abs(general - default).max() <= tol32
    assert np.abs(general - general64).max() <= tol32
    for e in (e32, e64):
        e.set_policy(None)


@pytest.mark.parametrize("geo", ["small", "big"])
@pytest.mark.parametrize("path", [0, 1])
def test_position_independence(shards, geo, path):
    """Rows 0 and 2 of a batch hold the same inputs: the same bits out; so does row 0 of a one-env shard"""
    import torch
    env, one = shards(geo + "32"), shards(geo + "32_1")
    H, n_filt = 3, 16
    w = P.make_weights(H, n_filt, seed=41, scale=SCALE)
    x = [t.copy() for t in _inputs(env, H, seed=23)]
    for t in x:
        t[2] = t[0]
    env.set_policy(w, path=path)
    one.set_policy(w, path=path)
    got = env.policy_action(*x)
    alone = one.policy_action(*(t[:1] for t in x))
    assert torch.equal(got[0], got[2]) and not torch.equal(got[0], got[1])
    assert torch.equal(got[0], alone[0])
    assert float(got[0].abs().max()) > 0
    env.set_policy(None)
    one.set_policy(None)


def _host(t):
    return t.detach().cpu().numpy()


def _past(env, H, seed, scale=0.05):
    _, po, pa = _inputs(env, H, seed, scale=scale)
    return po.astype(_np_dtype(env)), pa.astype(_np_dtype(env))


def _check_teacher_forced(env, tr, past, sigma_noise=None):
    """policy_action on the windows rebuilt from the trajectory and the caller's windows equals every recorded action"""
    obs, act = _host(tr.obs), _host(tr.action)
    for k in range(act.shape[0]):
        p = _host(env.policy_action(obs[k], P.window(past[0], obs, k), P.window(past[1], act, k)))
        want = p if sigma_noise is None else p + sigma_noise[k]
        assert np.array_equal(act[k], want), k
    return obs, act


@pytest.mark.parametrize("H,n_filt,n_steps", [(3, 16, 6), (20, 64, 4)])
def test_rollout_teacher_forced(H, n_filt, n_steps):
    """(3, 16, 6): both history sources (the caller's windows for k < 2, the trajectory after); (20, 64, 4): every past channel
    still from the caller's windows.  sigma = 0: the action is bit for bit the policy's output."""
    env = _make(3)
    w = P.make_weights(H, n_filt, seed=5, scale=(20.0, 1.5, 2.0))
    env.set_policy(w)
    _prologue(env)
    past = _past(env, H, seed=9)
    c0 = _counters(env)[1]
    tr, new_past = env.policy_rollout(0, n_steps, sigma=0.0, past=past)
    assert tuple(tr.obs.shape) == (n_steps + 1, 3, 9, 9) and tuple(tr.action.shape) == (n_steps, 3, 9, 9)
    obs, act = _check_teacher_forced(env, tr, past)
    assert np.isfinite(obs).all() and np.abs(act).max() > 1e-3
    assert np.array_equal(_host(new_past[0]), P.roll(past[0], obs, n_steps))
    assert np.array_equal(_host(new_past[1]), P.roll(past[1], act, n_steps))
    assert _counters(env)[1] == c0 + n_steps
    env.close()


KINDS = {
    "f32_fused": dict(dtype="f32"),
    "f64_batched": dict(dtype="f64"),
    "pyramid": dict(dtype="f32", geo=dict(SMALL, modulation=0.0), wfs="pyramid"),
}


@pytest.mark.parametrize("kind", list(KINDS))
def test_rollout_equals_stepping_bit_for_bit(kind):
    import torch
    env, twin = _make(3, **KINDS[kind]), _make(3, **KINDS[kind])
    if kind != "pyramid":
        assert env.fused_step == (kind == "f32_fused")
    w = P.make_weights(3, 16, seed=5, scale=(20.0, 1.5, 2.0))
    env.set_policy(w)
    obs0 = _prologue(env)
    tr, _ = env.policy_rollout(0, 6, past=_past(env, 3, seed=9))
    o = _prologue(twin)
    assert torch.equal(tr.obs[0], obs0) and torch.equal(o, obs0)
    for k in range(6):
        o, fr, r, s, _, _ = twin.step(k, tr.action[k])
        assert torch.equal(tr.obs[k + 1], o) and torch.equal(tr.reward[k], r) and torch.equal(tr.strehl[k], s), (kind, k)
    assert torch.equal(env._frame, fr)
    assert torch.equal(env._obs, tr.obs[-1]) and len(env.SR) == 6
    a, b = env.get_state(), twin.get_state()
    for key in ("screen", "coefs", "dm_prev", "mt", "signal"):
        assert np.array_equal(np.asarray(a[key]), np.asarray(b[key])), (kind, key)
    assert float(tr.action.abs().max()) > 1e-3
    env.close()
    twin.close()


@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_rollout_noise_is_the_exploration_stream(dtype):
    """sigma > 0: action = fl(policy + noise) with the noise rollout(gain = 0, sigma) draws on a twin for the same seed and counter
    (one addition in the env dtype, so the sum is reproduced exactly; the literal difference action - policy carries that
    addition's rounding and the subtraction's: 2 u (|action| + |noise|)).  Word 1 of the counters advances by n_steps; two calls
    in a row are one call of the summed length."""
    import torch
    sigma, H = 0.05, 3
    env, twin, whole = _make(3, dtype), _make(3, dtype), _make(3, dtype)
    w = P.make_weights(H, 16, seed=5, scale=(20.0, 1.5, 2.0))
    for e in (env, whole):
        e.set_policy(w)
        _prologue(e)
    _prologue(twin)
    past = _past(env, H, seed=9)
    t1, p1 = env.policy_rollout(0, 3, sigma=sigma, past=past, seed=11)
    assert _counters(env)[1] == 3
    t2, p2 = env.policy_rollout(3, 3, sigma=sigma, past=p1)
    assert _counters(env)[1] == 6
    noise = _host(twin.rollout(0, 6, sigma, gain=0.0, seed=11).action)
    assert np.abs(noise).max() > 0.01
    t, p = whole.policy_rollout(0, 6, sigma=sigma, past=past, seed=11)
    for name in ("action", "reward", "strehl"):
        assert torch.equal(getattr(t, name)[:3], getattr(t1, name)) and torch.equal(getattr(t, name)[3:], getattr(t2, name)), name
    assert torch.equal(t.obs[:4], t1.obs) and torch.equal(t.obs[3:], t2.obs)
    assert torch.equal(p[0], p2[0]) and torch.equal(p[1], p2[1])
    obs, act = _check_teacher_forced(whole, t, past, sigma_noise=noise)
    u = 2.0 ** -24 if dtype == "f32" else 2.0 ** -53
    for k in range(6):
        pol = _host(whole.policy_action(obs[k], P.window(past[0], obs, k), P.window(past[1], act, k)))
        assert (np.abs((act[k] - pol) - noise[k]) <= 2 * u * (np.abs(act[k]) + np.abs(noise[k]))).all(), k
    for e in (env, twin, whole):
        e.close()


def test_refusals_change_nothing():
    import torch
    from rlao_amd import _lib as L
    env, twin = _make(2), _make(2)
    _prologue(env)
    _prologue(twin)
    n, a = env.n_envs, env.nActuator
    H = 3
    w = P.make_weights(H, 16, seed=5, scale=(20.0, 1.5, 2.0))
    x = _inputs(env, H, seed=3)
    past = _past(env, H, seed=9)
    # no policy
    with pytest.raises(L.AoEnvError, match="no policy"):
        env.policy_action(*x)
    with pytest.raises(L.AoEnvError, match="no policy"):
        env.policy_rollout(0, 2, past=past)
    env.set_policy(w)
    twin.set_policy(w)
    want = env.policy_action(*x)
    before, c_before = env.get_state(), _counters(env)
    # a bad H (33: 65 channels), NaN weights, a bad clamp, a bad projection rank: the policy in use stays
    bad_h = P.make_weights(33, 16, seed=1)
    nan_w = dict(w, w2=w["w2"].copy())
    nan_w["w2"][3, 2, 1, 1] = np.nan
    for bad, kw in ((bad_h, {}), (nan_w, {}), (w, dict(clamp=0.0)), (w, dict(clamp=float("nan"))), (w, dict(path=2)),
                    (P.make_weights(2, 129, seed=1), {})):
        with pytest.raises(L.AoEnvError):
            env.set_policy(bad, **kw)
    A = env.nValidAct
    with pytest.raises(ValueError):
        env.set_policy(w, F=(np.zeros((3, A + 1)), np.zeros((A + 1, 3))))
    assert torch.equal(env.policy_action(*x), want)
    # frames outside n_loop, a bad sigma
    for args, kw in (((60, 10), {}), ((-1, 2), {}), ((0, 2), dict(sigma=-0.1)), ((0, 2), dict(sigma=float("nan")))):
        with pytest.raises(L.AoEnvError):
            env.policy_rollout(*args, past=past, **kw)
    with pytest.raises(ValueError):
        env.policy_rollout(0, -1, past=past)
    with pytest.raises(ValueError):
        env.policy_rollout(0, 2, past=(past[0][:, :1], past[1]))
    # at the ABI: gain != 0, null pointers; the caller's buffers keep their contents
    lib, h = env._shard.lib, env._shard.h
    ob = torch.full((3, n, a, a), 7.0, device=env.device)
    ac = torch.full((2, n, a, a), 8.0, device=env.device)
    po, pa = torch.full((n, H - 1, a, a), 9.0, device=env.device), torch.full((n, H - 1, a, a), 10.0, device=env.device)
    p = lambda t: C.c_void_p(t.data_ptr())
    good = L.AoRollout(i0=0, n_steps=2, gain=0.0, sigma=0.1, seed=1)
    resid = L.AoRollout(i0=0, n_steps=2, gain=0.4, sigma=0.1, seed=1)
    late = L.AoRollout(i0=63, n_steps=2, gain=0.0, sigma=0.1, seed=1)
    assert lib.aoenv_run_policy_rollout(h, C.byref(resid), p(ob), p(ac), None, None, None, p(po), p(pa), None) != 0
    assert b"gain" in lib.aoenv_last_error()
    assert lib.aoenv_run_policy_rollout(h, C.byref(late), p(ob), p(ac), None, None, None, p(po), p(pa), None) != 0
    assert lib.aoenv_run_policy_rollout(h, None, p(ob), p(ac), None, None, None, p(po), p(pa), None) != 0
    assert lib.aoenv_run_policy_rollout(h, C.byref(good), None, p(ac), None, None, None, p(po), p(pa), None) != 0
    assert lib.aoenv_run_policy_rollout(h, C.byref(good), p(ob), None, None, None, None, p(po), p(pa), None) != 0
    assert lib.aoenv_run_policy_rollout(h, C.byref(good), p(ob), p(ac), None, None, None, None, p(pa), None) != 0
    assert lib.aoenv_run_policy_rollout(h, C.byref(good), p(ob), p(ac), None, None, None, p(po), None, None) != 0
    assert lib.aoenv_policy_forward(h, None, p(po), p(pa), p(ac), None) != 0
    assert lib.aoenv_policy_forward(h, p(ob), None, p(pa), p(ac), None) != 0
    assert lib.aoenv_policy_forward(h, p(ob), p(po), p(pa), None, None) != 0
    torch.cuda.synchronize()
    for t, v in ((ob, 7.0), (ac, 8.0), (po, 9.0), (pa, 10.0)):
        assert bool((t == v).all())
    # nothing changed: counters, state, and the env goes on exactly like its twin
    assert np.array_equal(_counters(env), c_before)
    after = env.get_state()
    for key in ("screen", "coefs", "dm_prev", "mt", "signal", "counters", "obs"):
        assert np.array_equal(np.asarray(before[key]), np.asarray(after[key])), key
    (tx, px), (ty, py) = env.policy_rollout(0, 3, sigma=0.05, past=past, seed=8), twin.policy_rollout(0, 3, sigma=0.05, past=past, seed=8)
    assert all(torch.equal(u, v) for u, v in zip(tx, ty)) and torch.equal(px[0], py[0]) and torch.equal(px[1], py[1])
    # n_steps == 0 succeeds and does nothing
    tr0, p0 = env.policy_rollout(3, 0, past=px)
    assert tr0.action.shape[0] == 0 and torch.equal(p0[0], px[0]) and _counters(env)[1] == 3
    # forgotten: refused again
    env.set_policy(None)
    with pytest.raises(L.AoEnvError, match="no policy"):
        env.policy_action(*x)
    assert lib.aoenv_policy_forward(h, p(ob), p(po), p(pa), p(ac), None) != 0
    env.close()
    twin.close()


def test_history_one_and_wrappers():
    """H = 1: no windows are read (null pointers at the ABI).  TorchWrapper forwards in float32; TimeDelayEnv refuses."""
    import torch
    from rlao_amd import _lib as L
    from rlao_amd.wrappers import TimeDelayEnv, TorchWrapper
    env, twin = _make(2, "f64"), _make(2, "f64")
    w = P.make_weights(1, 16, seed=5, scale=(20.0, 1.5, 2.0))
    for e in (env, twin):
        e.set_policy(w)
        _prologue(e)
    n, a = env.n_envs, env.nActuator
    tr, past = env.policy_rollout(0, 3)
    assert tuple(past[0].shape) == (n, 0, a, a)
    act = torch.empty((n, a, a), device=env.device, dtype=env.tdtype)
    L.check(env._shard.lib.aoenv_policy_forward(env._shard.h, C.c_void_p(tr.obs[1].data_ptr()), None, None, C.c_void_p(act.data_ptr()),
                                                C.c_void_p(env._stream())))
    assert torch.equal(act, tr.action[1])
    tw = TorchWrapper(twin)
    tw.set_policy(w)
    trw, pw = tw.policy_rollout(0, 3)
    assert all(x.dtype == torch.float32 and torch.equal(x, y.float()) for x, y in zip(trw, tr))
    assert pw[0].dtype == torch.float32
    aw = tw.policy_action(tr.obs[1])
    assert aw.dtype == torch.float32 and torch.equal(aw, tr.action[1].float())
    with pytest.raises(NotImplementedError, match="action k in step k"):
        TimeDelayEnv(env, 1).policy_rollout(3, 2)
    env.close()
    twin.close()
