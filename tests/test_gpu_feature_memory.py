"""GPU: the device memory of every feature that comes and goes while a shard lives (rlao_amd/csrc/dev_block.hpp behind the
``aoenv_set_*`` calls of rlao_amd/csrc/env.hip).  A shard whose feature went through

    set small -> use -> set larger -> use -> set small again -> clear -> set final

runs the same 6 frames as a twin that was configured once with the final setting, and everything the loop hands out, the record or
the accumulators, and ``get_state()`` are the same bits: no stale pointer into a freed block, no part carved at the wrong place,
nothing of the larger setting left behind.  Sizes: the smallest that make the block grow for real and then shrink.  At the end one
shard is closed with every feature set, and a shard created after it in the same process runs like one that never had any.

The geometry is SMALL of tests/test_gpu_delay.py (8 x 8 lenslets of 6 pixels, one layer), 4 envs, with 4 controlled modes:
``set_params`` itself uploads the noise filter and the reconstructor's factors at rank nModes, and at SMALL's 20 the two grow-only
blocks would already be larger than anything the sequences below ask for.  One float32 shard (the fused step) and one float64
shard, each with its twin, are built once for the module.  Device-wide free memory is not measured (it moves with other work on
the card): the frees themselves are pinned on the host by tests/test_dev_block_host.py.

No existing module runs this sequence against a twin for any of the features, so none is left out here."""
import numpy as np
import pytest

import _policy_ref as P

pytestmark = pytest.mark.gpu

GEO = dict(diameter=3.2, nSubaperture=8, nPixelPerSubap=6, r0=0.13, L0=30.0, windSpeed=[10.0], windDirection=[72.0],
           fractionalR0=[1.0], altitude=[0.0], nModes=4, nLoop=64)
N, FRAMES, GAIN = 4, 6, 0.4
CLEAR, DEFAULT = "clear", "default"                                # no feature; what set_params itself uploaded
_ENVS = {}
_BASIS = {}


def _make(dtype):
    from rlao_amd.env import BatchedAOEnv
    env = BatchedAOEnv(n_envs=N, device=0, dtype=dtype)
    env.set_params(GEO, camera="ideal", wfs_type="shackhartmann", gainCL=GAIN)
    return env


def _env(dtype, tag):
    if (dtype, tag) not in _ENVS:
        _ENVS[(dtype, tag)] = _make(dtype)
    return _ENVS[(dtype, tag)]


@pytest.fixture(scope="module", autouse=True)
def _close_all():
    yield
    for env in _ENVS.values():
        env.close()
    _ENVS.clear()


def _np(t):
    return t.detach().cpu().numpy()


def _start(env, seed=5):
    from rlao_amd import _lib as L
    env.generate_new_phase_screen(seed)
    env.dm.coefs = 0
    env.dm_prev = 0
    env.measure()
    env.SR = []
    env.explore_seed = 0                                            # (the stream's seed and position: as on a new env)
    env._shard.upload_state(L.B_COUNTERS, np.zeros(4, dtype=np.uint32), env._stream(), dtype=np.uint32)
    return env.reset_soft()


def _same(a, b, what):
    if isinstance(a, dict):
        assert isinstance(b, dict) and a.keys() == b.keys(), what
        for k in a:
            _same(a[k], b[k], f"{what}.{k}")
    elif isinstance(a, (tuple, list)):
        assert isinstance(b, (tuple, list)) and len(a) == len(b), what
        for i, (x, y) in enumerate(zip(a, b)):
            _same(x, y, f"{what}[{i}]")
    elif a is None or b is None:
        assert a is None and b is None, what
    else:
        assert np.array_equal(np.asarray(a), np.asarray(b)), what


def _everything(env, handed):
    import torch
    torch.cuda.synchronize()
    out = {f"out[{j}]": _np(t) for j, t in enumerate(handed)}
    assert all(np.isfinite(v).all() for v in out.values())
    out["state"] = env.get_state()
    return out


def _basis(env, K):
    """(m2c [A, K], cm [K, nSignal], reconstructor [A, nSignal]) of the first K Zernike modes of the calibrated loop"""
    from rlao_amd import calib
    if K not in _BASIS:
        m2c = calib.zernike_m2c(env._dm_tables, env.pupil, env.param.diameter, 12)[:, :K]
        recon, _, cm = calib.reconstructor_from_imat(env.imat, m2c, True)
        _BASIS[K] = (np.ascontiguousarray(m2c), np.ascontiguousarray(cm), np.ascontiguousarray(recon))
    return _BASIS[K]


# ---- the loops ------------------------------------------------------------------------------------------------------------------------
def _integrator(env, n):
    _start(env)
    return list(env.run_integrator(0, n))


def _rollout(env, n):
    _start(env)
    return list(env.rollout(0, n, sigma=0.05, gain=GAIN, seed=9))


def _integrator_modal(env, n):
    _start(env)
    env.reset_soft_modal()
    return list(env.run_integrator_modal(0, n))


def _recorded(env, n):
    _start(env)
    rec = env.record_wavefront(0, n, ("residual", "atmosphere"))
    out = list(env.run_integrator(0, n)) + [rec, env.project_wavefront("residual")]
    env.stop_wavefront_record()
    return out


def _long_exposure(env, n):
    _start(env)
    env.start_long_exposure()
    out = list(env.run_integrator(0, n)) + list(env._le) + [env.science_psf()]
    env.stop_long_exposure()
    return out


def _policy_rollout(env, n):
    _start(env)
    tr, past = env.policy_rollout(0, n, seed=9)
    return list(tr) + list(past)


# ---- the features: apply(env, setting) with CLEAR for none, the loop that reads the feature, the settings in order ---------------------
def _disturbance(env, s):
    if s == CLEAR:
        return env.clear_disturbance()
    M, J, seed = s
    r = np.random.RandomState(seed)
    env.set_disturbance(r.normal(0, 1, (env.nValidAct, M)), 2e-8 * r.uniform(0.5, 1, (N, M, J)), r.uniform(20, 200, (N, M, J)),
                        r.uniform(0, 1, (N, M, J)), t0=3)


def _noise_filter(env, s):
    if s == CLEAR:
        return env.set_noise_filter()
    if s == DEFAULT:
        return env.set_noise_filter(np.linalg.pinv(env.M2C_CL), env.M2C_CL)
    K, seed = s
    r = np.random.RandomState(seed)
    env.set_noise_filter(r.normal(0, 1, (K, env.nValidAct)) / np.sqrt(env.nValidAct), r.normal(0, 1, (env.nValidAct, K)))


def _recon_factors(env, s):
    from rlao_amd import _lib as L
    if s == CLEAR:                                                  # (a reconstructor without factors: n_modes = 0)
        return env._shard.upload(L.C_RECON, env.reconstructor)
    m2c, cm, recon = (env.M2C_CL, env.modal_CM, env.reconstructor) if s == DEFAULT else _basis(env, s)
    env._shard.upload(L.C_RECON, recon)
    env._shard.upload(L.C_RECON_FACTORS, np.concatenate([cm.reshape(-1), m2c.reshape(-1)]))


def _modal(env, s):
    if s == CLEAR:
        return env.clear_modal()
    m2c, cm, _ = _basis(env, s)
    env.set_modal(m2c=m2c, cm=cm)
    env.set_modal_gain(np.linspace(0.2, 0.4, N)[:, None] * np.ones((1, s)))


def _wavefront(env, s):
    if s == CLEAR:
        return env.clear_wavefront_basis()
    K, seed = s
    n_pix = int(np.count_nonzero(env.pupil))
    env.set_wavefront_basis(opd2m=np.random.RandomState(seed).normal(0, 1, (K, n_pix)) / n_pix)


def _science(env, s):
    if s == CLEAR:
        return env.clear_science()
    env.set_science(zero_padding=4, window=s, first_frame=2, log10=True)


def _policy(env, s):
    if s == CLEAR:
        return env.set_policy(None)
    H, F, seed = s
    env.set_policy(P.make_weights(H, F, seed=seed, scale=(20.0, 1.5, 2.0)))


def _mirrors_and_stars(env, s):
    if s == CLEAR:
        env.clear_dm_per_env()
        return env.clear_star_per_env()
    env.set_dm_misregistration(shift_x=s * np.linspace(-0.02, 0.02, N), radial_scaling=s * np.linspace(0.0, 0.01, N))
    env.set_magnitude_per_env(float(env.param.magnitude) + s * np.array([0.0, 0.5, 1.0, 2.0]))
    env.set_threshold_per_env(s * np.array([0.0, 0.01, 0.02, 0.05]))


# name -> (apply, loop, settings: small, larger, small again, CLEAR, final; what the shard goes back to afterwards)
FEATURES = {
    "disturbance": (_disturbance, _integrator, [(1, 1, 1), (3, 2, 2), (1, 1, 1), CLEAR, (1, 1, 3)], CLEAR),
    "noise_filter": (_noise_filter, _rollout, [(2, 1), (8, 2), (2, 1), CLEAR, (2, 3)], DEFAULT),
    "recon_factors": (_recon_factors, _integrator, [5, 12, 5, CLEAR, 5], DEFAULT),
    "modal": (_modal, _integrator_modal, [3, 7, 3, CLEAR, 3], CLEAR),
    "wavefront_basis": (_wavefront, _recorded, [(4, 1), (17, 2), (4, 1), CLEAR, (4, 3)], CLEAR),
    "science": (_science, _long_exposure, [8, 16, 8, CLEAR, 8], CLEAR),
    "policy": (_policy, _policy_rollout, [(1, 16, 1), (3, 32, 2), (1, 16, 1), CLEAR, (1, 16, 3)], CLEAR),
    "mirrors_and_stars": (_mirrors_and_stars, _integrator, [1.0, CLEAR, 1.0, CLEAR, 0.5], CLEAR),
}
CASES = [(d, f) for d in ("f32", "f64") for f in FEATURES]


@pytest.mark.parametrize("dtype,feature", CASES, ids=[f"{d}-{f}" for d, f in CASES])
def test_cycled_feature_runs_like_one_set_once(dtype, feature):
    """Every tensor the loop hands out (observations, actions, reward, Strehl, the wavefront record, the long-exposure sums and
    counts, the policy's windows) and get_state(): bit for bit those of the twin.  The float32 shard stays on the fused step."""
    apply, loop, settings, after = FEATURES[feature]
    env, twin = _env(dtype, "a"), _env(dtype, "b")
    try:
        for s in settings[:-1]:
            apply(env, s)
            if s != CLEAR:
                loop(env, 2)                                        # use it
        apply(env, settings[-1])
        apply(twin, settings[-1])
        got, want = _everything(env, loop(env, FRAMES)), _everything(twin, loop(twin, FRAMES))
        assert env.fused_step == twin.fused_step == (dtype == "f32")
        assert got.keys() == want.keys() and len(got) >= 4
        for k in want:
            _same(got[k], want[k], f"{feature} {k}")
        assert not np.array_equal(got["out[0]"][0], got["out[0]"][1])                    # (the envs do differ)
    finally:
        apply(env, after)
        apply(twin, after)


def test_the_feature_changes_the_loop():
    """The comparison above is of loops that do read the feature: with the final setting the integrator's observation differs from
    the bare shard's (disturbance, mirrors and stars), and the recorded loops hand out what only the feature produces."""
    env = _env("f32", "a")
    bare = _np(_integrator(env, FRAMES)[0]).copy()
    for feature in ("disturbance", "mirrors_and_stars"):
        apply, loop, settings, after = FEATURES[feature]
        try:
            apply(env, settings[-1])
            assert not np.array_equal(_np(loop(env, FRAMES)[0]), bare), feature
        finally:
            apply(env, after)
    assert np.array_equal(_np(_integrator(env, FRAMES)[0]), bare)                       # ... and cleared, it is the bare shard again


def test_close_with_every_feature_set_then_create_again():
    """One shard is closed with every feature set (every block of it is then freed by the shard's own destruction), and a shard
    created afterwards in the same process runs the bare loop bit for bit like the twin that has no feature set."""
    env, twin = _ENVS.pop(("f32", "a")), _env("f32", "b")
    for feature, (apply, loop, settings, after) in FEATURES.items():
        apply(env, settings[1] if settings[1] != CLEAR else settings[0])                # the larger setting of each
    _integrator(env, 2)
    env.close()
    fresh = _ENVS[("f32", "a")] = _make("f32")
    got, want = _everything(fresh, _integrator(fresh, FRAMES)), _everything(twin, _integrator(twin, FRAMES))
    assert fresh.fused_step and twin.fused_step
    for k in want:
        _same(got[k], want[k], k)
