"""GPU: the policy convolutions over every band plan, tile count and filter grouping of k_policy_conv_mfma
(rlao_amd/csrc/policy_kernels.hip), on seven actuator grids from 5 to 53 across and about twenty (n_history, n_filt) shapes up to
the limits of the ABI (32, 128).

Exact data.  Inputs are integers in [-2, 2], the weights of the two wide layers ternary with 16 non-zeros per filter (more where
a filter needs them so that every tap (ci, ky, kx) is non-zero in some filter), w3 ternary with every tap non-zero, biases in
{-1, 0, 1}, negative_slope = 0.5, the clamp a power of two, the projection factors ternary.  Every partial sum of every summation
order is then a multiple of its layer's quantum (1, 0.5, 0.25, 0.25) below 2^24 quanta -- each case computes that bound from the
network of absolute values and asserts it, with the other input conditions, on the float64 reference alone before the device
is touched (_policy_ref.exact_case) -- so float32, float64, the MFMA kernel and the general kernel all give the reference's bits:
a tap taken from the neighbouring pixel at a band seam, from the frame of zeros, from another filter group or left out changes
them.  Targets: the float32 shard by its default path (the MFMA kernel: tests/test_policy_host.py pins the selection for every
case here against the library's own expression), the same shard with path = 1, and float64 twins at a = 5, 9, 17.

Real-valued parity at the new shapes by the rule and the helpers of tests/test_gpu_policy.py (8 x |torch f32 - torch f64| on the
test's inputs); batch position across bands; teacher-forced rollouts on a two-band shard.  The largest differences measured on
MI355X and every shard's build time are in profiles/policy_sweep_parity_maxima.json (AO_PARITY_REPORT=<file> with this module
alone rewrites it)."""
import json
import os
import time

import numpy as np
import pytest

import _policy_ref as P
import test_gpu_policy as G

pytestmark = pytest.mark.gpu


def _geo(n_sub, n_pix, n_modes=12):
    return dict(diameter=0.4 * n_sub, nSubaperture=n_sub, nPixelPerSubap=n_pix, r0=0.13, L0=30.0, windSpeed=[10.0], windDirection=[72.0],
                fractionalR0=[1.0], altitude=[0.0], nModes=n_modes, nLoop=16)


GEO = {5: _geo(4, 6, 8), 9: dict(G.SMALL, nModes=12, nLoop=16), 16: _geo(15, 4), 17: _geo(16, 4), 21: dict(G.BIG, nModes=12, nLoop=16),
       41: _geo(40, 4), 53: _geo(52, 4)}
N_ENVS = {5: 3, 9: 3, 16: 3, 17: 3, 21: 3, 41: 3, 53: 2}
TWINS = (5, 9, 17)                                                  # float64 shards: the general kernel is one template
SWEEP = [(a, H, F) for a, cases in P.SWEEP_CASES.items() for H, F in cases]
MAXIMA, BUILD = {}, {}


def _poly_m2c(geo):
    """A modes-to-commands matrix [A, nModes] for the wide shards: orthonormal polynomials of degree 1 .. 4 in the actuator
    coordinates.  The policy reads nothing of the modal basis but the projector M2C pinv(M2C), and the Zernike fit of set_params
    (a pseudo-inverse over every pupil pixel and actuator) would be most of such a shard's build time."""
    from rlao_amd import calib
    dmt = calib.DMTables(calib.params_from_args(geo))
    u, v = ((np.asarray(c, dtype=np.float64) - (dmt.nAct - 1) / 2) / (dmt.nAct / 2) for c in (dmt.xvalid, dmt.yvalid))
    cols = [u ** i * v ** (d - i) for d in range(1, 5) for i in range(d + 1)][:geo["nModes"]]
    return np.linalg.qr(np.stack(cols, axis=1))[0]


def _make(a, dtype):
    from rlao_amd.env import BatchedAOEnv
    env = BatchedAOEnv(n_envs=N_ENVS[a], device=0, dtype=dtype)
    env.set_params(GEO[a], camera="ideal", wfs_type="shackhartmann", gainCL=0.4, m2c=_poly_m2c(GEO[a]) if a >= 41 else None)
    return env


def _assert_plans():
    """Each case sits on the shape it is here for (the restatement of policy_bands that tests/test_policy_host.py pins against the
    library's): a changed band size or LDS limit cannot move one off it silently."""
    assert len(SWEEP) == 20 and all(P.mfma_fits(a, 2 * H - 1) and P.mfma_fits(a, F) for a, H, F in SWEEP)
    B, T = P.band_rows, P.wave_tiles
    for C in (1, 5, 48, 63, 128):
        assert B(5, C) == [5]
    assert T(25) == [1, 1, 0, 0]                                    # 2 tiles: waves 2 and 3 leave without one
    for C in (3, 11, 32, 63, 96, 128):
        assert B(9, C) == [9]
    assert T(81) == [2, 2, 1, 1] and 81 % 16 != 0                   # 6 tiles, a ragged tail
    assert B(16, 5) == B(16, 16) == B(16, 3) == B(16, 48) == [16] and T(256) == [4, 4, 4, 4]    # exactly 256 pixels, no tail lane
    assert B(16, 39) == [16] and B(16, 64) == [8, 8]                # (20, 64): the two layers on different plans, the second LDS-bound
    assert P.conv_lds_rows(16, 64, 16) > P.LDS_MAX // 2 >= P.conv_lds(16, 64)
    for C in (3, 32, 63, 64):
        assert B(17, C) == [9, 8]
    assert T(9 * 17) == [3, 3, 2, 2] and T(8 * 17) == [3, 2, 2, 2]  # 10 and 9 tiles
    assert (3 * 11 * 19) & 1                                        # (2, 32), layer 1: odd tile planes, the alignment word in LDS
    assert B(17, 11) == [9, 8] and B(17, 96) == [6, 6, 5]
    assert B(21, 5) == B(21, 48) == B(21, 63) == [11, 10] and P.conv_lds(21, 63) > 64 * 1024
    assert B(21, 128) == [4, 4, 4, 4, 4, 1]
    assert B(41, 5) == B(41, 16) == B(41, 39) == B(41, 7) == [6] * 6 + [5]
    assert B(41, 64) == [5] * 8 + [1] and T(41) == [1, 1, 1, 0]     # a last band of one row: 3 tiles, wave 3 idle
    assert B(41, 128) == [1] * 41
    assert B(53, 128) == [3] * 17 + [2] and P.conv_lds(53, 128) == 146432 > P.LDS_MAX // 2    # one workgroup holds the CU
    assert P.conv_lds_rows(53, 128, 1) > P.LDS_MAX // 2
    assert B(53, 63) == [3] * 17 + [2] and P.conv_lds(53, 63) == 72080
    assert B(53, 1) == B(53, 16) == B(53, 7) == [4] * 13 + [1] and B(53, 64) == [3] * 17 + [2]
    # filter groups: NT 1, 2, 4 with 1, 2 and 3 groups
    nt = lambda F: 4 if F // 16 % 4 == 0 else (2 if F // 16 % 2 == 0 else 1)
    assert {(nt(F), F // 16 // nt(F)) for _, _, F in SWEEP} == {(1, 1), (1, 3), (2, 1), (2, 3), (4, 1), (4, 2)}
    # k steps of the first layer: odd and even counts, K paddings of one and of three taps
    assert {P.ksteps(2 * H - 1) for _, H, _ in SWEEP} == {3, 7, 25, 12, 16, 142, 88}
    assert {(-9 * (2 * H - 1)) % 4 for _, H, _ in SWEEP} == {1, 3}
    assert max(H for _, H, _ in SWEEP) == 32 and max(F for _, _, F in SWEEP) == 128


_assert_plans()


@pytest.fixture(scope="module")
def shards():
    made = {}

    def get(a, dtype="f32"):
        if (a, dtype) not in made:
            t = time.perf_counter()
            made[a, dtype] = env = _make(a, dtype)
            BUILD[f"a{a}_{dtype}"] = round(time.perf_counter() - t, 2)
            assert env.nActuator == a
        return made[a, dtype]

    yield get
    for e in made.values():
        e.close()
    out = os.environ.get("AO_PARITY_REPORT")
    if out and MAXIMA:
        with open(out, "w") as f:
            f.write(json.dumps(dict(MAXIMA, shard_build_seconds=BUILD), indent=1, sort_keys=True) + "\n")


def _where(a, H, F, got, ref):
    """the first differing pixel of an exact case and the bands it lies in"""
    bad = np.argwhere(got != ref)
    e, y, x = bad[0]
    rows1, rows2 = P.bands(a, 2 * H - 1)[0], P.bands(a, F)[0]
    return (f"{len(bad)} pixels differ; first: env {e}, pixel ({y}, {x}): {got[e, y, x]!r} for {ref[e, y, x]!r}; band {y // rows1} "
            f"(row {y % rows1} of {rows1}) of layer 1, band {y // rows2} (row {y % rows2} of {rows2}) of layer 2, {F // 16} filter tiles")


@pytest.mark.parametrize("a,H,F", SWEEP)
def test_exact_data_gives_the_reference_bits(shards, a, H, F):
    env = shards(a)
    idx = G._act_idx(env)
    w = P.exact_weights(H, F, seed=1000 * a + 10 * H + F)
    x = P.exact_inputs(env.n_envs, H, a, seed=a + H)
    factors = P.exact_factors(idx.size, seed=a)
    case = P.exact_case(w, x, idx, factors)                         # asserts every input condition on the reference alone
    print(f"a={a} H={H} F={F}: clamp {case['clamp']}, {case['unclamped']:.2f} unclamped, quanta {[f'{q:.3g}' for q in case['quanta']]} of {2 ** 24}")
    assert np.abs(case["plain"]).max() == case["clamp"] and np.abs(case["proj"]).max() > 0
    targets = [("f32", 0), ("f32", 1)] + ([("f64", 0)] if a in TWINS else [])
    for dtype, path in targets:
        e = shards(a, dtype)
        for name, proj in (("plain", None), ("proj", factors)):
            e.set_policy(w, F=proj, clamp=case["clamp"], path=path)
            got = G._action(e, x)
            assert np.array_equal(got, case[name]), (dtype, path, name, _where(a, H, F, got, case[name]))
        e.set_policy(None)
    MAXIMA[f"exact_a{a}_H{H}_F{F}"] = {"clamp": case["clamp"], "unclamped": round(case["unclamped"], 3), "largest_sum_in_quanta": max(case["quanta"]),
                                       "bit_equal_on": [f"{d}_path{p}" for d, p in targets]}


PARITY = [(5, 3, 48), (16, 20, 64), (17, 6, 96), (41, 20, 64), (53, 4, 128)]


@pytest.mark.parametrize("a,H,F", PARITY)
def test_forward_parity_at_the_new_shapes(shards, a, H, F):
    env = shards(a)
    w = P.make_weights(H, F, seed=500 + a + H + F, scale=G.SCALE)
    x = G._inputs(env, H, seed=31 + a)
    ref, tol32, yard = G._reference(env, w, x, True)
    env.set_policy(w)
    got = G._action(env, x)
    err = float(np.abs(got - ref).max())
    MAXIMA[f"a{a}_H{H}_F{F}_proj_f32"] = {"gpu_vs_f64": err, "torch_f32_vs_f64": yard}
    print(f"a={a} H={H} F={F}: |gpu - f64| = {err:.3e}, |torch f32 - f64| = {yard:.3e}, tol = {tol32:.3e}")
    assert err <= tol32
    mask = np.ones(a * a, dtype=bool)
    mask[G._act_idx(env)] = False
    assert (got.reshape(env.n_envs, -1)[:, mask] == 0).all()
    env.set_policy(None)


@pytest.mark.parametrize("a,H,F", [(41, 20, 64), (53, 4, 128)])
def test_batch_position_across_bands(shards, a, H, F):
    """The same inputs in two rows of the batch: the same bits, in every band.  a = 53 has two rows: the rows swapped in a second
    call give the swapped outputs."""
    import torch
    env = shards(a)
    w = P.make_weights(H, F, seed=41, scale=G.SCALE)
    x = [t.copy() for t in G._inputs(env, H, seed=23)]
    env.set_policy(w)
    if env.n_envs == 3:
        for t in x:
            t[2] = t[0]
        got = env.policy_action(*x)
        assert torch.equal(got[0], got[2]) and not torch.equal(got[0], got[1])
    else:
        got = env.policy_action(*x)
        swapped = env.policy_action(*(t[::-1].copy() for t in x))
        assert torch.equal(got[0], swapped[1]) and torch.equal(got[1], swapped[0]) and not torch.equal(got[0], got[1])
    assert float(got[0].abs().max()) > 0
    env.set_policy(None)


@pytest.mark.parametrize("H,F,n_steps", [(2, 32, 5), (6, 96, 3)])
def test_rollout_teacher_forced_on_two_bands(shards, H, F, n_steps):
    """a = 17, two bands.  (2, 32, 5): the trajectory feeds every past channel from step 1 on; (6, 96, 3): n_steps below H - 1, the
    window roll shifts in place.  Every recorded action is policy_action on the rebuilt windows, bit for bit."""
    env = shards(17)
    w = P.make_weights(H, F, seed=5, scale=(20.0, 1.5, 2.0))
    env.set_policy(w)
    G._prologue(env)
    past = G._past(env, H, seed=9)
    tr, new_past = env.policy_rollout(0, n_steps, sigma=0.0, past=past)
    assert tuple(tr.obs.shape) == (n_steps + 1, 3, 17, 17) and tuple(tr.action.shape) == (n_steps, 3, 17, 17)
    obs, act = G._check_teacher_forced(env, tr, past)
    assert np.isfinite(obs).all() and np.abs(act).max() > 1e-3
    assert np.array_equal(G._host(new_past[0]), P.roll(past[0], obs, n_steps))
    assert np.array_equal(G._host(new_past[1]), P.roll(past[1], act, n_steps))
    env.set_policy(None)
