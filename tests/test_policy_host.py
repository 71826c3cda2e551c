"""CPU: the host side of the on-device policy (aoenv_set_policy / aoenv_policy_forward / aoenv_run_policy_rollout): the ctypes
mirror of AoPolicy against the compiled header, the float64 restatement of tests/_policy_ref.py against a torch module of the
reference's shape, the weight extraction of rlao_amd.env.policy_arrays, and the history roll against the literal lines of
MAIN/PO4AO/mbrl.py:80-81.  The host model of the MFMA convolution (rlao_amd/csrc/policy.hpp: the band plan, the kernel selection,
the weight relayout, the channel gather) through the stand-alone driver tests/native/policy_driver.cpp against NumPy
restatements, over every image size and channel count the ABI allows; the driver once more under ASan + UBSan."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import _policy_ref as P

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "aoenv.h")


@pytest.fixture(scope="module")
def built_lib():
    sys.path.insert(0, REPO)
    import __graft_entry__ as g
    g.build()
    from rlao_amd import _lib
    return _lib


def test_policy_struct_matches_header_and_abi_is_7(built_lib, tmp_path):
    L = built_lib
    prog = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', "int main(void){",
            'printf("size %zu\\n", sizeof(AoPolicy));']
    prog += [f'printf("{f[0]} %zu\\n", offsetof(AoPolicy, {f[0]}));' for f in L.AoPolicy._fields_]
    prog += ['printf("abi %d\\n", (int)AOENV_ABI_VERSION);', "return 0;}"]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(prog))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-o", str(exe), str(src)], check=True)
    out = dict(l.split() for l in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(out["size"]) == C.sizeof(L.AoPolicy)
    for f in L.AoPolicy._fields_:
        assert int(out[f[0]]) == getattr(L.AoPolicy, f[0]).offset, f[0]
    assert int(out["abi"]) == L.ABI_VERSION == 7
    lib = L.load()
    assert lib.aoenv_abi_version() == 7
    for name in ("aoenv_set_policy", "aoenv_policy_forward", "aoenv_run_policy_rollout"):
        assert hasattr(lib, name) and name in L.EXPORTS
    # no env: every entry point refuses a null handle
    assert lib.aoenv_set_policy(None, None, None) != 0
    assert lib.aoenv_policy_forward(None, None, None, None, None, None) != 0
    assert lib.aoenv_run_policy_rollout(None, None, None, None, None, None, None, None, None, None) != 0


def _inputs(n, H, a, seed):
    rng = np.random.RandomState(seed)
    return rng.normal(0, 1, (n, a, a)), rng.normal(0, 1, (n, H - 1, a, a)), rng.normal(0, 1, (n, H - 1, a, a))


@pytest.mark.parametrize("H,n_filt,proj", [(1, 16, False), (3, 24, True), (5, 8, True)])
def test_restatement_equals_the_torch_module_in_float64(H, n_filt, proj):
    a, n = 7, 3
    rng = np.random.RandomState(3)
    act_idx = np.sort(rng.choice(a * a, 37, replace=False))
    xv, yv = np.divmod(act_idx, a)
    F = rng.normal(0, 0.3, (37, 37)) if proj else None
    w = P.make_weights(H, n_filt, seed=11, scale=(1.0, 2.0, 3.0))
    obs, po, pa = _inputs(n, H, a, 5)
    ours = P.policy(w, obs, po, pa, act_idx, F)
    theirs = P.torch_eval(w, obs, po, pa, xv, yv, F)
    inner = np.abs(P.network(w, obs, po, pa).reshape(n, -1)[:, act_idx])
    assert 0.1 < (inner < 1).mean() < 0.9                           # the clamp takes part
    assert np.abs(ours - theirs).max() <= 1e-12
    mask = np.ones(a * a, dtype=bool)
    mask[act_idx] = False
    assert (ours.reshape(n, -1)[:, mask] == 0).all()


def test_weight_extraction_from_module_sequential_and_dict():
    import torch
    from rlao_amd.env import policy_arrays
    w = P.make_weights(3, 16, seed=2)
    w["negative_slope"] = 0.02
    mod = P.torch_module(w, np.arange(3), np.arange(3))
    got = [policy_arrays(mod), policy_arrays(mod.net), policy_arrays({k: w[k] for k in ("w1", "b1", "w2", "b2", "w3", "b3", "negative_slope")}),
           policy_arrays(dict(mod.state_dict(), negative_slope=0.02)), policy_arrays(dict(mod.net.state_dict(), negative_slope=0.02))]
    for g in got:
        assert g["n_history"] == 3 and g["n_filt"] == 16 and g["negative_slope"] == 0.02
        for k in ("w1", "b1", "w2", "b2", "w3", "b3"):
            assert g[k].dtype == np.float64 and g[k].flags["C_CONTIGUOUS"] and np.array_equal(g[k], w[k]), k
    # a float32 module: the arrays are the float32 values, widened
    m32 = P.torch_module(w, np.arange(3), np.arange(3), dtype=torch.float32)
    assert np.array_equal(policy_arrays(m32)["w2"], w["w2"].astype(np.float32).astype(np.float64))
    with pytest.raises(ValueError):
        policy_arrays(dict(w, w2=w["w2"][:, :-1]))
    with pytest.raises(ValueError):
        policy_arrays(dict(w, w1=w["w1"][:, :-1]))                  # an even channel count is no 2H - 1
    with pytest.raises(ValueError):
        policy_arrays(mod.net[:3])


@pytest.mark.parametrize("n_steps", [0, 1, 2, 3, 4, 9])
def test_history_roll_equals_the_trainer_loop(n_steps):
    """H = 4: n_steps below, at and above H - 1 = 3.  The literal lines of mbrl.py:80-81 on torch tensors against the index
    arithmetic of the library (restated in _policy_ref.window / roll), and every step's window on the way."""
    import torch
    H, n, a = 4, 2, 3
    rng = np.random.RandomState(n_steps)
    past0 = rng.normal(0, 1, (n, H - 1, a, a))
    traj = rng.normal(0, 1, (max(n_steps, 1), n, a, a))
    past = torch.as_tensor(past0)
    for k in range(n_steps):
        assert np.array_equal(P.window(past0, traj, k), past.numpy()), k
        new = torch.as_tensor(traj[k])
        past = torch.cat([past[:, 1:, :, :], new.unsqueeze(1)], dim=1)          # mbrl.py:80 with a leading env dimension
    assert np.array_equal(P.roll(past0, traj, n_steps), past.numpy())


# ---- the host model of the MFMA convolution: rlao_amd/csrc/policy.hpp through tests/native/policy_driver.cpp ---------------------
CHANNELS = list(range(1, 64, 2)) + list(range(16, 129, 16))          # 2H - 1 for H = 1 .. 32, and n_filt in whole N tiles
DOMAIN = [(a, c) for a in range(2, 257) for c in CHANNELS]


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = P.build_driver(tmp_path_factory.mktemp("policy"))
    if exe is None:
        pytest.skip("hipcc not available")
    return exe


@pytest.fixture(scope="module")
def plans(driver):
    got, _ = P.host_plans(driver, DOMAIN)
    return got


def test_band_plan_is_the_restatement_and_keeps_its_invariants(driver, plans):
    rows, bands, lds, lds1, fits, ksteps = plans.T
    a, c = np.array(DOMAIN).T
    want = np.array([P.bands(*p) + (P.conv_lds(*p), P.conv_lds_rows(*p, 1), int(P.mfma_fits(*p)), P.ksteps(p[1])) for p in DOMAIN])
    assert np.array_equal(plans, want)
    ok = fits == 1
    assert ((bands - 1) * rows < a)[ok].all() and (a <= bands * rows)[ok].all() and (rows >= 1).all() and (bands >= 1).all()   # no empty band
    assert ((rows * a <= P.BAND_PIXELS) | (rows == 1))[ok].all()
    assert (rows * a <= P.BAND_PIXELS)[ok].all()                    # (a <= 256: one row is a band, too)
    assert (lds <= P.LDS_MAX)[ok].all()
    # two workgroups share a CU exactly when one row fits in half a CU
    assert np.array_equal((lds <= P.LDS_MAX // 2)[ok], (lds1 <= P.LDS_MAX // 2)[ok])
    assert (ksteps == -(-9 * c // 4)).all()
    # the MFMA kernel is refused for an image above 256 or below 2 across and for an LDS overflow, and for nothing else
    assert np.array_equal(fits == 0, lds > P.LDS_MAX)
    extra = [(1, 1), (1, 128), (257, 1), (300, 16), (256, 1), (2, 1)]
    got, _ = P.host_plans(driver, extra)
    assert got[:, 4].tolist() == [0, 0, 0, 0, 1, 1] and (got[:4, 2] <= P.LDS_MAX).any()
    first = lambda ch: min(x for (x, cc), f in zip(DOMAIN, fits) if cc == ch and not f)
    assert first(128) == 102 and first(64) == 208


def test_staging_divides_exactly_by_multiplication(plans):
    """The staging loop of k_policy_conv_mfma splits i < C span into (channel, row, column) with two multiplications by
    ceil(2^32 / span) and ceil(2^32 / a) (the high word).  span: the source rows of a band, clipped to the image.  For every band
    of every fitting plan both are the true quotients (grouped by divisor: the longest range of a divisor covers the shorter)."""
    span_range, act_range, largest = {}, {}, 0
    for (a, c), (rows, bands, _, _, fits, _) in zip(DOMAIN, plans.tolist()):
        if not fits:
            continue
        for b in {0, 1, bands - 2, bands - 1} & set(range(bands)):
            y0 = b * rows
            r = min(rows, a - y0)
            span = (min(y0 + r + 1, a) - max(y0 - 1, 0)) * a
            span_range[span] = max(span_range.get(span, 0), c * span)
            act_range[a] = max(act_range.get(a, 0), span)
            largest = max(largest, c * span)
    assert largest < 128 * 768                                      # the range the kernel's comment claims
    for ranges in (span_range, act_range):
        for d, n in ranges.items():
            i = np.arange(n, dtype=np.uint64)
            m = np.uint64(((1 << 32) + d - 1) // d)
            assert np.array_equal((i * m) >> np.uint64(32), i // np.uint64(d)), d


@pytest.mark.parametrize("c_in", [1, 3, 5, 11, 63, 16, 128])
def test_relayout_puts_every_weight_in_its_lane(driver, c_in):
    """Weight (f, k) lands at [k / 4][f / 16][16 (k % 4) + f % 16]; the K padding is zero"""
    n_filt = 128 if c_in == 128 else (48 if c_in == 11 else 16)
    K = 9 * c_in
    w = (np.arange(n_filt * K, dtype=np.float64) + 1).reshape(n_filt, c_in, 3, 3)     # every weight its own value, exact in float32
    got, _ = P.host_relayout(driver, w)
    assert got.shape == (P.ksteps(c_in), n_filt // 16, 64) and got.dtype == np.float32
    f, k = np.divmod(np.arange(n_filt * K), K)
    want = np.zeros_like(got)
    want[k // 4, f // 16, 16 * (k % 4) + f % 16] = w.ravel()
    assert np.array_equal(got, want)
    assert (got != 0).sum() == n_filt * K and got.size - n_filt * K == n_filt * (4 * P.ksteps(c_in) - K)


@pytest.mark.parametrize("H", [1, 2, 4, 32])
def test_channel_gather_is_the_window_of_the_restatement(driver, H):
    """k below, at and above H - 1: every channel of the first layer comes from where _policy_ref.window takes it"""
    E = 3
    for k in sorted({0, 1, max(H - 2, 0), H - 1, H, H + 3}):
        # arrays of labels: value = kind * 10000 + index * 10 + env
        label = lambda kind, idx, e: kind * 10000 + idx * 10 + e
        traj = {kind: np.array([[label(kind, s, e) for e in range(E)] for s in range(k + 1)], dtype=np.float64)[:, :, None, None]
                for kind in (1, 2)}
        past = {kind: np.array([[label(kind, r, e) for r in range(H - 1)] for e in range(E)], dtype=np.float64).reshape(E, H - 1, 1, 1)
                for kind in (3, 4)}
        want = np.concatenate([traj[1][k][:, None], P.window(past[3], traj[1], k), P.window(past[4], traj[2], k)], axis=1)[:, :, 0, 0]
        for e in range(E):
            got, _ = P.host_channels(driver, H, k, E, e)
            assert len(got) == 2 * H - 1
            names = {"O": 1, "A": 2, "PO": 3, "PA": 4}
            assert [label(names[kind], idx, e) for kind, idx in got] == want[e].astype(int).tolist(), (H, k, e)


def test_exact_case_reference_is_the_restatement():
    """The reference of the GPU sweep's exact cases (_policy_ref.exact_case: the convolutions as matrix products) against the
    restatement the tests above pin to torch: the same bits on exact data, with and without the projection."""
    a, H, n_filt, n = 7, 3, 16, 3
    idx = np.sort(np.random.RandomState(3).choice(a * a, 37, replace=False))
    w = P.exact_weights(H, n_filt, seed=1)
    x = P.exact_inputs(n, H, a, seed=2)
    fr, fl = P.exact_factors(idx.size, seed=3)
    assert (np.abs(fr) > 0).sum(axis=1).max() <= 8 and set(np.unique(w["w2"])) == {-1.0, 0.0, 1.0} and np.abs(x[0]).max() == 2
    case = P.exact_case(w, x, idx, (fr, fl))
    assert np.array_equal(P.layers(w, *x)[2], P.network(w, *x))
    assert np.array_equal(case["plain"], P.policy(w, *x, idx, None, case["clamp"]))
    assert np.array_equal(case["proj"], P.policy(w, *x, idx, fl @ fr, case["clamp"]))
    assert np.log2(case["clamp"]) % 1 == 0 and max(case["quanta"]) < 2 ** 24


SWEEP = [(a, H, F) for a, cases in P.SWEEP_CASES.items() for H, F in cases]
GENERAL = [(4, 1, 64, 21, 39), (8, 0, 64, 21, 39), (4, 0, 24, 9, 5), (4, 0, 72, 9, 5), (4, 0, 128, 102, 7), (4, 0, 16, 300, 5),
           (4, 0, 64, 300, 63), (8, 1, 16, 9, 1)]                   # path 1, float64, n_filt % 16, LDS overflow, a > 256


def test_kernel_selection(driver):
    """Every case of the GPU sweep takes the MFMA kernel on a float32 shard with path 0 -- so the sweep cannot pass through the
    general kernel -- and path 1, a float64 shard, a ragged filter count and an image that does not fit take the general one."""
    got, _ = P.host_select(driver, [(4, 0, F, a, 2 * H - 1) for a, H, F in SWEEP])
    assert len(got) == 20 and all(got)
    for esz, path in ((4, 1), (8, 0), (8, 1)):
        got, _ = P.host_select(driver, [(esz, path, F, a, 2 * H - 1) for a, H, F in SWEEP])
        assert not any(got), (esz, path)
    got, _ = P.host_select(driver, GENERAL)
    assert not any(got)
    got, _ = P.host_select(driver, [(4, 0, 128, 101, 7), (4, 0, 64, 207, 7), (4, 0, 16, 256, 1), (4, 0, 16, 2, 1)])
    assert all(got)


def test_driver_is_clean_under_asan_and_ubsan(driver, tmp_path):
    """The same requests in a stand-alone sanitized program, run directly: a clean exit, no report, the same answers."""
    exe = P.build_driver(tmp_path, sanitize=True)
    if exe is None:
        pytest.skip("hipcc not available")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    clean = lambda err: "ERROR: AddressSanitizer" not in err and "runtime error" not in err
    pairs = DOMAIN[::7] + [(1, 1), (300, 16)]
    got, err = P.host_plans(exe, pairs, env=env)
    assert clean(err), err
    assert np.array_equal(got, P.host_plans(driver, pairs)[0])
    sel = [(4, 0, F, a, 2 * H - 1) for a, H, F in SWEEP] + GENERAL
    got, err = P.host_select(exe, sel, env=env)
    assert clean(err), err
    assert got == [True] * len(SWEEP) + [False] * len(GENERAL)
    for c_in, n_filt in ((1, 16), (63, 16), (128, 128)):
        w = (np.arange(n_filt * 9 * c_in, dtype=np.float64) + 1).reshape(n_filt, c_in, 3, 3)
        got, err = P.host_relayout(exe, w, env=env)
        assert clean(err), err
        assert np.array_equal(got, P.host_relayout(driver, w)[0])
    for H, k in ((1, 0), (1, 5), (2, 0), (4, 2), (4, 3), (32, 0), (32, 31), (32, 40)):
        got, err = P.host_channels(exe, H, k, 3, 2, env=env)
        assert clean(err), err
        assert got == P.host_channels(driver, H, k, 3, 2)[0]
