"""CPU: the host side of the command-space disturbance (aoenv_set_disturbance / BatchedAOEnv.set_disturbance).  The model
(rlao_amd/csrc/disturb.hpp, ONE host/device source for k_disturb_apply and the driver tests/native/disturb_driver.cpp) against
NumPy float64, the argument handling of the Python layer, the ABI that goes with it and the refusals that need no device.  No GPU."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import _disturb_ref as D
from rlao_amd import _lib as L
from rlao_amd.env import disturbance_value, resolve_disturbance
from rlao_amd.wrappers import HistoryEnv, TimeDelayEnv, TorchWrapper

HEADER = os.path.join(D.REPO, "include", "aoenv.h")
TS = 0.002                                                         # samplingTime of the argument tests [s]


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = D.build_driver(tmp_path_factory.mktemp("disturb"))
    if exe is None:
        pytest.skip("hipcc not available")
    return exe


def _params(seed, M, J):
    rng = np.random.RandomState(seed)
    amp = rng.uniform(0.0, 2e-7, (M, J))
    if M * J > 1:
        amp[0, 0] = 0.0                                             # a line that is switched off
    freq = rng.uniform(-0.5, 0.5, (M, J))                           # cycles per frame, 53 random bits each
    freq[-1, -1] = 1.0 / 3.0
    freq[0, -1] = 8.0 / 64.0                                        # and one that IS representable in few bits
    phase = rng.uniform(-2.0, 2.0, (M, J))
    return amp, freq, phase


@pytest.mark.parametrize("M,J", [(1, 1), (3, 2), (64, 8)])
def test_driver_against_numpy(driver, M, J):
    """v[m] of the driver against NumPy float64.  Small tau: the plain formula.  tau near 2^40 (and 10^9, the t0 of the GPU
    tests): the float64 product f tau alone is then uncertain by up to 2^-53 f tau cycles, so the checker forms and reduces the
    phase exactly and takes NumPy's float64 sine of that.  Tolerance per line, summed over a mode's lines:
    amp (2 pi 2^-52 (|f| tau + |phi| + 1) + 4 2^-53), D.line_tolerance."""
    amp, freq, phase = _params(10 * M + J, M, J)
    small, large = [0, 1, 2, 63, 64, 1000], [10 ** 9 + 1, 2 ** 40 - 1, 2 ** 40, 2 ** 40 + 12345]
    v, _ = D.host_modes(driver, amp, freq, phase, small + large)
    worst = 0.0
    for row, tau in zip(v, small + large):
        tol = D.line_tolerance(amp, freq, phase, tau).sum(axis=1)
        refs = [D.exact_phase_lines(amp, freq, phase, tau).sum(axis=1)]
        if tau in small:
            refs.append(D.numpy_lines(amp, freq, phase, tau).sum(axis=1))
        for want in refs:
            err = np.abs(row - want)
            worst = max(worst, float((err / np.maximum(tol, 1e-300)).max()))
            assert (err <= tol).all(), (tau, err.max(), tol.min())
    print(f"M={M} J={J}: max err / tol = {worst:.3f}")
    assert np.abs(v).max() > 1e-8                                   # the lines do something


def test_driver_properties(driver):
    """Zero amplitudes give +0 exactly; a line of period 8 frames repeats exactly (8 / 64 cycles per frame is a power of two,
    the phase reduction is exact); the sum runs over j in index order (a permutation of the lines may change the last bit, the
    same order twice never does)."""
    amp, freq, phase = _params(5, 3, 2)
    v0, _ = D.host_modes(driver, np.zeros_like(amp), freq, phase, [1, 2 ** 40])
    assert (v0 == 0).all() and not np.signbit(v0).any()
    f8 = np.full((1, 1), 8.0 / 64.0)
    v, _ = D.host_modes(driver, np.full((1, 1), 1e-7), f8, np.zeros((1, 1)), [1, 9, 2 ** 40 + 1, 3, 10 ** 9 + 3])
    assert v[0, 0] == v[1, 0] == v[2, 0] and v[3, 0] == v[4, 0]
    np.testing.assert_allclose(v[0, 0], 1e-7 * np.sin(2 * np.pi / 8), rtol=1e-15)
    a, b = D.host_modes(driver, amp, freq, phase, [7, 77])[0], D.host_modes(driver, amp, freq, phase, [7, 77])[0]
    assert np.array_equal(a, b)


def test_driver_is_clean_under_asan_and_ubsan(tmp_path):
    """The host instantiation of disturb.hpp in a stand-alone sanitized program: no report, and the same values."""
    exe = D.build_driver(tmp_path, sanitize=True)
    if exe is None:
        pytest.skip("hipcc not available")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    amp, freq, phase = _params(3, 64, 8)
    v, err = D.host_modes(exe, amp, freq, phase, [1, 2 ** 40], env=env)
    assert "ERROR: AddressSanitizer" not in err and "runtime error" not in err, err
    for row, tau in zip(v, [1, 2 ** 40]):
        assert (np.abs(row - D.exact_phase_lines(amp, freq, phase, tau).sum(axis=1)) <= D.line_tolerance(amp, freq, phase, tau).sum(axis=1)).all()


# ---- BatchedAOEnv.set_disturbance: the arguments ---------------------------------------------------------------------
A_, N_ = 7, 4
M2C = np.arange(A_ * 5, dtype=np.float64).reshape(A_, 5) / 10.0


def _resolve(modes, amp, freq, phase=None, t0=0, env_ids=None, current=None):
    return resolve_disturbance(modes, amp, freq, phase, t0, env_ids, N_, A_, TS, M2C, current)


def test_broadcast_units_and_modes():
    amp, hz = np.array([[1e-7, 2e-7], [3e-7, 0.0], [0.0, 5e-8]]), np.array([[10.0, 20.0], [30.0, 40.0], [50.0, 62.5]])
    d = _resolve(3, amp, hz)
    assert d["modes"].shape == (A_, 3) and np.array_equal(d["modes"], M2C[:, :3]) and d["modes"].flags["C_CONTIGUOUS"]
    for key in ("amp", "freq", "phase"):
        assert d[key].shape == (N_, 3, 2) and d[key].dtype == np.float64 and d[key].flags["C_CONTIGUOUS"]
    assert all(np.array_equal(d["amp"][e], amp) for e in range(N_))
    assert np.array_equal(d["freq"][2], hz * TS)                   # Hz -> cycles per frame: one multiply by samplingTime
    assert d["freq"][0, 2, 1] == 0.125 and (d["phase"] == 0).all() and d["t0"] == 0
    # per env, an explicit table (a tensor too), a phase, t0
    B = np.linspace(-1, 1, A_ * 2).reshape(A_, 2)
    pe = np.arange(N_ * 2 * 1, dtype=np.float64).reshape(N_, 2, 1)
    d = _resolve(torch.tensor(B), pe * 1e-8, pe + 1.0, phase=pe / 10.0, t0=10 ** 9)
    assert np.array_equal(d["modes"], B) and np.array_equal(d["amp"], pe * 1e-8) and np.array_equal(d["freq"], (pe + 1.0) * TS)
    assert np.array_equal(d["phase"], pe / 10.0) and d["t0"] == 10 ** 9
    # mixed: amp per env, freq shared
    d = _resolve(B, pe * 1e-8, np.array([[5.0], [6.0]]))
    assert np.array_equal(d["freq"][3], np.array([[5.0], [6.0]]) * TS)


def test_env_ids_replace_the_listed_rows_only():
    amp, hz = np.full((2, 3), 1e-7), np.full((2, 3), 25.0)
    first = _resolve(2, amp, hz, env_ids=[1, 3])                    # none in force: the others carry no lines
    assert (first["amp"][[0, 2]] == 0).all() and (first["amp"][[1, 3]] == 1e-7).all() and (first["freq"][[0, 2]] == 0).all()
    full = _resolve(2, np.arange(N_ * 6, dtype=np.float64).reshape(N_, 2, 3), hz, phase=np.full((2, 3), 0.25))
    blocks = np.stack([np.full((2, 3), 7.0), np.full((2, 3), 9.0)])
    out = _resolve(None, blocks, blocks * 10, env_ids=[3, 1], current=full, t0=5)
    assert (out["amp"][3] == 7.0).all() and (out["amp"][1] == 9.0).all() and (out["freq"][3] == 70.0 * TS).all()
    assert (out["phase"][[1, 3]] == 0).all()
    for key in ("amp", "freq", "phase"):
        assert np.array_equal(out[key][[0, 2]], full[key][[0, 2]]), key
    assert np.array_equal(out["modes"], full["modes"]) and out["t0"] == 5
    assert full["amp"][3, 0, 0] == 18.0 and out["amp"] is not full["amp"]      # the result is the caller's: not a view of `current`
    mask = _resolve(2, blocks, hz, env_ids=np.array([False, True, False, True]), current=full)      # a mask: ascending
    assert (mask["amp"][1] == 7.0).all() and (mask["amp"][3] == 9.0).all()
    one = _resolve(2, np.full((2, 3), 4.0), hz, env_ids=[2], current=full)      # [M, J] for every listed env
    assert (one["amp"][2] == 4.0).all() and np.array_equal(one["amp"][[0, 1, 3]], full["amp"][[0, 1, 3]])


def test_disturbance_value_is_the_formula():
    amp, freq, phase = (np.stack([D_ for D_ in x]) for x in zip(*(_params(s, 3, 2) for s in range(N_))))
    B = np.random.RandomState(1).normal(0, 1, (A_, 3))
    d = resolve_disturbance(B, amp, freq / TS, phase, 10 ** 9, None, N_, A_, TS, None, None)
    for i in (0, 1, 63):
        tau = 10 ** 9 + i + 1
        lines = [D.exact_phase_lines(d["amp"][e], d["freq"][e], d["phase"][e], tau) for e in range(N_)]
        want = np.stack([l.sum(axis=1) @ B.T for l in lines])
        tol = np.stack([D.line_tolerance(d["amp"][e], d["freq"][e], d["phase"][e], tau).sum(axis=1) @ np.abs(B).T for e in range(N_)])
        got = disturbance_value(d, i)
        assert got.shape == (N_, A_) and got.dtype == np.float64
        assert (np.abs(got - want) <= tol + 3 * 2.0 ** -53 * (np.abs(np.stack([l.sum(axis=1) for l in lines])) @ np.abs(B).T)).all()
    # one rounding of the phase: with a frequency of few bits the product is exact and the plain NumPy formula gives the same bits
    d2 = resolve_disturbance(B, d["amp"], np.full((3, 2), 0.125) / TS, d["phase"], 10 ** 9, None, N_, A_, TS, None, None)
    assert (d2["freq"] == 0.125).all()
    terms = np.stack([D.numpy_lines(d2["amp"][e], d2["freq"][e], d2["phase"][e], 10 ** 9 + 6) for e in range(N_)])
    plain = (terms[..., 0] + terms[..., 1]) @ B.T
    assert np.array_equal(disturbance_value(d2, 5), plain)


@pytest.mark.parametrize("kw, what", [
    (dict(modes=np.zeros((A_ + 1, 2)), amp=np.zeros((2, 1)), freq=np.zeros((2, 1))), "modes must have shape"),
    (dict(modes=np.zeros(A_), amp=np.zeros((1, 1)), freq=np.zeros((1, 1))), "modes must have shape"),
    (dict(modes=0, amp=np.zeros((1, 1)), freq=np.zeros((1, 1))), "columns"),
    (dict(modes=6, amp=np.zeros((6, 1)), freq=np.zeros((6, 1))), "columns"),
    (dict(modes=np.zeros((A_, 65)), amp=np.zeros((65, 1)), freq=np.zeros((65, 1))), "modes outside"),
    (dict(modes=2, amp=np.zeros((2, 9)), freq=np.zeros((2, 9))), "lines outside"),
    (dict(modes=2, amp=np.zeros((2, 0)), freq=np.zeros((2, 0))), "lines outside"),
    (dict(modes=2, amp=np.zeros((3, 2)), freq=np.zeros((3, 2))), "amp must have shape"),
    (dict(modes=2, amp=np.zeros(2), freq=np.zeros(2)), "amp must have shape"),
    (dict(modes=2, amp=np.zeros((3, 2, 2)), freq=np.zeros((2, 2))), "amp must have shape"),
    (dict(modes=2, amp=np.zeros((2, 2)), freq=np.zeros((2, 3))), "freq must have shape"),
    (dict(modes=2, amp=np.zeros((2, 2)), freq=np.zeros((2, 2)), phase=np.zeros((N_, 2, 1))), "phase must have shape"),
    (dict(modes=2, amp=np.zeros((N_, 2, 2)), freq=np.zeros((2, 2)), env_ids=[0, 1]), "amp must have shape"),
    (dict(modes=2, amp=np.full((2, 2), -1e-9), freq=np.zeros((2, 2))), "amp must be >= 0"),
    (dict(modes=2, amp=np.full((2, 2), np.nan), freq=np.zeros((2, 2))), "finite"),
    (dict(modes=2, amp=np.zeros((2, 2)), freq=np.full((2, 2), np.inf)), "finite"),
    (dict(modes=np.full((A_, 2), np.nan), amp=np.zeros((2, 2)), freq=np.zeros((2, 2))), "finite"),
    (dict(modes=None, amp=np.zeros((2, 2)), freq=np.zeros((2, 2))), "modes=None"),
    (dict(modes=None, amp=np.zeros((2, 2)), freq=np.zeros((2, 2)), env_ids=[1]), "modes=None"),
    (dict(modes=2, amp=np.zeros((2, 2)), freq=np.zeros((2, 2)), env_ids=[4]), "outside"),
    (dict(modes=2, amp=np.zeros((2, 2)), freq=np.zeros((2, 2)), env_ids=[1, 1]), "twice"),
    (dict(modes="abc", amp=np.zeros((2, 2)), freq=np.zeros((2, 2))), "numeric"),
])
def test_bad_arguments_raise(kw, what):
    with pytest.raises(ValueError, match=what):
        _resolve(**kw)


def test_env_ids_must_share_the_shape_in_force():
    full = _resolve(2, np.zeros((2, 3)), np.zeros((2, 3)))
    with pytest.raises(ValueError, match="in force"):
        _resolve(2, np.zeros((2, 2)), np.zeros((2, 2)), env_ids=[1], current=full)
    with pytest.raises(ValueError, match="in force"):
        _resolve(3, np.zeros((3, 3)), np.zeros((3, 3)), env_ids=[1], current=full)


# ---- the ABI ------------------------------------------------------------------------------------------------------------
def test_struct_enum_and_export_match_the_header(tmp_path):
    st = L.AoDisturbance
    prog = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', "int main(void){",
            'printf("size %zu\\n", sizeof(AoDisturbance));']
    prog += [f'printf("{f[0]} %zu\\n", offsetof(AoDisturbance, {f[0]}));' for f in st._fields_]
    prog += ['printf("seen %d\\n", (int)AOENV_B_COEFS_SEEN);', 'printf("count %d\\n", (int)AOENV_B_COUNT);',
             'printf("prev %d\\n", (int)AOENV_B_DM_PREV);', "return 0;}"]
    src, exe = tmp_path / "disturb_layout.c", tmp_path / "disturb_layout"
    src.write_text("\n".join(prog))
    subprocess.run(["gcc", "-std=c99", "-o", str(exe), str(src)], check=True)
    out = dict(l.split() for l in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(out["size"]) == C.sizeof(st)
    for f in st._fields_:
        assert int(out[f[0]]) == getattr(st, f[0]).offset, f[0]
    # appended in front of AOENV_B_COUNT: every earlier buffer id keeps its value
    assert int(out["seen"]) == L.B_COEFS_SEEN == int(out["prev"]) + 1 == int(out["count"]) - 1 and L.B_DM_PREV == 12
    hdr = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(r"\baoenv_set_disturbance\s*\(", hdr) and "aoenv_set_disturbance" in L.EXPORTS
    assert "vibrationEnv.py:119-123, 146-167" in open(HEADER).read()


def test_the_library_refuses_a_null_env():
    lib = L.load()
    z = np.zeros(8)
    p = z.ctypes.data_as(C.c_void_p)
    cfg = L.AoDisturbance(n_modes=1, n_lines=1, t0=0, h_modes=p, h_amp=p, h_freq=p, h_phase=p)
    assert lib.aoenv_set_disturbance(None, C.byref(cfg), None) != 0
    assert b"null" in lib.aoenv_last_error()
    assert lib.aoenv_set_disturbance(None, None, None) != 0


class _StubEnv:
    """The batched env's surface as far as the wrappers use it: records what reaches it."""
    output = "torch"
    nActuator = 3
    n_envs = 4
    device = "cpu"
    tdtype = torch.float64

    def __init__(self):
        self.calls = []
        self.param = type("P", (), {"nLoop": 50})()

    def set_disturbance(self, modes, amp, freq, phase=None, t0=0, env_ids=None):
        self.calls.append(("set", modes, t0, env_ids))

    def clear_disturbance(self):
        self.calls.append(("clear",))

    def disturbance(self, i):
        return ("value", i)


@pytest.mark.parametrize("wrap", [TorchWrapper, lambda e: TimeDelayEnv(e, 2), lambda e: HistoryEnv(e, n_history=3, delay=2)])
def test_wrappers_reach_the_disturbance(wrap):
    inner = _StubEnv()
    env = wrap(inner)
    env.set_disturbance(2, [[1e-7]], [[10.0]], t0=3, env_ids=[1])
    env.clear_disturbance()
    assert inner.calls == [("set", 2, 3, [1]), ("clear",)] and env.disturbance(5) == ("value", 5)
