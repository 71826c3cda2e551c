"""CPU: the host side of the modal control surface (aoenv_set_modal / BatchedAOEnv.set_modal, step_modal, run_integrator_modal).
The model (rlao_amd/csrc/modal.hpp, ONE host/device source for modal_kernels.hip and the driver tests/native/modal_driver.cpp)
against NumPy and exact integer arithmetic, the argument handling of the Python layer, the ABI that goes with it and the refusals
that need no device.  No GPU."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import _modal_ref as R
from rlao_amd import _lib as L
from rlao_amd.env import BatchedAOEnv, resolve_modal, resolve_modal_gain
from rlao_amd.wrappers import TimeDelayEnv, TorchWrapper

HEADER = os.path.join(R.REPO, "include", "aoenv.h")
SEED = 20261019                                                     # the committed seed of the expansion cases
SHAPES = [(1, 7), (2, 13), (5, 61), (50, 357)]                      # (K, A): A no multiple of 4


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = R.build_driver(tmp_path_factory.mktemp("modal"))
    if exe is None:
        pytest.skip("hipcc not available")
    return exe


def _basis(K, A, E=4):
    rng = np.random.RandomState(SEED + 1000 * K + A)
    return rng.normal(0.0, 1.0, (A, K)), rng.normal(0.0, 0.3, (E, K))


@pytest.mark.parametrize("K,A", SHAPES)
def test_expansion_is_the_fma_chain(driver, K, A):
    """float32: bit-exact against the chain emulated in NumPy (product and sum in float64, one more rounding to float32).  The
    emulation rounds twice where the fma rounds once; the chain in exact integer arithmetic with ONE rounding per step counts
    how often that matters for the committed seed: never.  Both are close to the plain float64 product."""
    m2c, a = _basis(K, A)
    v, _ = R.host_expand(driver, "f32", m2c, a)
    assert v.shape == (4, A) and v.dtype == np.float32
    emu = R.emulated_expand_f32(m2c, a)
    exact = R.exact_expand("f32", m2c, a)
    double_rounded = int((emu != exact).sum())
    print(f"K={K} A={A}: {double_rounded} of {emu.size} values double-rounded by the float64 emulation")
    assert double_rounded == 0
    assert np.array_equal(v, emu) and np.array_equal(v, exact)
    m32, a32 = m2c.astype(np.float32).astype(np.float64), a.astype(np.float32).astype(np.float64)
    assert (np.abs(v - a32 @ m32.T) <= K * 2.0 ** -24 * (np.abs(a32) @ np.abs(m32).T)).all()
    assert np.abs(v).max() > 0.1


@pytest.mark.parametrize("K,A", SHAPES[:3])
def test_expansion_in_float64(driver, K, A):
    """float64 has no wider NumPy type to emulate in: the exact chain with one rounding per step is the checker."""
    m2c, a = _basis(K, A)
    v, _ = R.host_expand(driver, "f64", m2c, a)
    assert v.dtype == np.float64 and np.array_equal(v, R.exact_expand("f64", m2c, a))
    assert (np.abs(v - a @ m2c.T) <= K * 2.0 ** -53 * (np.abs(a) @ np.abs(m2c).T)).all()


@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_integrator_action_is_one_multiply(driver, dtype):
    """a = g * o_prev in the env dtype, then the same chain: the bits a caller gets who forms g * o in a tensor of that dtype"""
    m2c, o = _basis(5, 61)
    g = np.random.RandomState(3).uniform(0.0, 1.0, (4, 5))
    g[2] = 0.0                                                      # an env that runs open loop
    t = R.DT[dtype]
    v, _ = R.host_expand(driver, dtype, m2c, o, gain=g)
    want, _ = R.host_expand(driver, dtype, m2c, g.astype(t) * o.astype(t))
    assert np.array_equal(v, want) and (v[2] == 0).all() and np.abs(v[0]).max() > 0


@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("K,S", [(1, 1), (5, 63), (20, 88), (3, 200), (70, 130)])
def test_projection_order_is_the_stated_one(driver, dtype, K, S):
    """The driver (modal.hpp on the host) against the order restated in Python without the header -- lane-strided fma chains with
    one rounding each, then the tree; the reward likewise in float64 -- bit for bit: this is the checker the GPU test holds
    k_modal_obs to.  The values are within the summation bound of the float64 product.  S below 64, above it and no multiple of
    it; K = 70: lanes of the reward sum with two terms."""
    rng = np.random.RandomState(SEED + K + S)
    cm, sig = rng.normal(0.0, 1.0, (K, S)), rng.normal(0.0, 1e-7, (3, S))
    o, r, _ = R.host_project(driver, dtype, cm, sig)
    want_o, want_r = R.exact_project(dtype, cm, sig)
    assert o.dtype == R.DT[dtype] and np.array_equal(o, want_o) and np.array_equal(r, want_r)
    t = R.DT[dtype]
    cm_t, sig_t = cm.astype(t).astype(np.float64), sig.astype(t).astype(np.float64)
    assert (np.abs(o - (-1e6 * sig_t @ cm_t.T)) <= R.projection_bound(dtype, cm_t, sig_t)).all()
    assert (r < 0).all() and np.abs(o).max() > 1e-3
    if S > 64:                                                      # the order matters: the plain NumPy sum has other last bits somewhere
        plain = (t(-1e6) * (sig.astype(t) @ cm.astype(t).T)).astype(t)
        print(f"{dtype} K={K} S={S}: {int((plain != o).sum())} of {o.size} values differ from NumPy's own order")


def test_the_device_loops_refuse_an_observation_of_the_other_surface():
    """run_integrator / the rollouts after a modal step, run_integrator_modal after a zonal one: refused with a message instead of
    going on from an old observation (no GPU: the check is in front of the library call)."""
    env = BatchedAOEnv.__new__(BatchedAOEnv)
    env._modal, env._modal_gain, env._mobs = {"m2c": np.zeros((7, 3)), "cm": np.zeros((3, 10))}, np.zeros(3), torch.zeros((2, 3))
    env._surface = "modal"
    with pytest.raises(L.AoEnvError, match=r"run_integrator: the last observation is modal; .*reset_soft\(\)"):
        env.run_integrator(0, 1, gain=0.5)
    env._surface = "zonal"
    with pytest.raises(L.AoEnvError, match=r"run_integrator_modal: the last observation is zonal; .*reset_soft_modal\(\)"):
        env.run_integrator_modal(0, 1)


def test_driver_is_clean_under_asan_and_ubsan(tmp_path):
    """The host instantiation of modal.hpp in a stand-alone sanitized program: no report, and the same values."""
    exe = R.build_driver(tmp_path, sanitize=True)
    if exe is None:
        pytest.skip("hipcc not available")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    m2c, a = _basis(5, 61)
    for dtype in ("f32", "f64"):
        v, err = R.host_expand(exe, dtype, m2c, a, env=env)
        assert "ERROR: AddressSanitizer" not in err and "runtime error" not in err, err
        assert np.array_equal(v, R.exact_expand(dtype, m2c, a))
        v, err = R.host_expand(exe, dtype, m2c, a, gain=np.full((4, 5), 0.5), env=env)
        assert "ERROR: AddressSanitizer" not in err and "runtime error" not in err, err
        cm, sig = np.random.RandomState(1).normal(0, 1, (5, 67)), np.random.RandomState(2).normal(0, 1e-7, (3, 67))
        o, r, err = R.host_project(exe, dtype, cm, sig, env=env)
        assert "ERROR: AddressSanitizer" not in err and "runtime error" not in err, err
        assert np.isfinite(o).all() and np.isfinite(r).all()


# ---- BatchedAOEnv.set_modal / set_modal_gain: the arguments ----------------------------------------------------------------
A_, N_, S_ = 7, 4, 10
M2C = np.arange(A_ * 5, dtype=np.float64).reshape(A_, 5) / 10.0 + np.eye(A_, 5)
IMAT = np.random.RandomState(7).normal(0.0, 1.0, (S_, A_))


def test_default_basis_is_m2c_cl_and_the_modal_command_matrix():
    from rlao_amd import calib
    d = resolve_modal(None, None, None, A_, S_, M2C, IMAT)
    assert d["m2c"].shape == (A_, 5) and np.array_equal(d["m2c"], M2C) and d["m2c"].flags["C_CONTIGUOUS"]
    assert d["cm"].shape == (5, S_) and d["cm"].dtype == np.float64 and d["cm"].flags["C_CONTIGUOUS"]
    assert np.array_equal(d["cm"], calib.reconstructor_from_imat(IMAT, M2C, True)[2])
    d2 = resolve_modal(2, None, None, A_, S_, M2C, IMAT)              # the reference's calib_tt: the command matrix of D @ M2C[:, :2]
    assert np.array_equal(d2["m2c"], M2C[:, :2]) and np.array_equal(d2["cm"], calib.reconstructor_from_imat(IMAT, M2C[:, :2], True)[2])
    np.testing.assert_allclose(d2["cm"] @ (IMAT @ M2C[:, :2]), np.eye(2), atol=1e-9)
    assert d2["m2c"] is not M2C and not np.shares_memory(d2["m2c"], M2C)


def test_explicit_tables_and_tensors():
    B, cm = np.random.RandomState(11).normal(0.0, 1.0, (A_, 3)), np.linspace(0, 1, 3 * S_).reshape(3, S_)
    d = resolve_modal(None, torch.tensor(B), torch.tensor(cm), A_, S_)
    assert np.array_equal(d["m2c"], B) and np.array_equal(d["cm"], cm)
    d = resolve_modal(2, B, cm[:2], A_, S_)                          # n_modes cuts the columns
    assert np.array_equal(d["m2c"], B[:, :2]) and d["cm"].shape == (2, S_)
    d = resolve_modal(np.int64(3), B, None, A_, S_, imat=IMAT)        # cm from the interaction matrix for a foreign basis
    np.testing.assert_allclose(d["cm"] @ (IMAT @ B), np.eye(3), atol=1e-9)


@pytest.mark.parametrize("args, what", [
    ((0, None, None), "outside"),
    ((6, None, None), "outside"),
    ((2.0, None, None), "n_modes must be an int"),
    ((True, None, None), "n_modes must be an int"),
    ((None, np.zeros((A_ + 1, 2)), None), "m2c must have shape"),
    ((None, np.zeros(A_), None), "m2c must have shape"),
    ((None, np.zeros((A_, A_ + 1)), np.zeros((A_ + 1, S_))), "outside"),
    ((2, None, np.zeros((3, S_))), "cm must have shape"),
    ((2, None, np.zeros((2, S_ + 1))), "cm must have shape"),
    ((2, np.full((A_, 2), np.nan), np.zeros((2, S_))), "finite"),
    ((2, None, np.full((2, S_), np.inf)), "finite"),
    ((None, "abc", None), "numeric"),
])
def test_bad_bases_raise(args, what):
    with pytest.raises(ValueError, match=what):
        resolve_modal(*args, A_, S_, M2C, IMAT)


def test_a_basis_needs_its_sources():
    with pytest.raises(ValueError, match="M2C_CL"):
        resolve_modal(2, None, None, A_, S_, None, IMAT)
    with pytest.raises(ValueError, match="interaction matrix"):
        resolve_modal(2, M2C, None, A_, S_, None, None)


def test_gains_shared_per_env_and_by_env_ids():
    g, per = resolve_modal_gain(0.4, None, N_, 3)
    assert not per and g.shape == (3,) and (g == 0.4).all() and g.dtype == np.float64
    g, per = resolve_modal_gain([0.1, 0.2, 0.3], None, N_, 3)
    assert not per and np.array_equal(g, [0.1, 0.2, 0.3])
    rows = np.arange(N_ * 3, dtype=np.float64).reshape(N_, 3) / 20.0
    g, per = resolve_modal_gain(torch.tensor(rows), None, N_, 3)
    assert per and np.array_equal(g, rows) and g.flags["C_CONTIGUOUS"] and not np.shares_memory(g, rows)
    g, per = resolve_modal_gain([[0.5, 0.5, 0.5], [0.25, 0.0, 1.0]], [3, 1], N_, 3)       # none in force: the others run open loop
    assert per and (g[[0, 2]] == 0).all() and (g[3] == 0.5).all() and np.array_equal(g[1], [0.25, 0.0, 1.0])
    g2, per = resolve_modal_gain(0.7, np.array([True, False, False, False]), N_, 3, current=g)
    assert per and (g2[0] == 0.7).all() and np.array_equal(g2[1:], g[1:]) and g[0, 0] == 0.0
    g3, _ = resolve_modal_gain([0.1, 0.2, 0.3], [2], N_, 3, current=np.broadcast_to(np.array([0.4, 0.4, 0.4]), (N_, 3)))
    assert np.array_equal(g3[2], [0.1, 0.2, 0.3]) and (g3[[0, 1, 3]] == 0.4).all()


@pytest.mark.parametrize("kw, what", [
    (dict(g=[0.1, 0.2]), "gains must be a scalar or have shape"),
    (dict(g=np.zeros((N_ + 1, 3))), "gains must be a scalar or have shape"),
    (dict(g=np.zeros((2, 2, 3))), "gains must be a scalar or have shape"),
    (dict(g=np.zeros((N_, 3)), env_ids=[0, 1]), "gains must be a scalar or have shape"),
    (dict(g=-0.1), "gains must be >= 0"),
    (dict(g=[0.1, np.nan, 0.2]), "finite"),
    (dict(g=np.inf), "finite"),
    (dict(g="abc"), "numeric"),
    (dict(g=0.5, env_ids=[4]), "outside"),
    (dict(g=0.5, env_ids=[1, 1]), "twice"),
    (dict(g=0.5, env_ids=[1], current=np.zeros((N_, 2))), "in force"),
])
def test_bad_gains_raise(kw, what):
    with pytest.raises(ValueError, match=what):
        resolve_modal_gain(kw["g"], kw.get("env_ids"), N_, 3, kw.get("current"))


def test_an_env_without_a_basis_refuses_the_modal_calls():
    """Before set_modal every modal call fails with a message, without touching the library (no GPU needed: no shard exists)."""
    env = BatchedAOEnv.__new__(BatchedAOEnv)                        # (the constructor wants a device)
    env._modal = env._modal_gain = env._mobs = None
    assert env.n_modal == 0
    for call in (lambda: env.step_modal(0, np.zeros((2, 3))), env.reset_soft_modal, lambda: env.run_integrator_modal(0, 1),
                 lambda: env.set_modal_gain(0.5)):
        with pytest.raises(L.AoEnvError, match="set_modal"):
            call()
    env._modal = {"m2c": np.zeros((7, 3)), "cm": np.zeros((3, 10))}
    assert env.n_modal == 3
    with pytest.raises(L.AoEnvError, match="set_modal_gain"):
        env.run_integrator_modal(0, 1)


# ---- the ABI --------------------------------------------------------------------------------------------------------------
NEW = ("aoenv_set_modal", "aoenv_set_modal_gain", "aoenv_reset_soft_modal", "aoenv_step_modal", "aoenv_run_integrator_modal")


def test_struct_enums_and_exports_match_the_header(tmp_path):
    st = L.AoModal
    prog = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', "int main(void){",
            'printf("size %zu\\n", sizeof(AoModal));']
    prog += [f'printf("{f[0]} %zu\\n", offsetof(AoModal, {f[0]}));' for f in st._fields_]
    prog += ['printf("abi %d\\n", (int)AOENV_ABI_VERSION);', 'printf("bufs %d\\n", (int)AOENV_B_COUNT);',
             'printf("kernels %d\\n", (int)AOENV_K_COUNT);', 'printf("gemm %d\\n", (int)AOENV_PATH_MODAL_GEMM);',
             'printf("rr %d\\n", (int)AOENV_PATH_PYR_ROUND_ROBIN);', "return 0;}"]
    src, exe = tmp_path / "modal_layout.c", tmp_path / "modal_layout"
    src.write_text("\n".join(prog))
    subprocess.run(["gcc", "-std=c99", "-o", str(exe), str(src)], check=True)
    out = dict(l.split() for l in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(out["size"]) == C.sizeof(st)
    for f in st._fields_:
        assert int(out[f[0]]) == getattr(st, f[0]).offset, f[0]
    # purely additive: the version, the buffer ids and the profiled kernels are what they were
    assert int(out["abi"]) == L.ABI_VERSION == 7 and int(out["bufs"]) == 14 and int(out["kernels"]) == 13 == len(L.KERNEL_NAMES)
    assert int(out["gemm"]) == L.PATH_MODAL_GEMM == 2048 and int(out["rr"]) == L.PATH_PYR_ROUND_ROBIN == 1024
    hdr = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name in NEW:
        assert re.search(rf"\b{name}\s*\(", hdr) and name in L.EXPORTS, name
    text = open(HEADER).read()
    assert "modalAOEnv.py:150-157" in text and "stay zonal" in text


def test_the_library_refuses_a_null_env():
    lib = L.load()
    z = np.zeros(8)
    p = z.ctypes.data_as(C.c_void_p)
    cfg = L.AoModal(n_modes=1, h_m2c=p, h_cm=p)
    for rc in (lib.aoenv_set_modal(None, C.byref(cfg), None), lib.aoenv_set_modal(None, None, None),
               lib.aoenv_set_modal_gain(None, p, 0, None), lib.aoenv_reset_soft_modal(None, p, None),
               lib.aoenv_step_modal(None, 0, p, p, None, None, None, None), lib.aoenv_run_integrator_modal(None, 0, 1, p, None, None, None, None)):
        assert rc != 0 and b"null" in lib.aoenv_last_error()


# ---- the wrappers -----------------------------------------------------------------------------------------------------------
class _StubEnv:
    """The batched env's surface as far as the wrappers use it: records what reaches it."""
    output = "torch"
    nActuator = 3
    n_envs = 4
    device = "cpu"
    tdtype = torch.float64

    def __init__(self):
        self.calls = []

    def set_modal(self, n_modes=None, m2c=None, cm=None):
        self.calls.append(("set", n_modes))

    def set_modal_gain(self, g, env_ids=None):
        self.calls.append(("gain", g, env_ids))

    def reset_soft_modal(self):
        return torch.ones((4, 2), dtype=torch.float64)

    def step_modal(self, i, action):
        self.calls.append(("step", i))
        s = torch.full((4,), 0.5, dtype=torch.float64)
        return action * 2, None, s, s, torch.zeros(4, dtype=torch.bool), {"strehl": s}

    def run_integrator_modal(self, i0, n_steps):
        return tuple(torch.zeros(4, dtype=torch.float64) for _ in range(3))


def test_torch_wrapper_forwards_the_modal_surface():
    inner = _StubEnv()
    env = TorchWrapper(inner)
    env.set_modal(2)
    env.set_modal_gain(0.3, env_ids=[1])
    assert inner.calls == [("set", 2), ("gain", 0.3, [1])]
    assert env.reset_soft_modal().dtype == torch.float32
    obs, _, _, _, _, info = env.step_modal(3, torch.ones((4, 2), dtype=torch.float64))
    assert obs.dtype == torch.float32 and (obs == 2).all() and info[0][0] == "strehl" and inner.calls[-1] == ("step", 3)
    assert all(t.dtype == torch.float32 for t in env.run_integrator_modal(0, 2))


def test_time_delay_env_refuses_the_modal_step():
    env = TimeDelayEnv(_StubEnv(), 2)
    with pytest.raises(NotImplementedError, match="set_delay"):
        env.step_modal(0, torch.zeros((4, 2)))
    with pytest.raises(NotImplementedError, match="set_delay"):
        env.run_integrator_modal(0, 1)
    env.set_modal(2)                                                # configuration still reaches the env
    assert env._env.calls == [("set", 2)]
