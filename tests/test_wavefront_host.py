"""CPU: the host side of the wavefront read-out (aoenv_set_wavefront_basis / aoenv_project_wavefront / aoenv_set_wavefront_record;
BatchedAOEnv.set_wavefront_basis, project_wavefront, record_wavefront).  The model (rlao_amd/csrc/wavefront.hpp, ONE host/device
source for wavefront_kernels.hip, env.hip and the driver tests/native/wavefront_driver.cpp) against its restatement in NumPy
(tests/_wavefront_ref.py): the scatter of [K][P] into the padded full-grid table, the slice plan, every refusal of the validation and
the general kernel's order of the sum; the argument handling of the Python layer, the ABI that goes with it and the wrappers.
No GPU."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import _wavefront_ref as W
from rlao_amd import _lib as L
from rlao_amd.env import BatchedAOEnv, resolve_wavefront_basis, wavefront_bits
from rlao_amd.wrappers import HistoryEnv, TimeDelayEnv, TorchWrapper

HEADER = os.path.join(W.REPO, "include", "aoenv.h")
SEED = 20261020
GEOMETRIES = [24, 30, 35]                                           # R: R^2 = 576; 900 (a multiple of 4, not of 16); 1225 (odd)
MODES = [1, 16, 17]


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = W.build_driver(tmp_path_factory.mktemp("wavefront"))
    if exe is None:
        pytest.skip("hipcc not available")
    return exe


def _case(R, K):
    pupil = W.disc_pupil(R, 0.2)
    P = int(pupil.sum())
    opd2m = np.random.RandomState(SEED + 100 * R + K).normal(0.0, 1.0, (K, P))
    return pupil, P, opd2m


@pytest.mark.parametrize("K", MODES)
@pytest.mark.parametrize("R", GEOMETRIES)
def test_slice_plan(driver, R, K):
    """The slices cover [0, R^2) once, in order, every one but the last a multiple of 16 long and at least 4 K (the slabs move
    at most a quarter of what X does) unless one slice is all there is; the plan is the NumPy restatement's, and nothing but
    (R^2, K) goes into it -- the driver is not even told a number of envs."""
    r2 = R * R
    n, length, stride, bounds = W.host_plan(driver, r2, K)
    assert (n, length, bounds) == W.plan(r2, K)
    assert stride == W.row_stride(r2) and stride % 4 == 0 and r2 <= stride < r2 + 4
    assert len(bounds) == n and 1 <= n <= W.MAX_SLICES and length % W.ROUND == 0
    assert bounds[0][0] == 0 and bounds[-1][1] == r2
    for (lo, hi), (lo2, _) in zip(bounds, bounds[1:]):
        assert hi == lo2 and hi - lo == length
    assert all(lo < hi for lo, hi in bounds)
    assert n == 1 or length >= 4 * K
    covered = np.zeros(r2, dtype=int)
    for lo, hi in bounds:
        covered[lo:hi] += 1
    assert (covered == 1).all()
    if r2 % 4 == 0:                                                 # 16-byte loads: no slice ends inside a quad
        assert all(lo % 4 == 0 and hi % 4 == 0 for lo, hi in bounds)


def test_plan_and_sum_do_not_depend_on_the_shard(driver):
    """The plan is a function of (R^2, K): the driver's `plan` takes nothing else.  And the model's sum of one env is the same bits
    alone and as row 3 of 5 (the device side of this property is the batch-position test of tests/test_gpu_wavefront.py)."""
    assert W.host_plan(driver, 14400, 30)[:2] == W.plan(14400, 30)[:2] == (60, 240)      # 14400 / 64 = 225 -> 240
    pupil, P, opd2m = _case(30, 17)
    table = W.scatter("f32", opd2m, pupil)
    x = np.random.RandomState(SEED).normal(0.0, 1.0, (5, 900))
    alone, _, _ = W.host_project(driver, "f32", table, x[3:4], 1e-7)
    among, _, _ = W.host_project(driver, "f32", table, x, 1e-7)
    assert np.array_equal(alone[0], among[3]) and not np.array_equal(among[2], among[3])


@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("K", MODES)
@pytest.mark.parametrize("R", GEOMETRIES)
def test_scatter_into_the_padded_grid(driver, dtype, R, K):
    pupil, P, opd2m = _case(R, K)
    got, _ = W.host_scatter(driver, dtype, opd2m, pupil)
    want = W.scatter(dtype, opd2m, pupil)
    assert got.dtype == W.DT[dtype] and got.shape == (K, W.row_stride(R * R)) and np.array_equal(got, want)
    flat = pupil.ravel()
    assert (got[:, R * R:] == 0).all()                              # the pad
    assert (got[:, :R * R][:, ~flat] == 0).all()                    # every column that is no pupil pixel
    assert np.array_equal(got[:, :R * R][:, flat], opd2m.astype(W.DT[dtype]))   # pixel p = the p-th of np.where(pupil)
    assert np.array_equal(np.where(flat)[0], np.ravel_multi_index(np.where(pupil), pupil.shape))


@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_every_refusal(driver, dtype):
    pupil, P, opd2m = _case(24, 3)
    ok = lambda *a, **kw: W.host_validate(driver, dtype, *a, **kw)[0]
    assert ok(3, P, pupil, opd2m) == W.OK == W.validate(dtype, 3, P, pupil, opd2m)
    big = np.zeros((P + 1, P))
    cases = [
        ((0, P, pupil, np.zeros((0, P))), {}, W.BAD_MODES),
        ((P + 1, P, pupil, big), {}, W.BAD_MODES),
        ((3, 0, pupil, np.zeros((3, 0))), {}, W.BAD_PIX),
        ((3, -1, pupil, np.zeros((3, 0))), {}, W.BAD_PIX),
        ((3, P - 1, pupil, opd2m[:, :P - 1]), {}, W.PUPIL_COUNT),
        ((3, P + 1, pupil, np.zeros((3, P + 1))), {}, W.PUPIL_COUNT),
        ((3, P, pupil, opd2m), {"case": "nopupil"}, W.NO_PUPIL),
        ((3, P, pupil, opd2m), {"case": "nulltable"}, W.NULL_TABLE),
    ]
    for bad in (np.nan, np.inf, -np.inf):
        t = opd2m.copy()
        t[2, P - 1] = bad
        cases.append(((3, P, pupil, t), {}, W.NOT_FINITE))
    for args, kw, want in cases:
        assert ok(*args, **kw) == want, (args[:2], kw)
        ref_pupil = None if kw.get("case") == "nopupil" else args[2]
        ref_table = None if kw.get("case") == "nulltable" else args[3]
        assert W.validate(dtype, args[0], args[1], ref_pupil, ref_table) == want
    # K above AOENV_MAX_WF_MODES on a pupil that has the pixels for it
    wide = W.disc_pupil(40)
    Pw = int(wide.sum())
    assert Pw > W.MAX_MODES
    assert ok(W.MAX_MODES + 1, Pw, wide, np.zeros((W.MAX_MODES + 1, Pw))) == W.BAD_MODES
    assert ok(W.MAX_MODES, Pw, wide, np.zeros((W.MAX_MODES, Pw))) == W.OK
    # a float64 beyond float32's range is not finite in a float32 shard
    t = opd2m.copy()
    t[0, 0] = 1e39
    assert ok(3, P, pupil, t) == (W.NOT_FINITE if dtype == "f32" else W.OK) == W.validate(dtype, 3, P, pupil, t)


@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("R,K", [(24, 1), (30, 3), (35, 2)])
def test_general_order_is_the_stated_one(driver, dtype, R, K):
    """The driver (wavefront.hpp on the host, what k_wf_project + k_wf_finish compute) against the order restated in Python: bit for
    bit.  Both are within the bound of any order of the float64 product."""
    pupil, P, opd2m = _case(R, K)
    table = W.scatter(dtype, opd2m, pupil)
    x = np.random.RandomState(SEED + R).normal(0.0, 1.0, (2, R * R))
    s = 0.79e-6 / (2 * np.pi)
    scaled, plain, _ = W.host_project(driver, dtype, table, x, s)
    assert np.array_equal(plain, W.exact_project(dtype, table, x)) and np.array_equal(scaled, W.exact_project(dtype, table, x, s))
    t = W.DT[dtype]
    x_t = x.astype(t).astype(np.float64)
    c64 = x_t[:, pupil.ravel()] @ opd2m.astype(t).astype(np.float64).T
    assert (np.abs(plain - c64) <= W.projection_bound(dtype, table, x_t)).all()
    assert (np.abs(scaled - float(t(s)) * c64) <= W.projection_bound(dtype, table, x_t, s)).all()
    assert np.abs(plain).max() > 1.0


def test_integer_data_is_exact(driver):
    """|x| <= 8, |p| <= 8 integers: every partial sum is an integer below 2^24, so float32 gives the integer product whatever the
    order -- the data of the GPU layout test"""
    R, K = 35, 17
    pupil = W.disc_pupil(R)
    P = int(pupil.sum())
    rng = np.random.RandomState(SEED)
    opd2m, x = rng.randint(-8, 9, (K, P)).astype(np.float64), rng.randint(-8, 9, (3, R * R)).astype(np.float64)
    table = W.scatter("f32", opd2m, pupil)
    scaled, plain, _ = W.host_project(driver, "f32", table, x, 1.5)
    want = x[:, pupil.ravel()] @ opd2m.T
    assert np.array_equal(plain.astype(np.float64), want) and np.array_equal(scaled, (want * 1.5).astype(np.float32))


def test_driver_is_clean_under_asan_and_ubsan(tmp_path):
    """The host instantiation of wavefront.hpp in a stand-alone sanitized program: no report, and the same values -- on the odd
    geometry (a pad of 3 elements behind every row) and through every refusal."""
    exe = W.build_driver(tmp_path, sanitize=True)
    if exe is None:
        pytest.skip("hipcc not available")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    clean = lambda err: "ERROR: AddressSanitizer" not in err and "runtime error" not in err
    pupil, P, opd2m = _case(35, 17)
    for dtype in ("f32", "f64"):
        table, err = W.host_scatter(exe, dtype, opd2m, pupil, env=env)
        assert clean(err), err
        assert np.array_equal(table, W.scatter(dtype, opd2m, pupil))
        x = np.random.RandomState(1).normal(0, 1, (2, 35 * 35))
        scaled, plain, err = W.host_project(exe, dtype, table, x, 1e-7, env=env)
        assert clean(err), err
        assert np.isfinite(scaled).all() and np.abs(plain).max() > 0
        bad = opd2m.copy()
        bad[16, P - 1] = np.nan
        for args, case in (((17, P, pupil, opd2m), "table"), ((17, P, pupil, bad), "table"), ((17, P - 1, pupil, opd2m[:, :P - 1]), "table"),
                           ((0, P, pupil, np.zeros((0, P))), "table"), ((17, P, pupil, opd2m), "nopupil"), ((17, P, pupil, opd2m), "nulltable")):
            rc, err = W.host_validate(exe, dtype, *args, case=case, env=env)
            assert clean(err), err
            assert rc in range(7)


# ---- the ABI --------------------------------------------------------------------------------------------------------------
NEW = ("aoenv_set_wavefront_basis", "aoenv_project_wavefront", "aoenv_set_wavefront_record")


def test_struct_enums_and_exports_match_the_header(tmp_path):
    st = L.AoWavefrontBasis
    prog = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', "int main(void){",
            'printf("size %zu\\n", sizeof(AoWavefrontBasis));']
    prog += [f'printf("{f[0]} %zu\\n", offsetof(AoWavefrontBasis, {f[0]}));' for f in st._fields_]
    prog += ['printf("abi %d\\n", (int)AOENV_ABI_VERSION);', 'printf("bufs %d\\n", (int)AOENV_B_COUNT);',
             'printf("kernels %d\\n", (int)AOENV_K_COUNT);', 'printf("general %d\\n", (int)AOENV_PATH_WF_GENERAL);',
             'printf("res %d\\n", (int)AOENV_WF_RESIDUAL);', 'printf("atm %d\\n", (int)AOENV_WF_ATMOSPHERE);',
             'printf("max %d\\n", (int)AOENV_MAX_WF_MODES);', "return 0;}"]
    src, exe = tmp_path / "wf_layout.c", tmp_path / "wf_layout"
    src.write_text("\n".join(prog))
    subprocess.run(["gcc", "-std=c99", "-o", str(exe), str(src)], check=True)
    out = dict(l.split() for l in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(out["size"]) == C.sizeof(st)
    for f in st._fields_:
        assert int(out[f[0]]) == getattr(st, f[0]).offset, f[0]
    # purely additive: the version, the buffer ids and the profiled kernels are what they were
    assert int(out["abi"]) == L.ABI_VERSION == 7 and int(out["bufs"]) == 14 and int(out["kernels"]) == 13 == len(L.KERNEL_NAMES)
    assert int(out["general"]) == L.PATH_WF_GENERAL == 8192
    assert int(out["res"]) == L.WF_RESIDUAL == 1 and int(out["atm"]) == L.WF_ATMOSPHERE == 2
    assert int(out["max"]) == L.MAX_WF_MODES == W.MAX_MODES == 1024
    hdr = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name in NEW:
        assert re.search(rf"\b{name}\s*\(", hdr) and name in L.EXPORTS, name
    text = open(HEADER).read()
    assert "SinEnv.py:150-204" in text and "EOF_POL.py:105-123" in text and "make_dataset.py:84-103" in text and "zernike_dist" in text


def test_the_library_refuses_a_null_env():
    lib = L.load()
    z = np.zeros(8)
    p = z.ctypes.data_as(C.c_void_p)
    cfg = L.AoWavefrontBasis(n_modes=1, n_pix=8, h_opd2m=p)
    for rc in (lib.aoenv_set_wavefront_basis(None, C.byref(cfg), None), lib.aoenv_set_wavefront_basis(None, None, None),
               lib.aoenv_project_wavefront(None, L.WF_RESIDUAL, p, None), lib.aoenv_set_wavefront_record(None, L.WF_RESIDUAL, p, 0, 1),
               lib.aoenv_set_wavefront_record(None, 0, None, 0, 0)):
        assert rc != 0 and b"null" in lib.aoenv_last_error()


# ---- BatchedAOEnv.set_wavefront_basis: the arguments ------------------------------------------------------------------------
P_ = 12
M2OPD = np.random.RandomState(5).normal(0.0, 1.0, (P_, 5))


def test_m2opd_is_inverted_on_its_first_columns():
    t = resolve_wavefront_basis(M2OPD, None, 3, P_)
    assert t.shape == (3, P_) and t.dtype == np.float64 and t.flags["C_CONTIGUOUS"]
    assert np.array_equal(t, np.linalg.pinv(M2OPD[:, :3]))          # the reference's opd2m = pinv(M2OPD), in float64
    np.testing.assert_allclose(t @ M2OPD[:, :3], np.eye(3), atol=1e-12)
    assert resolve_wavefront_basis(torch.tensor(M2OPD), None, None, P_).shape == (5, P_)


def test_opd2m_is_taken_as_given():
    given = np.arange(4 * P_, dtype=np.float64).reshape(4, P_)
    t = resolve_wavefront_basis(None, given, None, P_)
    assert np.array_equal(t, given) and not np.shares_memory(t, given)
    assert np.array_equal(resolve_wavefront_basis(None, given, np.int64(2), P_), given[:2])


@pytest.mark.parametrize("kw, what", [
    (dict(), "exactly one"),
    (dict(m2opd=M2OPD, opd2m=M2OPD.T), "exactly one"),
    (dict(m2opd=M2OPD[:-1]), "m2opd must have shape"),
    (dict(m2opd=M2OPD[:, 0]), "finite 2-d"),
    (dict(opd2m=M2OPD), "opd2m must have shape"),
    (dict(m2opd=M2OPD, n_modes=0), "outside"),
    (dict(m2opd=M2OPD, n_modes=6), "outside"),
    (dict(opd2m=np.zeros((P_ + 1, P_))), "outside"),
    (dict(m2opd=M2OPD, n_modes=2.0), "n_modes must be an int"),
    (dict(m2opd=M2OPD, n_modes=True), "n_modes must be an int"),
    (dict(m2opd=np.full((P_, 2), np.nan)), "finite"),
    (dict(opd2m=np.full((2, P_), np.inf)), "finite"),
    (dict(m2opd="abc"), "numeric"),
])
def test_bad_bases_raise(kw, what):
    with pytest.raises(ValueError, match=what):
        resolve_wavefront_basis(kw.get("m2opd"), kw.get("opd2m"), kw.get("n_modes"), P_)


def test_what_names_bits():
    assert wavefront_bits("residual") == L.WF_RESIDUAL and wavefront_bits(("atmosphere",)) == L.WF_ATMOSPHERE
    assert wavefront_bits(["atmosphere", "residual"]) == 3
    for bad in ("phase", (), ("residual", "residual"), ("residual", "opd")):
        with pytest.raises(ValueError, match="residual"):
            wavefront_bits(bad)


def test_an_env_without_a_basis_refuses_the_calls():
    """Before set_wavefront_basis the read-outs fail with a message, without touching the library (no shard exists)."""
    env = BatchedAOEnv.__new__(BatchedAOEnv)                        # (the constructor wants a device)
    env._wf = env._wf_rec = None
    assert env.n_wavefront_modes == 0
    for call in (env.project_wavefront, lambda: env.record_wavefront(0, 4)):
        with pytest.raises(L.AoEnvError, match="set_wavefront_basis"):
            call()
    env._wf = np.zeros((3, 10))
    assert env.n_wavefront_modes == 3
    with pytest.raises(ValueError, match="one of"):
        env.project_wavefront(("residual", "atmosphere"))
    with pytest.raises(ValueError, match="n_steps >= 1"):
        env.record_wavefront(0, 0)


# ---- the wrappers -----------------------------------------------------------------------------------------------------------
class _StubEnv:
    output = "torch"
    nActuator = 3
    n_envs = 4
    device = "cpu"
    tdtype = torch.float64
    n_wavefront_modes = 2

    def __init__(self):
        self.calls = []

    def set_wavefront_basis(self, m2opd=None, opd2m=None, n_modes=None):
        self.calls.append(("set", n_modes))

    def clear_wavefront_basis(self):
        self.calls.append(("clear",))

    def project_wavefront(self, what="residual"):
        self.calls.append(("project", what))
        return torch.ones((4, 2), dtype=torch.float64)

    def record_wavefront(self, i0, n_steps, what=("residual",)):
        self.calls.append(("record", i0, n_steps, tuple(what)))
        self.rec = torch.zeros((n_steps, len(what), 4, 2), dtype=torch.float64)
        return self.rec

    def stop_wavefront_record(self):
        self.calls.append(("stop",))


def test_torch_wrapper_forwards_everything():
    inner = _StubEnv()
    env = TorchWrapper(inner)
    env.set_wavefront_basis(opd2m=np.zeros((2, 5)), n_modes=2)
    assert env.n_wavefront_modes == 2
    c = env.project_wavefront("atmosphere")
    assert c.dtype == torch.float32 and c.shape == (4, 2)
    rec = env.record_wavefront(3, 5, ("residual", "atmosphere"))
    assert rec is inner.rec                                         # the tensor the library writes, not a converted copy
    env.stop_wavefront_record()
    env.clear_wavefront_basis()
    assert inner.calls == [("set", 2), ("project", "atmosphere"), ("record", 3, 5, ("residual", "atmosphere")), ("stop",), ("clear",)]


@pytest.mark.parametrize("wrap", [lambda e: TimeDelayEnv(e, 2), lambda e: HistoryEnv(e, n_history=3, delay=1)])
def test_delay_and_history_envs_forward_the_basis_and_the_projection(wrap):
    inner = _StubEnv()
    env = wrap(inner)
    for name in ("set_wavefront_basis", "clear_wavefront_basis", "project_wavefront", "n_wavefront_modes"):
        assert name in type(env).__dict__, name                      # a method of the wrapper, not the __getattr__ fall-through
    env.set_wavefront_basis(m2opd=np.zeros((5, 2)), n_modes=1)
    assert env.n_wavefront_modes == 2 and torch.equal(env.project_wavefront(), torch.ones((4, 2), dtype=torch.float64))
    env.clear_wavefront_basis()
    assert inner.calls == [("set", 1), ("project", "residual"), ("clear",)]
