"""CPU: the host side of the per-env DM mis-registration (aoenv_set_dm_env / BatchedAOEnv.set_dm_misregistration).  The factors of
``calib.dm_factors`` against the reference's dense expression restated in tests/_dm_misreg_ref.py, direction and sign of the shifts,
the defaults (bit-identical to the tables of before the feature), the parameter keys, the argument handling of the Python layer on a
stub shard, the ABI, and the table re-layout (rlao_amd/csrc/dm_tables.hpp) in a stand-alone sanitized program.  No GPU."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import _dm_misreg_ref as REF
from rlao_amd import _lib as L
from rlao_amd import calib
from rlao_amd.env import MISREG_KEYS, BatchedAOEnv, resolve_dm_misregistration
from rlao_amd.wrappers import HistoryEnv, TimeDelayEnv, TorchWrapper

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "aoenv.h")

GEOMETRIES = {"R24": dict(diameter=1.6, nSubaperture=4, nPixelPerSubap=6), "R48": dict(diameter=3.2, nSubaperture=8, nPixelPerSubap=6)}


def _sets(p):
    """zero, each parameter alone, all four together -- both signs"""
    pitch = p.diameter / p.nSubaperture
    return {"zero": dict(),
            "shift_x": dict(shift_x=0.3 * pitch), "shift_y": dict(shift_y=-0.5 * pitch),
            "radial": dict(radial_scaling=0.02), "tangential": dict(tangential_scaling=-0.03),
            "all+": dict(shift_x=0.21 * pitch, shift_y=0.4 * pitch, radial_scaling=0.015, tangential_scaling=0.04),
            "all-": dict(shift_x=-0.21 * pitch, shift_y=-0.4 * pitch, radial_scaling=-0.015, tangential_scaling=-0.04)}


@pytest.mark.parametrize("geo", sorted(GEOMETRIES))
def test_factors_against_the_dense_reference_expression(geo):
    """gy[:, iy] (x) gx[:, ix] of calib.dm_factors against G of OOPAO/DeformableMirror.py:497-510 at the positions of :331-346, for
    every valid actuator.  Bound 1e-15 absolute, derived: the values lie in (0, 1] and the absolute rounding error of exp(-t) is
    at most t e^-t <= 0.37 times a few ulp."""
    p = calib.params_from_args(None, **GEOMETRIES[geo])
    dmt = calib.DMTables(p)
    R, nA = p.resolution, dmt.nAct
    worst = 0.0
    for name, kw in _sets(p).items():
        gx, gy = calib.dm_factors(p, **kw)
        assert gx.shape == gy.shape == (R, nA) and gx.dtype == np.float64
        want = REF.dense_influence(R, p.diameter, p.nSubaperture, p.mechanicalCoupling, dmt.act_idx, **kw)
        got = np.stack([np.outer(gy[:, k // nA], gx[:, k % nA]) for k in dmt.act_idx], axis=-1)
        err = float(np.abs(got - want).max())
        worst = max(worst, err)
        print(f"{geo} {name}: max |product - dense| = {err:.3e}")
        assert err <= 1e-15, (name, err)
        assert 0 < got.min() and got.max() <= 1
        # ... and the same through DMTables.dense_modes, which the calibration's modal basis is built from
        t = calib.DMTables(p, **kw)
        assert np.array_equal(t.gx, gx) and np.array_equal(t.gy, gy)
        assert np.abs(t.dense_modes().reshape(R, R, -1) - want).max() <= 1e-15
    # the parameter sets are not all the same mirror
    assert np.abs(calib.dm_factors(p, **_sets(p)["all+"])[0] - dmt.gx).max() > 1e-2


@pytest.mark.parametrize("geo", sorted(GEOMETRIES))
def test_direction_and_sign_of_the_shifts(geo):
    """shift_x = D / (R - 1) is one step of the pixel grid linspace(0, 1, R) R scaled to metres ... a positive shiftX moves the
    surface towards -x (xIF = x - shiftX, :337): gx_shifted[p] == gx_nominal[p + 1]; gy is untouched bit for bit.  Likewise y."""
    p = calib.params_from_args(None, **GEOMETRIES[geo])
    R, D = p.resolution, p.diameter
    gx0, gy0 = calib.dm_factors(p)
    step = D / (R - 1)
    gx, gy = calib.dm_factors(p, shift_x=step)
    assert np.abs(gx[:R - 1] - gx0[1:]).max() <= 1e-15 and np.array_equal(gy, gy0)
    assert np.abs(gx - gx0).max() > 1e-2
    gx, gy = calib.dm_factors(p, shift_y=step)
    assert np.abs(gy[:R - 1] - gy0[1:]).max() <= 1e-15 and np.array_equal(gx, gx0)


def _pre_feature_tables(p, n_subap=None):
    """The expression calib.DMTables held before the feature (gx, gy, dense_modes), kept here as the yardstick of the defaults."""
    R, D = p.resolution, p.diameter
    ns = p.nSubaperture if n_subap is None else int(n_subap)
    nAct = ns + 1
    x = np.linspace(-D / 2, D / 2, nAct)
    centre = R / 2 + x * R / D
    width = (R / ns) / np.sqrt(2 * np.log(1.0 / p.mechanicalCoupling))
    pix = np.linspace(0, 1, R) * R
    gx = np.exp(-((pix[:, None] - centre[None, :]) ** 2) / (2 * width ** 2))
    a = 1.0 / (2 * width ** 2)
    XX, YY = np.meshgrid(pix, pix)

    def dense(act_idx):
        x0, y0 = centre[act_idx % nAct], centre[act_idx // nAct]
        return np.exp(-(a * (XX.reshape(-1, 1) - x0[None, :]) ** 2 + a * (YY.reshape(-1, 1) - y0[None, :]) ** 2))
    return gx, gx.copy(), dense


@pytest.mark.parametrize("kw", [dict(GEOMETRIES["R24"]), dict(GEOMETRIES["R48"]), dict(diameter=8.0, nSubaperture=20, nPixelPerSubap=6),
                                dict(diameter=3.0, nSubaperture=5, nPixelPerSubap=6, mechanicalCoupling=0.45, centralObstruction=0.2)])
def test_zero_arguments_are_bit_identical_to_the_tables_of_before(kw):
    p = calib.params_from_args(None, **kw)
    dmt = calib.DMTables(p)
    gx, gy, dense = _pre_feature_tables(p)
    assert np.array_equal(dmt.gx, gx) and np.array_equal(dmt.gy, gy) and np.array_equal(dmt.dense_modes(), dense(dmt.act_idx))
    f = calib.dm_factors(p, 0, 0, 0, 0)
    assert np.array_equal(f[0], gx) and np.array_equal(f[1], gy)
    d2 = calib.DMTables(p, n_subap=4)                              # the second mirror of a two-DM env
    g2x, _, dense2 = _pre_feature_tables(p, n_subap=4)
    assert np.array_equal(d2.gx, g2x) and np.array_equal(d2.dense_modes(), dense2(d2.act_idx))
    assert all(v == 0 for v in dmt.misreg.values())


def test_parameter_keys_reach_the_calibrated_mirror_and_a_rotation_raises():
    geo = GEOMETRIES["R48"]
    p = calib.params_from_args(None, MisReg_shiftX=0.05, MisReg_shiftY=-0.02, MisReg_rotationAngle=0.0, **geo)
    assert p.MisReg_shiftX == 0.05 and "MisReg_shiftX" not in p.extra
    dmt = calib.DMTables(p)
    gx, gy = calib.dm_factors(calib.params_from_args(None, **geo), shift_x=0.05, shift_y=-0.02)
    assert np.array_equal(dmt.gx, gx) and np.array_equal(dmt.gy, gy)
    assert not np.array_equal(dmt.gx, calib.DMTables(calib.params_from_args(None, **geo)).gx)
    want = REF.dense_influence(p.resolution, p.diameter, p.nSubaperture, p.mechanicalCoupling, dmt.act_idx, shift_x=0.05, shift_y=-0.02)
    assert np.abs(dmt.dense_modes().reshape(p.resolution, p.resolution, -1) - want).max() <= 1e-15
    c = calib.CompositeDM(p, 4)                                    # both mirrors of a two-DM env
    assert np.array_equal(c.gx[:, :9], gx) and c.dm2.misreg["shift_x"] == 0.05
    # a second shift is added to the calibrated one
    assert np.array_equal(calib.DMTables(p, shift_x=0.01).gx, calib.dm_factors(calib.params_from_args(None, **geo), shift_x=0.05 + 0.01)[0])
    with pytest.raises(NotImplementedError, match="not a product of two factors"):
        calib.DMTables(calib.params_from_args(None, MisReg_rotationAngle=1.5, **geo))
    with pytest.raises(NotImplementedError, match="not a product of two factors"):
        calib.CompositeDM(calib.params_from_args(None, MisReg_rotationAngle=-0.1, **geo), 4)


# ---- the arguments -------------------------------------------------------------------------------------------------------------
N_ = 4


def _resolve(env_ids=None, current=None, **kw):
    return resolve_dm_misregistration(kw, env_ids, N_, current)


def test_scalars_arrays_and_env_ids():
    d = _resolve(shift_x=0.01)
    assert set(d) == set(MISREG_KEYS) and all(v.shape == (N_,) and v.dtype == np.float64 for v in d.values())
    assert (d["shift_x"] == 0.01).all() and (d["shift_y"] == 0).all() and (d["radial_scaling"] == 0).all()
    d = _resolve(shift_x=[0.0, 0.01, 0.02, 0.03], tangential_scaling=torch.tensor([0.0, -0.1, 0.1, 0.2]))
    assert np.array_equal(d["shift_x"], [0.0, 0.01, 0.02, 0.03]) and d["tangential_scaling"][1] == np.float64(np.float32(-0.1))
    part = _resolve(env_ids=[3, 1], current=d, shift_y=[0.5, 0.7])
    assert np.array_equal(part["shift_y"], [0, 0.7, 0, 0.5])       # the caller's order
    assert np.array_equal(part["shift_x"], [0.0, 0.0, 0.02, 0.0])  # absolute per env: a listed env's arguments left out are 0 ...
    assert part["tangential_scaling"][2] == d["tangential_scaling"][2] and part["tangential_scaling"][1] == 0   # ... the others keep theirs
    assert d["shift_x"][1] == 0.01                                 # `current` is not written
    mask = _resolve(env_ids=np.array([True, False, False, True]), current=part, radial_scaling=[0.1, 0.2])
    assert np.array_equal(mask["radial_scaling"], [0.1, 0, 0, 0.2]) and mask["shift_y"][1] == 0.7
    none_yet = _resolve(env_ids=[2], shift_x=1e-3)
    assert np.array_equal(none_yet["shift_x"], [0, 0, 1e-3, 0])


@pytest.mark.parametrize("kw, what", [
    (dict(shift_x=[0.0, 0.1]), "shape"), (dict(shift_x=np.zeros((N_, 1))), "shape"), (dict(env_ids=[0, 1], shift_y=np.zeros(N_)), "shape"),
    (dict(shift_x=np.nan), "finite"), (dict(radial_scaling=[0, 0, np.inf, 0]), "finite"), (dict(shift_x="abc"), "numeric"),
    (dict(radial_scaling=-1.0), "above -1"), (dict(tangential_scaling=[0, 0, -2.0, 0]), "above -1"),
    (dict(env_ids=[4], shift_x=0.0), "outside"), (dict(env_ids=[1, 1], shift_x=0.0), "twice"), (dict(rotation=1.0), "unknown")])
def test_bad_arguments_raise(kw, what):
    with pytest.raises(ValueError, match=what):
        _resolve(**kw)


class _StubShard:
    """Records what reaches the library; holds the tables as a float32 shard would."""

    def __init__(self):
        self.calls, self.held = [], None

    def set_dm_env(self, gx, gy, stream=0):
        self.calls.append(None if gx is None else (np.array(gx), np.array(gy)))
        self.held = None if gx is None else (np.array(gx, dtype=np.float32).astype(np.float64), np.array(gy, dtype=np.float32).astype(np.float64))

    def get_dm_env(self, stream=0):
        return self.held[0].copy(), self.held[1].copy()


def _stub_env(second=False, **misreg):
    env = BatchedAOEnv.__new__(BatchedAOEnv)
    env.param = p = calib.params_from_args(None, **GEOMETRIES["R48"], **misreg)
    env._dm_tables = calib.CompositeDM(p, 4) if second else calib.DMTables(p)
    env.n_envs, env.R, env.nActuator = N_, p.resolution, env._dm_tables.nAct
    env._shard, env._dm_per_env, env._dm_misreg = _StubShard(), False, None
    env._stream = lambda: 0
    return env


def test_env_calls_on_a_stub_shard():
    env = _stub_env(MisReg_shiftX=0.05)
    p0 = calib.params_from_args(None, **GEOMETRIES["R48"])
    assert all((v == 0).all() for v in env.dm_misregistration.values())
    env.set_dm_misregistration(shift_x=[0.0, 0.01, 0.0, -0.02], radial_scaling=0.02)
    gx, gy = env._shard.calls[-1]
    assert gx.shape == gy.shape == (N_, 48, 9)
    for e, sx in enumerate([0.0, 0.01, 0.0, -0.02]):               # relative to the calibrated mirror: added to its MisReg_shiftX
        want = calib.dm_factors(p0, shift_x=0.05 + sx, radial_scaling=0.02)
        assert np.array_equal(gx[e], want[0]) and np.array_equal(gy[e], want[1])
    env.set_dm_misregistration(shift_y=0.03, env_ids=[2])          # the others keep what they have
    gx2, gy2 = env._shard.calls[-1]
    assert np.array_equal(gx2[[0, 1, 3]], gx[[0, 1, 3]]) and np.array_equal(gy2[[0, 1, 3]], gy[[0, 1, 3]])
    want = calib.dm_factors(p0, shift_x=0.05, shift_y=0.03)
    assert np.array_equal(gx2[2], want[0]) and np.array_equal(gy2[2], want[1])
    m = env.dm_misregistration
    assert np.array_equal(m["shift_x"], [0, 0.01, 0, -0.02]) and np.array_equal(m["shift_y"], [0, 0, 0.03, 0]) and np.array_equal(m["radial_scaling"], [0.02, 0.02, 0, 0.02])
    m["shift_x"][0] = 9.0
    assert env.dm_misregistration["shift_x"][0] == 0               # a copy
    # bad arguments raise before anything is touched
    n = len(env._shard.calls)
    with pytest.raises(ValueError):
        env.set_dm_misregistration(shift_x=[0.0, 0.1])
    with pytest.raises(NotImplementedError, match="not a product of two factors"):
        env.set_dm_misregistration(shift_x=0.01, rotation_angle=0.5)
    with pytest.raises(ValueError, match="shape"):
        env.set_dm_tables_per_env(np.zeros((N_, 48, 8)), np.zeros((N_, 48, 9)))
    with pytest.raises(ValueError, match="finite"):
        env.set_dm_tables_per_env(np.full((N_, 48, 9), np.nan), np.zeros((N_, 48, 9)))
    assert len(env._shard.calls) == n and np.array_equal(env.dm_misregistration["shift_y"], [0, 0, 0.03, 0])
    # the general form: env 1 with a dead actuator; the others keep the tables as held
    dead = gx2[1].copy()
    dead[:, 4] = 0
    env.set_dm_tables_per_env(dead[None], gy2[1][None], env_ids=[1])
    gx3, gy3 = env._shard.calls[-1]
    assert np.array_equal(gx3[1], dead) and np.array_equal(gx3[0], gx2[0].astype(np.float32).astype(np.float64)) and env.dm_misregistration is None
    with pytest.raises(ValueError, match="arbitrary per-env tables"):
        env.set_dm_misregistration(shift_x=0.01, env_ids=[0])
    env.set_dm_misregistration(shift_x=0.01)                       # every env: fine
    assert env.dm_misregistration is not None
    env.clear_dm_per_env()
    assert env._shard.calls[-1] is None and all((v == 0).all() for v in env.dm_misregistration.values()) and not env._dm_per_env
    # from the shared state, a partial table call fills the others with the calibrated mirror
    env.set_dm_tables_per_env(dead[None], gy2[1][None], env_ids=np.array([False, False, False, True]))
    gx4, _ = env._shard.calls[-1]
    assert np.array_equal(gx4[3], dead) and np.array_equal(gx4[0], env._dm_tables.gx)


def test_two_dm_env_moves_both_mirrors():
    env = _stub_env(second=True)
    env.set_dm_misregistration(shift_x=0.02, tangential_scaling=-0.01, env_ids=[1])
    gx, gy = env._shard.calls[-1]
    p = env.param
    a, b = calib.dm_factors(p, shift_x=0.02, tangential_scaling=-0.01), calib.dm_factors(p, shift_x=0.02, tangential_scaling=-0.01, n_subap=4)
    assert gx.shape == (N_, 48, 14)
    assert np.array_equal(gx[1], np.hstack([a[0], b[0]])) and np.array_equal(gy[1], np.hstack([a[1], b[1]]))
    assert np.array_equal(gx[0], env._dm_tables.gx) and np.array_equal(gy[3], env._dm_tables.gy)


class _StubEnv:
    output = "torch"
    nActuator = 3
    n_envs = 4
    device = "cpu"
    tdtype = torch.float64
    dm_misregistration = "the dict"

    def __init__(self):
        self.calls = []
        self.param = type("P", (), {"nLoop": 50})()

    def set_dm_misregistration(self, shift_x=0, shift_y=0, radial_scaling=0, tangential_scaling=0, env_ids=None, rotation_angle=0):
        self.calls.append(("misreg", shift_x, shift_y, radial_scaling, tangential_scaling, env_ids))

    def set_dm_tables_per_env(self, gx, gy, env_ids=None):
        self.calls.append(("tables", gx, gy, env_ids))

    def clear_dm_per_env(self):
        self.calls.append(("clear",))


@pytest.mark.parametrize("wrap", [TorchWrapper, lambda e: TimeDelayEnv(e, 2), lambda e: HistoryEnv(e, n_history=3, delay=2)])
def test_wrappers_forward_the_four_calls(wrap):
    inner = _StubEnv()
    env = wrap(inner)
    env.set_dm_misregistration(0.01, shift_y=0.02, env_ids=[1])
    env.set_dm_tables_per_env("gx", "gy", env_ids=[2])
    env.clear_dm_per_env()
    assert inner.calls == [("misreg", 0.01, 0.02, 0, 0, [1]), ("tables", "gx", "gy", [2]), ("clear",)]
    assert env.dm_misregistration == "the dict"
    assert "set_dm_misregistration" in type(env).__dict__ and "dm_misregistration" in type(env).__dict__     # forwarded, not fallen through


# ---- the ABI -------------------------------------------------------------------------------------------------------------------
def test_abi_is_unchanged_and_the_exports_exist(tmp_path):
    prog = ['#include <stdio.h>', f'#include "{HEADER}"', "int main(void){",
            'printf("version %d\\n", (int)AOENV_ABI_VERSION);', 'printf("bufs %d\\n", (int)AOENV_B_COUNT);',
            'printf("kernels %d\\n", (int)AOENV_K_COUNT);',
            "int (*s)(AoEnv*, const double*, const double*, void*) = aoenv_set_dm_env;",
            "int (*g)(AoEnv*, double*, double*, void*) = aoenv_get_dm_env;", 'printf("decl %d\\n", s != 0 && g != 0);', "return 0;}"]
    src, obj = tmp_path / "dm_env_abi.c", tmp_path / "dm_env_abi.o"
    src.write_text("\n".join(prog))
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-c", "-o", str(obj), str(src)], check=True)      # the prototypes, as C99
    prog[6:9] = ['printf("decl 1\\n");']
    src.write_text("\n".join(prog))
    exe = tmp_path / "dm_env_abi"
    subprocess.run(["gcc", "-std=c99", "-o", str(exe), str(src)], check=True)
    out = dict(l.split() for l in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(out["version"]) == 7 == L.ABI_VERSION and int(out["bufs"]) == 14 and int(out["kernels"]) == 13 == len(L.KERNEL_NAMES)
    text = open(HEADER).read()
    hdr = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in ("aoenv_set_dm_env", "aoenv_get_dm_env"):
        assert re.search(r"\b%s\s*\(" % name, hdr) and name in L.EXPORTS
    assert "DeformableMirror.py:326-351" in text and "OOPAOEnv.py:214-226" in text
    lib = L.load()                                                 # (declares every export: a missing symbol raises here)
    assert lib.aoenv_set_dm_env(None, None, None, None) != 0 and b"null" in lib.aoenv_last_error()
    z = np.zeros(4)
    assert lib.aoenv_get_dm_env(None, z.ctypes.data, z.ctypes.data, None) != 0


# ---- the re-layout, in a stand-alone sanitized program --------------------------------------------------------------------------
def _build_driver(out_dir, sanitize):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        return None
    exe = os.path.join(str(out_dir), "dm_env_driver" + ("_san" if sanitize else ""))
    flags = ["-O1", "-g", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-omit-frame-pointer"] if sanitize else ["-O2"]
    subprocess.run([hipcc, *flags, "-std=c++17", "-x", "hip", "--cuda-host-only", f"-I{REPO}/include", f"-I{REPO}/rlao_amd/csrc",
                    os.path.join(REPO, "tests", "native", "dm_env_driver.cpp"), "-o", exe], check=True, capture_output=True)
    return exe


@pytest.mark.parametrize("sanitize", [False, True])
def test_relayout_driver(tmp_path, sanitize):
    """tests/native/dm_env_driver.cpp: 3 envs at (R, n_act) = (24, 5), (30, 6), (144, 37), float and double -- every element of every
    layout against ga_index() and the transposed layout, the padding zero, env blocks disjoint; sanitize: the same program under
    ASan + UBSan, no report."""
    exe = _build_driver(tmp_path, sanitize)
    assert exe is not None, "hipcc not found: the library itself cannot be built without it"
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    out = subprocess.run([exe], capture_output=True, text=True, env=env)
    assert out.returncode == 0, out.stderr
    assert "ERROR: AddressSanitizer" not in out.stderr and "runtime error" not in out.stderr, out.stderr
    assert out.stdout.split()[0] == "ok" and int(out.stdout.split()[1]) > 400000
