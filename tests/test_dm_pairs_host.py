"""CPU: the host side of the rotated per-env mirror (aoenv_set_dm_pairs / BatchedAOEnv.set_dm_rotation / set_dm_pairs_per_env).  The
factor pairs of ``calib.dm_actuator_pairs`` against the reference's dense expression restated in tests/_dm_rot_ref.py and against
``dm.modes`` of the reference's own DeformableMirror (tests/golden/dm_rotated.npz, written by scripts/make_dm_rotated_golden.py),
rotation 0 against ``calib.dm_factors`` bit for bit, the argument handling of the Python layer on a stub shard, the wrappers, that
the feature matters to the oracle of tests/test_gpu_dm_pairs.py, the ABI, and the table re-layout
(rlao_amd/csrc/dm_pairs.hpp) in a stand-alone sanitized program.  No GPU."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import _dm_rot_ref as REF
from rlao_amd import _lib as L
from rlao_amd import calib
from rlao_amd.env import ROTATION_KEYS, BatchedAOEnv, resolve_dm_rotation
from rlao_amd.wrappers import HistoryEnv, TimeDelayEnv, TorchWrapper
from test_gpu_parity import F32_TOL

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "aoenv.h")
GOLDEN = os.path.join(REPO, "tests", "golden", "dm_rotated.npz")

GEOMETRIES = {"R24": dict(diameter=1.6, nSubaperture=4, nPixelPerSubap=6), "R30": dict(diameter=2.0, nSubaperture=5, nPixelPerSubap=6),
              "R48": dict(diameter=3.2, nSubaperture=8, nPixelPerSubap=6)}


def _sets(p):
    """rotations of both signs, alone and with shifts and scalings"""
    pitch = p.diameter / p.nSubaperture
    return {"zero": dict(), "rot+": dict(rotation_angle=1.5), "rot-": dict(rotation_angle=-3.0),
            "rot+shift": dict(rotation_angle=2.0, shift_x=0.3 * pitch, shift_y=-0.5 * pitch),
            "all+": dict(rotation_angle=3.0, shift_x=0.21 * pitch, shift_y=0.4 * pitch, radial_scaling=0.02, tangential_scaling=-0.03),
            "all-": dict(rotation_angle=-2.5, shift_x=-0.21 * pitch, shift_y=-0.4 * pitch, radial_scaling=-0.015, tangential_scaling=0.04),
            "quarter turn": dict(rotation_angle=90.0)}


def _product(py, px):
    return py[:, None, :] * px[None, :, :]                         # [y, x, k]


# ---- the restatement against the reference's own mirror --------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["R24", "R30"])
def test_restatement_and_pairs_match_the_reference_mirror(name):
    """dm.modes of the reference's DeformableMirror under a MisRegistration with rotation, both shifts and both scalings (the
    fixture) against tests/_dm_rot_ref.py and against py (x) px of calib.dm_actuator_pairs: 1e-15 absolute, the bound
    tests/test_dm_env_host.py derives for values in (0, 1]."""
    g = np.load(GOLDEN)
    assert list(g["param_names"]) == ["R", "D", "nsub", "mech_coupling", "rotation_angle", "shift_x", "shift_y", "radial_scaling", "tangential_scaling"]
    R, D, ns, mc, rot, sx, sy, rs, ts = g[name + "_params"]
    R, ns = int(R), int(ns)
    want = g[name + "_modes"]
    valid = np.flatnonzero(g[name + "_validAct"])
    kw = dict(rotation_angle=rot, shift_x=sx, shift_y=sy, radial_scaling=rs, tangential_scaling=ts)
    assert want.dtype == np.float64 and want.shape == (R * R, valid.size) and rot != 0 and sx != 0 and sy != 0 and rs != 0 and ts != 0
    err = float(np.abs(REF.dense_modes(R, D, ns, mc, valid, **kw) - want).max())
    p = calib.params_from_args(None, diameter=D, nSubaperture=ns, nPixelPerSubap=R // ns, mechanicalCoupling=mc)
    assert np.array_equal(calib.DMTables(p).act_idx, valid)
    py, px = calib.dm_actuator_pairs(p, **kw)
    err2 = float(np.abs(_product(py, px).reshape(R * R, -1) - want).max())
    moved = float(np.abs(want - REF.dense_modes(R, D, ns, mc, valid)).max())
    print(f"{name}: restatement {err:.3e}, pairs {err2:.3e}; the mirror differs from the nominal one by {moved:.3f} of the peak")
    assert err <= 1e-15 and err2 <= 1e-15 and moved > 0.1


@pytest.mark.parametrize("geo", sorted(GEOMETRIES))
def test_pairs_against_the_dense_expression(geo):
    p = calib.params_from_args(None, **GEOMETRIES[geo])
    dmt = calib.DMTables(p)
    R = p.resolution
    for name, kw in _sets(p).items():
        py, px = calib.dm_actuator_pairs(p, **kw)
        assert py.shape == px.shape == (R, dmt.nValidAct) and py.dtype == px.dtype == np.float64
        want = REF.dense_influence(R, p.diameter, p.nSubaperture, p.mechanicalCoupling, dmt.act_idx, **kw)
        err = float(np.abs(_product(py, px) - want).max())
        print(f"{geo} {name}: max |py (x) px - dense| = {err:.3e}")
        assert err <= 1e-15, (name, err)
    # the sign: a positive angle turns the grid from +x towards +y (:480-483) -- the actuator on the +x axis moves to larger y
    k = int(np.flatnonzero(dmt.act_idx == (dmt.nAct // 2) * dmt.nAct + dmt.nAct - 1)[0]) if dmt.nAct % 2 else None
    if k is not None:
        up, down = calib.dm_actuator_pairs(p, rotation_angle=5.0)[0][:, k], calib.dm_actuator_pairs(p, rotation_angle=-5.0)[0][:, k]
        assert np.argmax(up) > np.argmax(down)


@pytest.mark.parametrize("geo", sorted(GEOMETRIES))
def test_rotation_zero_is_dm_factors_bit_for_bit(geo):
    p = calib.params_from_args(None, **GEOMETRIES[geo])
    dmt = calib.DMTables(p)
    pitch = p.diameter / p.nSubaperture
    for kw in (dict(), dict(shift_x=0.3 * pitch, shift_y=-0.5 * pitch, radial_scaling=0.02, tangential_scaling=-0.03)):
        gx, gy = calib.dm_factors(p, **kw)
        py, px = calib.dm_actuator_pairs(p, rotation_angle=0, **kw)
        assert np.array_equal(py, gy[:, dmt.act_idx // dmt.nAct]) and np.array_equal(px, gx[:, dmt.act_idx % dmt.nAct])
    d2 = calib.DMTables(p, n_subap=4)                              # the second mirror of a two-DM env
    py, px = calib.dm_actuator_pairs(p, n_subap=4)
    assert np.array_equal(py, d2.gy[:, d2.act_idx // 5]) and np.array_equal(px, d2.gx[:, d2.act_idx % 5])


def test_the_refusals_of_the_calibrated_mirror_stay():
    geo = GEOMETRIES["R48"]
    assert "not a product of two factors" in calib.ROTATION_REFUSAL and "set_dm_rotation" in calib.ROTATION_REFUSAL
    with pytest.raises(NotImplementedError, match="not a product of two factors"):
        calib.DMTables(calib.params_from_args(None, MisReg_rotationAngle=1.5, **geo))
    with pytest.raises(NotImplementedError, match="not a product of two factors"):
        calib.dm_actuator_pairs(calib.params_from_args(None, MisReg_rotationAngle=1.5, **geo), rotation_angle=1.0)


# ---- the arguments ---------------------------------------------------------------------------------------------------------------
N_ = 4


def _resolve(env_ids=None, current=None, **kw):
    return resolve_dm_rotation(kw, env_ids, N_, current)


def test_scalars_arrays_and_env_ids():
    d = _resolve(rotation_angle=1.5)
    assert tuple(d) == ROTATION_KEYS and all(v.shape == (N_,) and v.dtype == np.float64 for v in d.values())
    assert (d["rotation_angle"] == 1.5).all() and (d["shift_x"] == 0).all()
    d = _resolve(rotation_angle=[0.0, 1.5, -3.0, 2.0], shift_x=torch.tensor([0.0, -0.1, 0.1, 0.2]))
    assert np.array_equal(d["rotation_angle"], [0.0, 1.5, -3.0, 2.0]) and d["shift_x"][1] == np.float64(np.float32(-0.1))
    part = _resolve(env_ids=[3, 1], current=d, rotation_angle=[0.5, 0.7])
    assert np.array_equal(part["rotation_angle"], [0, 0.7, -3.0, 0.5])    # the caller's order; the others keep theirs
    assert np.array_equal(part["shift_x"], [0.0, 0.0, np.float64(np.float32(0.1)), 0.0])   # a listed env's arguments left out are 0
    assert d["rotation_angle"][1] == 1.5                            # `current` is not written
    mask = _resolve(env_ids=np.array([True, False, False, True]), current=part, radial_scaling=[0.1, 0.2])
    assert np.array_equal(mask["radial_scaling"], [0.1, 0, 0, 0.2]) and mask["rotation_angle"][1] == 0.7 and mask["rotation_angle"][0] == 0
    assert np.array_equal(_resolve(env_ids=[2], rotation_angle=1e-3)["rotation_angle"], [0, 0, 1e-3, 0])


@pytest.mark.parametrize("kw, what", [
    (dict(rotation_angle=[0.0, 0.1]), "shape"), (dict(rotation_angle=np.zeros((N_, 1))), "shape"), (dict(env_ids=[0, 1], shift_y=np.zeros(N_)), "shape"),
    (dict(rotation_angle=np.nan), "finite"), (dict(radial_scaling=[0, 0, np.inf, 0]), "finite"), (dict(rotation_angle="abc"), "numeric"),
    (dict(radial_scaling=-1.0), "above -1"), (dict(tangential_scaling=[0, 0, -2.0, 0]), "above -1"),
    (dict(env_ids=[4], rotation_angle=0.0), "outside"), (dict(env_ids=[1, 1], rotation_angle=0.0), "twice"), (dict(anamorphosis=1.0), "unknown")])
def test_bad_arguments_raise(kw, what):
    with pytest.raises(ValueError, match=what):
        _resolve(**kw)


class _StubShard:
    """Records what reaches the library; holds the tables as a float32 shard would."""

    def __init__(self):
        self.calls, self.held, self.pairs = [], None, None

    def set_dm_env(self, gx, gy, stream=0):
        self.calls.append(("env", None if gx is None else (np.array(gx), np.array(gy))))
        self.held = None if gx is None else (np.array(gx, dtype=np.float32).astype(np.float64), np.array(gy, dtype=np.float32).astype(np.float64))

    def get_dm_env(self, stream=0):
        return self.held[0].copy(), self.held[1].copy()

    def set_dm_pairs(self, py, px, stream=0):
        self.calls.append(("pairs", None if py is None else (np.array(py), np.array(px))))
        self.pairs = None if py is None else (np.array(py, dtype=np.float32).astype(np.float64), np.array(px, dtype=np.float32).astype(np.float64))

    def get_dm_pairs(self, stream=0):
        return self.pairs[0].copy(), self.pairs[1].copy()


def _stub_env(second=False, new_attrs=True, **misreg):
    env = BatchedAOEnv.__new__(BatchedAOEnv)
    env.param = p = calib.params_from_args(None, **GEOMETRIES["R48"], **misreg)
    env._dm_tables = calib.CompositeDM(p, 4) if second else calib.DMTables(p)
    env.n_envs, env.R, env.nActuator = N_, p.resolution, env._dm_tables.nAct
    env._shard, env._dm_per_env, env._dm_misreg = _StubShard(), False, None
    if new_attrs:
        env._dm_pairs_on, env._dm_rot = False, None
    env._stream = lambda: 0
    return env


@pytest.mark.parametrize("new_attrs", [True, False])
def test_env_calls_on_a_stub_shard(new_attrs):
    """``new_attrs`` False: a stub with the attribute set of before the feature (tests/test_dm_env_host.py builds such stubs)."""
    env = _stub_env(new_attrs=new_attrs, MisReg_shiftX=0.05)
    p0 = calib.params_from_args(None, **GEOMETRIES["R48"])
    A = env._dm_tables.nValidAct
    assert env.dm_rotation is None
    env.set_dm_rotation([0.0, 1.5, -3.0, 2.0], shift_x=[0.0, 0.01, 0.0, -0.02], radial_scaling=0.02)
    kind, (py, px) = env._shard.calls[-1]
    assert kind == "pairs" and py.shape == px.shape == (N_, 48, A)
    for e, (rot, sx) in enumerate(zip([0.0, 1.5, -3.0, 2.0], [0.0, 0.01, 0.0, -0.02])):   # relative to the calibrated mirror
        want = calib.dm_actuator_pairs(p0, shift_x=0.05 + sx, rotation_angle=rot, radial_scaling=0.02)
        assert np.array_equal(py[e], want[0]) and np.array_equal(px[e], want[1])
    env.set_dm_rotation(-1.0, shift_y=0.03, env_ids=[2])           # the others keep what they have
    _, (py2, px2) = env._shard.calls[-1]
    assert np.array_equal(py2[[0, 1, 3]], py[[0, 1, 3]]) and np.array_equal(px2[[0, 1, 3]], px[[0, 1, 3]])
    want = calib.dm_actuator_pairs(p0, shift_x=0.05, shift_y=0.03, rotation_angle=-1.0)
    assert np.array_equal(py2[2], want[0]) and np.array_equal(px2[2], want[1])
    m = env.dm_rotation
    assert np.array_equal(m["rotation_angle"], [0, 1.5, -1.0, 2.0]) and np.array_equal(m["shift_y"], [0, 0, 0.03, 0]) and np.array_equal(m["radial_scaling"], [0.02, 0.02, 0, 0.02])
    m["rotation_angle"][0] = 9.0
    assert env.dm_rotation["rotation_angle"][0] == 0               # a copy
    # bad arguments raise before anything is touched; the refusal of set_dm_misregistration(rotation_angle) is what it was
    n = len(env._shard.calls)
    with pytest.raises(ValueError):
        env.set_dm_rotation([0.0, 0.1])
    with pytest.raises(NotImplementedError, match="not a product of two factors"):
        env.set_dm_misregistration(shift_x=0.01, rotation_angle=0.5)
    with pytest.raises(ValueError, match="shape"):
        env.set_dm_pairs_per_env(np.zeros((N_, 48, A - 1)), np.zeros((N_, 48, A)))
    with pytest.raises(ValueError, match="finite"):
        env.set_dm_pairs_per_env(np.full((N_, 48, A), np.nan), np.zeros((N_, 48, A)))
    # mutual exclusion: the factor tables are refused while pairs are in force, by a message that names the way out
    with pytest.raises(ValueError, match=r"clear_dm_per_env\(\)"):
        env.set_dm_misregistration(shift_x=0.01)
    with pytest.raises(ValueError, match=r"clear_dm_per_env\(\)"):
        env.set_dm_tables_per_env(np.zeros((N_, 48, 9)), np.zeros((N_, 48, 9)))
    assert len(env._shard.calls) == n and np.array_equal(env.dm_rotation["shift_y"], [0, 0, 0.03, 0])
    # the general form: env 1 with a dead actuator; the others keep the tables as held
    dead = py2[1].copy()
    dead[:, 4] = 0
    env.set_dm_pairs_per_env(dead[None], px2[1][None], env_ids=[1])
    _, (py3, px3) = env._shard.calls[-1]
    assert np.array_equal(py3[1], dead) and np.array_equal(py3[0], py2[0].astype(np.float32).astype(np.float64)) and env.dm_rotation is None
    with pytest.raises(ValueError, match="arbitrary actuator pairs"):
        env.set_dm_rotation(1.0, env_ids=[0])
    env.set_dm_rotation(1.0)                                       # every env: fine
    assert env.dm_rotation is not None
    env.clear_dm_per_env()
    assert env._shard.calls[-2] == ("pairs", None) and env._shard.calls[-1] == ("env", None)
    assert env.dm_rotation is None and not env._dm_pairs_on and not env._dm_per_env
    # from the cleared state, a partial pairs call fills the others with the calibrated mirror's columns
    env.set_dm_pairs_per_env(dead[None], px2[1][None], env_ids=np.array([False, False, False, True]))
    _, (py4, px4) = env._shard.calls[-1]
    dmt = env._dm_tables
    assert np.array_equal(py4[3], dead) and np.array_equal(py4[0], dmt.gy[:, dmt.act_idx // 9]) and np.array_equal(px4[0], dmt.gx[:, dmt.act_idx % 9])
    env.clear_dm_per_env()
    # ... and the reverse: pairs are refused while factor tables are in force
    env.set_dm_misregistration(shift_x=0.01)
    n = len(env._shard.calls)
    with pytest.raises(ValueError, match=r"clear_dm_per_env\(\)"):
        env.set_dm_rotation(1.0)
    with pytest.raises(ValueError, match=r"clear_dm_per_env\(\)"):
        env.set_dm_pairs_per_env(py2, px2)
    assert len(env._shard.calls) == n and env.dm_rotation is None
    env.clear_dm_per_env()
    assert env._shard.calls[-1] == ("env", None) and len(env._shard.calls) == n + 1     # no pairs to clear: the library is not asked


def test_two_dm_env_takes_pairs_only():
    env = _stub_env(second=True)
    with pytest.raises(ValueError, match="set_dm_pairs_per_env"):
        env.set_dm_rotation(1.0)
    assert env._shard.calls == []
    p, dmt = env.param, env._dm_tables
    a, b = calib.dm_actuator_pairs(p, rotation_angle=2.0), calib.dm_actuator_pairs(p, rotation_angle=2.0, n_subap=4)
    py, px = np.hstack([a[0], b[0]]), np.hstack([a[1], b[1]])
    assert py.shape == (48, dmt.nValidAct)
    env.set_dm_pairs_per_env(py[None], px[None], env_ids=[1])
    _, (qy, qx) = env._shard.calls[-1]
    assert np.array_equal(qy[1], py) and np.array_equal(qx[1], px)
    # the others: the composite mirror's own columns -- whose dense modes they reproduce
    n = dmt.nAct
    assert np.array_equal(qy[0], dmt.gy[:, dmt.act_idx // n]) and np.array_equal(qx[2], dmt.gx[:, dmt.act_idx % n])
    assert np.abs(_product(qy[0], qx[0]).reshape(48 * 48, -1) - dmt.dense_modes()).max() <= 1e-15


class _StubEnv:
    output = "torch"
    nActuator = 3
    n_envs = 4
    device = "cpu"
    tdtype = torch.float64
    dm_rotation = "the dict"

    def __init__(self):
        self.calls = []
        self.param = type("P", (), {"nLoop": 50})()

    def set_dm_rotation(self, rotation_angle, shift_x=0, shift_y=0, radial_scaling=0, tangential_scaling=0, env_ids=None):
        self.calls.append(("rotation", rotation_angle, shift_x, shift_y, radial_scaling, tangential_scaling, env_ids))

    def set_dm_pairs_per_env(self, py, px, env_ids=None):
        self.calls.append(("pairs", py, px, env_ids))

    def clear_dm_per_env(self):
        self.calls.append(("clear",))


@pytest.mark.parametrize("wrap", [TorchWrapper, lambda e: TimeDelayEnv(e, 2), lambda e: HistoryEnv(e, n_history=3, delay=2)])
def test_wrappers_forward_the_calls(wrap):
    inner = _StubEnv()
    env = wrap(inner)
    env.set_dm_rotation(1.5, shift_y=0.02, env_ids=[1])
    env.set_dm_pairs_per_env("py", "px", env_ids=[2])
    env.clear_dm_per_env()
    assert inner.calls == [("rotation", 1.5, 0, 0.02, 0, 0, [1]), ("pairs", "py", "px", [2]), ("clear",)]
    assert env.dm_rotation == "the dict"
    assert all(name in type(env).__dict__ for name in ("set_dm_rotation", "set_dm_pairs_per_env", "dm_rotation"))    # forwarded, not fallen through


# ---- the feature matters ---------------------------------------------------------------------------------------------------------
def test_dropping_one_envs_rotation_moves_the_oracle():
    """The oracle of tests/test_gpu_dm_pairs.py (SMALL, its mirrors, its steps): with any ONE env's mirror left nominal the residual
    OPD of that env after the steps moves by more than 100 x F32_TOL["opd_m"], the widest bound a GPU comparison holds it to -- a
    GPU test that passes cannot have missed the rotation.  (Env 0 IS the nominal mirror: it is the control, and does not move.)"""
    import _compose_ref as CR
    from oracle import ao_oracle as O
    geom = O.LayerGeometry(48, 3.2, 30.0)
    A, B = geom.AB(0.13)
    base = O.OracleEnv(resolution=48, diameter=3.2, n_subap=8, r0=0.13, L0=30.0, windSpeed=[10.0], windDirection=[72.0],
                       fractionalR0=[1.0], altitude=[0.0], n_modes=20, nLoop=16, geom_AB=(geom, A, B))
    steps, seed = 12, 5
    full = CR.drive(REF.rotated_oracle(base, range(4), seed), steps, rs_seed=13)            # (the GPU test's action stream)
    assert np.array_equal(REF.env_modes(48, 3.2, 8, 0.35, base.dm_valid_flat, 0.4, 0), base.dm_modes)
    for r in range(4):
        part = CR.drive(REF.rotated_oracle(base, range(4), seed, drop=(r,)), steps, actions=full["actions"])
        moved = np.abs(part["opd_res"] - full["opd_res"]).max(axis=(1, 2))
        print(f"env {r} nominal: residual OPD moves by {moved} m")
        for e in range(4):
            if e == r and r != 0:
                assert moved[e] > 100 * F32_TOL["opd_m"], (r, moved)
            else:
                assert moved[e] == 0, (r, e, moved)


# ---- the ABI -------------------------------------------------------------------------------------------------------------------
def test_abi_is_unchanged_and_the_exports_exist(tmp_path):
    text = open(HEADER).read()
    hdr = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"#define\s+AOENV_ABI_VERSION\s+7\b", hdr) and L.ABI_VERSION == 7
    assert re.search(r"AOENV_PATH_DM_PAIRS_GENERAL\s*=\s*32768", hdr) and L.PATH_DM_PAIRS_GENERAL == 32768
    for name in ("aoenv_set_dm_pairs", "aoenv_get_dm_pairs", "aoenv_get_dm_surface"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", hdr), name
        assert name in L.EXPORTS
    prog = ['#include "aoenv.h"', "#include <stdio.h>", "int main(void) {",
            "int (*s)(AoEnv*, const double*, const double*, void*) = aoenv_set_dm_pairs;",
            "int (*g)(AoEnv*, double*, double*, void*) = aoenv_get_dm_pairs;",
            "int (*f)(AoEnv*, double*, void*) = aoenv_get_dm_surface;", 'printf("%d\\n", s != 0 && g != 0 && f != 0);', "return 0;}"]
    src, obj = tmp_path / "dm_pairs_abi.c", tmp_path / "dm_pairs_abi.o"
    src.write_text("\n".join(prog))
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", f"-I{REPO}/include", "-c", "-o", str(obj), str(src)], check=True)   # the prototypes, as C99
    lib = L.load()
    z = np.zeros(4)
    for fn in (lib.aoenv_set_dm_pairs, lib.aoenv_get_dm_pairs):
        assert fn(None, z.ctypes.data, z.ctypes.data, None) != 0   # a null env is refused, not dereferenced
    assert lib.aoenv_get_dm_surface(None, z.ctypes.data, None) != 0


# ---- the re-layout, in a stand-alone sanitized program --------------------------------------------------------------------------
def _build_driver(out_dir, sanitize):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        return None
    exe = os.path.join(str(out_dir), "dm_pairs_driver" + ("_san" if sanitize else ""))
    flags = ["-O1", "-g", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-omit-frame-pointer"] if sanitize else ["-O2"]
    subprocess.run([hipcc, *flags, "-std=c++17", "-x", "hip", "--cuda-host-only", f"-I{REPO}/include", f"-I{REPO}/rlao_amd/csrc",
                    os.path.join(REPO, "tests", "native", "dm_pairs_driver.cpp"), "-o", exe], check=True, capture_output=True)
    return exe


@pytest.mark.parametrize("sanitize", [False, True])
def test_relayout_driver(tmp_path, sanitize):
    """tests/native/dm_pairs_driver.cpp: 3 envs at (R, A) = (24, 21), (30, 32), (48, 69), (144, 357), float and double -- every
    element of both layouts against the definition, the padding zero in R and in K, env blocks disjoint; sanitize: the same program
    under ASan + UBSan, no report."""
    exe = _build_driver(tmp_path, sanitize)
    assert exe is not None, "hipcc not found: the library itself cannot be built without it"
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    out = subprocess.run([exe], capture_output=True, text=True, env=env)
    assert out.returncode == 0, out.stderr
    assert "ERROR: AddressSanitizer" not in out.stderr and "runtime error" not in out.stderr, out.stderr
    assert out.stdout.split()[0] == "ok" and int(out.stdout.split()[1]) > 3000000
