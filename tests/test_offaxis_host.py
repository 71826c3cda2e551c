"""CPU: the host side of the off-axis science target (aoenv_set_science_direction and what goes with it; BatchedAOEnv.
set_science_direction, env.src.coordinates, the wrappers).

Against the golden (tests/golden/offaxis.npz, written by scripts/make_offaxis_golden.py from the reference's own Atmosphere and
Source): the restatement tests/_offaxis_ref.py gives the reference's OPD_no_pupil within F64_SAME_OPERATOR_TOL["opd_m"] of
tests/test_gpu_parity.py, and the host plan -- the Python mirror of rlao_amd/csrc/offaxis.hpp, and offaxis.hpp itself through
tests/native/offaxis_driver.cpp -- reproduces its footprint corners and fractions exactly.  The plan refuses a zenith above fov / 2
and holds its in-range assertion at zenith = fov / 2 for azimuth 0 / 90 / 180 / 270 / 45 / 225 on every case of tests/_fov_cases.py.

Conventions: on the inputs of tests/test_gpu_offaxis.py (its cases, seeds, directions and six atmosphere steps; the atmosphere does
not depend on the loop) dropping the fractions, flipping their sign, swapping rows and columns and rounding where the reference
truncates each move opd_atm_sci by more than 100 of that test's largest tolerance: no convention error can pass there.  No GPU."""
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import _fov_cases as F
import _offaxis_ref as X
from rlao_amd import _lib as L
from rlao_amd.env import BatchedAOEnv
from rlao_amd.wrappers import HistoryEnv, TimeDelayEnv, TorchWrapper
from test_gpu_offaxis import DIRS, SEEDS, STEPS, STRIDE
from test_gpu_parity import F32_TOL, F64_SAME_OPERATOR_TOL

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden", "offaxis.npz")
AZIMUTHS = (0.0, 90.0, 180.0, 270.0, 45.0, 225.0)


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    exe = os.path.join(str(tmp_path_factory.mktemp("offaxis")), "offaxis_driver")
    subprocess.run([hipcc, "-O2", "-std=c++17", "-x", "hip", "--cuda-host-only", f"-I{REPO}/include", f"-I{REPO}/rlao_amd/csrc",
                    os.path.join(REPO, "tests", "native", "offaxis_driver.cpp"), "-o", exe], check=True, capture_output=True)
    return exe


def _drive(exe, R, D, fov, layers, dirs):
    """the driver's answer: (refusal code, env, layer), rows [l][e] of parsed values"""
    args = [exe, str(R), repr(float(D)), repr(float(fov)), str(len(layers))]
    for h, n in layers:
        args += [repr(float(h)), str(int(n))]
    args.append(str(len(dirs)))
    for z, a in dirs:
        args += [repr(float(z)), repr(float(a))]
    lines = subprocess.run(args, check=True, capture_output=True, text=True).stdout.split("\n")
    head = tuple(int(v) for v in lines[0].split())
    rows = {}
    for ln in lines[1:]:
        t = ln.split()
        if t:
            rows[(int(t[0]), int(t[1]))] = dict(fy=int(t[2]), fx=int(t[3]), ty=float.fromhex(t[4]), tx=float.fromhex(t[5]), ix=int(t[6]),
                                                iy=int(t[7]), extra_sx=float.fromhex(t[8]), extra_sy=float.fromhex(t[9]), row0=int(t[10]),
                                                col0=int(t[11]), lo=int(t[12]), hi=int(t[13]))
    return head, rows


class _Lay:
    def __init__(self, phase, frac):
        self.phase, self.frac = phase, frac
        self.g = type("G", (), {"resolution": phase.shape[0]})()


class _Atm:
    def __init__(self, R, D, layers):
        self.R, self.D, self.layers = R, D, layers


# ---- against the golden ----------------------------------------------------------------------------------------------------------------
def test_restatement_gives_the_reference_opd(golden):
    g = golden
    R, D, fov = int(g["params"][0]), float(g["params"][1]), float(g["params"][2])
    assert g["opd_no_pupil"].shape[:2] == (3, 5) and list(g["grids"]) == [28, 43]
    worst = 0.0
    for u in range(g["opd_no_pupil"].shape[0]):
        atm = _Atm(R, D, [_Lay(g[f"phase_u{u}_l{l}"], g["frac"][l]) for l in range(len(g["altitude"]))])
        for d, (zen, az) in enumerate(g["directions"]):
            X.check_direction(zen, fov)
            got = X.science_opd(atm, g["altitude"], zen, az)
            worst = max(worst, float(np.abs(got - g["opd_no_pupil"][u, d]).max()))
    assert worst <= F64_SAME_OPERATOR_TOL["opd_m"], worst
    assert np.abs(g["opd_no_pupil"][:, 1:] - g["opd_no_pupil"][:, :1]).max() > 1e-8      # (the directions do see other air)


def test_plan_reproduces_the_golden_corners_and_fractions(golden, driver):
    g = golden
    R, D, fov = int(g["params"][0]), float(g["params"][1]), float(g["params"][2])
    layers = list(zip(g["altitude"], g["grids"]))
    head, rows = _drive(driver, R, D, fov, layers, g["directions"])
    assert head[0] == 0
    for d, (zen, az) in enumerate(g["directions"]):
        for l, (h, n) in enumerate(layers):
            s = X.ref_shift(h, zen, az, R, D, int(n))
            assert (s["row0"], s["col0"]) == tuple(g["corners"][0, d, l])
            assert (s["extra_sx"], s["extra_sy"]) == tuple(g["extra"][0, d, l])      # exactly: the same float64 operations
            fy, fx, ty, tx = X.device_shift(s)
            assert 0 <= ty < 1 and 0 <= tx < 1
            # floor + fraction is the same sampling point as int + extra
            assert fy + ty == pytest.approx(s["iy"] - s["extra_sy"], abs=1e-15) and fx + tx == pytest.approx(s["ix"] - s["extra_sx"], abs=1e-15)
            # offaxis.hpp on the host: the whole pixels exactly, the fractions to the last bits of libm's tan / cos / sin
            r = rows[(l, d)]
            assert (r["row0"], r["col0"], r["ix"], r["iy"], r["fy"], r["fx"]) == (s["row0"], s["col0"], s["ix"], s["iy"], fy, fx)
            for a, b in ((r["extra_sx"], s["extra_sx"]), (r["extra_sy"], s["extra_sy"]), (r["ty"], ty), (r["tx"], tx)):
                assert abs(a - b) <= 4e-15
            ok, lo, hi = X.plan_layer(h, zen, az, R, D, int(n))
            assert ok and (lo, hi) == (r["lo"], r["hi"])
    assert np.array_equal(g["corners"][0], g["corners"][-1]) and np.array_equal(g["extra"][0], g["extra"][-1])


def _cases():
    out = {n: (c["n_sub"] * c["ppx"], 0.4 * c["n_sub"], c["fov"], list(zip(c["altitude"], c["grids"]))) for n, c in F.CASES.items()}
    return out


@pytest.mark.parametrize("name", list(F.CASES))
def test_plan_holds_at_the_edge_of_the_field_and_refuses_beyond(name, driver):
    R, D, fov, layers = _cases()[name]
    dirs = [(fov / 2, az) for az in AZIMUTHS] + [(0.0, 0.0)]
    head, rows = _drive(driver, R, D, fov, layers, dirs)
    assert head[0] == 0, head
    for l, (h, n) in enumerate(layers):
        for e, (zen, az) in enumerate(dirs):
            ok, lo, hi = X.plan_layer(h, zen, az, R, D, n)
            assert ok and lo >= 1 and hi <= n - 2, (name, l, az, lo, hi)
            assert (rows[(l, e)]["lo"], rows[(l, e)]["hi"]) == (lo, hi)
    # beyond fov / 2, negative, not finite: refused, the env named
    for bad in (fov / 2 + 1e-9, -1e-9, float("nan"), float("inf")):
        head, rows = _drive(driver, R, D, fov, layers, [(0.0, 0.0), (bad, 0.0)])
        assert head[0] == 3 and head[1] == 1 and not rows
        with pytest.raises(ValueError):
            X.check_direction(bad, fov)
    assert _drive(driver, R, D, fov, layers, [(0.0, float("nan"))])[0][0] == 4
    assert _drive(driver, R, D, fov, [], [(0.0, 0.0)])[0][0] == 1                    # no layers
    # a grid two pixels too small for its field: the plan refuses what the grid rule would have allowed
    if any(h > 0 for h, _ in layers):
        small = [(h, n - 4 if h > 0 else n) for h, n in layers]
        refused = [_drive(driver, R, D, fov, small, [(fov / 2, az)])[0][0] for az in AZIMUTHS]
        assert 6 in refused, refused


# ---- conventions: on the GPU test's inputs ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["two", "p5_shared", "up70", "pyr"])
def test_every_convention_error_moves_the_gpu_tests_inputs_by_100_tolerances(name):
    from oracle import ao_oracle as O
    if name == "pyr":
        import test_gpu_pyramid_sweep as P
        c = P.CASES[F.PYR["base"]]
        g = P._geo(F.PYR["base"], **F.atmosphere(F.PYR, c["ppx"]))
    else:
        g = F.geo(name)
    R = g["nSubaperture"] * g["nPixelPerSubap"]
    need = 100 * max(F32_TOL["opd_m"], F64_SAME_OPERATOR_TOL["opd_m"])
    geoms = F.layer_geometries(g)
    AB = {id(q): q.AB(g["r0"]) for q in geoms}
    moved = {v: 0.0 for v in ("nofrac", "flipfrac", "swap", "round")}
    for k, (zen, az) in enumerate(DIRS[name]):
        atm = O.OracleAtmosphere(R, g["diameter"], 1.0 / F.FRAME_RATE, O.make_pupil(R), g["r0"], g["L0"], g["windSpeed"], g["fractionalR0"],
                                 g["windDirection"], g["altitude"], fov_rad=g["fov"] / 206265.0, geom_AB=[(q,) + AB[id(q)] for q in geoms])
        atm.generate_new_phase_screen(SEEDS[name] + STRIDE * k)
        for _ in range(STEPS):
            atm.update()
            true = X.science_opd(atm, g["altitude"], zen, az)
            for v in moved:
                moved[v] = max(moved[v], float(np.abs(X.science_opd(atm, g["altitude"], zen, az, variant=v) - true).max()))
    for v, m in moved.items():
        assert m > need, (name, v, m, need)


# ---- the Python layer through a fake shard ---------------------------------------------------------------------------------------------------
class _FakeLib:
    def __init__(self, fov):
        self.calls, self.fov, self.zen, self.az = [], fov, None, None

    @staticmethod
    def _arr(p, n):
        return None if p is None else np.ctypeslib.as_array((np.ctypeslib.ctypes.c_double * n).from_address(p.value)).copy()

    def aoenv_set_science_direction(self, h, zen, az, stream):
        zen, az = self._arr(zen, 3), self._arr(az, 3)
        self.calls.append(("set", None if zen is None else zen.tolist(), None if az is None else az.tolist()))
        if zen is not None and (zen > self.fov / 2).any():
            return 1
        self.zen, self.az = zen, az
        return 0

    def aoenv_get_science_direction(self, h, zen, az):
        np.ctypeslib.as_array((np.ctypeslib.ctypes.c_double * 3).from_address(zen.value))[:] = self.zen
        np.ctypeslib.as_array((np.ctypeslib.ctypes.c_double * 3).from_address(az.value))[:] = self.az
        return 0

    def aoenv_set_science_direction_record(self, h, rec, i_base, n_slots):
        self.calls.append(("rec", rec is not None and bool(rec.value), i_base, n_slots))
        return 0

    def aoenv_science_residual(self, h, phase, opd, rms, sr, stream):
        self.calls.append(("residual",) + tuple(p is not None and bool(p.value) for p in (phase, opd, rms, sr)))
        return 0

    def aoenv_last_error(self):
        return b"zenith above fov / 2"


def _fake_env(monkeypatch, fov=20.0):
    env = BatchedAOEnv.__new__(BatchedAOEnv)                        # (the constructor wants a device)
    env._shard = type("S", (), {"h": None, "lib": _FakeLib(fov)})()
    env._oa = env._oa_rec = None
    env.param = type("P", (), {"fov": fov})()
    env.R, env.n_envs, env.device, env.tdtype, env.output = 24, 3, "cpu", torch.float32, "torch"
    env._stream = lambda: 0
    from rlao_amd.env import _ScienceSourceProxy
    env.src = _ScienceSourceProxy(env)
    monkeypatch.setattr(L, "load", lambda: env._shard.lib)
    return env


def test_directions_through_a_fake_shard(monkeypatch):
    env = _fake_env(monkeypatch)
    calls = env._shard.lib.calls
    assert env.science_direction is None and not env.src.coordinates.any() and env.src.coordinates.shape == (3, 2)
    for call in (env.science_residual, env.science_atmosphere, lambda: env.record_science_direction(0, 4)):
        with pytest.raises(L.AoEnvError, match="set_science_direction"):
            call()
    env.src.coordinates = [0.4, 0]                                  # the reference's own line
    assert calls[-1] == ("set", [0.4, 0.4, 0.4], [0.0, 0.0, 0.0])
    env.set_science_direction([1.0, 2.0], 90.0, env_ids=[2, 0])      # the per-env rule: listed envs in the caller's order
    assert calls[-1] == ("set", [2.0, 0.4, 1.0], [90.0, 0.0, 90.0])
    assert np.array_equal(env.science_direction, [[2.0, 90.0], [0.4, 0.0], [1.0, 90.0]])
    env.src.coordinates = np.array([[0.0, 10.0], [3.0, 20.0], [10.0, 30.0]])
    assert np.array_equal(env.src.coordinates, [[0.0, 10.0], [3.0, 20.0], [10.0, 30.0]])
    n = len(calls)
    for bad in (10.5, -1.0, float("nan"), [1.0, 2.0]):
        with pytest.raises(ValueError):
            env.set_science_direction(bad)
    with pytest.raises(ValueError, match="coordinates"):
        env.src.coordinates = [1.0, 2.0, 3.0]
    with pytest.raises(AttributeError):
        env.src.magnitude = 3
    assert len(calls) == n and env.science_direction[2, 0] == 10.0  # refused before anything was touched
    phase, rms, sr = env.science_residual()
    assert phase.shape == (3, 24, 24) and rms.shape == sr.shape == (3,) and calls[-1] == ("residual", True, False, True, True)
    assert env.science_atmosphere().shape == (3, 24, 24) and calls[-1] == ("residual", False, True, False, False)
    rec = env.record_science_direction(2, 5)
    assert rec.shape == (5, 2, 3) and calls[-1] == ("rec", True, 2, 5) and env._oa_rec is rec
    with pytest.raises(ValueError):
        env.record_science_direction(-1, 5)
    env.stop_science_direction_record()
    assert calls[-1] == ("rec", False, 0, 0) and env._oa_rec is None
    env.clear_science_direction()
    assert calls[-1] == ("set", None, None) and env.science_direction is None and not env.src.coordinates.any()


def test_abi_declares_the_entry_points():
    text = open(os.path.join(REPO, "include", "aoenv.h")).read()
    for name in ("aoenv_set_field", "aoenv_set_science_direction", "aoenv_get_science_direction", "aoenv_science_residual",
                 "aoenv_set_science_direction_record"):
        assert f"int {name}(AoEnv* env" in text and name in L.EXPORTS
    assert "AOENV_WF_SCIENCE = 4" in text and L.WF_SCIENCE == 4
    from rlao_amd.env import wavefront_bits
    assert wavefront_bits("science") == 4


# ---- the wrappers -----------------------------------------------------------------------------------------------------------------------
CONFIG = ("set_science_direction", "clear_science_direction", "science_direction", "src", "science_residual", "science_atmosphere")
LOOPS = ("record_science_direction", "stop_science_direction_record")


class _StubEnv:
    output = "torch"
    nActuator = 3
    n_envs = 4
    device = "cpu"
    tdtype = torch.float64
    science_direction = "direction"
    src = "proxy"

    def __init__(self):
        self.calls = []

    def set_science_direction(self, zenith, azimuth=0.0, env_ids=None):
        self.calls.append(("set", zenith, azimuth, env_ids))

    def clear_science_direction(self):
        self.calls.append(("clear",))

    def science_residual(self):
        self.calls.append(("residual",))
        return "r"

    def science_atmosphere(self):
        self.calls.append(("atmosphere",))
        return "a"

    def record_science_direction(self, i0, n_steps):
        self.calls.append(("record", i0, n_steps))
        return "rec"

    def stop_science_direction_record(self):
        self.calls.append(("stop",))


def _drive_wrapper(env, inner, loops):
    env.set_science_direction(1.0, azimuth=30.0, env_ids=[2])
    assert env.science_direction == "direction" and env.src == "proxy"
    assert env.science_residual() == "r" and env.science_atmosphere() == "a"
    want = [("set", 1.0, 30.0, [2]), ("residual",), ("atmosphere",)]
    if loops:
        assert env.record_science_direction(1, 3) == "rec"
        env.stop_science_direction_record()
        want += [("record", 1, 3), ("stop",)]
    env.clear_science_direction()
    assert inner.calls == want + [("clear",)]


def test_torch_wrapper_forwards_everything():
    inner = _StubEnv()
    env = TorchWrapper(inner)
    for name in CONFIG + LOOPS:
        assert name in type(env).__dict__, name                      # a method of the wrapper, not a fall-through
    _drive_wrapper(env, inner, True)


@pytest.mark.parametrize("wrap", [lambda e: TimeDelayEnv(e, 2), lambda e: HistoryEnv(e, n_history=3, delay=1)])
def test_delay_and_history_envs_forward_the_configuration_and_the_read_outs(wrap):
    inner = _StubEnv()
    env = wrap(inner)
    for name in CONFIG:
        assert name in type(env).__dict__, name
    _drive_wrapper(env, inner, False)
