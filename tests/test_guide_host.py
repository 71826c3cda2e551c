"""CPU: the host side of the off-axis guide star (aoenv_set_guide_direction; BatchedAOEnv.set_guide_direction, env.ngs.coordinates,
the wrappers) and what makes tests/test_gpu_guide.py able to fail.

The model is pinned to the reference by tests/golden/offaxis.npz through tests/test_offaxis_host.py: `atm * source` at off-axis
coordinates is one code path whether the source is the guide star or the science target.  The library adds no host logic of its own:
aoenv_set_guide_direction plans with the science direction's oa_make (tests/native/offaxis_driver.cpp drives it under ASan + UBSan).

Here: the helper tests/_guide_ref.py at zenith 0 is the oracle's own `_collect`, exactly; on the GPU test's own cases, seeds and
directions an oracle that IGNORES the direction differs from the guided one, for every env with zenith > 0, by more than 100 of the
GPU test's tolerances in opd_m and in the WFS signal after the first step; every convention variant of tests/_offaxis_ref.py
("nofrac", "flipfrac", "swap", "round") moves opd_m AND the WFS signal over the GPU test's steps by more than 100 tolerances;
the Python surface through a fake shard; the wrappers."""
import os

import numpy as np
import pytest
import torch

import _fov_cases as F
import _guide_ref as R
from rlao_amd import _lib as L
from rlao_amd.env import BatchedAOEnv, _SourceProxy
from rlao_amd.wrappers import HistoryEnv, TimeDelayEnv, TorchWrapper
from test_gpu_guide import CASES, DIRS, N, SEEDS, STEPS, STRIDE, TOL, _geo

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_ORACLES = {}


def _oracle(name):
    """The case's oracle with its own calibration (the controller plays no part: the mirror is flat through the first step)."""
    if name not in _ORACLES:
        g = _geo(name)
        kw = dict(resolution=g["nSubaperture"] * g["nPixelPerSubap"], diameter=g["diameter"], n_subap=g["nSubaperture"], r0=g["r0"],
                  L0=g["L0"], windSpeed=g["windSpeed"], windDirection=g["windDirection"], fractionalR0=g["fractionalR0"],
                  altitude=g["altitude"], n_modes=4, nLoop=g["nLoop"], fov_arcsec=g["fov"])
        if name == "geo":
            import _geometric_ref as GR
            _ORACLES[name] = GR.GeometricOracle(**kw)
        elif name == "pyr":
            from oracle import ao_oracle as O
            _ORACLES[name] = O.OracleEnv(wfs_type="pyramid", modulation=g["modulation"], psf_centering=g["psfCentering"], **kw)
        else:
            from oracle import ao_oracle as O
            _ORACLES[name] = O.OracleEnv(**kw)
    return _ORACLES[name], _geo(name)


def _copy(base):
    import copy
    return copy.deepcopy(base, memo={id(x): x for x in (base.dm_modes, base.imat) if x is not None})


def _signal_need(name, o):
    """100 of the GPU test's signal tolerances (the larger of float32 and float64), as that test forms them"""
    if name != "geo":
        return 100 * max(TOL["f32"]["signal"], TOL["f64"]["signal"])
    import _geometric_ref as GR
    p = o.R // o.wfs.nSubap
    return 100 * GR.geo_signal_bound(max(TOL["f32"]["opd_m"], TOL["f64"]["opd_m"]), p, o.D / o.R, o.wfs.slopes_units, o.wavelength)


def test_zenith_zero_is_the_oracles_own_collect():
    base, g = _oracle("two")
    a, b = _copy(base), _copy(base)
    R.guide(a, g["altitude"], 0.0, 135.0)                           # (asserts the identity inside every _collect, too)
    for o in (a, b):
        o.new_episode(7)
    for i in range(3):
        act = np.zeros((a.nActuator, a.nActuator), dtype=np.float32)
        ra, rb = a.step(i, act), b.step(i, act)
        assert np.array_equal(a.atm.OPD_no_pupil, b.atm.OPD_no_pupil) and np.array_equal(a.atm.OPD, b.atm.OPD)
        assert np.array_equal(a.wfs.signal, b.wfs.signal) and np.array_equal(ra[0], rb[0]) and ra[3] == rb[3]
    assert a.atm.guide_direction == (0.0, 135.0)


@pytest.mark.parametrize("name", CASES)
def test_ignoring_the_direction_misses_by_100_tolerances(name):
    base, g = _oracle(name)
    need_opd = 100 * max(TOL["f32"]["opd_m"], TOL["f64"]["opd_m"])
    need_sig = _signal_need(name, base)
    act = np.zeros((base.nActuator, base.nActuator), dtype=np.float32)
    seen = 0
    for k, (zen, az) in enumerate(DIRS[name]):
        if zen == 0:
            continue
        seen += 1
        guided, blind = R.guide(_copy(base), g["altitude"], zen, az), R.guide(_copy(base), g["altitude"], zen, az, variant="ignore")
        for o in (guided, blind):
            o.new_episode(SEEDS[name] + STRIDE * k)
            o.step(0, act)
        d_opd = float(np.abs(guided.atm.OPD_no_pupil - blind.atm.OPD_no_pupil).max())
        d_sig = float(np.abs(guided.wfs.signal - blind.wfs.signal).max())
        print(f"{name} env {k}: opd_m {d_opd:.3e} (need {need_opd:.1e}), signal {d_sig:.3e} (need {need_sig:.1e})")
        assert d_opd > need_opd, (name, k, d_opd, need_opd)
        assert d_sig > need_sig, (name, k, d_sig, need_sig)
    assert seen >= 3 and len(DIRS[name]) == N


@pytest.mark.parametrize("name", CASES)
def test_every_convention_error_moves_the_gpu_tests_inputs_by_100_tolerances(name):
    """Over the GPU test's STEPS atmosphere steps, the maximum over the envs (as tests/test_offaxis_host.py takes it), flat mirror."""
    base, g = _oracle(name)
    need_opd = 100 * max(TOL["f32"]["opd_m"], TOL["f64"]["opd_m"])
    act = np.zeros((base.nActuator, base.nActuator), dtype=np.float32)
    moved = {v: [0.0, 0.0] for v in ("nofrac", "flipfrac", "swap", "round")}
    for k, (zen, az) in enumerate(DIRS[name]):
        runs = {v: R.guide(_copy(base), g["altitude"], zen, az, variant=v) for v in (None,) + tuple(moved)}
        for o in runs.values():
            o.new_episode(SEEDS[name] + STRIDE * k)
        for i in range(STEPS):
            for o in runs.values():
                o.step(i, act)
            for v, m in moved.items():
                m[0] = max(m[0], float(np.abs(runs[v].atm.OPD_no_pupil - runs[None].atm.OPD_no_pupil).max()))
                m[1] = max(m[1], float(np.abs(runs[v].wfs.signal - runs[None].wfs.signal).max()))
    for v, (m_opd, m_sig) in moved.items():
        print(f"{name} {v}: opd_m {m_opd:.3e} (need {need_opd:.1e}), signal {m_sig:.3e} (100 tolerances: {_signal_need(name, base):.1e})")
        assert m_opd > need_opd, (name, v, m_opd, need_opd)
        assert m_sig > _signal_need(name, base), (name, v, m_sig)


# ---- the Python layer through a fake shard ---------------------------------------------------------------------------------------------------
class _FakeLib:
    def __init__(self, fov):
        self.calls, self.fov, self.zen, self.az = [], fov, None, None

    @staticmethod
    def _arr(p, n):
        return None if p is None else np.ctypeslib.as_array((np.ctypeslib.ctypes.c_double * n).from_address(p.value)).copy()

    def aoenv_set_guide_direction(self, h, zen, az, stream):
        zen, az = self._arr(zen, 3), self._arr(az, 3)
        self.calls.append(("set", None if zen is None else zen.tolist(), None if az is None else az.tolist()))
        self.zen, self.az = zen, az
        return 0

    def aoenv_get_guide_direction(self, h, zen, az):
        np.ctypeslib.as_array((np.ctypeslib.ctypes.c_double * 3).from_address(zen.value))[:] = self.zen
        np.ctypeslib.as_array((np.ctypeslib.ctypes.c_double * 3).from_address(az.value))[:] = self.az
        return 0

    def aoenv_last_error(self):
        return b"refused"


def _fake_env(monkeypatch, fov=20.0):
    env = BatchedAOEnv.__new__(BatchedAOEnv)                        # (the constructor wants a device)
    env._shard = type("S", (), {"h": None, "lib": _FakeLib(fov)})()
    env._oa = env._oa_rec = env._guide = None
    env.param = type("P", (), {"fov": fov})()
    env.R, env.n_envs, env.device, env.tdtype, env.output = 24, 3, "cpu", torch.float32, "torch"
    env._stream = lambda: 0
    env.source = env.ngs = _SourceProxy(env)
    monkeypatch.setattr(L, "load", lambda: env._shard.lib)
    return env


def test_directions_through_a_fake_shard(monkeypatch):
    env = _fake_env(monkeypatch)
    calls = env._shard.lib.calls
    assert env.guide_direction is None and not env.ngs.coordinates.any() and env.ngs.coordinates.shape == (3, 2)
    env.ngs.coordinates = [0.4, 0]
    assert calls[-1] == ("set", [0.4, 0.4, 0.4], [0.0, 0.0, 0.0])
    env.set_guide_direction([1.0, 2.0], 90.0, env_ids=[2, 0])        # the per-env rule: listed envs in the caller's order
    assert calls[-1] == ("set", [2.0, 0.4, 1.0], [90.0, 0.0, 90.0])
    assert np.array_equal(env.guide_direction, [[2.0, 90.0], [0.4, 0.0], [1.0, 90.0]])
    env.source.coordinates = np.array([[0.0, 10.0], [3.0, 20.0], [10.0, 30.0]])
    assert np.array_equal(env.ngs.coordinates, [[0.0, 10.0], [3.0, 20.0], [10.0, 30.0]])
    n = len(calls)
    for bad in (10.5, -1.0, float("nan"), [1.0, 2.0]):
        with pytest.raises(ValueError):
            env.set_guide_direction(bad)
    with pytest.raises(ValueError, match="coordinates"):
        env.ngs.coordinates = [1.0, 2.0, 3.0]
    with pytest.raises(AttributeError):
        env.ngs.wavelength = 3
    assert len(calls) == n and env.guide_direction[2, 0] == 10.0     # refused before anything was touched
    assert env.science_direction is None                             # the science target is another matter
    env.clear_guide_direction()
    assert calls[-1] == ("set", None, None) and env.guide_direction is None and not env.ngs.coordinates.any()


def test_abi_declares_the_entry_points_and_no_new_ids():
    text = open(os.path.join(REPO, "include", "aoenv.h")).read()
    for name in ("aoenv_set_guide_direction", "aoenv_get_guide_direction"):
        assert f"int {name}(AoEnv* env" in text and name in L.EXPORTS and name in L._LATER_ENTRIES
    assert "k_guide_opd" in open(os.path.join(REPO, "rlao_amd", "csrc", "offaxis_kernels.hip")).read()
    assert "guide" not in " ".join(L.KERNEL_NAMES)


def test_the_direction_is_not_part_of_get_state():
    import inspect
    for fn in (BatchedAOEnv.get_state, BatchedAOEnv.set_state):
        assert "_guide" not in inspect.getsource(fn) and "guide_direction" not in inspect.getsource(fn)


# ---- the wrappers -----------------------------------------------------------------------------------------------------------------------
class _StubEnv:
    output = "torch"
    nActuator = 3
    n_envs = 4
    device = "cpu"
    tdtype = torch.float64
    guide_direction = "direction"

    def __init__(self):
        self.calls = []

    def set_guide_direction(self, zenith, azimuth=0.0, env_ids=None):
        self.calls.append(("set", zenith, azimuth, env_ids))

    def clear_guide_direction(self):
        self.calls.append(("clear",))


@pytest.mark.parametrize("wrap", [TorchWrapper, lambda e: TimeDelayEnv(e, 2), lambda e: HistoryEnv(e, n_history=3, delay=1)])
def test_the_wrappers_forward_the_configuration(wrap):
    inner = _StubEnv()
    env = wrap(inner)
    for name in ("set_guide_direction", "clear_guide_direction", "guide_direction"):
        assert name in type(env).__dict__, name                      # a method of the wrapper, not a fall-through
    env.set_guide_direction(1.0, azimuth=30.0, env_ids=[2])
    assert env.guide_direction == "direction"
    env.clear_guide_direction()
    assert inner.calls == [("set", 1.0, 30.0, [2]), ("clear",)]
