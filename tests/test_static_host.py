"""CPU: the host side of the static aberration maps (aoenv_set_static_opd; BatchedAOEnv.set_static_aberration, ncpa_map, the
wrappers) and what makes tests/test_gpu_static.py able to fail.

tests/golden/static_opd.npz (scripts/make_static_golden.py: the reference's own NCPA and OPD_map objects, `atm*ngs*tel*map*dm`) pins
rlao_amd.calib.ncpa_map -- the f2 law and the linear form -- and the restatement tests/_static_ref.py: the order (the map enters
before the mirror), the masking (tel*dm masks the sum) and the unmasked sum OPD_no_pupil = atm + map + dm.

On the GPU test's own cases, candidate seeds and maps an oracle that IGNORES the map differs from tests/_static_ref.py's, for every
env, by more than 100 of the GPU test's tolerances in opd_m and in the WFS signal after the first step; and each convention broken on
purpose moves what the GPU test compares by more than 100 tolerances: the map masked before the sum (the geometric sensor's unmasked
phase and signal), the map on the atmosphere's side of the sum (AOENV_B_OPD_ATM, `total`), the sign of S_s - S_w flipped and the two
arms swapped (phase_sci).  Then the Python surface through a fake shard, the ABI text and the wrappers.

The library adds no host-only header with layout logic (static_opd.hpp only declares what the kernels are handed), so there is no
stand-alone driver to build."""
import os

import numpy as np
import pytest
import torch

import _static_ref as ST
from rlao_amd import _lib as L
from rlao_amd import calib
from rlao_amd.env import BatchedAOEnv
from rlao_amd.wrappers import HistoryEnv, TimeDelayEnv, TorchWrapper
from test_gpu_static import AMPLITUDE, CASES, STRIDE, TOL, maps

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = np.load(os.path.join(REPO, "tests", "golden", "static_opd.npz"))
_ORACLES = {}


# ---- the golden ---------------------------------------------------------------------------------------------------------------------
def test_ncpa_map_is_the_references_ncpa():
    """`ncpa_f2` / `ncpa_lin` of the golden come from the reference's own NCPA and Zernike classes, with ONE stage that is not the
    reference's: aotools (third party, absent) supplies `zernIndex` and `zernikeRadialFunc` there, and scripts/make_static_golden.py
    wires in oracle.ao_oracle's restatements of the two.  The Noll indexing and the radial polynomials of `calib.ncpa_map` are
    therefore checked against the project's own restatement ("parity unpinned"); the pupil coordinates, the modes'
    normalisation, the f2 law's random stream and weights, the scaling to the amplitude and the linear form are pinned to the
    reference.  The `OPD_map` order, masking and unmasked sum (the next test) are the reference's throughout."""
    R, D, _ = GOLD["params"]
    pupil = GOLD["pupil"]
    assert np.array_equal(pupil, calib.telescope_pupil(int(R)))
    f2 = [float(x) for x in GOLD["f2"]]
    f2[1], f2[2] = int(f2[1]), int(f2[2])
    got = calib.ncpa_map(pupil, float(D), f2=f2, seed=int(GOLD["seed"]))
    # the same operations on the same modes: a few roundings of a 100 nm map
    assert np.abs(got - GOLD["ncpa_f2"]).max() <= 1e-12 * f2[0]
    assert abs(np.std(got[pupil]) - f2[0]) <= 1e-12 * f2[0] and not got[~pupil].any()
    lin = calib.ncpa_map(pupil, float(D), coefficients=list(GOLD["coefficients"]))
    assert np.abs(lin - GOLD["ncpa_lin"]).max() <= 1e-12 * np.abs(GOLD["coefficients"]).max()
    assert np.abs(GOLD["ncpa_lin"]).max() > 1e-8
    # another seed, another map; and the refusals
    assert np.abs(calib.ncpa_map(pupil, float(D), f2=f2, seed=6) - got).max() > 1e-8
    for bad in (dict(), dict(f2=f2, coefficients=[1e-9]), dict(f2=[1e-7, 2, 12]), dict(f2=[1e-7, 5, 5, 1.0]), dict(coefficients=[]),
                dict(coefficients=[np.nan]), dict(f2=f2, basis="KL")):
        with pytest.raises(ValueError):
            calib.ncpa_map(pupil, float(D), **bad)


def _r24(geometric=False):
    key = ("r24", geometric)
    if key not in _ORACLES:
        kw = dict(resolution=24, diameter=1.6, n_subap=4, n_modes=4, nLoop=8)
        if geometric:
            import _geometric_ref as GR
            _ORACLES[key] = GR.GeometricOracle(**kw)
        else:
            from oracle import ao_oracle as O
            _ORACLES[key] = O.OracleEnv(**kw)
    return _copy(_ORACLES[key])


def _copy(base):
    import copy
    return copy.deepcopy(base, memo={id(x): x for x in (base.dm_modes, base.imat) if x is not None})


@pytest.mark.parametrize("name", ["map", "ncpa"])
def test_static_ref_is_the_references_order_masking_and_unmasked_sum(name):
    """The oracle's own step with the golden's atmosphere OPD and command and the map attached: tel_OPD == the reference's tel.OPD,
    and the geometric oracle's unmasked sum == tel.OPD_no_pupil -- the free map is not zero outside the pupil, and stays there."""
    the_map = GOLD["free_map"] if name == "map" else GOLD["ncpa_f2"]
    pupil = GOLD["pupil"]
    for geometric in (False, True):
        o = ST.static(_r24(geometric), the_map)
        assert np.abs(o.dm_modes - GOLD["dm_modes"]).max() <= 1e-12 and np.array_equal(o.pupil, pupil)
        o.atm.update = lambda: None                                 # the atmosphere of the golden, as it stands
        o.atm.OPD_no_pupil = GOLD["atm_opd"].copy()
        o.atm.OPD = GOLD["atm_opd"] * pupil
        o.coefs = GOLD["coefs"].copy()
        o.step(0, np.zeros((o.nActuator, o.nActuator), dtype=np.float32))
        assert np.abs(o.tel_OPD - GOLD[f"opd_{name}"]).max() <= 1e-18
        assert not o.tel_OPD[~pupil].any()
        if geometric:
            assert np.abs(o.opd_no_pupil - GOLD[f"opd_no_pupil_{name}"]).max() <= 1e-18
    if name == "map":
        outside = GOLD["opd_no_pupil_map"] - GOLD["atm_opd"] - (GOLD["dm_modes"] @ GOLD["coefs"]).reshape(24, 24)
        assert np.abs(outside[~pupil] - the_map[~pupil]).max() <= 1e-18 and np.abs(the_map[~pupil]).max() > 1e-8


# ---- the GPU test's inputs ------------------------------------------------------------------------------------------------------------
def _oracle(case):
    """The case's oracle for a flat mirror and zero actions (the controller plays no part through the first step): its own
    calibration where that is cheap, none (a zero controller, the separable mirror) at the large size."""
    if case not in _ORACLES:
        from oracle import ao_oracle as O
        g, kw, _, _ = CASES[case]
        R = g["nSubaperture"] * g["nPixelPerSubap"]
        args = dict(resolution=R, diameter=g["diameter"], n_subap=g["nSubaperture"], r0=g["r0"], L0=g["L0"], windSpeed=g["windSpeed"],
                    windDirection=g["windDirection"], fractionalR0=g["fractionalR0"], altitude=g["altitude"], n_modes=4, nLoop=g["nLoop"],
                    fov_arcsec=g.get("fov", 0.0))
        if case == "geo":
            import _geometric_ref as GR
            o = GR.GeometricOracle(**args)
        elif case == "wide":
            n_valid = int(O.dm_geometry(R, g["diameter"], g["nSubaperture"], pitch=g["diameter"] / (g["nSubaperture"] + 1), dense=False)["validAct"].sum())
            o = O.OracleEnv(dm_dense=False, m2c=np.zeros((n_valid, 4)), modal_cm=np.zeros((4, 1)), **args)
            o.reconstructor = np.zeros((n_valid, o.wfs.nSignal))
        elif kw.get("wfs_type") == "pyramid":
            o = O.OracleEnv(wfs_type="pyramid", modulation=g["modulation"], psf_centering=g["psfCentering"], **args)
        elif "second_dm" in kw:
            o = O.OracleEnv(second_dm_nsub=kw["second_dm"]["nSubaperture"], **args)
        else:
            o = O.OracleEnv(**args)
        _ORACLES[case] = o
    return _ORACLES[case]


def _need(case, o):
    need_opd = 100 * max(TOL["f32"]["opd_m"], TOL["f64"]["opd_m"])
    if case != "geo":
        return need_opd, 100 * max(TOL["f32"]["signal"], TOL["f64"]["signal"])
    import _geometric_ref as GR
    p = o.R // o.wfs.nSubap
    return need_opd, 100 * GR.geo_signal_bound(max(TOL["f32"]["opd_m"], TOL["f64"]["opd_m"]), p, o.D / o.R, o.wfs.slopes_units, o.wavelength)


def _first_step(o, seed):
    o.new_episode(seed)
    o.step(0, np.zeros((o.nActuator, o.nActuator), dtype=np.float32))
    return o


@pytest.mark.parametrize("case", list(CASES))
def test_ignoring_the_map_misses_by_100_tolerances(case):
    base = _oracle(case)
    g, _, n, seed0 = CASES[case]
    need_opd, need_sig = _need(case, base)
    s_w = maps(base.R, g["diameter"], 4)[-n:]
    assert 0.5 * AMPLITUDE < np.std(s_w[0][base.pupil]) < 2.5 * AMPLITUDE      # about 100 nm rms: the amplitude the GPU test runs at
    for seed in range(seed0, seed0 + 4):                            # (the GPU test takes the first of these that is clear of the cut)
        for k in range(n):
            seeing, blind = (_first_step(ST.static(_copy(base), s_w[k], v), seed + STRIDE * k) for v in (None, "ignore"))
            d_opd = float(np.abs(seeing.tel_OPD - blind.tel_OPD).max())
            d_sig = float(np.abs(seeing.wfs.signal - blind.wfs.signal).max())
            if seed == seed0:
                print(f"{case} env {k}: opd_m {d_opd:.3e} (need {need_opd:.1e}), signal {d_sig:.3e} (need {need_sig:.1e})")
            assert d_opd > need_opd, (case, seed, k, d_opd, need_opd)
            assert d_sig > need_sig, (case, seed, k, d_sig, need_sig)
            assert np.array_equal(seeing.atm.OPD_no_pupil, blind.atm.OPD_no_pupil) and seeing.total[0] == blind.total[0]


def test_the_map_masked_before_the_sum_moves_the_unmasked_phase_by_100_tolerances():
    """`geo`: only the unmasked phase (and the slopes at the pupil's edge) can tell; the masked residual cannot, by construction."""
    base = _oracle("geo")
    g, _, n, seed = CASES["geo"]
    need_opd, need_sig = _need("geo", base)
    s_w = maps(base.R, g["diameter"], 4)
    for k in range(n):
        right, masked = (_first_step(ST.static(_copy(base), s_w[k], v), seed + STRIDE * k) for v in (None, "masked"))
        d_np = float(np.abs(right.opd_no_pupil - masked.opd_no_pupil).max())
        d_sig = float(np.abs(right.wfs.signal - masked.wfs.signal).max())
        print(f"geo env {k}: unmasked opd_m {d_np:.3e} (need {need_opd:.1e}), signal {d_sig:.3e} (need {need_sig:.1e})")
        assert d_np > need_opd and d_sig > need_sig, (k, d_np, d_sig)
        assert np.abs(right.tel_OPD - masked.tel_OPD).max() <= 1e-18


@pytest.mark.parametrize("case", ["small", "top_first", "geo"])
def test_the_map_on_the_atmospheres_side_moves_the_atmospheres_numbers_by_100_tolerances(case):
    base = _oracle(case)
    g, _, n, seed = CASES[case]
    need_opd = _need(case, base)[0]
    need_rms = 100 * max(TOL["f32"]["rms_nm"], TOL["f64"]["rms_nm"])
    s_w = maps(base.R, g["diameter"], 4)
    for k in range(n):
        right, wrong = (_first_step(ST.static(_copy(base), s_w[k], v), seed + STRIDE * k) for v in (None, "atm_side"))
        d_atm = float(np.abs(right.atm.OPD_no_pupil - wrong.atm.OPD_no_pupil).max())
        d_tot = float(abs(right.total[0] - wrong.total[0]))
        print(f"{case} env {k}: atm opd_m {d_atm:.3e} (need {need_opd:.1e}), total {d_tot:.3e} nm (need {need_rms:.1e})")
        assert d_atm > need_opd and d_tot > need_rms, (case, k, d_atm, d_tot)
        assert np.abs(right.tel_OPD - wrong.tel_OPD).max() <= 1e-15      # the residual is the same sum either way


@pytest.mark.parametrize("variant", ["flip", "swap"])
def test_a_flipped_difference_and_swapped_arms_move_the_science_phase_by_100_tolerances(variant):
    base = _oracle("top_first")
    g, _, n, seed = CASES["top_first"]
    need = 100 * max(TOL["f32"]["opd_m"], TOL["f64"]["opd_m"])
    s_w, s_s = maps(base.R, g["diameter"], 4), maps(base.R, g["diameter"], 4, "science")
    for k in range(n):
        k_opd = base.wavelength / (2 * np.pi)
        o = _first_step(ST.static(_copy(base), s_w[k]), seed + STRIDE * k)
        right = ST.science_phase(o.phase, o.pupil, s_w[k], s_s[k], o.wavelength)[0]
        if variant == "flip":
            wrong = ST.science_phase(o.phase, o.pupil, s_w[k], s_s[k], o.wavelength, variant="flip")[0]
        else:
            a_w, a_s = ST.arms(s_w[k], s_s[k], "swap")
            p = _first_step(ST.static(_copy(base), a_w), seed + STRIDE * k)
            wrong = ST.science_phase(p.phase, p.pupil, a_w, a_s, p.wavelength)[0]
        d = float(np.abs(right - wrong).max() * k_opd)
        print(f"top_first env {k} {variant}: phase_sci opd_m {d:.3e} (need {need:.1e})")
        assert d > need, (variant, k, d)
        # ... and the restatement is the reference's sum with the science arm's map in place of the sensor's
        want = (o.atm.OPD_no_pupil + s_s[k] + (o.dm_opd(np.zeros(o.nValidAct)) - s_w[k])) * o.pupil
        assert np.abs(right * k_opd - want).max() <= 1e-18


# ---- the Python layer through a fake shard --------------------------------------------------------------------------------------------
class _FakeLib:
    def __init__(self, n, R):
        self.calls, self.n, self.R, self.held = [], n, R, None

    def _arr(self, p, count):
        if p is None:
            return None
        return np.ctypeslib.as_array((np.ctypeslib.ctypes.c_double * (count * self.R * self.R)).from_address(p.value)).reshape(count, self.R, self.R).copy()

    def aoenv_set_static_opd(self, h, wfs, sci, per_env, stream):
        count = per_env if per_env else 1
        wfs, sci = self._arr(wfs, count), self._arr(sci, count)
        self.calls.append(("set", per_env, None if wfs is None else wfs.shape, None if sci is None else sci.shape))
        self.held = None if wfs is None and sci is None else (wfs, sci)
        return 0

    def aoenv_get_static_opd(self, h, wfs, sci):
        for dst, src in zip((wfs, sci), self.held):
            out = np.ctypeslib.as_array((np.ctypeslib.ctypes.c_double * (self.n * self.R * self.R)).from_address(dst.value)).reshape(self.n, self.R, self.R)
            out[:] = 0.0 if src is None else np.broadcast_to(src, out.shape)
        return 0

    def aoenv_static_surface_path(self, h, launches):
        return 0 if self.held is None or self.held[0] is None else 1

    def aoenv_last_error(self):
        return b"refused"


def _fake_env(monkeypatch, n=3, R=6):
    from rlao_amd.env import Shard
    env = BatchedAOEnv.__new__(BatchedAOEnv)                        # (the constructor wants a device)
    sh = Shard.__new__(Shard)
    sh.h, sh.lib = None, _FakeLib(n, R)
    sh.cfg = type("C", (), {"n_env": n, "resolution": R})()
    env._shard, env._static, env._oa = sh, False, None
    env.R, env.n_envs = R, n
    env._stream = lambda: 0
    monkeypatch.setattr(L, "load", lambda: sh.lib)
    return env


def test_maps_through_a_fake_shard(monkeypatch):
    env = _fake_env(monkeypatch)
    lib, R = env._shard.lib, env.R
    rs = np.random.RandomState(0)
    a, b = rs.randn(R, R), rs.randn(3, R, R)
    assert env.static_aberration is None
    env.set_static_aberration(wfs=a)                                # one map for the shard: one copy, per_env = 0
    assert lib.calls[-1] == ("set", 0, (1, R, R), None)
    assert np.array_equal(env.static_aberration["wfs"], np.tile(a, (3, 1, 1))) and not env.static_aberration["science"].any()
    env.set_static_aberration(wfs=a, science=b)                     # one arm per env: both go per env
    assert lib.calls[-1] == ("set", 3, (3, R, R), (3, R, R))
    assert np.array_equal(env.static_aberration["science"], b) and np.array_equal(env.static_aberration["wfs"], np.tile(a, (3, 1, 1)))
    env.set_static_aberration(science=b[:2] * 2, env_ids=[2, 0])    # the per-env rule: listed envs in the caller's order, the sensor
    got = env.static_aberration                                     # arm as held
    assert np.array_equal(got["science"], np.stack([b[1] * 2, b[1], b[0] * 2])) and np.array_equal(got["wfs"], np.tile(a, (3, 1, 1)))
    env.set_static_aberration(science=a, env_ids=[1])
    assert np.array_equal(env.static_aberration["science"][1], a)
    n = len(lib.calls)
    for bad in (dict(), dict(wfs=np.zeros((R, R + 1))), dict(wfs=np.zeros((2, R, R))), dict(science=np.full((R, R), np.nan)),
                dict(wfs=np.zeros((2, R, R)), env_ids=[0]), dict(wfs=a, env_ids=[3]), dict(wfs="map")):
        with pytest.raises(ValueError):
            env.set_static_aberration(**bad)
    assert len(lib.calls) == n                                      # refused before anything was touched
    env.clear_static_aberration()
    assert lib.calls[-1] == ("set", 0, None, None) and env.static_aberration is None
    env.set_static_aberration(science=b[0], env_ids=[1])            # nothing held: the others are zero, the sensor arm stays absent
    assert lib.calls[-1] == ("set", 3, None, (3, R, R)) and not env.static_aberration["science"][[0, 2]].any()


def test_abi_declares_the_entry_points_and_no_new_ids():
    text = open(os.path.join(REPO, "include", "aoenv.h")).read()
    for name in ("aoenv_set_static_opd", "aoenv_get_static_opd", "aoenv_static_surface_path"):
        assert f"int {name}(AoEnv* env" in text and name in L.EXPORTS and name in L._LATER_ENTRIES
    assert "AOENV_PATH_DM_STATIC_GENERAL = 65536" in text and L.PATH_DM_STATIC_GENERAL == 65536
    assert "#define AOENV_ABI_VERSION 7" in text and L.ABI_VERSION == 7
    kernels = open(os.path.join(REPO, "rlao_amd", "csrc", "static_kernels.hip")).read()
    for k in ("k_dm_static_mfma", "k_dm_static", "k_static_add", "k_science_static"):
        assert k in kernels
    assert "static" not in " ".join(L.KERNEL_NAMES)
    doc = open(os.path.join(REPO, "INTEGRATION.md")).read()
    assert "aoenv_set_static_opd" in doc and "aoenv_get_static_opd" in doc


def test_the_maps_are_not_part_of_get_state():
    import inspect
    for fn in (BatchedAOEnv.get_state, BatchedAOEnv.set_state):
        assert "_static" not in inspect.getsource(fn) and "static_aberration" not in inspect.getsource(fn)


# ---- the wrappers -----------------------------------------------------------------------------------------------------------------------
class _StubEnv:
    output = "torch"
    nActuator = 3
    n_envs = 4
    device = "cpu"
    tdtype = torch.float64
    static_aberration = "maps"

    def __init__(self):
        self.calls = []

    def set_static_aberration(self, wfs=None, science=None, env_ids=None):
        self.calls.append(("set", wfs, science, env_ids))

    def clear_static_aberration(self):
        self.calls.append(("clear",))

    def ncpa_map(self, f2=None, coefficients=None, seed=5, basis="zernike"):
        self.calls.append(("ncpa", f2, coefficients, seed, basis))
        return "a map"


@pytest.mark.parametrize("wrap", [TorchWrapper, lambda e: TimeDelayEnv(e, 2), lambda e: HistoryEnv(e, n_history=3, delay=1)])
def test_the_wrappers_forward_the_configuration(wrap):
    inner = _StubEnv()
    env = wrap(inner)
    for name in ("set_static_aberration", "clear_static_aberration", "static_aberration", "ncpa_map"):
        assert name in type(env).__dict__, name                      # a method of the wrapper, not a fall-through
    env.set_static_aberration("w", science="s", env_ids=[2])
    assert env.static_aberration == "maps"
    assert env.ncpa_map(f2=[1e-7, 2, 9, 1.0], seed=7) == "a map"
    env.clear_static_aberration()
    assert inner.calls == [("set", "w", "s", [2]), ("ncpa", [1e-7, 2, 9, 1.0], None, 7, "zernike"), ("clear",)]
