"""CPU: the laser-guide-star Shack-Hartmann on the host -- the restatement tests/_lgs_ref.py and rlao_amd/calib.py against the
reference's golden tests/golden/lgs_sh.npz (scripts/make_lgs_golden.py), the binned-tap identity the device relies on, the table's
validation and launch plan (rlao_amd/csrc/sh_lgs.hpp) in a stand-alone sanitized program, and the Python argument handling and the
wrappers against recording stand-ins.  No GPU."""
import os
import re
import shutil
import subprocess
import warnings

import numpy as np
import pytest
import torch

import _lgs_ref as G
from rlao_amd import _lib as L
from rlao_amd import calib
from rlao_amd.env import BatchedAOEnv, _SourceProxy, _WfsProxy, resolve_lgs, resolve_lgs_per_env
from rlao_amd.wrappers import HistoryEnv, TimeDelayEnv, TorchWrapper
from test_gpu_parity import CAL_TOL, F32_TOL, F64_SAME_OPERATOR_TOL

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "aoenv.h")
TOL = F64_SAME_OPERATOR_TOL


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(G.GOLDEN))


_ORC = {}


def _lgs(gold, tag):
    return dict(Na_profile=gold[f"{tag}_Na_profile"], FWHM_spot_up=float(gold[f"{tag}_FWHM_spot_up"]),
                laser_coordinates=gold[f"{tag}_laser_coordinates"])


def _oracle(gold, tag, lgs=True, name="", **kw):
    """the oracle env of the case (its own calibration on elongated spots); lgs=False: the NGS twin, or with kernels_of= / shift= a
    sensor with those kernels (`name` tells such sensors apart)"""
    key = (tag, lgs, name)
    if key not in _ORC:
        R, ns, D, _, _ = G.CASES[tag]
        geo = dict(resolution=R, diameter=D, n_subap=ns, band=G.BAND, magnitude=G.MAGNITUDE, n_modes=6, r0=0.13, L0=30.0, nLoop=8)
        if lgs:
            _ORC[key] = G.lgs_oracle_env(_lgs(gold, tag), **geo)
        else:
            from oracle import ao_oracle as O
            O._PHOTOMETRY.setdefault("Na", (0.589e-6, 0, 3.3e12))
            saved = O.OracleSH
            if kw:
                O.OracleSH = G.make_lgs_sh(saved, kw["kernels_of"], shift=kw.get("shift", True))
            try:
                _ORC[key] = O.OracleEnv(wfs_type="sh", **geo)
            finally:
                O.OracleSH = saved
    return _ORC[key]


def _sht(tag):
    R, ns, D, _, _ = G.CASES[tag]
    p = calib.params_from_args(dict(diameter=D, nSubaperture=ns, nPixelPerSubap=R // ns, opticalBand=G.BAND, magnitude=G.MAGNITUDE))
    return p, calib.SHTables(p, calib.telescope_pupil(R, 0.0), calib.source(G.BAND, G.MAGNITUDE)[1])


def _signals(env, gold, tag):
    """the golden's four OPD signals and frames through an oracle env's sensor"""
    k = 2 * np.pi / env.wavelength
    sig, frames = [], []
    for opd in gold[f"{tag}_opd"]:
        sig.append(env.wfs.measure(opd * env.pupil * k).copy())
        frames.append(env.wfs.frame.copy())
    return np.array(sig), np.array(frames)


# ---- the restatement against the golden ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", list(G.CASES))
def test_restatement_matches_the_reference(gold, tag):
    env = _oracle(gold, tag)
    w, ns = env.wfs, G.CASES[tag][1]
    assert np.array_equal(w.valid_2d, gold[f"{tag}_valid"]) and np.array_equal(env.pupil, gold[f"{tag}_pupil"])
    assert abs(env.wavelength - float(gold[f"{tag}_wavelength"])) == 0
    assert np.abs(w.reference_slopes_maps - gold[f"{tag}_reference_slopes_maps"]).max() <= CAL_TOL["ref"]
    np.testing.assert_allclose(w.slopes_units, float(gold[f"{tag}_slopes_units"]), rtol=1e-9)
    sig, frames = _signals(env, gold, tag)
    peak = gold[f"{tag}_frame_opd"].max(axis=(1, 2))
    assert np.abs(sig - gold[f"{tag}_sig_opd"]).max() <= TOL["signal"]
    assert (np.abs(frames - gold[f"{tag}_frame_opd"]).max(axis=(1, 2)) / peak).max() <= TOL["frame_rel"]
    k = 2 * np.pi / env.wavelength
    for c, want in zip(gold[f"{tag}_coefs"], gold[f"{tag}_sig_dm"]):
        assert np.abs(w.measure(env.dm_opd(c) * env.pupil * k) - want).max() <= TOL["signal"]
    cols = np.stack([env.poke_signal(a, env.wavelength / 16) for a in gold[f"{tag}_poke_idx"]], axis=1)
    want = gold[f"{tag}_poke_cols"]
    assert np.abs(cols - want).max() <= CAL_TOL["imat_rel"] * np.abs(want).max()


@pytest.mark.parametrize("tag", list(G.CASES))
def test_calib_kernels_match_the_reference(gold, tag):
    """calib.lgs_spot_kernels (the reference's loops restated) and tests/_lgs_ref.spot_kernels (array at once) against K =
    real(ifft2(wfs.C)), the elongation factor and the Na-weighted altitude."""
    R, ns, D, launch, fwhm = G.CASES[tag]
    p, sht = _sht(tag)
    K_ref = np.real(np.fft.ifft2(gold[f"{tag}_C"]))
    assert np.abs(np.imag(np.fft.ifft2(gold[f"{tag}_C"]))).max() <= 1e-16
    K, el = calib.lgs_spot_kernels(p, sht, gold[f"{tag}_Na_profile"], fwhm, launch)
    K2, el2 = G.spot_kernels(R, ns, D, calib.source(G.BAND, 0)[0], sht.valid_1d, gold[f"{tag}_Na_profile"], fwhm, launch)
    assert K.shape == K_ref.shape == (sht.nValid, sht.n, sht.n)
    assert np.abs(K - K_ref).max() <= 1e-15 and np.abs(K2 - K_ref).max() <= 1e-15
    assert np.allclose(K.sum(axis=(1, 2)), 1, rtol=0, atol=1e-15) and (K >= 0).all()
    want = float(gold[f"{tag}_elungation_factor"])
    assert abs(el - want) <= 1e-13 * want and abs(el2 - want) <= 1e-13 * want
    assert abs(calib.lgs_altitude(gold[f"{tag}_Na_profile"]) - float(gold[f"{tag}_altitude"])) <= 1e-9
    zeros = (K == 0).sum(axis=(1, 2))
    if tag == "r24":
        assert zeros.min() >= 100 and np.abs(K - K[0]).max() > 0.01 * K.max()      # truncated kernels that differ between lenslets
    if tag == "r24d":
        assert zeros.max() == 0                                                     # the dense case


# ---- the binned taps and the box -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", list(G.CASES))
def test_binned_taps_and_the_box(gold, tag):
    """camera = bin2x2(fftshift(ifft2(fft2(I) fft2(K)))) == sum_{s,t} I[s][t] Kb[(2P + n/2 - s) mod n][(2Q + n/2 - t) mod n], on random
    non-negative intensities; the box holds every non-zero tap and is the smallest that does."""
    R, ns, D, launch, fwhm = G.CASES[tag]
    p, sht = _sht(tag)
    K, _ = calib.lgs_spot_kernels(p, sht, gold[f"{tag}_Na_profile"], fwhm, launch)
    Kb, box = calib.lgs_binned_taps(K)
    assert Kb.shape == K.shape and box.dtype == np.int32 and box.shape == (4,)
    assert np.abs(Kb - G.binned_taps(K)).max() <= 1e-16
    rs = np.random.RandomState(3)
    I = rs.uniform(0, 1, K.shape) ** 3 * 2.4e3
    want = G.convolve_and_bin(I, K)
    got = G.tap_sum(I, Kb)
    assert np.abs(got - want).max() <= 1e-12 * want.max()
    assert np.abs(got.sum(axis=(1, 2)) - I.sum(axis=(1, 2))).max() <= 1e-12 * I.sum(axis=(1, 2)).max()      # energy: the taps sum to 4 x 1/4
    n = sht.n
    x0, y0, nx, ny = (int(v) for v in box)
    rows, cols = (x0 + np.arange(nx)) % n, (y0 + np.arange(ny)) % n
    inside = np.zeros((n, n), bool)
    inside[np.ix_(rows, cols)] = True
    used = (Kb != 0).any(axis=0)
    assert not used[~inside].any()
    if tag == "r24d":
        assert (nx, ny) == (n, n)
    else:
        assert nx < n and ny < n
        for edge in (used[rows[0]], used[rows[-1]], used[:, cols[0]], used[:, cols[-1]]):
            assert edge.any()                                       # no smaller box: every edge holds a tap
    # a box that wraps, and a table of several envs: the union
    rolled = np.roll(K, (5, 3), axis=(-2, -1))
    _, b2 = calib.lgs_binned_taps(np.stack([K, rolled]))
    u2 = ((Kb != 0) | (calib.lgs_binned_taps(rolled)[0] != 0)).any(axis=0)
    r2, c2 = (b2[0] + np.arange(b2[2])) % n, (b2[1] + np.arange(b2[3])) % n
    in2 = np.zeros((n, n), bool)
    in2[np.ix_(r2, c2)] = True
    assert not u2[~in2].any()
    with pytest.raises(ValueError):
        calib.lgs_binned_taps(np.zeros((3, 5, 5)))


# ---- what the tolerances are worth ---------------------------------------------------------------------------------------------------
def test_every_mutant_misses_the_golden_by_a_hundred_tolerances(gold):
    """Ignoring the elongation, dropping the fftshift, dropping the transpose and dropping the truncation each move a compared
    quantity of the R = 24 case by more than 100 tolerances (F32_TOL["signal"] = 6e-4, the widest the GPU tests apply)."""
    tag = "r24"
    R, ns, D, launch, fwhm = G.CASES[tag]
    want = gold[f"{tag}_sig_opd"]
    wl = calib.source(G.BAND, 0)[0]

    def kernels(**kw):
        return lambda sh: G.spot_kernels(R, ns, D, wl, sh.valid_1d, gold[f"{tag}_Na_profile"], fwhm, launch, **kw)[0]

    mutants = {"no elongation": dict(lgs=False),
               "no fftshift": dict(lgs=False, kernels_of=kernels(), shift=False),
               "no transpose": dict(lgs=False, kernels_of=kernels(transpose=False)),
               "no truncation": dict(lgs=False, kernels_of=kernels(truncate=False))}
    good = _signals(_oracle(gold, tag, lgs=False, name="unmutated", kernels_of=kernels()), gold, tag)[0]
    assert np.abs(good - want).max() <= TOL["signal"]              # (the harness itself: the unmutated kernels pass)
    for name, kw in mutants.items():
        sig, frames = _signals(_oracle(gold, tag, name=name, **kw), gold, tag)
        miss = np.abs(sig - want).max()
        print(f"{name}: signal off by {miss:.3g} = {miss / F32_TOL['signal']:.0f} tolerances")
        assert miss > 100 * F32_TOL["signal"], (name, miss)


# ---- sh_lgs.hpp in a stand-alone sanitized program --------------------------------------------------------------------------------------
def _build_driver(out_dir, sanitize):
    cxx = shutil.which("g++") or shutil.which("clang++") or "/opt/rocm/llvm/bin/clang++"
    exe = os.path.join(str(out_dir), "lgs_driver" + ("_san" if sanitize else ""))
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer"] if sanitize else ["-O2"]
    subprocess.run([cxx, *flags, "-std=c++17", "-Wall", "-Werror", f"-I{REPO}/rlao_amd/csrc",
                    os.path.join(REPO, "tests", "native", "lgs_driver.cpp"), "-o", exe], check=True, capture_output=True)
    return exe


@pytest.mark.parametrize("sanitize", [False, True])
def test_validation_and_plan_driver(tmp_path, sanitize):
    """tests/native/lgs_driver.cpp over rlao_amd/csrc/sh_lgs.hpp: the launch plan (4, 2 or 1 lenslets per workgroup within 64 KB of
    LDS, a plan for every lenslet size the generic spots kernel takes), the ascending pieces of a cyclic box, every refusal with
    where it was found; sanitize: the same program under ASan + UBSan, no report."""
    exe = _build_driver(tmp_path, sanitize)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    out = subprocess.run([exe, "plan"], capture_output=True, text=True, env=env)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "ERROR: AddressSanitizer" not in out.stderr and "runtime error" not in out.stderr, out.stderr
    lines = out.stdout.split("\n")
    assert lines[-2].split()[0] == "ok" and int(lines[-2].split()[1]) > 1000
    plan = {(int(a), int(b)): (int(c), int(d)) for a, b, c, d in (l.split() for l in lines[:-2])}
    assert plan[(6, 4)] == (4, 4 * (2 * 12 + 4 * (2 * (36 + 72) + 4 * 144)))         # the golden sizes: four lenslets per workgroup
    assert plan[(4, 8)][0] == 4 and plan[(8, 8)][0] == 4 and plan[(8, 4)][0] == 4
    assert plan[(12, 4)][0] == 4 and plan[(16, 4)][0] == 2 and plan[(10, 8)][0] == 2 and plan[(16, 8)][0] == 1 and plan[(18, 8)][0] == 1      # where the image outgrows four lenslets, it halves


# ---- the ABI ----------------------------------------------------------------------------------------------------------------------------
def test_abi_is_unchanged_and_the_exports_exist(tmp_path):
    prog = ['#include <stdio.h>', f'#include "{HEADER}"', "int main(void){",
            'printf("version %d\\n", (int)AOENV_ABI_VERSION);', 'printf("bufs %d\\n", (int)AOENV_B_COUNT);',
            'printf("kernels %d\\n", (int)AOENV_K_COUNT);',
            "int (*s)(AoEnv*, const double*, size_t, int, const int32_t*, void*) = aoenv_set_lgs_spots;",
            "int (*g)(AoEnv*, double*, int32_t*, int32_t*) = aoenv_get_lgs_spots;",
            'printf("decl %d\\n", s != 0 && g != 0);', "return 0;}"]
    src, obj = tmp_path / "lgs_abi.c", tmp_path / "lgs_abi.o"
    src.write_text("\n".join(prog))
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-c", "-o", str(obj), str(src)], check=True)      # the prototypes, as C99
    prog[6:9] = ['printf("decl 1\\n");']
    src.write_text("\n".join(prog))
    exe = tmp_path / "lgs_abi"
    subprocess.run(["gcc", "-std=c99", "-o", str(exe), str(src)], check=True)
    out = dict(l.split() for l in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(out["version"]) == 7 == L.ABI_VERSION and int(out["bufs"]) == 14 and int(out["kernels"]) == 13 == len(L.KERNEL_NAMES)
    hdr = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name in ("aoenv_set_lgs_spots", "aoenv_get_lgs_spots"):
        assert len(re.findall(rf"\b{name}\s*\(", hdr)) == 1 and name in L.EXPORTS
    lib = L.load()
    z = np.zeros(4)
    assert lib.aoenv_set_lgs_spots(None, z.ctypes.data, 32, 0, None, None) != 0 and b"null" in lib.aoenv_last_error()
    assert lib.aoenv_get_lgs_spots(None, None, None, None) != 0


# ---- the arguments -----------------------------------------------------------------------------------------------------------------------
def test_resolve_lgs():
    prof = G.na_profile()
    out = resolve_lgs(dict(Na_profile=prof.tolist(), FWHM_spot_up=0.3, laser_coordinates=(40, 0)))
    assert np.array_equal(out["Na_profile"], prof) and out["FWHM_spot_up"] == 0.3 and np.array_equal(out["laser_coordinates"], [40.0, 0.0])
    assert out["threshold_convolution"] == 0.05
    assert resolve_lgs(dict(Na_profile=torch.as_tensor(prof), FWHM_spot_up=1, threshold_convolution=0.1))["laser_coordinates"].tolist() == [0, 0]
    base = dict(Na_profile=prof, FWHM_spot_up=0.3, laser_coordinates=[40, 0])
    for bad in ([1, 2], dict(base, Na_profile=prof[0]), dict(base, Na_profile=np.ones((3, 5))), dict(base, Na_profile=-prof),
                dict(base, Na_profile=np.stack([prof[0], np.zeros(11)])), dict(base, Na_profile=np.full((2, 4), np.nan)),
                dict(base, FWHM_spot_up=-1), dict(base, FWHM_spot_up=[0.3, 0.4]), dict(base, FWHM_spot_up=np.inf),
                dict(base, laser_coordinates=[1, 2, 3]), dict(base, laser_coordinates=[np.nan, 0]), dict(base, threshold_convolution=1.0),
                dict(base, padding_extension_factor=2), dict(base, cone=True), dict(Na_profile=prof), dict(FWHM_spot_up=0.3)):
        with pytest.raises(ValueError):
            resolve_lgs(bad)
    assert resolve_lgs(dict(base, padding_extension_factor=1))["FWHM_spot_up"] == 0.3


def test_resolve_lgs_per_env():
    N = 4
    prof = G.na_profile()
    cur = dict(Na_profile=np.broadcast_to(prof, (N, 2, 11)).copy(), FWHM_spot_up=np.full(N, 0.3), laser_coordinates=np.tile([40.0, 0.0], (N, 1)))
    out = resolve_lgs_per_env(None, 0.5, None, None, N, cur)
    assert (out["FWHM_spot_up"] == 0.5).all() and np.array_equal(out["Na_profile"], cur["Na_profile"]) and (cur["FWHM_spot_up"] == 0.3).all()
    other = G.na_profile(skew=0.5)
    out = resolve_lgs_per_env(other, None, [[1.0, 2.0], [3.0, 4.0]], [3, 1], N, cur)
    assert np.array_equal(out["Na_profile"][3], other) and np.array_equal(out["Na_profile"][1], other) and np.array_equal(out["Na_profile"][0], prof)
    assert np.array_equal(out["laser_coordinates"], [[40, 0], [3, 4], [40, 0], [1, 2]])       # the caller's order
    out = resolve_lgs_per_env(np.stack([prof, other]), [0.3, 0.9], None, np.array([True, False, False, True]), N, cur)
    assert np.array_equal(out["Na_profile"][3], other) and np.array_equal(out["Na_profile"][1], prof)
    assert np.array_equal(out["FWHM_spot_up"], [0.3, 0.3, 0.3, 0.9])
    for args in ((None, None, None, None), (np.ones((2, 7)), None, None, None), (None, [0.3, 0.4], None, None), (None, 0.0, None, None),
                 (None, None, [1.0, 2.0, 3.0], None), (-prof, None, None, None), (None, np.nan, None, None), (None, 0.4, None, [7])):
        with pytest.raises(ValueError):
            resolve_lgs_per_env(*args[:3], args[3], N, cur)


class _StubShard:
    """Records what reaches the library."""

    def __init__(self):
        self.calls = []

    def set_lgs_spots(self, taps, box=None, per_env=False, stream=0):
        self.calls.append((None if taps is None else np.array(taps), None if box is None else np.array(box), per_env))


def _stub_env(tag="r24", lgs=True):
    R, ns, D, launch, fwhm = G.CASES[tag]
    env = BatchedAOEnv.__new__(BatchedAOEnv)
    env.param, env._sh_tables = _sht(tag)
    env.n_envs, env.wfs_type = 4, "sh"
    env.src_wavelength, env.nPhoton = calib.source(G.BAND, G.MAGNITUDE)
    env._shard, env._stream = _StubShard(), (lambda: 0)
    env._lgs = env._lgs_env = env._lgs_taps = None
    if lgs:
        env._lgs = resolve_lgs(dict(Na_profile=G.na_profile(), FWHM_spot_up=fwhm, laser_coordinates=launch))
        env._lgs_K, env._lgs_elongation = calib.lgs_spot_kernels(env.param, env._sh_tables, **env._lgs)
        env._lgs_taps = calib.lgs_binned_taps(env._lgs_K)
    env.source = env.ngs = _SourceProxy(env)
    env.wfs = object.__new__(_WfsProxy)
    env.wfs._e = env
    return env


def test_env_calls_on_a_stub_shard():
    env = _stub_env()
    calls = env._shard.calls
    assert env.ngs.type == "LGS" and env.wfs.is_LGS and abs(env.wfs.elungation_factor - 0.345) < 0.01
    assert abs(env.ngs.altitude - 90e3) < 1e-6 and env.ngs.Na_profile.shape == (2, 11) and env.ngs.FWHM_spot_up == 0.3
    assert np.array_equal(env.ngs.laser_coordinates, [40.0, 0.0])
    assert env.wfs.lgs_kernels().shape == (12, 12, 12) and env.wfs.lgs_kernels(per_env=True).shape == (4, 12, 12, 12)
    held = env.lgs
    assert not held["per_env"] and held["Na_profile"].shape == (4, 2, 11) and (held["FWHM_spot_up"] == 0.3).all()
    other = G.na_profile(skew=0.6)
    env.set_lgs_per_env(Na_profile=other, laser_coordinates=[0.0, 30.0], env_ids=[2])
    taps, box, per_env = calls[-1]
    assert per_env and taps.shape == (4, 12, 12, 12) and box.shape == (4,)
    cal = env._lgs_taps[0]
    assert np.array_equal(taps[0], cal) and np.array_equal(taps[1], cal) and np.array_equal(taps[3], cal)      # the others: the calibrated kernels
    p, sht = env.param, env._sh_tables
    want = calib.lgs_binned_taps(calib.lgs_spot_kernels(p, sht, other, 0.3, [0.0, 30.0])[0])[0]
    assert np.array_equal(taps[2], want) and not np.array_equal(want, cal)
    union = calib.lgs_binned_taps(np.stack([env._lgs_K, calib.lgs_spot_kernels(p, sht, other, 0.3, [0.0, 30.0])[0]]))[1]
    assert np.array_equal(box, union)                               # one box for the table: the union
    assert env.lgs["per_env"] and np.array_equal(env.lgs["laser_coordinates"][2], [0.0, 30.0]) and env.ngs.altitude.shape == (4,)
    assert np.array_equal(env.wfs.lgs_kernels(per_env=True)[2], calib.lgs_spot_kernels(p, sht, other, 0.3, [0.0, 30.0])[0])
    env.set_lgs_per_env(FWHM_spot_up=[0.3, 0.4, 0.5, 0.6])          # an argument left out stays as held
    assert np.array_equal(env.lgs["Na_profile"][2], other) and np.array_equal(env.lgs["FWHM_spot_up"], [0.3, 0.4, 0.5, 0.6])
    n = len(calls)
    for call in (lambda: env.set_lgs_per_env(), lambda: env.set_lgs_per_env(Na_profile=np.ones((2, 5))),
                 lambda: env.set_lgs_per_env(FWHM_spot_up=-0.1), lambda: env.set_lgs_per_env(FWHM_spot_up=0.3, env_ids=[9]),
                 lambda: env.set_lgs_per_env(laser_coordinates=[1.0])):
        with pytest.raises(ValueError):
            call()
    assert len(calls) == n and np.array_equal(env.lgs["FWHM_spot_up"], [0.3, 0.4, 0.5, 0.6])      # raised before anything was touched
    env.clear_lgs_per_env()
    taps, box, per_env = calls[-1]
    assert not per_env and np.array_equal(taps, cal) and np.array_equal(box, env._lgs_taps[1]) and not env.lgs["per_env"]
    assert np.isscalar(env.ngs.altitude) or np.ndim(env.ngs.altitude) == 0


def test_an_ngs_env_refuses_before_the_library_is_asked():
    env = _stub_env(lgs=False)
    assert env.ngs.type == "NGS" and not env.wfs.is_LGS and env.lgs is None and env.ngs.altitude == np.inf
    for call in (lambda: env.set_lgs_per_env(FWHM_spot_up=0.5), env.clear_lgs_per_env):
        with pytest.raises(ValueError, match="laser guide star"):
            call()
    for name in ("elungation_factor", "lgs_kernels"):
        with pytest.raises(AttributeError):
            getattr(env.wfs, name)() if name == "lgs_kernels" else getattr(env.wfs, name)
    with pytest.raises(AttributeError):
        env.ngs.Na_profile
    assert env._shard.calls == []


def test_set_params_refuses_before_anything_is_built():
    """a Pyramid, the geometric sensor and a malformed profile raise ValueError ahead of the first shard (no GPU is touched)"""
    lgs = dict(Na_profile=G.na_profile(), FWHM_spot_up=0.3, laser_coordinates=[40, 0])
    geo = dict(diameter=8.0, nSubaperture=4, nPixelPerSubap=6, opticalBand="Na")
    for kw in (dict(wfs_type="pyramid", lgs=lgs), dict(wfs_type="shackhartmann", lgs=lgs, is_geometric=True),
               dict(wfs_type="shackhartmann", lgs=dict(lgs, Na_profile=np.ones(11))),
               dict(wfs_type="shackhartmann", lgs=dict(lgs, padding_extension_factor=2))):
        env = BatchedAOEnv.__new__(BatchedAOEnv)
        env._lgs = env._lgs_env = env._lgs_taps = None
        with pytest.raises(ValueError):
            BatchedAOEnv.set_params(env, dict(geo), camera="ideal", **kw)
    assert calib.params_from_args(dict(geo, lgs=lgs)).lgs is lgs    # the parameter-file key


def test_the_wrap_warning_rule():
    p, sht = _sht("r24")
    wide = G.na_profile(width=80e3, sigma=20e3)
    assert calib.lgs_spot_kernels(p, sht, wide, 0.3, [40.0, 0.0])[1] > 1 > calib.lgs_spot_kernels(p, sht, G.na_profile(), 0.3, [40.0, 0.0])[1]
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        calib.lgs_spot_kernels(p, sht, wide, 0.3, [40.0, 0.0])      # (the env warns, the table function does not)


class _StubEnv:
    output = "torch"
    nActuator = 3
    n_envs = 4
    device = "cpu"
    tdtype = torch.float64
    lgs = "the guide stars"

    def __init__(self):
        self.calls = []
        self.param = type("P", (), {"nLoop": 50})()

    def set_lgs_per_env(self, Na_profile=None, FWHM_spot_up=None, laser_coordinates=None, env_ids=None):
        self.calls.append(("set", Na_profile, FWHM_spot_up, laser_coordinates, env_ids))

    def clear_lgs_per_env(self):
        self.calls.append(("clear",))


@pytest.mark.parametrize("wrap", [TorchWrapper, lambda e: TimeDelayEnv(e, 2), lambda e: HistoryEnv(e, n_history=3, delay=2)])
def test_wrappers_forward_the_calls(wrap):
    inner = _StubEnv()
    env = wrap(inner)
    env.set_lgs_per_env("prof", FWHM_spot_up=0.4, env_ids=[1])
    env.set_lgs_per_env(laser_coordinates=[1.0, 2.0])
    env.clear_lgs_per_env()
    assert inner.calls == [("set", "prof", 0.4, None, [1]), ("set", None, None, [1.0, 2.0], None), ("clear",)]
    assert env.lgs == "the guide stars"
    for name in ("set_lgs_per_env", "clear_lgs_per_env", "lgs"):
        assert name in type(env).__dict__, name                    # forwarded, not fallen through
