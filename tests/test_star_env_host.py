"""CPU: the host side of the per-env guide stars (aoenv_set_flux_env / aoenv_set_threshold_env; BatchedAOEnv.set_magnitude_per_env /
set_threshold_per_env).  ``calib.flux_scale`` against the ratio of two ``calib.source`` values and against the reference restated in
tests/_star_ref.py, the resolver of the arguments, the env methods and the reference's names on a stub shard, the wrappers, the
ABI, and the validation and factors (rlao_amd/csrc/star_env.hpp) in a stand-alone sanitized program.  No GPU."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import _star_ref as REF
from rlao_amd import _lib as L
from rlao_amd import calib
from rlao_amd.env import BatchedAOEnv, _SourceProxy, _WfsProxy, resolve_star_per_env
from rlao_amd.wrappers import HistoryEnv, TimeDelayEnv, TorchWrapper

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "aoenv.h")
N_ = 4


# ---- the flux ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("band", sorted(REF.PHOTOMETRY))
def test_flux_scale_against_the_photometry(band):
    """flux_scale(m, m_cal) against nPhoton(m) / nPhoton(m_cal) of calib.source and of the restatement (Source.py:104-109), to 1e-15
    relative: the quotient of the two powers of ten is two roundings from either (the zero point's product and the division)."""
    assert calib.PHOTOMETRY[band] == REF.PHOTOMETRY[band]
    worst = 0.0
    for m_cal in (0.0, 3.0, 8.0, 12.5):
        for m in np.concatenate([np.arange(3.0, 6.0, 0.5), [m_cal, m_cal - 2.5, m_cal + 1, m_cal + 4, -1.25, 17.0]]):
            got = float(calib.flux_scale(m, m_cal))
            a = calib.source(band, m)[1] / calib.source(band, m_cal)[1]
            b = REF.change_mag(band, m) / REF.n_photon(band, m_cal)
            worst = max(worst, abs(got / a - 1), abs(got / b - 1))
            assert abs(got / a - 1) <= 1e-15 and abs(got / b - 1) <= 1e-15, (band, m, m_cal, got, a, b)
            assert abs(np.sqrt(got) / REF.amplitude_factor(band, m, m_cal) - 1) <= 1e-15
        assert calib.flux_scale(m_cal, m_cal) == 1.0                # exactly
    print(f"{band}: largest relative difference {worst:.2e}")
    s = calib.flux_scale(np.array([8.0, 5.5, 9.0, 12.0]), 8.0)
    assert s.shape == (4,) and s.dtype == np.float64 and s[0] == 1.0 and abs(s[1] / 10 - 1) < 1e-15 and s[3] < s[2] < 1 < s[1]
    # fluxMap is linear in nPhoton (Source.py:151): its ratio is the scale, whatever the other factors
    f = [REF.flux_map(band, m, 0.9, 2e-3, 8.0, 120) for m in (8.0, 9.5)]
    assert abs(f[1] / f[0] / float(calib.flux_scale(9.5, 8.0)) - 1) <= 1e-15


def test_the_threshold_of_the_restatement():
    """ShackHartmann.py:314-324: the cut is relative to the maximum over ALL spots; a higher threshold removes more."""
    rs = np.random.RandomState(2)
    im = rs.uniform(0, 1, (5, 6, 6)) ** 4
    im[2] *= 10
    c0, c2 = REF.centroid(im, 0.0), REF.centroid(im, 0.2)
    assert np.isfinite(c0).all() and not np.allclose(c0, c2)
    cut = 0.2 * im.max()
    kept = np.where(im < cut, 0, im)
    with np.errstate(invalid="ignore"):
        want = np.array([[(k.sum(1) * np.arange(6)).sum() / k.sum(), (k.sum(0) * np.arange(6)).sum() / k.sum()] for k in kept])
    assert np.allclose(c2[np.isfinite(c2).all(1)], want[np.isfinite(want).all(1)], rtol=1e-14, atol=0)
    assert np.array_equal(REF.centroid(3.7 * im, 0.2)[2], c2[2]) or np.allclose(REF.centroid(3.7 * im, 0.2)[2], c2[2], rtol=1e-14)   # flux invariant


# ---- the arguments -------------------------------------------------------------------------------------------------------------
def test_resolver_scalars_arrays_and_env_ids():
    cur = np.full(N_, 8.0)
    m = resolve_star_per_env("magnitude", 9.5, None, N_, cur)
    assert m.shape == (N_,) and m.dtype == np.float64 and (m == 9.5).all() and (cur == 8.0).all()     # `current` is not written
    m = resolve_star_per_env("magnitude", [8.0, 5.5, 9.0, 12.0], None, N_, cur)
    assert np.array_equal(m, [8.0, 5.5, 9.0, 12.0])
    part = resolve_star_per_env("magnitude", [3.0, 4.0], [3, 1], N_, m)
    assert np.array_equal(part, [8.0, 4.0, 9.0, 3.0]) and m[1] == 5.5                                  # the caller's order
    mask = resolve_star_per_env("magnitude", torch.tensor([1.0, 2.0]), np.array([True, False, False, True]), N_, part)
    assert np.array_equal(mask, [1.0, 4.0, 9.0, 2.0])
    one = resolve_star_per_env("magnitude", -1.5, [2], N_, cur)                                        # any finite magnitude
    assert np.array_equal(one, [8.0, 8.0, -1.5, 8.0])
    t = resolve_star_per_env("threshold", [0.0, 0.05], [0, 2], N_, np.full(N_, 0.01))
    assert np.array_equal(t, [0.0, 0.01, 0.05, 0.01])
    t = resolve_star_per_env("threshold", np.float32(0.2), None, N_, np.full(N_, 0.01))
    assert (t == np.float64(np.float32(0.2))).all()


@pytest.mark.parametrize("kind, kw, what", [
    ("magnitude", dict(value=[8.0, 9.0]), "shape"), ("magnitude", dict(value=np.zeros((N_, 1))), "shape"),
    ("magnitude", dict(value=np.zeros(N_), env_ids=[0, 1]), "shape"), ("magnitude", dict(value=np.nan), "finite"),
    ("magnitude", dict(value=[8.0, np.inf, 8.0, 8.0]), "finite"), ("magnitude", dict(value="abc"), "numeric"),
    ("threshold", dict(value=-0.01), "below 0"), ("threshold", dict(value=[0.0, 0.1, -1e-9, 0.0]), "below 0"),
    ("threshold", dict(value=np.nan), "finite"), ("threshold", dict(value=[0.1], env_ids=[4]), "outside"),
    ("magnitude", dict(value=[1.0, 2.0], env_ids=[1, 1]), "twice"), ("nPhoton", dict(value=1.0), "unknown")])
def test_resolver_bad_arguments_raise(kind, kw, what):
    with pytest.raises(ValueError, match=what):
        resolve_star_per_env(kind, kw["value"], kw.get("env_ids"), N_, np.full(N_, 8.0 if kind != "threshold" else 0.01))


class _StubShard:
    """Records what reaches the library."""

    def __init__(self):
        self.calls = []

    def set_flux_env(self, scale, stream=0):
        self.calls.append(("flux", None if scale is None else np.array(scale)))

    def set_threshold_env(self, thr, stream=0):
        self.calls.append(("thr", None if thr is None else np.array(thr)))


def _stub_env(wfs_type="sh", **kw):
    env = BatchedAOEnv.__new__(BatchedAOEnv)
    env.param = calib.params_from_args(None, diameter=3.2, nSubaperture=8, nPixelPerSubap=6, **kw)
    env.n_envs, env.wfs_type = N_, wfs_type
    env.src_wavelength, env.nPhoton = calib.source(env.param.opticalBand, env.param.magnitude)
    env._shard, env._mag_env, env._thr_env = _StubShard(), None, None
    env._stream = lambda: 0
    env.source = env.ngs = _SourceProxy(env)
    env.wfs = object.__new__(_WfsProxy)
    env.wfs._e = env
    return env


def test_env_calls_on_a_stub_shard():
    env = _stub_env(magnitude=7.0, threshold_cog=0.02)
    calls = env._shard.calls
    assert np.array_equal(env.magnitude, np.full(N_, 7.0)) and np.array_equal(env.threshold_cog, np.full(N_, 0.02))   # off: the calibrated values
    mags = np.array([7.0, 4.5, 8.0, 11.0])
    env.set_magnitude_per_env(mags)
    assert calls[-1][0] == "flux" and np.array_equal(calls[-1][1], calib.flux_scale(mags, 7.0)) and calls[-1][1][0] == 1.0
    assert abs(calls[-1][1][1] / 10 - 1) < 1e-15
    env.set_magnitude_per_env(9.0, env_ids=[2])                     # the others keep theirs
    assert np.array_equal(env.magnitude, [7.0, 4.5, 9.0, 11.0]) and np.array_equal(calls[-1][1], calib.flux_scale([7.0, 4.5, 9.0, 11.0], 7.0))
    env.set_threshold_per_env([0.02, 0.0, 0.05, 0.2])
    assert calls[-1][0] == "thr" and np.array_equal(calls[-1][1], [0.02, 0.0, 0.05, 0.2])
    env.set_threshold_per_env(0.1, env_ids=np.array([False, True, False, False]))
    assert np.array_equal(env.threshold_cog, [0.02, 0.1, 0.05, 0.2])
    got = env.magnitude
    got[0] = 99.0
    assert env.magnitude[0] == 7.0                                 # a copy
    # bad arguments raise before anything is touched
    n = len(calls)
    for call in (lambda: env.set_magnitude_per_env([1.0, 2.0]), lambda: env.set_magnitude_per_env(np.nan),
                 lambda: env.set_threshold_per_env(-0.1), lambda: env.set_threshold_per_env([0.0, 0.1]),
                 lambda: env.set_magnitude_per_env(8.0, env_ids=[7]), lambda: setattr(env.source, "nPhoton", -1.0)):
        with pytest.raises(ValueError):
            call()
    assert len(calls) == n and np.array_equal(env.magnitude, [7.0, 4.5, 9.0, 11.0]) and np.array_equal(env.threshold_cog, [0.02, 0.1, 0.05, 0.2])
    # the reference's names
    env.change_mag(5.0)                                            # OOPAOEnvRazor.py:644-647
    assert (env.magnitude == 5.0).all() and np.allclose(calls[-1][1], 10 ** 0.8, rtol=1e-15)
    assert np.allclose(env.source.nPhoton, REF.change_mag("I", 5.0), rtol=1e-15) and env.ngs is env.source
    assert env.source.zeroPoint == REF.zero_point("I") and (env.source.magnitude == 5.0).all()
    env.wfs.threshold_cog = 0.07                                   # integrator_threshold.py: env.wfs.threshold_cog = t
    assert calls[-1][0] == "thr" and (calls[-1][1] == 0.07).all() and (env.wfs.threshold_cog == 0.07).all()
    env.wfs.threshold_cog = np.array([0.0, 0.01, 0.02, 0.03])
    assert np.array_equal(env.threshold_cog, [0.0, 0.01, 0.02, 0.03])
    env.source.magnitude = [6.0, 7.0, 8.0, 9.0]
    assert np.array_equal(env.magnitude, [6.0, 7.0, 8.0, 9.0])
    env.source.nPhoton = REF.n_photon("I", 7.5)
    assert np.allclose(env.magnitude, 7.5, rtol=0, atol=1e-13)
    with pytest.raises(AttributeError):
        env.source.wavelength = 1e-6
    env.clear_star_per_env()
    assert calls[-2:] == [("flux", None), ("thr", None)]
    assert np.array_equal(env.magnitude, np.full(N_, 7.0)) and np.array_equal(env.threshold_cog, np.full(N_, 0.02))


def test_a_pyramid_env_refuses_a_threshold_before_the_library_is_asked():
    env = _stub_env(wfs_type="pyr")
    with pytest.raises(ValueError, match="centre of gravity"):
        env.set_threshold_per_env(0.05)
    assert env._shard.calls == []
    env.set_magnitude_per_env([8.0, 9.0, 10.0, 11.0])              # the flux is fine
    assert env._shard.calls[-1][0] == "flux"


class _StubEnv:
    output = "torch"
    nActuator = 3
    n_envs = 4
    device = "cpu"
    tdtype = torch.float64
    magnitude = "the magnitudes"
    threshold_cog = "the thresholds"

    def __init__(self):
        self.calls = []
        self.param = type("P", (), {"nLoop": 50})()

    def set_magnitude_per_env(self, mag, env_ids=None):
        self.calls.append(("mag", mag, env_ids))

    def set_threshold_per_env(self, thr, env_ids=None):
        self.calls.append(("thr", thr, env_ids))

    def clear_star_per_env(self):
        self.calls.append(("clear",))

    def change_mag(self, mag):
        self.calls.append(("change_mag", mag))


@pytest.mark.parametrize("wrap", [TorchWrapper, lambda e: TimeDelayEnv(e, 2), lambda e: HistoryEnv(e, n_history=3, delay=2)])
def test_wrappers_forward_the_calls(wrap):
    inner = _StubEnv()
    env = wrap(inner)
    env.set_magnitude_per_env([1.0], env_ids=[1])
    env.set_threshold_per_env(0.05)
    env.change_mag(4.0)
    env.clear_star_per_env()
    assert inner.calls == [("mag", [1.0], [1]), ("thr", 0.05, None), ("change_mag", 4.0), ("clear",)]
    assert env.magnitude == "the magnitudes" and env.threshold_cog == "the thresholds"
    for name in ("set_magnitude_per_env", "set_threshold_per_env", "clear_star_per_env", "change_mag", "magnitude", "threshold_cog"):
        assert name in type(env).__dict__, name                    # forwarded, not fallen through


# ---- the ABI -------------------------------------------------------------------------------------------------------------------
def test_abi_is_unchanged_and_the_exports_exist(tmp_path):
    prog = ['#include <stdio.h>', f'#include "{HEADER}"', "int main(void){",
            'printf("version %d\\n", (int)AOENV_ABI_VERSION);', 'printf("bufs %d\\n", (int)AOENV_B_COUNT);',
            'printf("kernels %d\\n", (int)AOENV_K_COUNT);',
            "int (*s)(AoEnv*, const double*, void*) = aoenv_set_flux_env;", "int (*g)(AoEnv*, double*, void*) = aoenv_get_flux_env;",
            "int (*t)(AoEnv*, const double*, void*) = aoenv_set_threshold_env;", "int (*u)(AoEnv*, double*, void*) = aoenv_get_threshold_env;",
            'printf("decl %d\\n", s != 0 && g != 0 && t != 0 && u != 0);', "return 0;}"]
    src, obj = tmp_path / "star_env_abi.c", tmp_path / "star_env_abi.o"
    src.write_text("\n".join(prog))
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-c", "-o", str(obj), str(src)], check=True)      # the prototypes, as C99
    prog[6:11] = ['printf("decl 1\\n");']
    src.write_text("\n".join(prog))
    exe = tmp_path / "star_env_abi"
    subprocess.run(["gcc", "-std=c99", "-o", str(exe), str(src)], check=True)
    out = dict(l.split() for l in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(out["version"]) == 7 == L.ABI_VERSION and int(out["bufs"]) == 14 and int(out["kernels"]) == 13 == len(L.KERNEL_NAMES)
    text = open(HEADER).read()
    hdr = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    names = ("aoenv_set_flux_env", "aoenv_get_flux_env", "aoenv_set_threshold_env", "aoenv_get_threshold_env")
    for name in names:
        assert re.search(r"\b%s\s*\(" % name, hdr) and name in L.EXPORTS
    assert "OOPAOEnvRazor.py:644-647" in text and "integrator_threshold.py:34-106" in text and "aoenv_compute_psf keeps the calibrated star" in text
    lib = L.load()                                                 # (declares every export: a missing symbol raises here)
    z = np.ones(4)
    for name in names:
        assert getattr(lib, name)(None, z.ctypes.data, None) != 0 and b"null" in lib.aoenv_last_error()


# ---- validation and factors, in a stand-alone sanitized program -------------------------------------------------------------------
def _build_driver(out_dir, sanitize):
    cxx = shutil.which("g++") or shutil.which("clang++") or "/opt/rocm/llvm/bin/clang++"
    exe = os.path.join(str(out_dir), "star_env_driver" + ("_san" if sanitize else ""))
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer"] if sanitize else ["-O2"]
    subprocess.run([cxx, *flags, "-std=c++17", "-Wall", "-Werror", f"-I{REPO}/rlao_amd/csrc",
                    os.path.join(REPO, "tests", "native", "star_env_driver.cpp"), "-o", exe], check=True, capture_output=True)
    return exe


@pytest.mark.parametrize("sanitize", [False, True])
def test_validation_and_factors_driver(tmp_path, sanitize):
    """tests/native/star_env_driver.cpp over rlao_amd/csrc/star_env.hpp, the header the library validates and converts with: scale
    1 -> exactly 1, the factors and thresholds in float and double, every refusal with its index; sanitize: the same program under
    ASan + UBSan, no report."""
    exe = _build_driver(tmp_path, sanitize)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    out = subprocess.run([exe], capture_output=True, text=True, env=env)
    assert out.returncode == 0, out.stderr
    assert "ERROR: AddressSanitizer" not in out.stderr and "runtime error" not in out.stderr, out.stderr
    assert out.stdout.split()[0] == "ok" and int(out.stdout.split()[1]) > 200
