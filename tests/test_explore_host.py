"""CPU: the exploration noise stream of the on-device rollout (rlao_amd/csrc/explore.hpp, ONE host/device source for
k_rollout_action and the driver tests/native/explore_driver.cpp) and the ABI that goes with it (AoRollout, aoenv_run_rollout,
aoenv_set_noise_filter).  The stream is pinned against a NumPy restatement, its law against N(0, 1); the driver is also run under
ASan + UBSan as a stand-alone host program."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import _explore_ref as X

REPO = X.REPO
HEADER = os.path.join(REPO, "include", "aoenv.h")


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = X.build_driver(tmp_path_factory.mktemp("explore"))
    if exe is None:
        pytest.skip("hipcc not available")
    return exe


@pytest.mark.parametrize("seed,env0,n_env,c0,n_c,A", [(1, 0, 3, 0, 4, 69), (0xDEADBEEF12345678, 4094, 4, 4294967290, 5, 7),
                                                      (X.SEED, 17, 2, 100, 3, 316)])
def test_stream_is_pinned_by_a_numpy_restatement(driver, seed, env0, n_env, c0, n_c, A):
    """Philox4x32-7 in uint64 arithmetic and Box-Muller in float64 against the float32 driver (A not a multiple of 4, a 64-bit seed,
    env index and counter near their wrap).  Tolerance: X.STREAM_ATOL, derived there."""
    z, _ = X.host_normals(driver, seed, env0, n_env, c0, n_c, A)
    want = X.numpy_normals(seed, env0, n_env, c0, n_c, A)
    assert np.isfinite(z).all() and np.abs(z).max() <= np.sqrt(48 * np.log(2)) + 1e-5
    err = np.abs(z - want).max()
    print("max |driver - numpy| =", err)
    assert err <= X.STREAM_ATOL
    # a quad is a function of (q, env, counter) alone: a shorter vector is a prefix, another env offset a shifted block
    z2, _ = X.host_normals(driver, seed, env0 + 1, n_env - 1, c0, n_c, max(A - 5, 1))
    assert np.array_equal(z2, z[1:, :, :max(A - 5, 1)])


def test_law_of_the_normals(driver):
    """64 envs x 64 steps x 64 actuators = 2^18 normals of the fixed seed: mean, variance, excess kurtosis, Kolmogorov distance to
    Phi and the lag-1 correlations along the actuator, env and counter axes, each inside the bound of a 4-sigma (Kolmogorov: 1.95 /
    sqrt(n), the 0.1 % point) fluctuation of n independent N(0, 1) draws."""
    z, _ = X.host_normals(driver, X.SEED, 0, 64, 0, 64, 64)
    assert z.size >= 2 ** 18
    X.assert_law(z, "host")


def test_rollout_struct_matches_header(tmp_path):
    from rlao_amd import _lib as L
    st = L.AoRollout
    prog = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', "int main(void){",
            'printf("size %zu\\n", sizeof(AoRollout));']
    prog += [f'printf("{f[0]} %zu\\n", offsetof(AoRollout, {f[0]}));' for f in st._fields_]
    prog += ['printf("abi %d\\n", (int)AOENV_ABI_VERSION);', "return 0;}"]
    src, exe = tmp_path / "rollout_layout.c", tmp_path / "rollout_layout"
    src.write_text("\n".join(prog))
    subprocess.run(["gcc", "-std=c99", "-o", str(exe), str(src)], check=True)
    out = dict(l.split() for l in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(out["size"]) == C.sizeof(st)
    for f in st._fields_:
        assert int(out[f[0]]) == getattr(st, f[0]).offset, f[0]
    assert int(out["abi"]) == L.ABI_VERSION == 7                   # additive: the ABI version stays


def test_new_exports_in_header_library_and_ctypes():
    sys.path.insert(0, REPO)
    import __graft_entry__ as g
    g.build()
    from rlao_amd import _lib as L
    lib = L.load()
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name in ("aoenv_run_rollout", "aoenv_set_noise_filter"):
        assert re.search(rf"\b{name}\s*\(", src), name
        assert name in L.EXPORTS and hasattr(lib, name), name
    # without a device (or with a null env) the calls report an error instead of crashing
    assert lib.aoenv_run_rollout(None, None, None, None, None, None, None, None) != 0
    assert lib.aoenv_set_noise_filter(None, None, 0, None) != 0
    assert len(lib.aoenv_last_error()) > 0


def test_driver_is_clean_under_asan_and_ubsan(tmp_path):
    """The host instantiation of explore.hpp in a stand-alone sanitized program: no report, and the same normals."""
    exe = X.build_driver(tmp_path, sanitize=True)
    if exe is None:
        pytest.skip("hipcc not available")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    z, err = X.host_normals(exe, X.SEED, 3, 2, 4294967295, 3, 69, env=env)
    assert "ERROR: AddressSanitizer" not in err and "runtime error" not in err, err
    np.testing.assert_allclose(z, X.numpy_normals(X.SEED, 3, 2, 4294967295, 3, 69), atol=X.STREAM_ATOL, rtol=0)
