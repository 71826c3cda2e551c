"""Shared by tests/test_explore_host.py (CPU) and tests/test_gpu_rollout.py (GPU): the host driver of the exploration noise
stream (tests/native/explore_driver.cpp over rlao_amd/csrc/explore.hpp), a NumPy restatement of the stream, and the law bounds both
tests hold the normals to."""
import math
import os
import shutil
import subprocess

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 20240607                                                    # the fixed seed of the law tests (host and device)
PURPOSE = 0x45585031                                               # kExplorePurpose
# |driver - float64 restatement| and |device - driver|: 2 pi u in float32 has an ulp of 4.8e-7 near 6.28; times r <= 5.77 that
# is 3e-6; logf and sqrtf add a few ulp of r; 2e-5 is about 6 x the sum
STREAM_ATOL = 2e-5


def build_driver(out_dir, sanitize=False):
    """Compiles the driver for the host; None when there is no hipcc."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        return None
    exe = os.path.join(str(out_dir), "explore_driver" + ("_san" if sanitize else ""))
    flags = ["-O1", "-g", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-omit-frame-pointer"] if sanitize else ["-O2"]
    subprocess.run([hipcc, *flags, "-std=c++17", "-x", "hip", "--cuda-host-only", f"-I{REPO}/include", f"-I{REPO}/rlao_amd/csrc",
                    os.path.join(REPO, "tests", "native", "explore_driver.cpp"), "-o", exe], check=True, capture_output=True)
    return exe


def host_normals(exe, seed, env0, n_env, c0, n_c, A, env=None):
    """float32 z[n_env][n_c][A] of the host driver"""
    out = subprocess.run([exe, str(seed), str(env0), str(n_env), str(c0), str(n_c), str(A)], check=True, capture_output=True, env=env)
    z = np.frombuffer(out.stdout, dtype=np.float32)
    assert z.size == n_env * n_c * A, (z.size, out.stderr)
    return z.reshape(n_env, n_c, A).copy(), out.stderr.decode("utf-8", "replace")


def philox4x32_7(c0, c1, c2, c3, seed):
    """Philox4x32-7 in uint64 arithmetic: the four output words (uint64 arrays holding 32-bit values) of the counters c0 .. c3
    (broadcast against each other) under the 64-bit key `seed`.  The one copy of the round function: the exploration stream below
    and the camera streams of tests/_camera_ref.py both draw from it."""
    M = np.uint64(0xFFFFFFFF)
    x = [np.ascontiguousarray(a) & M for a in np.broadcast_arrays(*(np.asarray(c, dtype=np.uint64) for c in (c0, c1, c2, c3)))]
    seed = int(seed)
    k0, k1 = np.uint64(seed & 0xFFFFFFFF), np.uint64((seed >> 32) & 0xFFFFFFFF)
    for _ in range(7):
        p0, p1 = np.uint64(0xD2511F53) * x[0], np.uint64(0xCD9E8D57) * x[2]
        x = [(p1 >> np.uint64(32)) ^ x[1] ^ k0, p1 & M, (p0 >> np.uint64(32)) ^ x[3] ^ k1, p0 & M]
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & M, (k1 + np.uint64(0xBB67AE85)) & M
    return x


def numpy_normals(seed, env0, n_env, c0, n_c, A):
    """The stream restated: Philox4x32-7 in uint64 arithmetic, Box-Muller in float64.  z[n_env][n_c][A] float64."""
    nq = (A + 3) // 4
    q, e, c = np.meshgrid(np.arange(nq, dtype=np.uint64), np.arange(env0, env0 + n_env, dtype=np.uint64),
                          np.arange(c0, c0 + n_c, dtype=np.uint64), indexing="ij")
    x = philox4x32_7(q.ravel(), e.ravel(), c.ravel(), PURPOSE, seed)
    u = [((w >> np.uint64(9)).astype(np.float64) + 0.5) / 8388608.0 for w in x]
    z = np.empty((4, q.size))
    for h in range(2):
        r, t = np.sqrt(-2.0 * np.log(u[2 * h])), 2.0 * np.pi * u[2 * h + 1]
        z[2 * h], z[2 * h + 1] = r * np.cos(t), r * np.sin(t)
    z = z.reshape(4, nq, n_env, n_c).transpose(2, 3, 1, 0).reshape(n_env, n_c, 4 * nq)
    return z[..., :A]


def law_figures(z):
    """z [n_env][n_c][A] -> the figures of the law test and their bounds, as {name: (value, bound)}"""
    z = np.asarray(z, dtype=np.float64)
    n = z.size
    v = z.ravel()
    m, var = v.mean(), v.var()
    kurt = ((v - m) ** 4).mean() / var ** 2 - 3.0
    s = np.sort(v)
    cdf = 0.5 * (1.0 + np.array([math.erf(t) for t in s / math.sqrt(2.0)]))
    i = np.arange(1, n + 1)
    ks = max(np.abs(i / n - cdf).max(), np.abs(cdf - (i - 1) / n).max())
    out = {"mean": (abs(m), 4 / math.sqrt(n)), "var": (abs(var - 1), 4 * math.sqrt(2 / n)),
           "kurtosis": (abs(kurt), 4 * math.sqrt(24 / n)), "kolmogorov": (ks, 1.95 / math.sqrt(n))}
    zc = (z - m) / math.sqrt(var)
    for name, ax in (("lag1_env", 0), ("lag1_counter", 1), ("lag1_actuator", 2)):
        a, b = np.take(zc, range(0, z.shape[ax] - 1), axis=ax), np.take(zc, range(1, z.shape[ax]), axis=ax)
        out[name] = (abs((a * b).mean()), 4 / math.sqrt(n))
    return out


def assert_law(z, label):
    figs = law_figures(z)
    print(label, {k: (float(f"{v:.3e}"), float(f"{b:.3e}")) for k, (v, b) in figs.items()})
    for name, (v, b) in figs.items():
        assert v < b, (label, name, v, b)
