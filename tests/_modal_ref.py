"""Shared by tests/test_modal_host.py (CPU) and tests/test_gpu_modal.py (GPU): the host driver of the modal surface's model
(tests/native/modal_driver.cpp over rlao_amd/csrc/modal.hpp) and the model restated in exact integer arithmetic."""
import math
import os
import shutil
import subprocess

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DT = {"f32": np.float32, "f64": np.float64}


def build_driver(out_dir, sanitize=False):
    """Compiles the driver for the host; None when there is no hipcc."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        return None
    exe = os.path.join(str(out_dir), "modal_driver" + ("_san" if sanitize else ""))
    flags = ["-O1", "-g", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-omit-frame-pointer"] if sanitize else ["-O2"]
    subprocess.run([hipcc, *flags, "-std=c++17", "-x", "hip", "--cuda-host-only", f"-I{REPO}/include", f"-I{REPO}/rlao_amd/csrc",
                    os.path.join(REPO, "tests", "native", "modal_driver.cpp"), "-o", exe], check=True, capture_output=True)
    return exe


def _run(exe, what, dtype, K, N, E, arrays, env=None):
    t = DT[dtype]
    blob = b"".join(np.ascontiguousarray(a, dtype=t).tobytes() for a in arrays)
    out = subprocess.run([exe, what, dtype, str(K), str(N), str(E)], input=blob, check=True, capture_output=True, env=env)
    return out.stdout, out.stderr.decode("utf-8", "replace")


def host_expand(exe, dtype, m2c, a, gain=None, env=None):
    """v[E][A] of the driver in the env dtype: m2c [A][K] (as handed to set_modal), a [E][K] coefficients, or with ``gain`` [E][K]
    the previous observation the gains multiply.  Returns (v, stderr)."""
    t = DT[dtype]
    m2c, a = np.asarray(m2c).astype(t), np.asarray(a).astype(t)
    A, K = m2c.shape
    E = a.shape[0]
    arrays = [m2c.T, a] + ([np.broadcast_to(np.asarray(gain).astype(t), a.shape)] if gain is not None else [])
    raw, err = _run(exe, "expandg" if gain is not None else "expand", dtype, K, A, E, arrays, env)
    v = np.frombuffer(raw, dtype=t)
    assert v.size == E * A, (v.size, err)
    return v.reshape(E, A).copy(), err


def host_project(exe, dtype, cm, signal, env=None):
    """(o [E][K] in the env dtype, reward [E] float64, stderr) of the driver: the fixed order of k_modal_obs"""
    t = DT[dtype]
    cm, signal = np.asarray(cm).astype(t), np.asarray(signal).astype(t)
    K, S = cm.shape
    E = signal.shape[0]
    raw, err = _run(exe, "project", dtype, K, S, E, [cm, signal], env)
    n = E * K * np.dtype(t).itemsize
    assert len(raw) == n + 8 * E, (len(raw), err)
    return np.frombuffer(raw[:n], dtype=t).reshape(E, K).copy(), np.frombuffer(raw[n:], dtype=np.float64).copy(), err


BITS = {"f32": 24, "f64": 53}


def _split(x):
    """a finite float as (integer mantissa, exponent): x == m * 2**e exactly"""
    m, e = math.frexp(float(x))
    return int(m * (1 << 53)), e - 53


def fma_exact(a, b, c, dtype):
    """a * b + c rounded ONCE to ``dtype`` (nearest, ties to even), the rounding of a hardware fma: integer arithmetic, so that
    neither float64 nor float32 is rounded twice.  (Results in the subnormal range are not handled: the tests have none.)"""
    (ma, ea), (mb, eb), (mc, ec) = _split(a), _split(b), _split(c)
    e = min(ea + eb, ec)
    s = ((ma * mb) << (ea + eb - e)) + (mc << (ec - e))
    neg, s = s < 0, abs(s)
    drop = s.bit_length() - BITS[dtype]
    if drop > 0:
        q, rem, half = s >> drop, s & ((1 << drop) - 1), 1 << (drop - 1)
        if rem > half or (rem == half and (q & 1)):
            q += 1
        s, e = q, e + drop
    v = math.ldexp(float(s), e)                                     # exact: s has at most BITS[dtype] (+ 1 on a carry) bits
    return DT[dtype](-v if neg else v)


def exact_expand(dtype, m2c, a):
    """The fma chain of modal.hpp in exact arithmetic, one rounding per step: v[E][A] in the env dtype.  m2c [A][K], a [E][K]"""
    t = DT[dtype]
    m2c, a = np.asarray(m2c).astype(t), np.asarray(a).astype(t)
    A, K = m2c.shape
    out = np.zeros((a.shape[0], A), dtype=t)
    rows, cols = m2c.tolist(), a.tolist()
    for e in range(a.shape[0]):
        for k in range(A):
            v = 0.0
            for m in range(K):
                v = float(fma_exact(rows[k][m], cols[e][m], v, dtype))
            out[e, k] = v
    return out


def exact_project(dtype, cm, signal):
    """The projection and the reward in the fixed order of modal.hpp ("lane-strided, then the tree"), restated without the header:
    lane l of 64 chains the terms l, l + 64, ... by fma from 0 (one rounding each, ``fma_exact``), the 64 partial sums fold by
    p[l] += p[l + off], off = 32 .. 1, o = (T)(-1e6) * p[0]; the reward the same way over (double)o^2 in float64.
    cm [K][S], signal [E][S] -> (o [E][K] in the env dtype, reward [E] float64)"""
    t = DT[dtype]
    cm, signal = np.asarray(cm).astype(t), np.asarray(signal).astype(t)
    K, S = cm.shape
    rows, sig = cm.tolist(), signal.tolist()

    def tree(p):
        off = 32
        while off:
            p[:off] = p[:off] + p[off:2 * off]                       # elementwise in the array's dtype: one rounding per add
            off //= 2
        return p[0]

    o = np.zeros((signal.shape[0], K), dtype=t)
    r = np.zeros(signal.shape[0])
    for e in range(signal.shape[0]):
        for m in range(K):
            p = np.zeros(64, dtype=t)
            for lane in range(min(64, S)):
                v = 0.0
                for j in range(lane, S, 64):
                    v = float(fma_exact(rows[m][j], sig[e][j], v, dtype))
                p[lane] = v
            o[e, m] = t(-1e6) * tree(p)
        q = np.zeros(64)
        for lane in range(min(64, K)):
            v = np.float64(0.0)
            for m in range(lane, K, 64):
                v = v + np.float64(o[e, m]) * np.float64(o[e, m])
            q[lane] = v
        r[e] = -tree(q)
    return o, r


def emulated_expand_f32(m2c, a):
    """The float32 chain emulated in NumPy float64: the product of two float32 values is exact in float64, the sum is rounded to
    float64 and then to float32 -- two roundings where the fma makes one.  v[E][A] float32"""
    m2c, a = np.asarray(m2c).astype(np.float32).astype(np.float64), np.asarray(a).astype(np.float32).astype(np.float64)
    v = np.zeros((a.shape[0], m2c.shape[0]), dtype=np.float32)
    for m in range(m2c.shape[1]):
        v = (a[:, m:m + 1] * m2c[None, :, m] + v.astype(np.float64)).astype(np.float32)
    return v


def to_image(v, act_idx, n_act):
    """vec_to_img: v [E][A] onto [E][n_act][n_act], zeros elsewhere"""
    img = np.zeros((v.shape[0], n_act * n_act), dtype=v.dtype)
    img[:, np.asarray(act_idx)] = v
    return img.reshape(v.shape[0], n_act, n_act)


def projection_bound(dtype, cm, signal, n_signal=None):
    """|o - o64| <= 1e6 (n_signal + 4) u sum_j |cm[m][j]| |signal[e][j]|, u = 2^-24 / 2^-53: the bound of any summation order, the
    +4 for rounding cm to the env dtype and the scale.  cm [K][S], signal [E][S] (float64) -> [E][K]"""
    u = 2.0 ** -24 if dtype == "f32" else 2.0 ** -53
    S = cm.shape[1] if n_signal is None else n_signal
    return 1e6 * (S + 4) * u * (np.abs(np.asarray(signal, dtype=np.float64)) @ np.abs(np.asarray(cm, dtype=np.float64)).T)
