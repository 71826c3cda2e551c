"""Shared by tests/test_wavefront_host.py (CPU) and tests/test_gpu_wavefront.py (GPU): the host driver of the wavefront read-out's
model (tests/native/wavefront_driver.cpp over rlao_amd/csrc/wavefront.hpp) and the model restated in NumPy without the header --
the scatter of opd2m [K][P] into the padded full-grid table, the slice plan, the refusals, the general kernel's order of the sum and
the bound of any order."""
import os
import shutil
import subprocess

import numpy as np

from _modal_ref import fma_exact

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DT = {"f32": np.float32, "f64": np.float64}
MAX_MODES, MAX_SLICES, ROUND = 1024, 64, 16
# enum WfRefusal of wavefront.hpp
OK, BAD_MODES, BAD_PIX, NO_PUPIL, PUPIL_COUNT, NULL_TABLE, NOT_FINITE = range(7)


def build_driver(out_dir, sanitize=False):
    """Compiles the driver for the host; None when there is no hipcc."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        return None
    exe = os.path.join(str(out_dir), "wavefront_driver" + ("_san" if sanitize else ""))
    flags = ["-O1", "-g", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-omit-frame-pointer"] if sanitize else ["-O2"]
    subprocess.run([hipcc, *flags, "-std=c++17", "-x", "hip", "--cuda-host-only", f"-I{REPO}/include", f"-I{REPO}/rlao_amd/csrc",
                    os.path.join(REPO, "tests", "native", "wavefront_driver.cpp"), "-o", exe], check=True, capture_output=True)
    return exe


# ---- the model in NumPy ------------------------------------------------------------------------------------------------------------
def plan(r2, n_modes):
    """(n_slices, slice_len, [(lo, hi), ...]) of (R^2, K): slices at least 4 K elements long, at most 64 of them, their length a
    multiple of 16 -- from (R^2, K) alone"""
    want = min(max(r2 // (4 * n_modes), 1), MAX_SLICES)
    length = -(-r2 // want)
    length = -(-length // ROUND) * ROUND
    n = -(-r2 // length)
    return n, length, [(z * length, min((z + 1) * length, r2)) for z in range(n)]


def row_stride(r2):
    return (r2 + 3) // 4 * 4


def scatter(dtype, opd2m, pupil):
    """opd2m [K][P] onto the full grid: [K][row_stride(R^2)] in the env dtype, column q of pupil pixel p = the p-th of
    np.where(pupil.ravel()), zero everywhere else"""
    opd2m = np.asarray(opd2m, dtype=np.float64)
    flat = np.asarray(pupil).ravel() != 0
    out = np.zeros((opd2m.shape[0], row_stride(flat.size)), dtype=DT[dtype])
    out[:, np.where(flat)[0]] = opd2m.astype(DT[dtype])
    return out


def validate(dtype, n_modes, n_pix, pupil, opd2m):
    """the refusal of aoenv_set_wavefront_basis, in the order the library checks"""
    if n_pix < 1:
        return BAD_PIX
    if n_modes < 1 or n_modes > n_pix or n_modes > MAX_MODES:
        return BAD_MODES
    if pupil is None:
        return NO_PUPIL
    if int(np.count_nonzero(pupil)) != n_pix:
        return PUPIL_COUNT
    if opd2m is None:
        return NULL_TABLE
    t = np.asarray(opd2m, dtype=np.float64).ravel()[:n_modes * n_pix]
    if not np.isfinite(t).all() or (np.abs(t) > float(np.finfo(DT[dtype]).max)).any():
        return NOT_FINITE
    return OK


def exact_project(dtype, table, x, scale=None):
    """The general kernel's order restated without the header: per slice one fma chain in index order from 0 (one rounding per
    step, ``fma_exact``), the slice sums added in slice order starting from slice 0's, then one multiply.  table [K][stride],
    x [E][R^2] -> [E][K] in the env dtype"""
    t = DT[dtype]
    table, x = np.asarray(table).astype(t), np.asarray(x).astype(t)
    K, (E, r2) = table.shape[0], x.shape
    _, _, bounds = plan(r2, K)
    rows, cols = table.tolist(), x.tolist()
    out = np.zeros((E, K), dtype=t)
    for e in range(E):
        for m in range(K):
            acc = None
            for lo, hi in bounds:
                v = 0.0
                for q in range(lo, hi):
                    if rows[m][q] != 0.0 and cols[e][q] != 0.0:      # (a zero term leaves the chain's value as it is)
                        v = float(fma_exact(rows[m][q], cols[e][q], v, dtype))
                acc = t(v) if acc is None else t(acc + t(v))
            out[e, m] = acc if scale is None else t(acc * t(scale))
    return out


def projection_bound(dtype, table, x, scale=1.0):
    """|c - c64| <= (R^2 + 4) u s sum_q |P[m][q]| |X[e][q]|, u = 2^-24 / 2^-53: the bound of any summation order, the +4 for
    rounding P and s to the env dtype and the multiply.  table [K][>= R^2], x [E][R^2] (float64) -> [E][K]"""
    u = 2.0 ** -24 if dtype == "f32" else 2.0 ** -53
    x = np.asarray(x, dtype=np.float64)
    r2 = x.shape[1]
    return (r2 + 4) * u * abs(scale) * (np.abs(x) @ np.abs(np.asarray(table, dtype=np.float64)[:, :r2]).T)


def disc_pupil(R, obstruction=0.0):
    """a round pupil on R x R pixels (bool), as a telescope's: the tests only need SOME mask with pixels set and unset in every row"""
    y, x = (np.indices((R, R)) - (R - 1) / 2.0) / (R / 2.0)
    r = np.hypot(x, y)
    return (r <= 1.0) & (r >= obstruction)


# ---- the driver ------------------------------------------------------------------------------------------------------------------------
def host_plan(exe, r2, n_modes):
    out = subprocess.run([exe, "plan", str(r2), str(n_modes)], check=True, capture_output=True, text=True).stdout.split("\n")
    n, length, stride = (int(v) for v in out[0].split())
    bounds = [tuple(int(v) for v in l.split()) for l in out[1:] if l.strip()]
    return n, length, stride, bounds


def _blob(pupil, opd2m):
    return np.ascontiguousarray(np.asarray(pupil).ravel() != 0, dtype=np.uint8).tobytes() + \
        np.ascontiguousarray(opd2m, dtype=np.float64).tobytes()


def host_scatter(exe, dtype, opd2m, pupil, env=None):
    opd2m = np.asarray(opd2m, dtype=np.float64)
    K, P = opd2m.shape
    r2 = np.asarray(pupil).size
    out = subprocess.run([exe, "scatter", dtype, str(r2), str(K), str(P)], input=_blob(pupil, opd2m), check=True, capture_output=True, env=env)
    return np.frombuffer(out.stdout, dtype=DT[dtype]).reshape(K, row_stride(r2)).copy(), out.stderr.decode("utf-8", "replace")


def host_validate(exe, dtype, n_modes, n_pix, pupil, opd2m, case="table", env=None):
    """the driver's refusal number; ``opd2m`` is sent as [max(K, 0)][max(P, 0)] float64 whatever the validation will say"""
    r2 = np.asarray(pupil).size
    out = subprocess.run([exe, "validate", dtype, str(r2), str(n_modes), str(n_pix), case], input=_blob(pupil, opd2m), check=True,
                         capture_output=True, env=env)
    return int(out.stdout.decode().strip()), out.stderr.decode("utf-8", "replace")


def host_project(exe, dtype, table, x, scale, env=None):
    """(scaled, unscaled) [E][K] of the driver in the env dtype"""
    t = DT[dtype]
    table, x = np.ascontiguousarray(table, dtype=t), np.ascontiguousarray(x, dtype=t)
    K, (E, r2) = table.shape[0], x.shape
    blob = table.tobytes() + x.tobytes() + np.array([scale], dtype=t).tobytes()
    out = subprocess.run([exe, "project", dtype, str(r2), str(K), str(E)], input=blob, check=True, capture_output=True, env=env)
    v = np.frombuffer(out.stdout, dtype=t)
    assert v.size == 2 * E * K, (v.size, out.stderr)
    return v[:E * K].reshape(E, K).copy(), v[E * K:].reshape(E, K).copy(), out.stderr.decode("utf-8", "replace")
