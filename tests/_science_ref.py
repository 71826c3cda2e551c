"""Shared by tests/test_science_host.py (CPU) and tests/test_gpu_science.py (GPU): the science window's model
(rlao_amd/csrc/science.hpp) restated in NumPy without the header -- geometry, table, plan, refusals, the window itself -- and the
host driver (tests/native/science_driver.cpp over the header)."""
import os
import shutil
import subprocess

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DT = {"f32": np.float32, "f64": np.float64}
# enum SciRefusal of science.hpp
OK, BAD_ZP, ODD_IMAGE, WINDOW_ODD, WINDOW_RANGE, FIRST_FRAME, BAD_FLAGS, NOT_FINITE = range(8)
LOG10 = 1
MESSAGES = {                                                          # a fragment of the message aoenv_set_science gives with each
    BAD_ZP: "outside [1, 8]", ODD_IMAGE: "odd image sizes are not built", WINDOW_ODD: "is odd", WINDOW_RANGE: "outside [2,",
    FIRST_FRAME: "first_frame", BAD_FLAGS: "flags", NOT_FINITE: "is not finite in the env dtype"}


def build_driver(out_dir, sanitize=False):
    """Compiles the driver for the host; None when there is no hipcc."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        return None
    exe = os.path.join(str(out_dir), "science_driver" + ("_san" if sanitize else ""))
    flags = ["-O1", "-g", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-omit-frame-pointer"] if sanitize else ["-O2"]
    subprocess.run([hipcc, *flags, "-std=c++17", "-x", "hip", "--cuda-host-only", f"-I{REPO}/include", f"-I{REPO}/rlao_amd/csrc",
                    os.path.join(REPO, "tests", "native", "science_driver.cpp"), "-o", exe], check=True, capture_output=True)
    return exe


# ---- the model in NumPy ------------------------------------------------------------------------------------------------------------
def geom(R, zp, W):
    """dict(M, U, pad, n_fft): the reference pads by ceil((2 M - R) / 2) on both sides, so the transform is 2 M long for even R and
    2 M + 1 for odd R (OOPAO/Telescope.py:320-325)"""
    M = zp * R
    pad = -(-(2 * M - R) // 2)
    return dict(R=R, zp=zp, W=W, M=M, U=2 * W, pad=pad, n_fft=R + 2 * pad)


def reduced_integer(R, zp, W):
    """m[u][x] = (2 (j - M)(x + pad - M) + (x + pad)) mod 2 n_fft with j = M - W + u, in Python integers"""
    g = geom(R, zp, W)
    a = np.arange(-W, W, dtype=np.int64)[:, None]
    x = np.arange(R, dtype=np.int64)[None, :]
    return np.mod(2 * a * (x + g["pad"] - g["M"]) + (x + g["pad"]), 2 * g["n_fft"]), g


def octant_cos_sin(m, n_fft):
    """cos(pi m / n_fft), sin(pi m / n_fft) through the symmetries of the circle on the INTEGER m in [0, 2 n_fft): the angle handed
    to NumPy lies in [0, pi / 4]; the values on the axes are exact"""
    m = np.asarray(m, dtype=np.int64)
    n = int(n_fft)
    neg_sin = m > n                                                 # the lower half: (cos, sin)(2 pi - t) = (cos, -sin)(t)
    m = np.where(neg_sin, 2 * n - m, m)                             # [0, n]
    neg_cos = 2 * m > n                                             # the second quadrant: (cos, sin)(pi - t) = (-cos, sin)(t)
    m = np.where(neg_cos, n - m, m)                                 # [0, n / 2]
    swap = 4 * m > n                                                # above pi / 4: (cos, sin)(pi / 2 - t) = (sin, cos)(t)
    num = np.where(swap, n - 2 * m, 2 * m)                          # t = pi num / (2 n), num in [0, n / 2]
    t = np.pi * num.astype(np.float64) / float(2 * n)
    c, s = np.where(swap, np.sin(t), np.cos(t)), np.where(swap, np.cos(t), np.sin(t))
    return np.where(neg_cos, -c, c), np.where(neg_sin, -s, s)


def dft_table(R, zp, W):
    """F [U][R] complex128: exp(-i pi m / n_fft) on the reduced integer, folded into the first octant"""
    m, g = reduced_integer(R, zp, W)
    c, s = octant_cos_sin(m, g["n_fft"])
    return c - 1j * s


def dft_table_plain(R, zp, W):
    """the same table with np.cos / np.sin of the angle pi m / n_fft itself"""
    m, g = reduced_integer(R, zp, W)
    ang = np.pi * m.astype(np.float64) / g["n_fft"]
    return np.cos(ang) - 1j * np.sin(ang)


def plan(R, W):
    U = 2 * W
    rp, up = -(-R // 16) * 16, -(-U // 32) * 32
    tiles = -(-U // 16)
    per_wave = -(-tiles // 4)
    tpw = min(per_wave, 8)
    lds = (2 * 16 * (rp + 4) + 2 * 32 * 20) * 4
    return dict(rp=rp, up=up, n_row_tiles=tiles, tiles_per_wave=tpw, n_row_groups=-(-tiles // (4 * tpw)), n_col_blocks=up // 32,
                lds_bytes=lds, mfma_ok=int(lds <= 64 * 1024), general_blocks=-(-U // 8))


def validate(dtype, R, zp, W, first_frame=16, flags=0, dft=None):
    """the refusal of aoenv_set_science, in the order the library checks"""
    if zp < 1 or zp > 8:
        return BAD_ZP
    if (zp * R) % 2:
        return ODD_IMAGE
    if W % 2:
        return WINDOW_ODD
    if W < 2 or W > zp * R:
        return WINDOW_RANGE
    if first_frame < 0:
        return FIRST_FRAME
    if flags & ~LOG10:
        return BAD_FLAGS
    if dft is not None:
        t = np.asarray(dft, dtype=np.float64).ravel()
        if not np.isfinite(t).all() or (np.abs(t) > float(np.finfo(DT[dtype]).max)).any():
            return NOT_FINITE
    return OK


def bin2x2(p):
    """sum-binning in the model's order: (rows of column 2b) + (rows of column 2b + 1)"""
    return (p[0::2, 0::2] + p[1::2, 0::2]) + (p[0::2, 1::2] + p[1::2, 1::2])


def window(field, table, n_fft):
    """bin2x2(|F E F^T|^2) / n_fft^2 in float64 (or exact integers when both are integer-valued)"""
    P = table @ field @ table.T
    return bin2x2(P.real ** 2 + P.imag ** 2) / float(n_fft) ** 2


def crop(full, W):
    """the window of a full M x M image"""
    lo = full.shape[-1] // 2 - W // 2
    return full[..., lo:lo + W, lo:lo + W]


def default_window(R, zp):
    return 130 if zp * R >= 130 else zp * R


# ---- the driver ------------------------------------------------------------------------------------------------------------------------
def host_plan(exe, R, W):
    out = subprocess.run([exe, "plan", str(R), str(W)], check=True, capture_output=True, text=True).stdout.split()
    keys = ("rp", "up", "n_row_tiles", "tiles_per_wave", "n_row_groups", "n_col_blocks", "lds_bytes", "mfma_ok", "general_blocks")
    return dict(zip(keys, (int(v) for v in out)))


def host_geom(exe, R, zp, W):
    out = subprocess.run([exe, "geom", str(R), str(zp), str(W)], check=True, capture_output=True, text=True).stdout.split()
    return dict(zip(("M", "U", "pad", "n_fft"), (int(v) for v in out)))


def host_table(exe, dtype, R, zp, W, dft=None, env=None):
    """the padded table of the driver as complex [up][rp] in the env dtype's precision, and its stderr"""
    blob = b"" if dft is None else np.ascontiguousarray(dft, dtype=np.float64).tobytes()
    out = subprocess.run([exe, "table", dtype, str(R), str(zp), str(W), "given" if dft is not None else "own"], input=blob, check=True,
                         capture_output=True, env=env)
    p = plan(R, W)
    v = np.frombuffer(out.stdout, dtype=DT[dtype]).reshape(2, p["up"], p["rp"])
    return v[0] + 1j * v[1], out.stderr.decode("utf-8", "replace")


def host_validate(exe, dtype, R, zp, W, first_frame=16, flags=0, dft=None, env=None):
    blob = b"" if dft is None else np.ascontiguousarray(dft, dtype=np.float64).tobytes()
    out = subprocess.run([exe, "validate", dtype, str(R), str(zp), str(W), str(first_frame), str(flags), "given" if dft is not None else "own"],
                         input=blob, check=True, capture_output=True, env=env)
    return int(out.stdout.decode().strip()), out.stderr.decode("utf-8", "replace")


# ---- the exact-data recipe of tests/test_gpu_science.py (and its precondition, asserted on the CPU) -----------------------------------
def exact_case(R, W, seed=0):
    """(dft [U][R][2] float64 of sparse integers, amplitude [R][R] in {0, 1, 2} on a disc): the recipe of the exact-data test"""
    rs = np.random.RandomState(seed)
    U = 2 * W
    dft = (rs.randint(-1, 2, size=(U, R, 2)) * (rs.rand(U, R, 2) < 0.25)).astype(np.float64)
    y, x = (np.indices((R, R)) - (R - 1) / 2.0) / (R / 2.0)
    amp = rs.randint(0, 3, size=(R, R)).astype(np.float64) * (np.hypot(x, y) <= 1.0)
    return dft, amp


def exact_window(dft, amp):
    """(int64 bins [W][W], largest absolute-value partial sum of P, largest bin): the product in integers"""
    fr, fi = dft[..., 0].astype(np.int64), dft[..., 1].astype(np.int64)
    e = amp.astype(np.int64)
    tr, ti = e @ fr.T, e @ fi.T                                      # T1[y][c], the field is real (zero phase)
    pr = fr @ tr - fi @ ti
    pi = fr @ ti + fi @ tr
    # every partial sum of either product, in any order, is bounded by the sum of absolute values
    t_abs = np.abs(e) @ (np.abs(fr) + np.abs(fi)).T
    p_abs = (np.abs(fr) + np.abs(fi)) @ t_abs
    bins = bin2x2(pr * pr + pi * pi)
    return bins, int(max(t_abs.max(), p_abs.max())), int(bins.max())
