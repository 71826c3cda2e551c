"""Shared by tests/test_camera_host.py (CPU), tests/test_poisson_alias.py and tests/test_gpu_camera_streams.py (GPU): the WFS camera
of rlao_amd/csrc/detector.hpp, camera_sh6.hpp and poisson_alias.hpp restated in NumPy.  No device code.

Every random number of the camera is a Philox4x32-7 word of (quad id, global env index, frame number, purpose) under the detector
seed, so a noisy frame is a pure function of the ideal frame and those integers: `noisy_frame` reproduces it count for count.
What it cannot reproduce is the last bit of the device's float32 transcendentals (__expf, __logf, v_sqrt, v_cos / v_sin, v_rcp)
and its fused multiply-adds where their result is compared with a boundary (rintf, truncf, u > cdf, the PTRS tests): every such
step takes `exact` -- False: float32 NumPy, the device's arithmetic as written; True: float64 -- and the share of pixels on which
the two disagree (`flip_figures`) bounds how often a correct device may differ from either.

Stream layout (detector.hpp): one Philox call per (quad, purpose) serves the 4 pixels of a quad, slot s takes word s.
  purpose 0 fine alias draw / U of PTRS round 0      purpose 3 remainder inversion      purpose 4 coarse alias draw / V of round 0
  purpose 1 dark current (5: V of its PTRS round 0)  purpose 2 read-out: slots (0, 1) and (2, 3) are the cos / sin of a pair
  purpose 16 + j: call j of the per-pixel stream of a pixel whose PTRS round 0 was rejected (dark current: pixel | 0x80000000)"""
from dataclasses import dataclass

import numpy as np
from scipy import stats

from _explore_ref import philox4x32_7

HEADER, FINE_ROWS = 4, 128
PTRS_FROM = 10.0
DRAW_PHOTON, DRAW_DARK, DRAW_READOUT, DRAW_PHOTON2, DRAW_PHOTON3, DRAW_DARK2, DRAW_PIXEL_STREAM = 0, 1, 2, 3, 4, 5, 16
DARK_STREAM = 0x80000000
# device against restatement, and restatement against itself in float64 (half of it, so that the reference alone stays inside):
# the share of pixels that may differ, by one count / one ADC step (tests/test_gpu_detector.py grants the camera the same 2e-3)
DEVICE_FLIP_CAP, REFERENCE_FLIP_CAP = 2e-3, 1e-3


def _f(exact):
    return np.float64 if exact else np.float32


def _c(x, F):
    """a float32 literal of the device code, in the working precision"""
    return F(np.float32(x))


def u01(w, F=np.float32):
    """detector.hpp:57: strictly inside (0, 1), 23 bits + 1/2 (exact in float32)"""
    return ((np.asarray(w, dtype=np.uint64) >> np.uint64(9)).astype(F) + F(0.5)) * F(1.0 / 8388608.0)


# ---- camera settings ---------------------------------------------------------------------------------------------------------
@dataclass
class CameraCfg:
    """DetectorCfg as aoenv_set_detector fills it: the float fields are float32."""
    photon_noise: bool = False
    bits: int = 0
    emccd: bool = False
    qe: float = 1.0
    dark_e: float = 0.0
    fwc: float = 0.0
    gain: float = 1.0
    readout_noise: float = 0.0
    seed: int = 0

    @classmethod
    def from_fields(cls, sampling_time, seed=0, photonNoise=False, readoutNoise=0, QE=1, darkCurrent=0, integrationTime=None, FWC=None,
                    bits=None, gain=1, sensor="CCD"):
        """From the fields of env.wfs.cam (BatchedAOEnv._push_detector, then the casts of aoenv_set_detector)."""
        t_int = integrationTime if integrationTime is not None else sampling_time
        if bits and not FWC:
            raise ValueError("the ADC needs a full-well capacity")
        f32 = lambda x: float(np.float32(x))
        return cls(photon_noise=bool(photonNoise), bits=int(bits or 0), emccd=sensor == "EMCCD", qe=f32(QE),
                   dark_e=f32(float(darkCurrent) * float(t_int)), fwc=f32(FWC or 0), gain=f32(gain), readout_noise=f32(readoutNoise),
                   seed=int(seed) & 0xFFFFFFFFFFFFFFFF)

    @property
    def step(self):
        """What one count of a sampler is worth in the output: one ADC step with the ADC on, the gain without."""
        return 1.0 if self.bits else max(self.gain, 1.0)


# ---- the two quad layouts: (cam, n_subap) -> (quad id, slot) of every pixel ----------------------------------------------------------
def generic_layout(cam, n_subap=None):
    """4 consecutive pixels of a row, ceil(cam / 4) quads per row (the last one of a row may be cut); id = its slot-0 pixel."""
    r, c = np.divmod(np.arange(cam * cam, dtype=np.int64), cam)
    slot = c & 3
    return (r * cam + c - slot).astype(np.uint64), slot


def sh6_layout(cam, n_subap):
    """sh6_quad_pixels: 9 quads per 6 x 6 lenslet -- column j rows 0..3 (j < 6); rows 4, 5 of the columns c (slots 0, 1) and c + 3
    (slots 2, 3), c < 3.  id = its slot-0 pixel."""
    assert cam == 6 * n_subap
    y, x = np.divmod(np.arange(cam * cam, dtype=np.int64), cam)
    ry, rx = y % 6, x % 6
    y0, x0 = y - ry, x - rx
    top = ry < 4
    quad = np.where(top, y0 * cam + x, (y0 + 4) * cam + x0 + rx % 3)
    slot = np.where(top, ry, (ry - 4) + 2 * (rx // 3))
    return quad.astype(np.uint64), slot


def layout_for(cam, n_subap, shack_hartmann):
    """launch_detector's choice; the refusal included."""
    if shack_hartmann and cam == 6 * n_subap:
        return sh6_layout(cam, n_subap)
    if shack_hartmann and (cam // n_subap) % 4 != 0:
        raise ValueError("camera noise on a Shack-Hartmann frame needs 6 or a multiple of 4 pixels per lenslet")
    return generic_layout(cam, n_subap)


def _words(quad, env, frame, purpose, seed):
    """the four words of every pixel's quad: env [E, 1] against quad [P] -> 4 x [E, P]"""
    return philox4x32_7(quad[None, :], env, np.uint64(frame), np.uint64(purpose), seed)


def _slot_word(w4, slot):
    return np.choose(slot[None, :], w4)


# ---- the alias sampler (poisson_alias.hpp) -------------------------------------------------------------------------------------
def table_lmax(t, budget=None):
    """The photon count the first `budget` words of the table reach (PoissonAliasHost::prefix: whole coarse rows are dropped from
    the end; rows are stored back to back, so coarse row c starts where the rows before it end): pixels at and above it are drawn
    by PTRS.  The whole table: 32 photons x 32 coarse rows = 1024."""
    nf, nc = int(t[0]), int(t[1])
    budget = t.size if budget is None else min(int(budget), t.size)
    upto = lambda c: int(t[HEADER + 2 * (nf + c)]) if c < nc else int(t.size)
    c = nc
    while c > 0 and ((upto(c) + 3) & ~3) > budget:
        c -= 1
    return 32.0 * c


def step_alias_capacity(n_act):
    """step_lds_layout(n_act).tab_cap (step_kernel.hip): the words of LDS the fused step kernel has for the tables -- where stage A
    kept the command image, Gy C (2 x 64 rows of stride nAp + 1) and the 16 waves' layer tiles (19 x 36)."""
    r4 = lambda w: (w + 3) & ~3
    return r4(n_act * n_act) + r4(2 * 64 * (r4(n_act) + 1)) + r4(16 * 19 * 36)


def env_lmax(t, shack_hartmann, ppx, resolution, n_act):
    """The hand-over to PTRS of an env (aoenv_create): a geometry the fused step kernel can take keeps, for EVERY camera kernel and
    dtype, the prefix of the table that fits in that kernel's LDS; every other env the whole table."""
    fused_geometry = shack_hartmann and ppx == 6 and resolution <= 128 and n_act <= 32
    return table_lmax(t, step_alias_capacity(n_act) if fused_geometry else None)


def alias_poisson(t, lam, wf, wr, wc, exact=False):
    """Poisson(lam), 0 <= lam < table_lmax(t): poisson_alias4 / alias_draw / poisson_small on the tables the kernels read.
    wf: the word of the fine draw (purpose 0), wr: of the remainder's uniform (purpose 3), wc: of the coarse draw (purpose 4)."""
    F = _f(exact)
    lam = np.asarray(lam, dtype=np.float32)
    wf, wr, wc = (np.asarray(w, dtype=np.uint64) for w in (wf, wr, wc))
    c = np.floor(lam * np.float32(1 / 32))
    r = (lam - np.float32(32) * c).astype(np.float32)             # exact (an fma on the device)
    j = np.minimum(np.floor(r * np.float32(4)), 127)
    dl = np.maximum(r - np.float32(0.25) * j, 0).astype(F)        # exact

    def draw(row, w):
        base = t[HEADER + 2 * row].astype(np.int64)
        d = t[HEADER + 2 * row + 1].astype(np.int64)
        n, kmin = d & 0xFFFF, d >> 16
        prod = w * n.astype(np.uint64)
        cell, frac = (prod >> np.uint64(32)).astype(np.int64), (prod & np.uint64(0xFFFFFFFF)).astype(np.int64)
        en = t[base + cell].astype(np.int64)
        return kmin + np.where((frac >> 9) < (en >> 9), cell, en & 511)

    k = draw(j.astype(np.int64), wf) + draw(FINE_ROWS + c.astype(np.int64), wc)
    u = u01(wr, F)
    p = np.exp(-dl).astype(F)
    cdf = p.copy()
    for s in range(7):
        k = k + (u > cdf)
        p = (p * (dl * F(np.float32(1.0 / (s + 1))))).astype(F)
        cdf = (cdf + p).astype(F)
    return k


# ---- PTRS (detector.hpp: ptrs_const, ptrs_squeeze, ptrs_logs, ptrs_full, poisson_ptrs_rounds) --------------------------------------
def log_factorial(k, F=np.float32):
    kk = np.maximum(k, F(4))
    r = F(1) / kk
    r2 = r * r
    st = ((kk + F(0.5)) * np.log(kk) - kk + _c(0.918938533, F)
          + r * (_c(0.0833333333, F) + r2 * (_c(-0.00277777778, F) + r2 * _c(0.000793650794, F))))
    small = np.where(k < 2, F(0), np.where(k < 3, _c(0.693147181, F), _c(1.791759469, F)))
    return np.where(k < 4, small, st).astype(F)


def ptrs_poisson(lam, wu, wv, stream, env, frame, seed, exact=False):
    """Poisson(lam), lam >= 10, for flat arrays: round 0 from the words (wu, wv); a pixel it rejects goes on with the stream
    (stream, env, frame, 16 + call): two rounds per call, 32 calls at the most, then floorf(lam + 0.5f)."""
    F = _f(exact)
    lam = np.asarray(lam).astype(F)
    b = _c(0.931, F) + _c(2.53, F) * np.sqrt(lam)
    a = _c(-0.059, F) + _c(0.02483, F) * b
    loglam = np.log(lam)
    invalpha = _c(1.1239, F) + _c(1.1328, F) * (F(1) / (b - _c(3.4, F)))
    result = np.floor(lam + F(0.5))
    done = np.zeros(lam.shape, dtype=bool)

    def one_round(idx, wu, wv):
        l, bb, aa = lam[idx], b[idx], a[idx]
        U = u01(wu, F) - F(0.5)
        V = u01(wv, F)
        us = F(0.5) - np.abs(U)
        rus = F(1) / us
        kf = np.floor((F(2) * aa * rus + bb) * U + l + _c(0.43, F))
        acc = (us >= _c(0.07, F)) & ((_c(0.9277, F) - V) * (bb - F(2)) >= _c(3.6224, F))
        with np.errstate(invalid="ignore", divide="ignore"):
            lhs = np.log(V * invalpha[idx] * (F(1) / (aa * rus * rus + bb)))
            rhs = -l + kf * loglam[idx] - log_factorial(kf, F)
        full = ~((kf < 0) | ((us < _c(0.013, F)) & (V > us))) & (lhs <= rhs)
        acc = acc | full
        result[idx[acc]] = kf[acc]
        done[idx[acc]] = True

    one_round(np.arange(lam.size), np.asarray(wu, dtype=np.uint64), np.asarray(wv, dtype=np.uint64))
    stream, env = np.asarray(stream, dtype=np.uint64), np.asarray(env, dtype=np.uint64)
    for call in range(32):
        idx = np.nonzero(~done)[0]
        if idx.size == 0:
            break
        o = philox4x32_7(stream[idx], env[idx], np.uint64(frame), np.uint64(DRAW_PIXEL_STREAM + call), seed)
        one_round(idx, o[0], o[1])
        keep = ~done[idx]
        one_round(idx[keep], o[2][keep], o[3][keep])
    return result.astype(np.float64)


# ---- dark current, read-out noise, detector_finish ---------------------------------------------------------------------------------
def dark_inversion(lam, u, exact=False):
    """poisson_inversion: X = #{t < 64 : u > F(t) and P(t) > 0}.  The device walks t four at a time and leaves when no lane is above
    its running sum or the terms have underflowed: neither vote changes the count of a lane that has found its value."""
    F = _f(exact)
    lam = F(np.float32(lam))
    p = F(np.exp(-lam))
    cdf = np.full(u.shape, p, dtype=F)
    k = np.zeros(u.shape)
    for t in range(64):
        k += (u > cdf) & (p > 0)
        p = F(p * F(lam * (F(1) / F(t + 1))))
        cdf = (cdf + p).astype(F)
    return k


def readout_normals(layout, env, frame, seed, exact=False):
    """quad_normals: the standard normal of every pixel, [E, P]; the angle is in revolutions (v_cos / v_sin)."""
    F = _f(exact)
    quad, slot = layout
    o = _words(quad, env, frame, DRAW_READOUT, seed)
    h = (slot >> 1)[None, :]
    r = np.sqrt(F(-2) * np.log(u01(np.choose(h, [o[0], o[2]]), F)))
    t = F(2 * np.pi) * u01(np.choose(h, [o[1], o[3]]), F)
    return (r * np.where((slot & 1)[None, :] == 1, np.sin(t), np.cos(t))).astype(F)


def detector_finish(f, cfg, dark, normal, exact=False):
    """QE, dark electrons, clip to the FWC, EMCCD gain, rint(normal sigma), CCD / CMOS gain, ADC (toward zero, clipped from above)."""
    F = _f(exact)
    f = (f.astype(F) * F(cfg.qe)).astype(F)
    f = (f + dark.astype(F)).astype(F)
    if cfg.fwc > 0:
        f = np.minimum(np.maximum(f, F(0)), F(cfg.fwc))
    if cfg.emccd:
        f = (f * F(cfg.gain)).astype(F)
    if cfg.readout_noise != 0:
        f = (f + np.rint((normal.astype(F) * F(cfg.readout_noise)).astype(F))).astype(F)
    if not cfg.emccd:
        f = (f * F(cfg.gain)).astype(F)
    if cfg.bits > 0:
        top = F((1 << cfg.bits) - 1)
        f = np.trunc(((f / F(cfg.fwc)).astype(F) * top).astype(F))
        f = np.minimum(f, top)
    return f.astype(np.float64)


# ---- the camera ----------------------------------------------------------------------------------------------------------------
def noisy_frame(ideal_f32, cfg, layout, env_index, frame_number, table, valid2d=None, exact=False, lmax=None):
    """The counts of the frame(s) `ideal_f32` -- [cam, cam] with a scalar env_index, [E, cam, cam] with E global env indices -- at
    frame number `frame_number` of the noise streams, and the mask of the pixels that went through PTRS.  valid2d
    [n_subap, n_subap]: the lenslets that carry light; the others take no photon draw (the fused step kernel gives them dark and
    read-out noise only; the stand-alone kernels draw Poisson(0) = 0 there).  lmax: the photon count from which the env draws by
    PTRS (env_lmax; default: the end of the whole table)."""
    quad, slot = layout
    ideal = np.asarray(ideal_f32, dtype=np.float32)
    shape = ideal.shape
    env = np.atleast_1d(np.asarray(env_index, dtype=np.uint64))[:, None]
    v = ideal.reshape(env.shape[0], -1)
    E, P = v.shape
    assert quad.size == P
    pix = np.broadcast_to(np.arange(P, dtype=np.uint64)[None, :], (E, P))
    envs = np.broadcast_to(env, (E, P))
    ptrs = np.zeros((E, P), dtype=bool)
    word = lambda purpose: _slot_word(_words(quad, env, frame_number, purpose, cfg.seed), slot)
    f = v.astype(np.float64)
    if cfg.photon_noise:
        lit = np.ones((E, P), dtype=bool)
        if valid2d is not None:
            cam = int(round(np.sqrt(P)))
            p = cam // valid2d.shape[0]
            lit = np.broadcast_to(np.asarray(valid2d, dtype=bool).repeat(p, 0).repeat(p, 1).reshape(1, P), (E, P))
        lam = np.maximum(v, np.float32(0))
        big = lit & (lam >= np.float32(table_lmax(table) if lmax is None else lmax))
        w0, w4 = word(DRAW_PHOTON), word(DRAW_PHOTON3)
        k = alias_poisson(table, np.where(big | ~lit, np.float32(0), lam), w0, word(DRAW_PHOTON2), w4, exact).astype(np.float64)
        if big.any():
            k[big] = ptrs_poisson(lam[big], w0[big], w4[big], pix[big], envs[big], frame_number, cfg.seed, exact)
        f = np.where(lit, k, f)
        ptrs |= big
    dark = np.zeros((E, P))
    if cfg.dark_e > 0:
        w1 = word(DRAW_DARK)
        if cfg.dark_e < PTRS_FROM:
            dark = dark_inversion(cfg.dark_e, u01(w1, _f(exact)), exact)
        else:
            lam = np.full(E * P, np.float32(cfg.dark_e))
            dark = ptrs_poisson(lam, w1.ravel(), word(DRAW_DARK2).ravel(), pix.ravel() | np.uint64(DARK_STREAM), envs.ravel(),
                                frame_number, cfg.seed, exact).reshape(E, P)
            ptrs[:] = True
    normal = readout_normals(layout, env, frame_number, cfg.seed, exact) if cfg.readout_noise != 0 else np.zeros((E, P))
    out = detector_finish(f, cfg, dark, normal, exact)
    return out.reshape(shape), ptrs.reshape(shape)


# ---- comparisons ---------------------------------------------------------------------------------------------------------------
def flip_figures(got, want, ptrs, cfg):
    """(share of all pixels that differ, largest difference on a pixel that did not go through PTRS in units of cfg.step).  With the
    ADC on the output is whole steps and any difference counts; without it the output is counts times float32 factors (QE, gain),
    where a fused multiply-add or the float64 arithmetic moves the last bits: a difference below 2e-6 of the frame's largest value
    (some 16 float32 roundings of it; one count is worth at least min(gain, 1)) is not one."""
    want = np.asarray(want, dtype=np.float64)
    d = np.abs(np.asarray(got, dtype=np.float64) - want)
    tol = 0.0 if cfg.bits else 2e-6 * max(float(np.abs(want).max()), 1.0)
    assert tol < 0.1 * min(cfg.gain, 1.0)
    off = d[~ptrs]
    return float((d > tol).mean()), float(off.max() / cfg.step) if off.size else 0.0


def assert_flips(got, want, ptrs, cfg, cap, label):
    share, worst = flip_figures(got, want, ptrs, cfg)
    print(label, "flip share", share, "largest alias-pixel difference [steps]", worst)
    assert worst <= 1 + 1e-5, (label, worst)
    assert share <= cap, (label, share)
    return share, worst


def pit(x, lam, rs):
    """Randomised probability-integral transform: uniform on (0, 1) iff x ~ Poisson(lam), whatever lam each sample has."""
    return stats.poisson.cdf(x - 1, lam) + rs.uniform(size=np.shape(x)) * stats.poisson.pmf(x, lam)


def assert_uniform(u, what):
    n = u.size
    h = np.histogram(u, bins=64, range=(0, 1))[0]
    chi2 = float(((h - n / 64) ** 2 / (n / 64)).sum())
    ks = float(stats.kstest(u.ravel(), "uniform").statistic) * np.sqrt(n)
    assert chi2 < stats.chi2.ppf(1 - 1e-6, 63), (what, chi2)      # 63 dof: 99.9999 % point = 137
    assert ks < 2.2, (what, ks)                                   # P(sqrt(n) D > 2.2) = 1.2e-4


# ---- the camera settings the GPU tests cross with the kernel paths (fields of env.wfs.cam) -------------------------------------------
RAZOR = dict(sensor="CMOS", FWC=10000, bits=10, QE=0.56, darkCurrent=5, integrationTime=1 / 500, photonNoise=True, readoutNoise=14)
SETTINGS = {
    "photon": dict(photonNoise=True),
    "readout": dict(readoutNoise=3.5),
    "readout-adc": dict(readoutNoise=3.5, FWC=1000, bits=10),     # 3.6 ADC steps of noise: negative counts behind the ADC
    "dark3": dict(darkCurrent=1500, integrationTime=1 / 500),
    "dark40": dict(darkCurrent=20000, integrationTime=1 / 500),
    "razor": RAZOR,
    "emccd": dict(sensor="EMCCD", gain=3.7, readoutNoise=14, photonNoise=True),
    "ccd": dict(sensor="CCD", gain=3.7, readoutNoise=14, photonNoise=True),
}
# (0.39 ADC steps per electron; a pixel above 810 photons reaches the top of the ADC, one above 3000 the full well)
EVERYTHING = dict(sensor="EMCCD", gain=3.7, FWC=2400, bits=8, QE=0.8, darkCurrent=1500, integrationTime=1 / 500, photonNoise=True,
                  readoutNoise=14)
