"""Float64 restatement of the laser-guide-star Shack-Hartmann (OOPAO/ShackHartmann.py:189-192, 239-240, 396-503, 554-556) for the
tests: no reference import, no GPU.

A ``Source`` with a sodium profile and an up-link FWHM is an LGS; the diffractive sensor then convolves every valid lenslet's
unbinned ``n x n`` spot (``n = 2 p``) with a kernel of that lenslet's own, before the 2 x 2 binning, the camera and the centroid::

    I = fftshift(abs(ifft2(fft2(I) * C)), axes=[1, 2])          C[k] = fft2(I_k.T), I_k the truncated, normalised sum of Gaussians

Here the kernel builder is written array-at-once (``spot_kernels``; rlao_amd/calib.py restates the reference loop by loop) and the
measurement goes through the FFTs as the reference's does (``convolve_and_bin``; the library sums real-space taps).
tests/test_lgs_host.py holds both against tests/golden/lgs_sh.npz (scripts/make_lgs_golden.py, from the reference's own classes)."""
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

GOLDEN = os.path.join(REPO, "tests", "golden", "lgs_sh.npz")
BAND, MAGNITUDE, THRESHOLD_CONVOLUTION = "Na", 8.0, 0.05
# tag -> (R, nSubap, D [m], launch [x, y] in m, FWHM_spot_up): three boxed kernels and the dense one
CASES = {"r24": (24, 4, 8.0, (40.0, 0.0), 0.3), "r20": (20, 5, 8.0, (30.0, 30.0), 0.3), "r32": (32, 4, 8.0, (40.0, -20.0), 0.3),
         "r24d": (24, 4, 8.0, (4.0, 0.0), 1.0)}


def na_profile(centre=90e3, width=20e3, n_z=11, sigma=5e3, skew=0.0):
    """[2, n_z]: altitudes over ``width`` around ``centre`` and a Gaussian density (``skew`` tilts it), normalised to sum 1."""
    h = np.linspace(centre - width / 2, centre + width / 2, n_z)
    w = np.exp(-0.5 * ((h - centre) / sigma) ** 2) * (1 + skew * (h - centre) / width)
    return np.stack([h, w / w.sum()])


def spot_kernels(R, n_subap, D, wavelength, valid_1d, Na_profile, fwhm, launch, threshold=THRESHOLD_CONVOLUTION, shannon=True,
                 transpose=True, truncate=True):
    """``(K [n_valid, n, n], elungation_factor)``, ``K[k] = real(ifft2(C[k]))``.  ``transpose`` / ``truncate`` = False leave out
    the reference's ``I.T`` / its cut of the wings (the mutants tests/test_lgs_host.py tells from the golden)."""
    na = np.asarray(Na_profile, dtype=np.float64)
    h, w = na[0], na[1]
    p = R // n_subap
    n = 2 * p
    X0, Y0 = launch[1], -launch[0]
    sub = np.linspace(-D // 2, D // 2, n_subap)
    d_pix = (D / n_subap) / n
    v = np.linspace(-n * d_pix / 2, n * d_pix / 2, n)
    sigma = fwhm / (2 * np.sqrt(np.log(2)))
    fov_pixel = (p * 206265 * wavelength / (D / n_subap)) / (1 + bool(shannon)) / p
    c3 = np.stack([(D / 4) * (X0 / h), (D / 4) * (Y0 / h), D ** 2. / (8. * h) / (2. * np.sqrt(3.))])
    ref = c3 - c3[:, [h.size // 2]]
    k = np.flatnonzero(np.asarray(valid_1d).reshape(-1))
    g = np.sqrt(3) * (4 / D) ** 2
    sx = 206265 * fov_pixel * (ref[0][None, :] * (4 / D) + ref[2][None, :] * g * sub[k // n_subap][:, None])      # [n_valid, n_z]
    sy = 206265 * fov_pixel * (ref[1][None, :] * (4 / D) + ref[2][None, :] * g * sub[k % n_subap][:, None])
    ax, ay = v[None, None, None, :], v[None, None, :, None]                                 # meshgrid(v, v): x along axis 1
    terms = (w / h ** 2)[None, :, None, None] * np.exp(-((ax - sx[:, :, None, None]) ** 2 + (ay - sy[:, :, None, None]) ** 2)
                                                         / (2 * sigma ** 2))
    I = np.zeros((k.size, n, n))
    for i in range(h.size):                                      # (the reference's order of summation)
        I += terms[:, i]
    if truncate:
        I[I < threshold * I.max(axis=(1, 2), keepdims=True)] = 0
    I /= I.sum(axis=(1, 2), keepdims=True)
    elung = max((sx.max(axis=1) - sx.min(axis=1)).max(), (sy.max(axis=1) - sy.min(axis=1)).max()) / (D / n_subap)
    return (I.transpose(0, 2, 1).copy() if transpose else I), float(elung)


def convolve_and_bin(I, K, shift=True):
    """Unbinned spots ``I [m, n, n]`` -> camera blocks ``[m, p, p]`` through the reference's own operations (:556, :565).
    ``shift=False`` leaves out the ``fftshift`` (what the reference's multi-wavefront branch does, :641-642)."""
    out = np.abs(np.fft.ifft2(np.fft.fft2(I) * np.fft.fft2(K)))
    if shift:
        out = np.fft.fftshift(out, axes=[1, 2])
    m, n = out.shape[0], out.shape[1]
    return out.reshape(m, n // 2, 2, n // 2, 2).sum(axis=(2, 4))


def make_lgs_sh(base, kernels_of, shift=True):
    """A subclass of the oracle's ``OracleSH`` (``base``) whose ``spots`` are the elongated ones.  ``kernels_of(sh)`` returns
    ``K [n_valid, n, n]`` once the geometry and the valid lenslets are known, i.e. before the calibration measures anything; None
    = no elongation."""

    class LgsOracleSH(base):
        lgs_K = None

        def spots(self, phase):
            p, n = self.p, self.n
            if self.lgs_K is None:
                self.lgs_K = kernels_of(self)
            if self.lgs_K is None:
                return super().spots(phase)
            em = np.zeros((self.nSubap ** 2, n, n), dtype=complex)
            lo = n // 2 - p // 2
            em[:, lo:lo + p, lo:lo + p] = np.sqrt(self.flux_tiles) * np.exp(1j * self._tiles(phase))
            em *= self.phasor[None]
            I = np.abs(np.fft.fft2(em, axes=(1, 2)) / n) ** 2
            out = I.reshape(-1, p, 2, p, 2).sum(axis=(2, 4))       # (the lenslets that are not valid: never read)
            out[self.valid_1d] = convolve_and_bin(I[self.valid_1d], self.lgs_K, shift=shift)
            return out

    return LgsOracleSH


def lgs_oracle_env(lgs, **kw):
    """``oracle.ao_oracle.OracleEnv`` whose Shack-Hartmann sees the elongated spots of ``lgs = dict(Na_profile, FWHM_spot_up,
    laser_coordinates[, threshold_convolution])`` from its first measurement on, so reference slopes, slope units, interaction
    matrix and reconstructor are all calibrated on them (the oracle module is imported and subclassed, not edited)."""
    from oracle import ao_oracle as O

    D, ns, R = kw["diameter"], kw["n_subap"], kw["resolution"]

    def kernels_of(sh):
        return spot_kernels(R, ns, D, sh.wavelength, sh.valid_1d, lgs["Na_profile"], lgs["FWHM_spot_up"], lgs["laser_coordinates"],
                            lgs.get("threshold_convolution", THRESHOLD_CONVOLUTION))[0]

    O._PHOTOMETRY.setdefault("Na", (0.589e-6, 0, 3.3e12))         # OOPAO/Source.py:229, the band the oracle's table leaves out
    saved = O.OracleSH
    O.OracleSH = make_lgs_sh(saved, kernels_of)
    try:
        return O.OracleEnv(wfs_type="sh", **kw)
    finally:
        O.OracleSH = saved


def binned_taps(K):
    """``Kb`` of the issue's identity, by explicit index arithmetic (rlao_amd/calib.py uses np.roll)."""
    n = K.shape[-1]
    x = np.arange(n)
    x1 = (x + 1) % n
    return K[..., x[:, None], x[None, :]] + K[..., x1[:, None], x[None, :]] + K[..., x[:, None], x1[None, :]] + K[..., x1[:, None], x1[None, :]]


def tap_sum(I, Kb):
    """camera[P][Q] = sum_{s,t} I[s][t] Kb[(2P + n/2 - s) mod n][(2Q + n/2 - t) mod n] for ``I, Kb [m, n, n]``: what the device forms."""
    m, n = I.shape[0], I.shape[1]
    p = n // 2
    s = np.arange(n)
    out = np.zeros((m, p, p))
    for P in range(p):
        for Q in range(p):
            rows = (2 * P + n // 2 - s) % n
            cols = (2 * Q + n // 2 - s) % n
            out[:, P, Q] = (I * Kb[:, rows[:, None], cols[None, :]]).sum(axis=(1, 2))
    return out
