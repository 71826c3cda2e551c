"""The reference's guide-star photometry, ``change_mag`` and thresholded centre of gravity, restated in NumPy float64 -- the checker
of ``rlao_amd.calib.flux_scale`` and of the per-env star model (tests/test_star_env_host.py), written from the reference alone and
importing nothing of the package.  Citations: OOPAO/Source.py, OOPAO/ShackHartmann.py, MAIN/OOPAOEnvRazor/OOPAOEnvRazor.py."""
import numpy as np

# OOPAO/Source.py (the photometry table): band -> (wavelength [m], bandwidth [m], zero point [photons / m^2 / s])
PHOTOMETRY = {"V": (0.550e-6, 0.090e-6, 3.31e12), "R": (0.640e-6, 0.150e-6, 4.01e12), "I": (0.790e-6, 0.150e-6, 2.69e12),
              "J": (1.215e-6, 0.260e-6, 1.90e12), "H": (1.654e-6, 0.290e-6, 1.05e12), "K": (2.179e-6, 0.410e-6, 0.70e12)}


def zero_point(band):
    """Source.py:104: ``self.zeroPoint = tmp[2] / 368``"""
    return PHOTOMETRY[band][2] / 368


def n_photon(band, magnitude):
    """Source.py:109: ``self.nPhoton = self.zeroPoint * 10**(-0.4 * magnitude)``  [photons / m^2 / s]"""
    return zero_point(band) * 10 ** (-0.4 * magnitude)


def flux_map(band, magnitude, reflectivity, sampling_time, diameter, resolution):
    """Source.py:151: ``fluxMap = pupilReflectivity * nPhoton * samplingTime * (D / resolution)**2``: linear in nPhoton"""
    return reflectivity * n_photon(band, magnitude) * sampling_time * (diameter / resolution) ** 2


def change_mag(band, mag):
    """OOPAOEnvRazor.py:644-647: ``source.nPhoton = source.zeroPoint * 10**(-0.4 * mag)``, then ``source * tel * wfs`` -- the
    propagation recomputes fluxMap (Source.py:151) and the WFS its cube_flux from it (ShackHartmann.py:327-338, 515-517).  Returns
    the new nPhoton."""
    return zero_point(band) * 10 ** (-0.4 * mag)


def amplitude_factor(band, mag, mag_cal):
    """sqrt(fluxMap(mag) / fluxMap(mag_cal)): the WFS field amplitude is sqrt of the flux (ShackHartmann.py:340-347), every other
    factor of :151 cancelling."""
    return np.sqrt(change_mag(band, mag) / n_photon(band, mag_cal))


def centroid(image, threshold=0.01):
    """ShackHartmann.py:314-324 for a stack ``[n, p, p]``: ``im[im < threshold * im.max()] = 0`` (the maximum over ALL spots),
    then the centre of gravity along both axes.  Returns ``[n, 2]``; 0 / 0 is NaN, as there."""
    im = np.array(image, dtype=np.float64, copy=True)
    im[im < threshold * im.max()] = 0
    x_map, y_map = np.meshgrid(np.arange(im.shape[1]), np.arange(im.shape[2]))
    norma = im.sum(axis=(1, 2))
    with np.errstate(invalid="ignore", divide="ignore"):
        cx = (im * x_map.T[None]).sum(axis=(1, 2)) / norma
        cy = (im * y_map.T[None]).sum(axis=(1, 2)) / norma
    return np.stack([cx, cy], axis=1)
