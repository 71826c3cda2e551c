"""The off-axis science target in float64 NumPy, on top of oracle.ao_oracle.OracleAtmosphere's layers (lay.phase, lay.g, lay.frac):
a restatement of OOPAO/Atmosphere.py:313-334 (set_pupil_footprint) and :439-450 (fill_phase_support) for a source at
coordinates = [zenith arcsec, azimuth deg], and the Python mirror of the host plan of rlao_amd/csrc/offaxis.hpp.

    [x_z, y_z] = pol2cart(h tan(zenith / 206265) layer.resolution / layer.D, deg2rad(azimuth))
    ix, iy = int(x_z), int(y_z);  extra_sx, extra_sy = ix - x_z, iy - y_z
    footprint = rows iy + N//2 - R//2 .. + R, columns ix + N//2 - R//2 .. + R          (y_z moves rows, x_z columns)
    _im = layer.phase;  if extra_sx != 0 or extra_sy != 0: _im = interpolate_image(_im, 1, 1, N, shift_x=extra_sx, shift_y=extra_sy)
    phase_support += _im[footprint] * sqrt(fractionalR0);  OPD_no_pupil = phase_support * 500e-9 / 2 pi

The bilinear stage (bilinear_translate) is restated from scikit-image's documented warp(order=1, mode='constant', cval=0) for a
pure translation, in the convention of oracle.ao_oracle.warp_translate: out[r, c] = in[r - shift_y, c - shift_x].  scikit-image is
not a dependency: this one stage is "parity unpinned" (DESIGN.md).

`variant` breaks one convention on purpose (tests/test_offaxis_host.py shows that each moves the result by far more than the GPU
test's tolerance on that test's inputs): "nofrac" drops the fractions, "flipfrac" flips their sign, "swap" swaps rows and columns,
"round" rounds the whole pixels where the reference truncates (the fractions stay the truncation's: rounding both would name the
same sampling point)."""
import numpy as np

ARCSEC = 206265.0
ATM_WAVELENGTH = 500e-9


def pol2cart(rho, phi):
    return rho * np.cos(phi), rho * np.sin(phi)


def ref_shift(altitude, zenith, azimuth, R, D, N):
    """What set_pupil_footprint computes for one layer: dict(x_z, y_z, ix, iy, extra_sx, extra_sy, row0, col0)."""
    layer_D = N * D / R                                            # Atmosphere.py:219
    x_z, y_z = pol2cart(altitude * np.tan(zenith / ARCSEC) * N / layer_D, np.deg2rad(azimuth))
    ix, iy = int(x_z), int(y_z)
    return dict(x_z=float(x_z), y_z=float(y_z), ix=ix, iy=iy, extra_sx=ix - x_z, extra_sy=iy - y_z,
                row0=iy + N // 2 - R // 2, col0=ix + N // 2 - R // 2)


def device_shift(s):
    """floor + fraction in [0, 1) of a ref_shift: (fy, fx, ty, tx), what the library uploads (oa_shift)."""
    ky, kx = np.floor(s["y_z"]), np.floor(s["x_z"])
    return int(ky), int(kx), float(s["y_z"] - ky), float(s["x_z"] - kx)


def plan_layer(altitude, zenith, azimuth, R, D, N):
    """The in-range assertion of one (layer, env) (oa_plan_layer): (ok, lo, hi) with [lo, hi] the rows / columns of layer.phase
    the patch takes; ok = every one of them in [1, N - 2], so that every Catmull-Rom tap lies inside the (N + 2)^2 screen."""
    fy, fx, ty, tx = device_shift(ref_shift(altitude, zenith, azimuth, R, D, N))
    foot0, more = N // 2 - R // 2, int(ty != 0.0 or tx != 0.0)
    lo = min(foot0 + fy, foot0 + fx)
    hi = max(foot0 + fy, foot0 + fx) + R - 1 + more
    return lo >= 1 and hi <= N - 2, lo, hi


def check_direction(zenith, fov):
    """The refusals of aoenv_set_science_direction that do not need a layer."""
    if not np.isfinite(zenith) or zenith < 0 or zenith > fov / 2:
        raise ValueError(f"zenith {zenith} arcsec is negative, not finite or above fov / 2 = {fov / 2}")


def bilinear_translate(img, shift_x, shift_y):
    """warp(img, translation(shift_x, shift_y), order=1, mode='constant', cval=0): out[r, c] = img[r - shift_y, c - shift_x]."""
    rows, cols = img.shape
    rr = np.arange(rows, dtype=np.float64) - shift_y
    cc = np.arange(cols, dtype=np.float64) - shift_x
    r0, c0 = np.floor(rr).astype(np.int64), np.floor(cc).astype(np.int64)
    tr, tc = (rr - r0)[:, None], (cc - c0)[None, :]
    pad = np.zeros((rows + 4, cols + 4))
    pad[2:-2, 2:-2] = img
    ri, ci = np.clip(r0 + 2, 0, rows + 2), np.clip(c0 + 2, 0, cols + 2)
    p00, p01 = pad[ri][:, ci], pad[ri][:, ci + 1]
    p10, p11 = pad[ri + 1][:, ci], pad[ri + 1][:, ci + 1]
    return (1 - tr) * ((1 - tc) * p00 + tc * p01) + tr * ((1 - tc) * p10 + tc * p11)


def layer_footprint(phase, altitude, zenith, azimuth, R, D, variant=None):
    """_im[footprint] of one layer toward the target, [R, R] (before the layer weight)."""
    N = phase.shape[0]
    s = ref_shift(altitude, zenith, azimuth, R, D, N)
    x_z, y_z = s["x_z"], s["y_z"]
    if variant == "swap":
        x_z, y_z = y_z, x_z
    ix, iy = int(x_z), int(y_z)
    ex, ey = ix - x_z, iy - y_z
    if variant == "round":                                         # the whole pixels rounded, the fractions those of the truncation
        ix, iy = int(np.round(x_z)), int(np.round(y_z))
    if variant == "nofrac":
        ex = ey = 0.0
    if variant == "flipfrac":
        ex, ey = -ex, -ey
    im = phase
    if ex != 0 or ey != 0:
        im = bilinear_translate(im, ex, ey)
    r0, c0 = iy + N // 2 - R // 2, ix + N // 2 - R // 2
    assert r0 >= 0 and c0 >= 0 and r0 + R <= N and c0 + R <= N
    return im[r0:r0 + R, c0:c0 + R]


def science_opd(atm, altitudes, zenith, azimuth, variant=None):
    """atm.OPD_no_pupil toward [zenith, azimuth] from the layers of an OracleAtmosphere as they stand, [R, R] metres."""
    sup = np.zeros((atm.R, atm.R))
    for lay, h in zip(atm.layers, altitudes):
        assert lay.phase.shape[0] == lay.g.resolution
        sup += layer_footprint(lay.phase, h, zenith, azimuth, atm.R, atm.D, variant) * np.sqrt(lay.frac)
    return sup * ATM_WAVELENGTH / 2 / np.pi


def science_residual(opd_sci, dm_opd, pupil, src_wavelength):
    """(OPD_sci, phase_sci, rms_nm, strehl): the residual toward the target behind the mirror surface dm_opd."""
    pupil = np.asarray(pupil, dtype=bool)
    opd = (opd_sci + dm_opd) * pupil
    phase = opd * 2 * np.pi / src_wavelength
    return opd, phase, float(np.std(opd[pupil]) * 1e9), float(np.exp(-np.var(phase[pupil])))
