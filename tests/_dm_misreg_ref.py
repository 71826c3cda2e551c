"""The reference's DENSE influence-function expression for a mis-registered Cartesian DM, restated in NumPy float64 -- the checker of
``rlao_amd.calib.dm_factors`` (tests/test_dm_env_host.py), written from the reference alone and importing nothing of the package.
Citations: OOPAO/DeformableMirror.py."""
import numpy as np


def actuator_grid(D, n_act):
    """xIF0, yIF0 of the full Cartesian grid (:286-299: ``x = linspace(-D/2, D/2, nAct); X, Y = meshgrid(x, x)``), flattened
    row-major: index iy * n_act + ix."""
    x = np.linspace(-D / 2, D / 2, n_act)
    X, Y = np.meshgrid(x, x)
    return X.reshape(-1), Y.reshape(-1)


def dense_influence(R, D, n_subap, mech_coupling, valid, shift_x=0.0, shift_y=0.0, radial_scaling=0.0, tangential_scaling=0.0):
    """``[R, R, n_valid]``: the Gaussian of :494-510 for the actuators ``valid`` (flat indices iy * n_act + ix) at the positions of
    :326-346, with the anamorphosis angle and the rotation angle both 0 -- the only mirror the separable kernels show."""
    x0, y0 = actuator_grid(D, n_subap + 1)
    x0, y0 = x0[valid], y0[valid]                                  # :327-328
    # :331 hands (tangentialScaling, radialScaling) to the slots (mRad, mNorm) of the anamorphosis, :485-490.  At angle 0 its
    # cos^2 term is 1 and every sin term 0: x is stretched by 1 + mRad = 1 + tangential, y by 1 + mNorm = 1 + radial.
    stretch = np.array([1.0 + tangential_scaling, 1.0 + radial_scaling])
    # :334 at rotation 0 is the identity; :337-338 subtract the shifts; :345-346 go to the pixel grid
    u0 = R / 2 + (np.stack([x0, y0]) * stretch[:, None] - np.array([[shift_x], [shift_y]])) * R / D
    # :497-498 -- the WIDTHS take the scalings the other way round: radial along x, tangential along y; :289 nActAlongDiameter = nAct - 1
    sigma = np.array([1.0 + radial_scaling, 1.0 + tangential_scaling]) * (R / n_subap) / np.sqrt(2 * np.log(1.0 / mech_coupling))
    # :506-508 at theta = 0: a = 1 / (2 cx^2), b = 0, c = 1 / (2 cy^2)
    a, b, c = 1.0 / (2 * sigma[0] ** 2), 0.0, 1.0 / (2 * sigma[1] ** 2)
    grid = np.linspace(0, 1, R) * R                                # :502-503
    dx = grid[None, :, None] - u0[0][None, None, :]                # X - x0: X varies along the second axis
    dy = grid[:, None, None] - u0[1][None, None, :]
    return np.exp(-(a * dx ** 2 + 2 * b * dx * dy + c * dy ** 2))  # :510
