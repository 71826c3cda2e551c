"""The reference's DENSE influence-function expression for a ROTATED, shifted and scaled Cartesian DM, restated in NumPy float64 --
the checker of ``rlao_amd.calib.dm_actuator_pairs`` (tests/test_dm_pairs_host.py) and the mirror of the oracles of
tests/test_gpu_dm_pairs.py, written from the reference alone and importing nothing of the package.  The sibling of
tests/_dm_misreg_ref.py.  Citations: OOPAO/DeformableMirror.py."""
import numpy as np


def actuator_grid(D, n_act):
    """xIF0, yIF0 of the full Cartesian grid (:286-299: ``x = linspace(-D/2, D/2, nAct); X, Y = meshgrid(x, x)``), flattened
    row-major: index iy * n_act + ix."""
    x = np.linspace(-D / 2, D / 2, n_act)
    X, Y = np.meshgrid(x, x)
    return X.reshape(-1), Y.reshape(-1)


def rotated_positions(D, n_subap, valid, rotation_angle=0.0, shift_x=0.0, shift_y=0.0, radial_scaling=0.0, tangential_scaling=0.0):
    """xIF, yIF [n_valid] in metres (:326-338) at anamorphosis angle 0; ``rotation_angle`` in degrees."""
    x0, y0 = actuator_grid(D, n_subap + 1)
    x0, y0 = x0[valid], y0[valid]                                  # :327-328: the valid actuators of the NOMINAL grid
    # :331 hands (tangentialScaling, radialScaling) to the slots (mRad, mNorm) of the anamorphosis, :485-490; at angle 0 the
    # cos^2 term is 1 and every sin term 0: x is stretched by 1 + tangential, y by 1 + radial
    x3, y3 = x0 * (1.0 + tangential_scaling), y0 * (1.0 + radial_scaling)
    t = rotation_angle * np.pi / 180                               # :334
    x4 = x3 * np.cos(t) - y3 * np.sin(t)                           # :480-483
    y4 = y3 * np.cos(t) + x3 * np.sin(t)
    return x4 - shift_x, y4 - shift_y                              # :337-338


def dense_influence(R, D, n_subap, mech_coupling, valid, rotation_angle=0.0, shift_x=0.0, shift_y=0.0, radial_scaling=0.0,
                    tangential_scaling=0.0):
    """``[R, R, n_valid]``: the Gaussian of :494-510 (anamorphosis angle 0) for the actuators ``valid`` (flat indices
    iy * n_act + ix) at the rotated positions."""
    xIF, yIF = rotated_positions(D, n_subap, valid, rotation_angle, shift_x, shift_y, radial_scaling, tangential_scaling)
    u0x, u0y = R / 2 + xIF * R / D, R / 2 + yIF * R / D            # :345-346
    # :497-498 -- the WIDTHS take the scalings the other way round: radial along x, tangential along y; :289 nActAlongDiameter = nAct - 1
    cx = (1.0 + radial_scaling) * (R / n_subap) / np.sqrt(2 * np.log(1.0 / mech_coupling))
    cy = (1.0 + tangential_scaling) * (R / n_subap) / np.sqrt(2 * np.log(1.0 / mech_coupling))
    theta = 0.0                                                    # :501
    a = np.cos(theta) ** 2 / (2 * cx ** 2) + np.sin(theta) ** 2 / (2 * cy ** 2)      # :506-508
    b = -np.sin(2 * theta) / (4 * cx ** 2) + np.sin(2 * theta) / (4 * cy ** 2)
    c = np.sin(theta) ** 2 / (2 * cx ** 2) + np.cos(theta) ** 2 / (2 * cy ** 2)
    grid = np.linspace(0, 1, R) * R                                # :502-503
    dx = grid[None, :, None] - u0x[None, None, :]                  # X - x0: X varies along the second axis
    dy = grid[:, None, None] - u0y[None, None, :]
    return np.exp(-(a * dx ** 2 + 2 * b * dx * dy + c * dy ** 2))  # :510


def dense_modes(R, D, n_subap, mech_coupling, valid, **kw):
    """dm.modes ``[R * R, n_valid]`` (:511: each G reshaped to R^2, row-major)."""
    return dense_influence(R, D, n_subap, mech_coupling, valid, **kw).reshape(R * R, -1)


# ---- the mirrors of tests/test_gpu_dm_pairs.py's 4-env shard and their oracles ---------------------------------------------------
def mirrors(pitch):
    """env 0 nominal; env 1 +1.5 degrees; env 2 -3 degrees and shift_x = +0.3 pitch; env 3 +2 degrees, shift_y = -0.5 pitch, radial
    0.02, tangential -0.03 (and one actuator dead: ``dead_actuator``)."""
    return [dict(), dict(rotation_angle=1.5), dict(rotation_angle=-3.0, shift_x=0.3 * pitch),
            dict(rotation_angle=2.0, shift_y=-0.5 * pitch, radial_scaling=0.02, tangential_scaling=-0.03)]


def dead_actuator(n_valid):
    """index (among the valid actuators) of env 3's dead actuator"""
    return n_valid // 2


def env_modes(R, D, n_subap, mech_coupling, valid, pitch, e):
    """dm.modes [R^2, n_valid] of mirror e of ``mirrors``"""
    m = dense_modes(R, D, n_subap, mech_coupling, valid, **mirrors(pitch)[e])
    if e == 3:
        m[:, dead_actuator(m.shape[1])] = 0.0
    return m


def rotated_oracle(base, rows, seed, seed_stride=100, n_subap=None, mech_coupling=0.35, m2c=None, modal_cm=None, modal=None,
                   modal_cm_K=None, drop=()):
    """A ``ComposedOracle`` (tests/_compose_ref.py) whose env r carries mirror ``rows[r]``: ``dm_modes`` replaced after
    construction, the reconstructor staying that of the calibrated mirror.  ``drop``: shard rows left with the nominal mirror."""
    import _compose_ref as CR
    n_subap = int(base.wfs.nSubap if n_subap is None else n_subap)
    orc = CR.ComposedOracle(base, [CR.env_spec(seed=seed + seed_stride * r) for r in range(len(rows))], m2c=m2c, modal_cm=modal_cm,
                            modal=modal, modal_cm_K=modal_cm_K, n_subap=n_subap, mech_coupling=mech_coupling)
    pitch = base.D / n_subap
    for r, e in enumerate(rows):
        if r not in drop:
            orc.envs[r].dm_modes = env_modes(base.R, base.D, n_subap, mech_coupling, base.dm_valid_flat, pitch, e)
    return orc
