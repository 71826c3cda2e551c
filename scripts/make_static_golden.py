#!/usr/bin/env python
"""Writes tests/golden/static_opd.npz: the reference's own static optical-path objects at R = 24 (D = 1.6 m, 4 lenslets across):

* ``NCPA(tel, dm, atm, modal_basis='Zernike', f2=[amplitude, first, last, cutoff], seed=...).OPD`` and the linear form
  ``NCPA(..., modal_basis='Zernike', coefficients=[...]).OPD`` (OOPAO/NCPA.py) -- what ``rlao_amd.calib.ncpa_map`` restates;
* ``tel.OPD`` and ``tel.OPD_no_pupil`` after ``ngs*tel*map*dm`` with a non-zero command on the mirror, for an ``OPD_map`` that is NOT
  zero outside the pupil and for the NCPA object, behind the reference's own atmosphere (``tel + atm``, then
  ``atm*ngs*tel*map*dm``; OOPAO/Telescope.py:502-512, 533-544, OOPAO/DeformableMirror.py:452-478): they pin the
  order (the map enters before the mirror), the masking (``tel*dm`` masks the sum) and the unmasked sum
  ``OPD_no_pupil = atm + map + dm`` -- what tests/_static_ref.py restates.

aotools (third party, not part of the reference) is not installed: its ``zernike.zernIndex`` and ``zernike.zernikeRadialFunc``, which
the reference's ``Zernike`` class calls, are replaced by the restatements ``oracle.ao_oracle.noll_to_nm`` / ``zernike_radial``, as
``_ref_loader`` replaces the wind's warp.  That one stage is "parity unpinned" (DESIGN.md); the pupil coordinates, the
normalisation of the modes, the f2 law's random stream, its ``1 / sqrt(i + cutoff)`` weights, the scaling to the amplitude and the
linear form are executed by the reference's own code.

Data only.  It needs the reference checkout that ``oracle/_ref_loader.py`` names and is run where that exists; no test imports the
reference.

    python scripts/make_static_golden.py
"""
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from oracle import _ref_loader as RL  # noqa: E402

R, D, N_SUB = 24, 1.6, 4
F2, SEED = [100e-9, 2, 12, 1.0], 5
COEFFICIENTS = [0.0, 0.0, 30e-9, -20e-9, 10e-9, 0.0, 15e-9]


def main():
    ref = RL.load()
    import types
    from oracle import ao_oracle as O
    sys.modules["aotools"].zernike = types.SimpleNamespace(zernIndex=O.noll_to_nm, zernikeRadialFunc=O.zernike_radial)
    from OOPAO.NCPA import NCPA
    from OOPAO.OPD_map import OPD_map
    rs = np.random.RandomState(3)
    with RL.quiet():
        tel = ref.Telescope(resolution=R, diameter=D, samplingTime=1 / 500, centralObstruction=0, display_optical_path=False)
        ngs = ref.Source(optBand="I", magnitude=8)
        ngs * tel
        dm = ref.DeformableMirror(telescope=tel, nSubap=N_SUB, mechCoupling=0.35)
        ncpa_f2 = NCPA(tel, dm, None, modal_basis="Zernike", f2=list(F2), seed=SEED)
        ncpa_lin = NCPA(tel, dm, None, modal_basis="Zernike", coefficients=list(COEFFICIENTS))
        atm = ref.Atmosphere(telescope=tel, r0=0.13, L0=30.0, windSpeed=[10.0], fractionalR0=[1.0], windDirection=[72.0], altitude=[0.0])
        atm.initializeAtmosphere(tel)
        tel + atm                                                    # paired: the mirror adds to what the telescope holds
    pupil = np.asarray(tel.pupil, dtype=bool)
    atm_opd = np.array(atm.OPD_no_pupil, dtype=np.float64)           # the atmosphere's OPD_no_pupil of the one screen used
    free_map = rs.normal(0.0, 80e-9, (R, R))                         # an OPD_map that does not vanish outside the pupil
    coefs = rs.normal(0.0, 60e-9, dm.nValidAct)
    out = dict(params=np.array([R, D, N_SUB]), f2=np.array(F2), seed=np.array(SEED), coefficients=np.array(COEFFICIENTS),
               pupil=pupil, ncpa_f2=np.array(ncpa_f2.OPD, dtype=np.float64), ncpa_lin=np.array(ncpa_lin.OPD, dtype=np.float64),
               atm_opd=atm_opd, free_map=free_map, coefs=coefs, dm_modes=np.array(dm.modes, dtype=np.float64))
    for name, obj in (("map", OPD_map(tel, OPD=free_map.copy())), ("ncpa", ncpa_f2)):
        with RL.quiet():
            dm.coefs = coefs.copy()
            atm * ngs * tel * obj * dm
        out[f"opd_{name}"] = np.array(tel.OPD, dtype=np.float64)
        out[f"opd_no_pupil_{name}"] = np.array(tel.OPD_no_pupil, dtype=np.float64)
    dm_opd = (out["dm_modes"] @ coefs).reshape(R, R)
    assert np.abs(out["opd_no_pupil_map"] - (atm_opd + free_map + dm_opd)).max() < 1e-18
    assert np.abs(out["opd_map"] - (atm_opd + free_map + dm_opd) * pupil).max() < 1e-18
    assert abs(np.std(out["ncpa_f2"][pupil]) - F2[0]) < 1e-15 and np.abs(free_map[~pupil]).max() > 0
    path = os.path.join(REPO, "tests", "golden", "static_opd.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
