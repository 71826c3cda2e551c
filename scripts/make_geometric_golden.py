#!/usr/bin/env python
"""Writes tests/golden/geometric_sh.npz from the reference's own ``Telescope``, ``Source``, ``DeformableMirror`` and
``ShackHartmann(..., is_geometric=True)`` (OOPAO/ShackHartmann.py:382-394, 676-695) at three geometries -- R = 24 with 4 x 4 lenslets
(p = 6), R = 20 with 5 x 5 (odd count, p = 4), R = 30 with 6 x 6 (odd p = 5) and central obstruction 0.3 -- the fixture
tests/test_geometric_host.py holds the restatement tests/_geometric_ref.py against and tests/test_gpu_geometric.py the library.
Per geometry (keys prefixed r24_ / r20_ / r30_):

    slopes_units, valid (valid_subapertures), pupil
    opd [4, R, R]    random unmasked OPDs, about 50 nm rms, non-zero outside the pupil;  sig_opd [4, nSignal]  wfs.signal of each
    coefs [4, A]     random DM commands;  sig_dm [4, nSignal]  wfs.signal through tel*dm*wfs;  validAct
    poke_idx [6], poke_cols [nSignal, 6]   interaction-matrix columns of six pokes through the multi-wavefront branch (:687-695)

The reference's ``initialize_flux`` (:327-338) cuts every lenslet's flux tile into a window of ``2 (p // 2)`` pixels and cannot
build a sensor with an odd p in either mode; for R = 30 alone that one method is replaced by ``_flux_per_lenslet`` below (the same
tiles in the same order, summed whole), so the valid-lenslet selection of that geometry is "parity unpinned"  while its
gradient, binning, unit ramp, valid selection rule and multi-wavefront branch are executed by the reference's own code.

Data only.  It needs the reference checkout that ``oracle/_ref_loader.py`` names and is run where that exists; no test imports the
reference.

    python scripts/make_geometric_golden.py
"""
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

import _geometric_ref as G  # noqa: E402
from oracle import _ref_loader as RL  # noqa: E402


def _flux_per_lenslet(self, input_flux_map=None):
    """Photons per lenslet for any p: tile i * nSubap + j is flux.T[j p:(j + 1) p, i p:(i + 1) p], as :331-335 orders them."""
    f = np.asarray(self.telescope.src.fluxMap.T if input_flux_map is None else input_flux_map, dtype=np.float64)
    ns, p = self.nSubap, self.n_pix_subap_init
    self.cube_flux = f.reshape(ns, p, ns, p).transpose(2, 0, 1, 3).reshape(ns * ns, p, p)
    self.photon_per_subaperture = self.cube_flux.sum(axis=(1, 2)).reshape(-1, 1, 1)
    self.current_nPhoton = self.telescope.src.nPhoton


def one_geometry(ref, tag, R, ns, D, obstruction, seed):
    sh_class = ref.ShackHartmann
    if (R // ns) % 2:
        sh_class = type("ShackHartmannAnyP", (ref.ShackHartmann,), {"initialize_flux": _flux_per_lenslet})
    with RL.quiet():
        tel = ref.Telescope(resolution=R, diameter=D, samplingTime=1 / 500, centralObstruction=obstruction, display_optical_path=False,
                            fov=0)
        ngs = ref.Source(optBand="I", magnitude=8, coordinates=[0, 0])
        ngs * tel
        dm = ref.DeformableMirror(telescope=tel, nSubap=ns, mechCoupling=0.35, coordinates=None, pitch=tel.D / (ns + 1))
        tel.isPaired = False
        tel.resetOPD()
        wfs = sh_class(telescope=tel, nSubap=ns, lightRatio=0.5, is_geometric=True, shannon_sampling=True)
    assert wfs.is_geometric and not np.any(wfs.reference_slopes_maps)
    rs = np.random.RandomState(seed)
    nv = int(dm.nValidAct)
    out = {"params": np.array([R, ns, D, obstruction]), "slopes_units": np.float64(wfs.slopes_units),
           "valid": np.asarray(wfs.valid_subapertures, bool), "pupil": np.asarray(tel.pupil, bool),
           "validAct": np.asarray(dm.validAct, bool), "wavelength": np.float64(ngs.wavelength)}
    opd = rs.normal(size=(4, R, R)) * 50e-9
    sig_opd = []
    for k in range(4):
        with RL.quiet():
            tel.resetOPD()
            tel.OPD_no_pupil = opd[k].copy()
            tel.OPD = opd[k] * tel.pupil
            tel * wfs
        assert not np.any(wfs.cam.frame)
        sig_opd.append(np.asarray(wfs.signal, dtype=np.float64).copy())
    coefs = rs.normal(size=(4, nv)) * 80e-9
    sig_dm = []
    for k in range(4):
        with RL.quiet():
            tel.resetOPD()
            dm.coefs = coefs[k]
            tel * dm * wfs
        sig_dm.append(np.asarray(wfs.signal, dtype=np.float64).copy())
    poke_idx = np.sort(rs.choice(nv, size=6, replace=False))
    m2c = np.zeros((nv, 6))
    m2c[poke_idx, np.arange(6)] = 1.0
    with RL.quiet():
        tel.resetOPD()
        cal = ref.InteractionMatrix(ngs=ngs, atm=None, tel=tel, dm=dm, wfs=wfs, M2C=m2c, stroke=ngs.wavelength / 16, nMeasurements=6,
                                    noise="off", invert=False, display=False, single_pass=True)
    out.update(opd=opd, sig_opd=np.array(sig_opd), coefs=coefs, sig_dm=np.array(sig_dm), poke_idx=poke_idx.astype(np.int64),
               poke_cols=np.asarray(cal.D, dtype=np.float64).reshape(wfs.nSignal, 6))
    return {f"{tag}_{k}": v for k, v in out.items()}


def main():
    ref = RL.load()
    out = {}
    for seed, (tag, (R, ns, D, obstruction)) in enumerate(G.GEOMETRIES.items()):
        out.update(one_geometry(ref, tag, R, ns, D, obstruction, 100 + seed))
    np.savez_compressed(G.GOLDEN, **out)
    print(G.GOLDEN, os.path.getsize(G.GOLDEN), "bytes")


if __name__ == "__main__":
    main()
