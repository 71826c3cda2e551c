#!/usr/bin/env python
"""Writes tests/golden/lgs_sh.npz from the reference's own ``Telescope``, ``Source(optBand="Na", Na_profile=..., FWHM_spot_up=...,
laser_coordinates=...)``, ``DeformableMirror`` and diffractive ``ShackHartmann`` behind that LGS source (OOPAO/ShackHartmann.py:189-192,
239-240, 396-503, 554-556) at the four cases of tests/_lgs_ref.py::CASES -- R = 24 / 4 x 4 (p = 6), R = 20 / 5 x 5 (p = 4, a valid
count that is no multiple of four), R = 32 / 4 x 4 (p = 8), all three with FWHM 0.3 and truncated (boxed) kernels, and R = 24 / 4 x 4
with FWHM 1.0 and a launch close to the axis, whose kernels are dense -- every case with the 11-sample, 20 km sodium profile at
90 km.  The fixture tests/test_lgs_host.py holds the restatement tests/_lgs_ref.py and rlao_amd/calib.py against, and
tests/test_gpu_lgs.py the library.  Per case (keys prefixed with the tag):

    C [n_valid, n, n] complex   wfs.C;   elungation_factor;   reference_slopes_maps;   slopes_units;   valid;   pupil;   validAct
    Na_profile, FWHM_spot_up, laser_coordinates, wavelength, altitude (src.altitude)
    opd [4, R, R]    random OPDs, about 50 nm rms;  frame_opd [4, cam, cam] wfs.cam.frame;  maps_opd [4, n_valid, p, p] wfs.maps_intensity;
                     sig_opd [4, nSignal] wfs.signal
    coefs [4, A]     random DM commands;  sig_dm [4, nSignal] wfs.signal through tel*dm*wfs;  frame_dm [4, cam, cam]
    poke_idx [6], poke_cols [nSignal, 6]   push-only interaction columns, ONE wavefront at a time, (poked - flat) / stroke.  The
                     reference's multi-wavefront branch (:641-642) leaves out the fftshift and is not used.

The script asserts for every stored measurement that no pixel lies within 1e-3 (relative) of the centroid cut ``threshold_cog * max``,
so that a float32 rounding of the frame cannot move a pixel across it: the first seed (steps of 10 from the case's number) whose
measurements all stay clear is taken and stored, and the six poked actuators are drawn from those whose frame stays clear.

Data only.  It needs the reference checkout that ``oracle/_ref_loader.py`` names and is run where that exists; no test imports the
reference.

    python scripts/make_lgs_golden.py
"""
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

import _lgs_ref as G  # noqa: E402
from oracle import _ref_loader as RL  # noqa: E402

CLEAR = 1e-3


def assert_clear(maps, thr, what):
    """no pixel within CLEAR (relative) of the cut thr * max"""
    mx = float(np.max(maps))
    lo, hi = thr * mx * (1 - CLEAR), thr * mx * (1 + CLEAR)
    near = (maps > lo) & (maps < hi)
    assert not near.any(), f"{what}: {int(near.sum())} pixel(s) within {CLEAR} of the centroid cut; pick another seed"


def one_case(ref, tag, R, ns, D, launch, fwhm, seed):
    prof = G.na_profile()
    with RL.quiet():
        tel = ref.Telescope(resolution=R, diameter=D, samplingTime=1 / 500, centralObstruction=0.0, display_optical_path=False, fov=0)
        lgs = ref.Source(optBand=G.BAND, magnitude=G.MAGNITUDE, coordinates=[0, 0], Na_profile=prof, FWHM_spot_up=fwhm,
                         laser_coordinates=list(launch))
        lgs * tel
        dm = ref.DeformableMirror(telescope=tel, nSubap=ns, mechCoupling=0.35, coordinates=None, pitch=tel.D / (ns + 1))
        tel.isPaired = False
        tel.resetOPD()
        wfs = ref.ShackHartmann(telescope=tel, nSubap=ns, lightRatio=0.5, is_geometric=False, shannon_sampling=True,
                                threshold_convolution=G.THRESHOLD_CONVOLUTION)
    assert lgs.type == "LGS" and wfs.is_LGS and not wfs.is_geometric
    thr = float(wfs.threshold_cog)
    rs = np.random.RandomState(seed)
    nv = int(dm.nValidAct)
    out = {"params": np.array([R, ns, D]), "C": np.asarray(wfs.C), "elungation_factor": np.float64(wfs.elungation_factor),
           "reference_slopes_maps": np.asarray(wfs.reference_slopes_maps, dtype=np.float64), "slopes_units": np.float64(wfs.slopes_units),
           "valid": np.asarray(wfs.valid_subapertures, bool), "pupil": np.asarray(tel.pupil, bool),
           "validAct": np.asarray(dm.validAct, bool), "wavelength": np.float64(lgs.wavelength), "altitude": np.float64(lgs.altitude),
           "Na_profile": prof, "FWHM_spot_up": np.float64(fwhm), "laser_coordinates": np.array(launch, dtype=np.float64),
           "threshold_cog": np.float64(thr)}

    def measure(what):
        assert_clear(wfs.maps_intensity, thr, f"{tag} {what}")
        return (np.asarray(wfs.signal, dtype=np.float64).copy(), np.asarray(wfs.cam.frame, dtype=np.float64).copy(),
                np.asarray(wfs.maps_intensity, dtype=np.float64).copy())

    opd = rs.normal(size=(4, R, R)) * 50e-9
    res = []
    for k in range(4):
        with RL.quiet():
            tel.resetOPD()
            tel.OPD_no_pupil = opd[k].copy()
            tel.OPD = opd[k] * tel.pupil
            tel * wfs
        res.append(measure(f"opd {k}"))
    out.update(opd=opd, sig_opd=np.array([r[0] for r in res]), frame_opd=np.array([r[1] for r in res]),
               maps_opd=np.array([r[2] for r in res]))
    coefs = rs.normal(size=(4, nv)) * 80e-9
    res = []
    for k in range(4):
        with RL.quiet():
            tel.resetOPD()
            dm.coefs = coefs[k]
            tel * dm * wfs
        res.append(measure(f"dm {k}"))
    out.update(coefs=coefs, sig_dm=np.array([r[0] for r in res]), frame_dm=np.array([r[1] for r in res]))

    stroke = float(lgs.wavelength) / 16
    with RL.quiet():
        tel.resetOPD()
        dm.coefs = np.zeros(nv)
        tel * dm * wfs
    flat = np.asarray(wfs.signal, dtype=np.float64).copy()
    maps, sigs = [], []
    for a in range(nv):                                          # every single poke: the range of the frame maxima
        cf = np.zeros(nv)
        cf[a] = stroke
        with RL.quiet():
            tel.resetOPD()
            dm.coefs = cf
            tel * dm * wfs
        maps.append(np.asarray(wfs.maps_intensity, dtype=np.float64).copy())
        sigs.append(np.asarray(wfs.signal, dtype=np.float64).copy())
    clear = []
    for a in range(nv):                                          # the six columns come from pokes that stay clear of their own cut
        try:
            assert_clear(maps[a], thr, f"{tag} poke {a}")
            clear.append(a)
        except AssertionError:
            pass
    assert len(clear) >= 6, f"{tag}: only {len(clear)} pokes stay clear of the centroid cut"
    poke_idx = np.sort(rs.choice(clear, size=6, replace=False))
    out.update(poke_idx=poke_idx.astype(np.int64), poke_cols=np.stack([(sigs[a] - flat) / stroke for a in poke_idx], axis=1))
    with RL.quiet():
        tel.resetOPD()
    return {f"{tag}_{k}": v for k, v in out.items()}


def main():
    ref = RL.load()
    out = {}
    for first, (tag, (R, ns, D, launch, fwhm)) in enumerate(G.CASES.items()):
        for seed in range(first, first + 400, 10):               # the first seed whose measurements all stay clear of the cut
            try:
                case = one_case(ref, tag, R, ns, D, launch, fwhm, seed)
            except AssertionError as err:
                print(err)
                continue
            case[f"{tag}_seed"] = np.int64(seed)
            out.update(case)
            break
        else:
            raise SystemExit(f"{tag}: no seed stays clear of the centroid cut")
    np.savez_compressed(G.GOLDEN, **out)
    print(G.GOLDEN, os.path.getsize(G.GOLDEN), "bytes")


if __name__ == "__main__":
    main()
