#!/usr/bin/env python
"""Writes tests/golden/offaxis.npz: ``atm.OPD_no_pupil`` of the reference's own Atmosphere toward off-axis Sources (``atm * src``,
OOPAO/Atmosphere.py:313-334, 439-450, 632-668) at R = 24 (D = 1.6 m), two layers at 0 and 10 km under fov = 20 arcsec, five
directions -- zenith 0; zenith 10 at azimuth 0, 90 and 225; zenith 3.7 at azimuth 30 -- after each of three ``update()``s, with the
footprint corners and ``extra_sx`` / ``extra_sy`` of every layer and the layers' ``phase`` the footprints were cut from: the fixture
tests/test_offaxis_host.py checks the restatement tests/_offaxis_ref.py and the host plan against.  Data only.  It needs the
reference checkout that ``oracle/_ref_loader.py`` names and is run where that exists; no test imports the reference.

scikit-image is not installed: ``OOPAO.Atmosphere.interpolate_image`` (order 1, ratio 1, a pure translation here) is replaced by the
restatement ``_offaxis_ref.bilinear_translate``, as ``_ref_loader`` replaces the wind's warp.  That one stage is "parity unpinned"
(DESIGN.md); the footprint, the truncation, the signs, the row / column swap, the crop, the layer sum and the scaling are executed by
the reference's own code.

    python scripts/make_offaxis_golden.py
"""
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

import _offaxis_ref as X  # noqa: E402
from oracle import _ref_loader as RL  # noqa: E402

R, D, FOV = 24, 1.6, 20.0
ALTITUDE = [0.0, 10000.0]
FRAC = [0.65, 0.35]
WIND_SPEED, WIND_DIR = [9.0, 14.0], [72.0, 200.0]
DIRECTIONS = [(0.0, 0.0), (10.0, 0.0), (10.0, 90.0), (10.0, 225.0), (3.7, 30.0)]
UPDATES = 3


def _interpolate_image(image_in, pixel_size_in, pixel_size_out, resolution_out, rotation_angle=0, shift_x=0, shift_y=0, **kw):
    assert pixel_size_in == pixel_size_out == 1 and rotation_angle == 0 and resolution_out == image_in.shape[0]
    assert not any(kw.get(k, 0) for k in ("anamorphosisAngle", "tangentialScaling", "radialScaling")) and kw.get("order", 1) == 1
    return X.bilinear_translate(np.asarray(image_in, dtype=np.float64), float(shift_x), float(shift_y))


def main():
    ref = RL.load()
    import OOPAO.Atmosphere as A
    A.interpolate_image = _interpolate_image
    with RL.quiet():
        tel = ref.Telescope(resolution=R, diameter=D, samplingTime=1 / 500, centralObstruction=0, display_optical_path=False, fov=FOV)
        ngs = ref.Source(optBand="I", magnitude=8, coordinates=[0, 0])
        ngs * tel
        atm = ref.Atmosphere(telescope=tel, r0=0.13, L0=30.0, windSpeed=WIND_SPEED, fractionalR0=FRAC, windDirection=WIND_DIR,
                             altitude=ALTITUDE)
        atm.initializeAtmosphere(tel)
        srcs = [ref.Source(optBand="I", magnitude=8, coordinates=list(d)) for d in DIRECTIONS]
    layers = [getattr(atm, f"layer_{l + 1}") for l in range(len(ALTITUDE))]
    out = dict(params=np.array([R, D, FOV]), altitude=np.array(ALTITUDE), frac=np.array(FRAC), directions=np.array(DIRECTIONS),
               grids=np.array([lay.resolution for lay in layers]))
    opd = np.zeros((UPDATES, len(DIRECTIONS), R, R))
    corners = np.zeros((UPDATES, len(DIRECTIONS), len(layers), 2), dtype=np.int64)
    extra = np.zeros((UPDATES, len(DIRECTIONS), len(layers), 2))
    for u in range(UPDATES):
        with RL.quiet():
            atm * ngs
            atm.update()
        for l, lay in enumerate(layers):
            out[f"phase_u{u}_l{l}"] = np.array(lay.phase, dtype=np.float64)
        for d, src in enumerate(srcs):
            with RL.quiet():
                atm * src
            opd[u, d] = atm.OPD_no_pupil
            for l, lay in enumerate(layers):
                rows, cols = np.nonzero(lay.pupil_footprint)
                assert rows.size == R * R
                corners[u, d, l] = rows.min(), cols.min()
                extra[u, d, l] = lay.extra_sx, lay.extra_sy
    with RL.quiet():
        try:
            atm * ref.Source(optBand="I", magnitude=8, coordinates=[FOV / 2 + 0.01, 0])
            refused = False
        except ValueError:
            refused = True
    assert refused and np.abs(opd[:, 1:] - opd[:, :1]).max() > 1e-8
    out.update(opd_no_pupil=opd, corners=corners, extra=extra)
    path = os.path.join(REPO, "tests", "golden", "offaxis.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
