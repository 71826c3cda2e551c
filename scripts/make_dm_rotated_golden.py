#!/usr/bin/env python
"""Writes tests/golden/dm_rotated.npz: ``dm.modes`` of the reference's own DeformableMirror under a MisRegistration with a rotation,
both shifts and both scalings, at R = 24 (4 subapertures) and R = 30 (5 subapertures) -- the fixture tests/test_dm_pairs_host.py
checks the restatement tests/_dm_rot_ref.py and ``calib.dm_actuator_pairs`` against.  Data only.  It needs the reference checkout
that ``oracle/_ref_loader.py`` names and is run where that exists; no test imports the reference.

    python scripts/make_dm_rotated_golden.py
"""
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from oracle import _ref_loader as RL  # noqa: E402

CASES = {
    "R24": dict(R=24, D=1.6, nsub=4, rotation_angle=3.0, shift_x=0.05, shift_y=-0.02, radial_scaling=0.02, tangential_scaling=-0.03),
    "R30": dict(R=30, D=2.0, nsub=5, rotation_angle=-2.0, shift_x=-0.03, shift_y=0.07, radial_scaling=-0.015, tangential_scaling=0.04),
}
MECH_COUPLING = 0.35


def main():
    ref = RL.load()
    from OOPAO.MisRegistration import MisRegistration
    out = {}
    for name, c in CASES.items():
        with RL.quiet():
            tel = ref.Telescope(resolution=c["R"], diameter=c["D"], samplingTime=1 / 500, centralObstruction=0, display_optical_path=False, fov=0)
            m = MisRegistration()
            m.rotationAngle = c["rotation_angle"]
            m.shiftX, m.shiftY = c["shift_x"], c["shift_y"]
            m.radialScaling, m.tangentialScaling = c["radial_scaling"], c["tangential_scaling"]
            m.anamorphosisAngle = 0
            dm = ref.DeformableMirror(telescope=tel, nSubap=c["nsub"], mechCoupling=MECH_COUPLING, coordinates=None, misReg=m,
                                      pitch=tel.D / (c["nsub"] + 1))
        modes = np.asarray(dm.modes, dtype=np.float64)
        assert modes.shape == (c["R"] ** 2, int(dm.nValidAct))
        out[name + "_modes"] = modes
        out[name + "_validAct"] = np.asarray(dm.validAct, dtype=bool)
        out[name + "_params"] = np.array([c["R"], c["D"], c["nsub"], MECH_COUPLING, c["rotation_angle"], c["shift_x"], c["shift_y"],
                                          c["radial_scaling"], c["tangential_scaling"]], dtype=np.float64)
    out["param_names"] = np.array(["R", "D", "nsub", "mech_coupling", "rotation_angle", "shift_x", "shift_y", "radial_scaling", "tangential_scaling"])
    path = os.path.join(REPO, "tests", "golden", "dm_rotated.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
