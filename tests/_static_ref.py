"""Static aberration maps for oracle.ao_oracle.OracleEnv, without touching oracle/: the reference's OPD_map / NCPA objects in
`ngs*tel*map*dm*wfs` add their OPD to tel.OPD and tel.OPD_no_pupil (OOPAO/Telescope.py:502-512), the mirror behind them adds its
own and masks the sum (tel*dm), so with a sensor-arm map S_w

    OPD_no_pupil = atm.OPD_no_pupil + S_w + dm.OPD,      OPD = OPD_no_pupil * pupil

(tests/golden/static_opd.npz pins the order, the masking and the unmasked sum).  `static` wraps the INSTANCE's `dm_opd` by
`orig(c) + S_w`: every place the oracle forms the residual -- new_episode, step, the geometric oracle's unmasked phase -- then
carries the map on the mirror side of the sum, and `atm.OPD`, `total` and the calibration never see it.  The wrap is made after the
instance is built (so calibration is untouched) and after any deep copy: a closure is bound to the object it was made for, a copy
of a wrapped oracle would go on calling the original's (the order tests/_guide_ref.py documents).

The science arm sees S_s where the sensor sees S_w:

    phase_sci = phase + ((opd_atm_sci - opd_atm) + (S_s - S_w)) 2 pi / lambda_src    inside the pupil, 0 outside

(`science_phase`; the first bracket only while a science direction is set).

`variant` breaks one convention on purpose (tests/test_static_host.py shows that each moves what the GPU test compares by more than
100 of its tolerances on that test's inputs): "ignore" an oracle that does not look at the map; "masked" the map masked before the
sum (the unmasked phase of a geometric sensor loses it outside the pupil); "atm_side" the map on the atmosphere's side of the sum
(atm.OPD, OPD_no_pupil and `total` then contain it); "flip" the sign of S_s - S_w; `arms(..., "swap")` the two arms swapped."""
import numpy as np


def static(orc, s_w, variant=None):
    """Gives the OracleEnv `orc` the sensor-arm map `s_w` [R, R] metres; returns it.  Takes effect with the next residual formed."""
    s_w = np.array(s_w, dtype=np.float64, copy=True)
    assert s_w.shape == (orc.R, orc.R)
    original = orc.dm_opd                                           # (the class's method, bound to THIS instance)
    assert "dm_opd" not in vars(orc), "wrap once, and after the deep copy"
    if variant == "atm_side":
        atm = orc.atm
        collect = atm._collect

        def _collect():
            collect()
            atm.OPD_no_pupil = atm.OPD_no_pupil + s_w
            atm.OPD = atm.OPD_no_pupil * atm.pupil

        atm._collect = _collect
        orc.static_map = s_w
        return orc
    add = {None: s_w, "ignore": 0.0 * s_w, "masked": s_w * orc.pupil}[variant]

    def dm_opd(coefs):
        return original(coefs) + add

    orc.dm_opd = dm_opd
    orc.static_map = s_w
    return orc


def arms(s_w, s_s, variant=None):
    """(S_w, S_s) as float64 [R, R] arrays, a None arm as zeros; "swap": the two exchanged."""
    shape = np.shape(s_w if s_w is not None else s_s)
    s_w = np.zeros(shape) if s_w is None else np.asarray(s_w, dtype=np.float64)
    s_s = np.zeros(shape) if s_s is None else np.asarray(s_s, dtype=np.float64)
    return (s_s, s_w) if variant == "swap" else (s_w, s_s)


def science_phase(phase, pupil, s_w, s_s, src_wavelength, opd_atm_sci=None, opd_atm=None, variant=None):
    """(phase_sci [R, R] rad, rms_nm, strehl) from the sensor arm's phase (which contains S_w): the restatement above, float64."""
    pupil = np.asarray(pupil, dtype=bool)
    s_w, s_s = arms(s_w, s_s)
    delta = s_s - s_w
    if variant == "flip":
        delta = -delta
    if opd_atm_sci is not None:
        delta = (np.asarray(opd_atm_sci, dtype=np.float64) - opd_atm) + delta
    phase_sci = (np.asarray(phase, dtype=np.float64) + delta * (2 * np.pi / src_wavelength)) * pupil
    opd = phase_sci * src_wavelength / (2 * np.pi)
    return phase_sci, float(np.std(opd[pupil]) * 1e9), float(np.exp(-np.var(phase_sci[pupil])))
