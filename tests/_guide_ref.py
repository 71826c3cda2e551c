"""An off-axis guide star for oracle.ao_oracle.OracleEnv, without touching oracle/: the reference's `ngs.coordinates = [zenith arcsec,
azimuth deg]` with `atm * ngs` moves every layer's footprint (OOPAO/Atmosphere.py:313-334, 439-450) and `tel * dm * wfs` then
measures that line of sight.  `atm * source` is one code path whatever the source is called, so the restatement pinned to the
reference for the science target (tests/_offaxis_ref.py, tests/golden/offaxis.npz) is the guide star's too: `guide` replaces the
instance's `atm._collect` by one that forms

    OPD_no_pupil = _offaxis_ref.science_opd(atm, altitudes, zenith, azimuth),   OPD = OPD_no_pupil * pupil

and everything the oracle derives from the atmosphere -- the residual, the sensor, observation, reward, Strehl, the telemetry --
follows.  At zenith 0 the replaced `_collect` equals the original exactly (asserted on every call there).  `variant` is passed on to
science_opd: a convention broken on purpose, or "ignore" for an oracle that does not look at the direction at all."""
import numpy as np

import _offaxis_ref as X


def guide(orc, altitudes, zenith, azimuth, variant=None):
    """Gives the OracleEnv `orc` (or a bare OracleAtmosphere) a guide star at [zenith, azimuth]; returns it.  Takes effect with the
    next `_collect`: new_episode() / atm.generate_new_phase_screen() / atm.update()."""
    atm = getattr(orc, "atm", orc)
    original = type(atm)._collect
    altitudes = [float(h) for h in altitudes]
    assert len(altitudes) == len(atm.layers)

    def _collect():
        if variant == "ignore":
            original(atm)
            return
        atm.OPD_no_pupil = X.science_opd(atm, altitudes, zenith, azimuth, variant)
        atm.OPD = atm.OPD_no_pupil * atm.pupil
        if zenith == 0 and variant is None:
            got, got_p = atm.OPD_no_pupil, atm.OPD
            original(atm)
            assert np.array_equal(got, atm.OPD_no_pupil) and np.array_equal(got_p, atm.OPD)

    atm._collect = _collect
    atm.guide_direction = (float(zenith), float(azimuth))
    return orc
