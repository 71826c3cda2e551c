"""The float64 oracle of a shard whose envs each carry their own atmosphere, star, mirror and disturbance behind one control delay:
``ComposedOracle``, a thin wrapper around ``oracle.ao_oracle.OracleEnv`` with one instance per env.  Shared by
tests/test_compose_host.py (CPU: the reference pinned on its own) and tests/test_gpu_compose.py (GPU: every loop of the library
held to it).  Nothing of ``rlao_amd`` is imported here: what the library does per env is restated from the documented meaning of
its setters, feature by feature --

* r0: the first screens of env e come from ``ft_sh_phase_screen(r0_e, ...)``, its ring innovations from ``B (r0_cal / r0_e)^(5/6)``
  with ``A`` untouched (B goes as r0^(-5/6), A not at all: the arithmetic of ``set_r0_per_env``);
* wind: speed and direction of the env's layers; a wind of a pixel per frame or more makes whole-pixel ring rounds in
  ``OracleLayer.update`` (OOPAO/Atmosphere.py:350-407);
* magnitude: ``flux_map`` at the env's magnitude (Source.py:109, 151), the calibration staying that of the calibrated star;
* threshold: ``threshold_cog`` of the env's centre of gravity (ShackHartmann.py:314-324), the reference slopes and slope units
  staying those of the calibrated threshold;
* mirror: ``dm_modes`` = the dense influence functions of the mis-registered mirror (tests/_dm_misreg_ref.py), the mode-to-command
  matrix and the modal command matrix staying those of the calibrated one;
* disturbance: the measurement of frame i sees ``coefs + modes @ v(t0 + i + 1)``, ``v[m] = sum_j amp sin(2 pi (f tau + phi))`` with
  f in cycles per frame; ``coefs`` is swapped around ``OracleEnv.step`` only, so that ``dm_prev`` integrates the pure command;
* delay: a FIFO of d zero images, used as ``TimeDelayEnv.step`` uses ``action_buffer`` (MAIN/PO4AO/util_simple.py:46-52);
* modal: the action is ``M2C[:, :K] @ a``, the observation ``-1e6 cm_K @ signal`` and the reward ``-sum(obs^2)``
  (MAIN/OOPAOEnv/modalAOEnv.py:150-171, 190 as ``step_modal`` states them).

With every feature off a ``ComposedOracle`` step IS an ``OracleEnv.step``: no arithmetic is added (tests/test_compose_host.py
holds it to that bit for bit)."""
import copy
from fractions import Fraction

import numpy as np

from oracle import ao_oracle as O
import _dm_misreg_ref as DM

MISREG_KEYS = ("shift_x", "shift_y", "radial_scaling", "tangential_scaling")
QUANTITIES = ("signal", "obs", "reward", "strehl", "frame")


def cut_gap(frame, thr):
    """Distance of the closest pixel of an oracle frame from the centroid cut ``thr * max``, relative to the brightest pixel (the
    pixels of the invalid lenslets are 0: ``thr`` away).  ``thr == 0`` cuts nothing: the gap is infinite."""
    if thr == 0:
        return np.inf
    mx = float(frame.max())
    return float(np.abs(frame - thr * mx).min() / mx)


def line_value(amp, freq, phase, tau):
    """``v[m] = sum_j amp[m, j] sin(2 pi frac(freq[m, j] tau + phase[m, j]))`` in float64, the phase formed exactly (rational
    arithmetic, one rounding) before it is reduced -- written here from the model's definition, compared with
    ``rlao_amd.env.disturbance_value`` in tests/test_compose_host.py.  amp, freq (cycles per frame), phase (cycles): [M, J]."""
    amp, freq, phase = (np.asarray(x, dtype=np.float64) for x in (amp, freq, phase))
    v = np.zeros(amp.shape[0])
    for m in range(amp.shape[0]):
        for j in range(amp.shape[1]):
            x = Fraction(float(freq[m, j])) * int(tau) + Fraction(float(phase[m, j]))
            v[m] = v[m] + amp[m, j] * np.sin(2.0 * np.pi * float(x - (x.numerator // x.denominator)))
    return v


def scaled_B(B, r0_cal, r0):
    """The innovation operator of an env at ``r0`` from the table at ``r0_cal``: B goes as r0^(-5/6)."""
    return np.asarray(B, dtype=np.float64) * (float(r0_cal) / float(r0)) ** (5.0 / 6.0)


# scaled B against the factor formed at r0_e: measured on the CPU 2.7e-9 of max |B_e| (A: 7.6e-13 of max |A|).  The Schur complement
# XXt - A ZXt itself is well conditioned (28), but A comes through the pseudo-inverse of ZZt (condition 1.5e6 at this size) and the
# complement is what is left of XXt after a cancellation of several digits: A's 1e-12 is amplified by that ratio.  The bound is 10 x
# the measured figure (profiles/compose_parity_maxima.json holds it with both condition numbers).  The device never forms B at
# r0_e: it scales the draws, as ComposedOracle does, so this difference is the reference's own and enters no GPU comparison.
SCALED_B_BOUND = 2.7e-8


def scaled_B_error(geom, A, B, r0_cal, r0_list):
    """``scaled_B`` against ``LayerGeometry.AB(r0_e)`` (the factor formed at r0_e from scratch), relative to max |B_e| / max |A|,
    the largest over ``r0_list``; beside it the condition numbers of the Schur complement ``XXt - A ZXt`` the factor is taken of and of ``ZZt`` (whose pseudo-inverse
    gives A), and how much of ``XXt`` cancels in the complement."""
    ZZt, ZXt, XXt, _ = geom.covariances()
    s = (geom.r0_def / r0_cal) ** (5.0 / 3)
    schur = XXt * s - np.matmul(A, ZXt * s)
    out = dict(B_rel=0.0, A_rel=0.0, schur_condition=float(np.linalg.cond(schur)), ZZt_condition=float(np.linalg.cond(ZZt)),
               cancellation=float(np.abs(XXt * s).max() / np.abs(schur).max()))
    for r0 in r0_list:
        A_e, B_e = geom.AB(r0)
        out["B_rel"] = max(out["B_rel"], float(np.abs(scaled_B(B, r0_cal, r0) - B_e).max() / np.abs(B_e).max()))
        out["A_rel"] = max(out["A_rel"], float(np.abs(A_e - A).max() / np.abs(A).max()))
    out["B_rel_r0_cal"] = float(np.abs(scaled_B(B, r0_cal, r0_cal) - B).max())
    return out


def env_spec(seed, r0=None, wind_speed=None, wind_dir=None, threshold=None, magnitude=None, misreg=None, dist_amp=None,
             dist_period=None, dist_phase=None):
    """One env's values; None: the base's own (the feature is off for that env).  ``dist_amp`` [m] and ``dist_period`` [frames]:
    scalars (one line on the first disturbed mode) or arrays [M, J]."""
    return dict(seed=int(seed), r0=r0, wind_speed=wind_speed, wind_dir=wind_dir, threshold=threshold, magnitude=magnitude,
                misreg=None if misreg is None else dict(misreg), dist_amp=dist_amp, dist_period=dist_period, dist_phase=dist_phase)


class ComposedOracle:
    """``base``: an ``OracleEnv`` of the calibrated geometry (never stepped: every env is a deep copy that shares its large constant
    arrays).  ``specs``: one ``env_spec`` per env.  ``m2c`` / ``modal_cm``: the controller (default: the base's own).  ``delay``:
    frames.  ``dist_modes`` [A, M]: the command-space directions of the disturbance.  ``modal``: K, the modes of the modal surface
    (``m2c[:, :K]``); ``modal_cm_K`` [K, nSignal]: its command matrix (default ``calibration_vault_M(imat @ m2c[:, :K])``).
    ``band`` / ``mech_coupling``: what the base was built with."""

    def __init__(self, base, specs, m2c=None, modal_cm=None, delay=0, dist_modes=None, t0=0, modal=None, modal_cm_K=None,
                 band="I", mech_coupling=0.35, n_subap=None):
        self.base, self.specs, self.delay, self.t0 = base, [dict(s) for s in specs], int(delay), int(t0)
        self.n = len(self.specs)
        self.M2C = np.asarray(base.M2C if m2c is None else m2c, dtype=np.float64)
        self.modal_cm = np.asarray(base.modal_cm if modal_cm is None else modal_cm, dtype=np.float64)
        self.dist_modes = None if dist_modes is None else np.asarray(dist_modes, dtype=np.float64)
        self.sh = base.wfs_type == "sh"
        self.n_subap = int(base.wfs.nSubap if n_subap is None else n_subap)
        self.band, self.mech_coupling = band, mech_coupling
        self.K = None
        if modal is not None:
            self.K = int(modal)
            self.M2C_K = self.M2C[:, :self.K]
            self.cm_K = (O.calibration_vault_M(base.imat @ self.M2C_K) if modal_cm_K is None
                         else np.asarray(modal_cm_K, dtype=np.float64))
        self.r0_cal = float(base.atm.r0)
        self.envs = [self._build(s) for s in self.specs]
        self.fifo = [np.zeros((self.n, base.nActuator, base.nActuator)) for _ in range(self.delay)]
        self.whole_rounds = np.zeros((self.n, base.atm.nLayer), dtype=int)   # of the last step
        self.crossed = np.zeros((self.n, base.atm.nLayer), dtype=bool)

    # -- one env ---------------------------------------------------------------------------------------------------------------
    def _build(self, s):
        b = self.base
        share = [x for x in (b.dm_modes, b.imat, b.reconstructor, b.F) if x is not None]
        share += [a for lay in b.atm.layers for a in (lay.A, lay.B)]
        o = copy.deepcopy(b, memo={id(x): x for x in share})
        if self.M2C is not b.M2C or self.modal_cm is not b.modal_cm:
            o.M2C, o.modal_cm = self.M2C, self.modal_cm
            o.reconstructor = o.M2C @ o.modal_cm
        if s["r0"] is not None:
            o.atm.r0 = float(s["r0"])
            for lay in o.atm.layers:
                lay.B = scaled_B(lay.B, self.r0_cal, s["r0"])
        if s["wind_speed"] is not None or s["wind_dir"] is not None:
            for l, lay in enumerate(o.atm.layers):
                sp = lay.speed if s["wind_speed"] is None else np.atleast_1d(s["wind_speed"])[l]
                di = lay.direction if s["wind_dir"] is None else np.atleast_1d(s["wind_dir"])[l]
                lay.set_wind(float(sp), float(di))
        if s["magnitude"] is not None:
            _, n_photon = O.source_photometry(self.band, float(s["magnitude"]))
            flux = b.pupil.astype(float) * n_photon * b.dt * (b.D / b.R) ** 2
            if self.sh:
                o.wfs.flux_tiles = o.wfs._tiles(flux)
            else:
                o.wfs.flux_map = flux
        if s["threshold"] is not None:
            if not self.sh:
                raise ValueError("a Pyramid has no centre of gravity to threshold")
            o.wfs.thr = float(s["threshold"])
        if s["misreg"] is not None:
            unknown = set(s["misreg"]) - set(MISREG_KEYS)
            if unknown:
                raise ValueError(f"unknown mis-registration parameter(s) {sorted(unknown)}")
            o.dm_modes = DM.dense_influence(b.R, b.D, self.n_subap, self.mech_coupling, b.dm_valid_flat,
                                            **s["misreg"]).reshape(b.R * b.R, -1)
        return o

    def lines(self, e):
        """(amp, freq [cycles per frame], phase) [M, J] of env e, None without a disturbance"""
        s = self.specs[e]
        if s["dist_amp"] is None or self.dist_modes is None:
            return None
        M = self.dist_modes.shape[1]
        amp = np.asarray(s["dist_amp"], dtype=np.float64)
        if amp.ndim == 0:
            full = np.zeros((M, 1))
            full[0, 0] = amp
            amp = full
        per = np.asarray(1.0 if s["dist_period"] is None else s["dist_period"], dtype=np.float64)
        freq = np.zeros(amp.shape)
        freq[...] = 1.0 / per
        ph = np.zeros(amp.shape) if s["dist_phase"] is None else np.broadcast_to(np.asarray(s["dist_phase"], dtype=np.float64), amp.shape)
        return amp, freq, ph

    def disturbance(self, e, i):
        """``modes @ v(t0 + i + 1)`` of env e [A]: what the measurement of frame i sees on top of the command"""
        ln = self.lines(e)
        if ln is None:
            return None
        return self.dist_modes @ line_value(*ln, self.t0 + int(i) + 1)

    # -- the shard's surface ---------------------------------------------------------------------------------------------------
    def new_episode(self, envs=None):
        """new screens (at the env's r0 and seed), flat mirror, one measurement; ``dm_prev`` of a fresh copy is 0"""
        for e in (range(self.n) if envs is None else envs):
            o = self.envs[e]
            o.dm_prev = np.zeros(o.nValidAct)
            o.new_episode(self.specs[e]["seed"])

    def restart(self, e, seed, r0=None):
        """``reset_envs([e], seed, r0)``: env e rebuilt from its spec with the new seed (and r0) -- new screens, a flat mirror,
        ``dm_prev`` = 0 and one measurement; the delay line, the disturbance's clock and every other env stay"""
        self.specs[e]["seed"] = int(seed)
        if r0 is not None:
            self.specs[e]["r0"] = float(r0)
        self.envs[e] = self._build(self.specs[e])
        self.new_episode([e])
        for x in self.fifo:                                         # the env's pending actions go too (TimeDelayEnv clears its rows)
            x[e] = 0
        return self.envs[e].reset_soft()

    def _clear_line(self):
        self.fifo = [np.zeros_like(x) for x in self.fifo]

    def reset_soft(self):
        self._clear_line()
        return np.stack([o.reset_soft() for o in self.envs])

    def _modal_obs(self, o):
        return -1e6 * (self.cm_K @ o.wfs.signal)

    def reset_soft_modal(self):
        self._clear_line()
        return np.stack([self._modal_obs(o) for o in self.envs])

    def _delayed(self, action):
        """TimeDelayEnv.step: append, apply the oldest, drop it"""
        self.fifo.append(np.array(action, copy=True))
        return self.fifo.pop(0)

    def _advance(self, i, applied):
        out = {q: [] for q in QUANTITIES}
        for e, o in enumerate(self.envs):
            b0 = [lay.buff.copy() for lay in o.atm.layers]
            first = [lay.notDoneOnce for lay in o.atm.layers]
            v = self.disturbance(e, i)
            if v is None:
                res = o.step(i, applied[e])
            else:
                o.coefs = o.coefs + v                               # what the sensor sees in frame i
                res = o.step(i, applied[e])                         # (step integrates dm_prev, the pure command, and replaces coefs)
            for l, lay in enumerate(o.atm.layers):
                ratio = np.abs(lay.ratio)                           # (set by the first update of an episode)
                self.whole_rounds[e, l] = int(ratio.astype(int).max())
                start = np.zeros(2) if first[l] else b0[l]
                self.crossed[e, l] = bool((np.abs(start + (ratio % 1) * np.sign(lay.ratio)) >= 1).any())
            for q, x in zip(QUANTITIES, (o.wfs.signal, res[0], res[2], res[3], res[1])):
                out[q].append(np.array(x, dtype=np.float64, copy=True))
        return {q: np.stack(x) for q, x in out.items()}

    def step(self, i, action):
        """``action`` [n, a, a] (float32 for a float32-representable action: NumPy then forms action * 1e-6 in float32, as the
        library does).  Returns dict(signal, obs, reward, strehl, frame), each stacked over the envs."""
        action = np.asarray(action)
        if action.shape[0] != self.n:
            raise ValueError("one action per env")
        return self._advance(i, self._delayed(action))

    def step_modal(self, i, a):
        """``a`` [n, K] modal coefficients; ``obs`` [n, K], ``reward`` = -sum(obs^2)"""
        a = np.asarray(a, dtype=np.float64)
        img = np.stack([o.vec_to_img(self.M2C_K @ a[e]) for e, o in enumerate(self.envs)])
        out = self._advance(i, self._delayed(img))
        out["obs"] = np.stack([self._modal_obs(o) for o in self.envs])
        out["reward"] = -(out["obs"] ** 2).sum(axis=1)
        return out

    # -- read-outs ---------------------------------------------------------------------------------------------------------------
    def screens(self):
        return [[lay.mapShift.copy() for lay in o.atm.layers] for o in self.envs]        # [env][layer][S, S]

    def residual_opd(self):
        return np.stack([o.tel_OPD.copy() for o in self.envs])

    def atm_opd(self):
        return np.stack([o.atm.OPD.copy() for o in self.envs])

    def telemetry(self, steps):
        return (np.stack([o.total[:steps] for o in self.envs], axis=1), np.stack([o.residual[:steps] for o in self.envs], axis=1))

    def gaps(self):
        """per env: the cut gap of the last frame at the env's threshold (Shack-Hartmann)"""
        return np.array([cut_gap(o.wfs.frame, o.wfs.thr) for o in self.envs]) if self.sh else np.full(self.n, np.inf)


# ---- the composed case of the issue: four envs, every per-env feature at once -----------------------------------------------------
PITCH_SMALL = 3.2 / 8                                               # actuator pitch of the 8 x 8 geometry [m]
CASE_MIXED = dict(
    r0=[0.13, 0.09, 0.16, 0.11],
    wind_speed=[10.0, 30.0, 22.0, 50.0],                           # env 3: 1.5 pixels per frame -> wind ceiling 2
    wind_dir=[72.0, 200.0, 144.0, 310.0],
    threshold=[0.01, 0.0, 0.05, 0.2],
    magnitude=[8.0, 5.5, 9.0, 12.0],
    misreg=[dict(), dict(shift_x=0.2), dict(shift_y=-0.1, tangential_scaling=0.01), dict(radial_scaling=0.02)],   # shifts in pitches
    dist_amp=[0.0, 2e-7, 1e-7, 3e-7],                              # metres on column 0 of M2C
    dist_period=[None, 40.0, 17.0, 9.0],                           # frames
    delay=1, wind_ceiling=2, n_envs=4, steps=12, seed=5, seed_stride=100, t0=0)
FEATURES = ("r0", "wind", "threshold", "magnitude", "misreg", "disturbance", "delay")


def mixed_misreg(e, pitch, case=CASE_MIXED):
    """env e's mis-registration in the units of the setters (shifts in metres)"""
    m = dict(case["misreg"][e])
    for k in ("shift_x", "shift_y"):
        if k in m:
            m[k] = m[k] * pitch
    return m


def mixed_specs(pitch, sh=True, case=CASE_MIXED, envs=None, off=()):
    """The env_spec list of CASE_MIXED.  ``envs``: which case env each env of the shard is (a twin shard: [e] * 4; the seeds stay
    those of the ROWS).  ``off``: features left at the base's values.  ``sh`` False (Pyramid): no thresholds."""
    rows = list(range(case["n_envs"])) if envs is None else list(envs)
    specs = []
    for row, e in enumerate(rows):
        specs.append(env_spec(
            seed=case["seed"] + case["seed_stride"] * row,
            r0=None if "r0" in off else case["r0"][e],
            wind_speed=None if "wind" in off else [case["wind_speed"][e]],
            wind_dir=None if "wind" in off else [case["wind_dir"][e]],
            threshold=None if ("threshold" in off or not sh) else case["threshold"][e],
            magnitude=None if "magnitude" in off else case["magnitude"][e],
            misreg=None if ("misreg" in off or not case["misreg"][e]) else mixed_misreg(e, pitch, case),
            dist_amp=None if "disturbance" in off else case["dist_amp"][e],
            dist_period=case["dist_period"][e]))
    return specs


def mixed_oracle(base, pitch, m2c=None, modal_cm=None, modal=None, modal_cm_K=None, case=CASE_MIXED, envs=None, off=(), sh=None):
    sh = (base.wfs_type == "sh") if sh is None else sh
    M2C = np.asarray(base.M2C if m2c is None else m2c, dtype=np.float64)
    return ComposedOracle(base, mixed_specs(pitch, sh, case, envs, off), m2c=m2c, modal_cm=modal_cm,
                          delay=0 if "delay" in off else case["delay"], dist_modes=None if "disturbance" in off else M2C[:, :1],
                          t0=case["t0"], modal=modal, modal_cm_K=modal_cm_K)


def drive(orc, steps, modal_gain=None, rs_seed=9, actions=None, events=None):
    """One closed-loop episode of ``orc`` from its reset: the actions are ``0.5 * obs + 0.05 * randn`` of RandomState(9), cast to
    float32 and masked (zonal), or ``modal_gain * obs`` cast to float32 (modal) -- or the recorded ``actions`` replayed.  Returns
    the record the GPU tests replay: per step the actions and every compared quantity, the conditions of the case (cut gap,
    crossings, whole-pixel rounds) from the oracle alone, and the end state.  ``events``: {frame: [(env, seed, r0), ...]} -- those envs are restarted (``restart``) in front of
    that frame, their rows of the observation replaced (``rec["reset_obs"]``: {frame: [obs, ...]})."""
    modal = modal_gain is not None
    orc.new_episode()
    rec = dict(obs0=orc.reset_soft_modal() if modal else orc.reset_soft(), screen0=orc.screens(), actions=[], gap=[orc.gaps()],
               rounds=[], crossed=[], **{q: [] for q in QUANTITIES})
    rs = np.random.RandomState(rs_seed)
    mask = orc.base.dm_mask[None].astype(np.float32)
    obs = rec["obs0"]
    rec["reset_obs"] = {}
    for i in range(steps):
        if events and i in events:
            obs = obs.copy()
            for e, seed, r0 in events[i]:
                obs[e] = orc.restart(e, seed, r0)
            rec["reset_obs"][i] = [obs[e].copy() for e, _, _ in events[i]]
        if actions is not None:
            act = actions[i]
        elif modal:
            act = (modal_gain * obs).astype(np.float32)
        else:
            act = (0.5 * obs + 0.05 * rs.randn(*obs.shape)).astype(np.float32) * mask
        out = orc.step_modal(i, act) if modal else orc.step(i, act)
        rec["actions"].append(act)
        for q in QUANTITIES:
            rec[q].append(out[q])
        rec["gap"].append(orc.gaps())
        rec["rounds"].append(orc.whole_rounds.copy())
        rec["crossed"].append(orc.crossed.copy())
        obs = out["obs"]
    rec["screen"] = orc.screens()
    rec["opd_res"] = orc.residual_opd()
    rec["opd_atm"] = orc.atm_opd()
    rec["total"], rec["residual"] = orc.telemetry(steps)
    rec["min_gap"] = float(np.min(rec["gap"]))
    rec["crossings"] = np.sum(rec["crossed"], axis=0)              # [env, layer]: steps on which the sub-pixel clock crossed a pixel
    rec["rounds"] = np.stack(rec["rounds"])                        # [step, env, layer]
    return rec
