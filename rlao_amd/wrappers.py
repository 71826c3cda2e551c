"""The thin wrappers drl4ao puts around its env (MAIN/PO4AO/util_simple.py), for the batched env.

``TorchWrapper`` (util_simple.py:201-221) converts torch <-> numpy around a NumPy env; the batched env
already speaks torch on the device, so here it only reproduces the *return convention* (float32
tensors, info as a list of pairs).  ``TimeDelayEnv`` (util_simple.py:25-52) is an action FIFO.
"""
from __future__ import annotations


def _torch():
    import torch
    return torch


def _env_rows(env, env_ids):
    """The listed envs in the caller's order (``normalize_env_ids`` checks them), as a host int64 array."""
    from .env import normalize_env_ids
    return normalize_env_ids(env_ids, getattr(env, "n_envs", 1), return_order=True)[1].astype("int64")


def _reset_envs(env, env_ids, seed, r0):
    """``env.reset_envs``; ``r0`` (a new Fried parameter for the listed envs) is passed on only when it is given."""
    return env.reset_envs(env_ids, seed) if r0 is None else env.reset_envs(env_ids, seed, r0=r0)


def _with_rows_cleared(buffered, rows):
    """Copies of the buffered actions with the rows of the listed envs zeroed (the buffered tensors are the caller's own)."""
    out = []
    for a in buffered:
        if hasattr(a, "clone"):
            a = a.clone()
            if a.dim() == 3:
                a[_torch().as_tensor(rows, device=a.device)] = 0
            elif len(rows):
                a.zero_()
        else:                                                       # the single-env NumPy flavour: one image
            a = a * 0 if len(rows) else a.copy()
        out.append(a)
    return out


class TorchWrapper:
    def __init__(self, env):
        self._env = env
        self.env = env

    def __getattr__(self, name):                 # gym.Wrapper attribute forwarding
        return getattr(self._env, name)

    def step(self, i, action):
        torch = _torch()
        if getattr(self._env, "output", "torch") == "numpy":
            next_obs, wfsf, reward, strehl, done, info = self._env.step(i, action.cpu().numpy())
            return (torch.tensor(next_obs, dtype=torch.float32), wfsf, reward, strehl, done,
                    [(k, torch.tensor(v, dtype=torch.float32)) for k, v in info.items()])
        next_obs, wfsf, reward, strehl, done, info = self._env.step(i, action)
        return next_obs.float(), wfsf, reward, strehl, done, [(k, v.float()) for k, v in info.items()]

    def reset(self):
        return _torch().as_tensor(self._env.reset(), dtype=_torch().float32)

    def reset_soft(self):
        return _torch().as_tensor(self._env.reset_soft(), dtype=_torch().float32)

    def reset_envs(self, env_ids, seed=None, r0=None):
        return _torch().as_tensor(_reset_envs(self._env, env_ids, seed, r0), dtype=_torch().float32)

    def set_dm_misregistration(self, *args, **kw):
        return self._env.set_dm_misregistration(*args, **kw)

    def set_dm_tables_per_env(self, gx, gy, env_ids=None):
        return self._env.set_dm_tables_per_env(gx, gy, env_ids)

    def clear_dm_per_env(self):
        return self._env.clear_dm_per_env()

    def set_dm_rotation(self, *args, **kw):
        return self._env.set_dm_rotation(*args, **kw)

    def set_dm_pairs_per_env(self, py, px, env_ids=None):
        return self._env.set_dm_pairs_per_env(py, px, env_ids)

    @property
    def dm_rotation(self):
        return self._env.dm_rotation

    @property
    def dm_misregistration(self):
        return self._env.dm_misregistration

    def set_magnitude_per_env(self, mag, env_ids=None):
        return self._env.set_magnitude_per_env(mag, env_ids)

    def set_threshold_per_env(self, thr, env_ids=None):
        return self._env.set_threshold_per_env(thr, env_ids)

    def clear_star_per_env(self):
        return self._env.clear_star_per_env()

    def change_mag(self, mag):
        return self._env.change_mag(mag)

    @property
    def magnitude(self):
        return self._env.magnitude

    @property
    def threshold_cog(self):
        return self._env.threshold_cog

    def set_r0_per_env(self, r0, env_ids=None):
        return self._env.set_r0_per_env(r0, env_ids)

    def step_modal(self, i, action):
        """``BatchedAOEnv.step_modal`` in this wrapper's return convention (``step``'s): a float32 modal observation."""
        torch = _torch()
        if getattr(self._env, "output", "torch") == "numpy":
            next_obs, wfsf, reward, strehl, done, info = self._env.step_modal(i, action.cpu().numpy())
            return (torch.tensor(next_obs, dtype=torch.float32), wfsf, reward, strehl, done,
                    [(k, torch.tensor(v, dtype=torch.float32)) for k, v in info.items()])
        next_obs, wfsf, reward, strehl, done, info = self._env.step_modal(i, action)
        return next_obs.float(), wfsf, reward, strehl, done, [(k, v.float()) for k, v in info.items()]

    def reset_soft_modal(self):
        return _torch().as_tensor(self._env.reset_soft_modal(), dtype=_torch().float32)

    def run_integrator_modal(self, i0, n_steps):
        """``BatchedAOEnv.run_integrator_modal`` in this wrapper's return convention: float32 tensors."""
        return tuple(_torch().as_tensor(t).float() for t in self._env.run_integrator_modal(i0, n_steps))

    def set_wavefront_basis(self, m2opd=None, opd2m=None, n_modes=None):
        return self._env.set_wavefront_basis(m2opd=m2opd, opd2m=opd2m, n_modes=n_modes)

    def clear_wavefront_basis(self):
        return self._env.clear_wavefront_basis()

    @property
    def n_wavefront_modes(self):
        return self._env.n_wavefront_modes

    def project_wavefront(self, what="residual"):
        """``BatchedAOEnv.project_wavefront`` in this wrapper's return convention: a float32 tensor."""
        return _torch().as_tensor(self._env.project_wavefront(what), dtype=_torch().float32)

    def record_wavefront(self, i0, n_steps, what=("residual",)):
        """``BatchedAOEnv.record_wavefront``: the record itself, in the env dtype (the library writes into this very tensor)."""
        return self._env.record_wavefront(i0, n_steps, what)

    def stop_wavefront_record(self):
        return self._env.stop_wavefront_record()

    def set_science(self, zero_padding=4, window=None, first_frame=16, log10=False, dft=None):
        return self._env.set_science(zero_padding=zero_padding, window=window, first_frame=first_frame, log10=log10, dft=dft)

    def clear_science(self):
        return self._env.clear_science()

    @property
    def science(self):
        return self._env.science

    def science_psf(self, flat=False):
        return self._env.science_psf(flat)

    def set_science_direction(self, zenith, azimuth=0.0, env_ids=None):
        return self._env.set_science_direction(zenith, azimuth, env_ids)

    def clear_science_direction(self):
        return self._env.clear_science_direction()

    @property
    def science_direction(self):
        return self._env.science_direction

    def set_guide_direction(self, zenith, azimuth=0.0, env_ids=None):
        return self._env.set_guide_direction(zenith, azimuth, env_ids)

    def clear_guide_direction(self):
        return self._env.clear_guide_direction()

    @property
    def guide_direction(self):
        return self._env.guide_direction

    def set_static_aberration(self, wfs=None, science=None, env_ids=None):
        return self._env.set_static_aberration(wfs, science, env_ids)

    def clear_static_aberration(self):
        return self._env.clear_static_aberration()

    def ncpa_map(self, f2=None, coefficients=None, seed=5, basis="zernike"):
        return self._env.ncpa_map(f2, coefficients, seed, basis)

    @property
    def static_aberration(self):
        return self._env.static_aberration

    def set_lgs_per_env(self, Na_profile=None, FWHM_spot_up=None, laser_coordinates=None, env_ids=None):
        return self._env.set_lgs_per_env(Na_profile, FWHM_spot_up, laser_coordinates, env_ids)

    def clear_lgs_per_env(self):
        return self._env.clear_lgs_per_env()

    @property
    def lgs(self):
        return self._env.lgs

    @property
    def src(self):
        return self._env.src

    def science_residual(self):
        return self._env.science_residual()

    def science_atmosphere(self):
        return self._env.science_atmosphere()

    def record_science_direction(self, i0, n_steps):
        """``BatchedAOEnv.record_science_direction``: the record itself, in the env dtype (the library writes into this very tensor)."""
        return self._env.record_science_direction(i0, n_steps)

    def stop_science_direction_record(self):
        return self._env.stop_science_direction_record()

    def long_exposure(self):
        return self._env.long_exposure()

    def long_exposure_log10(self):
        return self._env.long_exposure_log10()

    def long_exposure_strehl(self):
        return self._env.long_exposure_strehl()

    def start_long_exposure(self):
        return self._env.start_long_exposure()

    def zero_long_exposure(self, env_ids=None):
        return self._env.zero_long_exposure(env_ids)

    def stop_long_exposure(self):
        return self._env.stop_long_exposure()

    def rollout(self, i0, n_steps, sigma, gain=None, seed=None, sigma_env=None):
        """``BatchedAOEnv.rollout`` in this wrapper's return convention: float32 tensors."""
        torch = _torch()
        tr = self._env.rollout(i0, n_steps, sigma, gain=gain, seed=seed, sigma_env=sigma_env)
        return type(tr)(*(torch.as_tensor(t).float() for t in tr))

    def set_policy(self, policy, F=True, clamp=1.0, path=0):
        return self._env.set_policy(policy, F=F, clamp=clamp, path=path)

    def policy_action(self, obs, past_obs=None, past_act=None):
        """``BatchedAOEnv.policy_action`` in this wrapper's return convention: a float32 tensor."""
        return _torch().as_tensor(self._env.policy_action(obs, past_obs, past_act)).float()

    def policy_rollout(self, i0, n_steps, sigma=0.0, past=None, seed=None, sigma_env=None):
        """``BatchedAOEnv.policy_rollout`` in this wrapper's return convention: float32 tensors (the windows too: on a float64
        shard pass the env's own windows to the next call where the last bits matter)."""
        torch = _torch()
        tr, past = self._env.policy_rollout(i0, n_steps, sigma=sigma, past=past, seed=seed, sigma_env=sigma_env)
        return type(tr)(*(torch.as_tensor(t).float() for t in tr)), tuple(torch.as_tensor(t).float() for t in past)


class TimeDelayEnv:
    """Control delay of ``delay`` frames: the env receives the action issued ``delay`` steps earlier."""

    def __init__(self, env, delay):
        self._env = env
        self.env = env
        self.d = int(delay)
        self.action_buffer = []
        self._fill()

    def __getattr__(self, name):
        return getattr(self._env, name)

    def _zero(self):
        e = self._env
        if getattr(e, "output", "torch") == "numpy":
            import numpy as np
            return np.zeros((e.nActuator, e.nActuator))
        return _torch().zeros((e.n_envs, e.nActuator, e.nActuator), device=e.device, dtype=e.tdtype)

    def _fill(self):
        self.action_buffer = [self._zero() for _ in range(self.d)]

    def reset(self):
        obs = self._env.reset()
        self._fill()
        return obs

    def reset_soft(self):
        obs = self._env.reset_soft()
        self._fill()
        return obs

    def reset_envs(self, env_ids, seed=None, r0=None):
        """A new episode for the listed envs (``BatchedAOEnv.reset_envs``): their rows of the delayed actions are cleared too."""
        rows = _env_rows(self._env, env_ids)
        obs = _reset_envs(self._env, env_ids, seed, r0)
        self.action_buffer = _with_rows_cleared(self.action_buffer, rows)
        return obs

    def set_dm_misregistration(self, *args, **kw):
        return self._env.set_dm_misregistration(*args, **kw)

    def set_dm_tables_per_env(self, gx, gy, env_ids=None):
        return self._env.set_dm_tables_per_env(gx, gy, env_ids)

    def clear_dm_per_env(self):
        return self._env.clear_dm_per_env()

    def set_dm_rotation(self, *args, **kw):
        return self._env.set_dm_rotation(*args, **kw)

    def set_dm_pairs_per_env(self, py, px, env_ids=None):
        return self._env.set_dm_pairs_per_env(py, px, env_ids)

    @property
    def dm_rotation(self):
        return self._env.dm_rotation

    @property
    def dm_misregistration(self):
        return self._env.dm_misregistration

    def set_magnitude_per_env(self, mag, env_ids=None):
        return self._env.set_magnitude_per_env(mag, env_ids)

    def set_threshold_per_env(self, thr, env_ids=None):
        return self._env.set_threshold_per_env(thr, env_ids)

    def clear_star_per_env(self):
        return self._env.clear_star_per_env()

    def change_mag(self, mag):
        return self._env.change_mag(mag)

    @property
    def magnitude(self):
        return self._env.magnitude

    @property
    def threshold_cog(self):
        return self._env.threshold_cog

    def set_r0_per_env(self, r0, env_ids=None):
        return self._env.set_r0_per_env(r0, env_ids)

    def set_wavefront_basis(self, m2opd=None, opd2m=None, n_modes=None):
        return self._env.set_wavefront_basis(m2opd=m2opd, opd2m=opd2m, n_modes=n_modes)

    def clear_wavefront_basis(self):
        return self._env.clear_wavefront_basis()

    @property
    def n_wavefront_modes(self):
        return self._env.n_wavefront_modes

    def project_wavefront(self, what="residual"):
        return self._env.project_wavefront(what)

    def set_science(self, zero_padding=4, window=None, first_frame=16, log10=False, dft=None):
        return self._env.set_science(zero_padding=zero_padding, window=window, first_frame=first_frame, log10=log10, dft=dft)

    def clear_science(self):
        return self._env.clear_science()

    @property
    def science(self):
        return self._env.science

    def science_psf(self, flat=False):
        return self._env.science_psf(flat)

    def set_science_direction(self, zenith, azimuth=0.0, env_ids=None):
        return self._env.set_science_direction(zenith, azimuth, env_ids)

    def clear_science_direction(self):
        return self._env.clear_science_direction()

    @property
    def science_direction(self):
        return self._env.science_direction

    def set_guide_direction(self, zenith, azimuth=0.0, env_ids=None):
        return self._env.set_guide_direction(zenith, azimuth, env_ids)

    def clear_guide_direction(self):
        return self._env.clear_guide_direction()

    @property
    def guide_direction(self):
        return self._env.guide_direction

    def set_static_aberration(self, wfs=None, science=None, env_ids=None):
        return self._env.set_static_aberration(wfs, science, env_ids)

    def clear_static_aberration(self):
        return self._env.clear_static_aberration()

    def ncpa_map(self, f2=None, coefficients=None, seed=5, basis="zernike"):
        return self._env.ncpa_map(f2, coefficients, seed, basis)

    @property
    def static_aberration(self):
        return self._env.static_aberration

    def set_lgs_per_env(self, Na_profile=None, FWHM_spot_up=None, laser_coordinates=None, env_ids=None):
        return self._env.set_lgs_per_env(Na_profile, FWHM_spot_up, laser_coordinates, env_ids)

    def clear_lgs_per_env(self):
        return self._env.clear_lgs_per_env()

    @property
    def lgs(self):
        return self._env.lgs

    @property
    def src(self):
        return self._env.src

    def science_residual(self):
        return self._env.science_residual()

    def science_atmosphere(self):
        return self._env.science_atmosphere()

    def long_exposure(self):
        return self._env.long_exposure()

    def long_exposure_log10(self):
        return self._env.long_exposure_log10()

    def long_exposure_strehl(self):
        return self._env.long_exposure_strehl()

    def step(self, i, action):
        self.action_buffer.append(action)
        out = self._env.step(i, self.action_buffer[0])
        del self.action_buffer[0]
        return out

    def step_modal(self, i, action):
        """Refused: this FIFO holds action images for ``step``.  A modal loop takes its delay from the library --
        ``env.set_delay(d)`` -- which ``step_modal`` and ``run_integrator_modal`` honour on the device."""
        raise NotImplementedError("TimeDelayEnv delays step() only: use env.set_delay(d) for step_modal / run_integrator_modal")

    def run_integrator_modal(self, i0, n_steps):
        raise NotImplementedError("TimeDelayEnv delays step() only: use env.set_delay(d) for step_modal / run_integrator_modal")

    def rollout(self, *args, **kw):
        raise NotImplementedError(
            "TimeDelayEnv cannot run rollout(): the library loop applies action k in step k, and this wrapper exists to apply it "
            f"{self.d} step(s) later; step the wrapper frame by frame, or call rollout() on the env it wraps")

    def policy_rollout(self, *args, **kw):
        raise NotImplementedError(
            "TimeDelayEnv cannot run policy_rollout(): the library loop applies action k in step k, and this wrapper exists to apply it "
            f"{self.d} step(s) later; step the wrapper frame by frame, or call policy_rollout() on the env it wraps")


class Box:
    """Minimal stand-in for ``gym.spaces.Box`` (gymnasium is not a dependency of the env)."""

    def __init__(self, low, high, shape, dtype="float32"):
        self.low, self.high, self.shape, self.dtype = low, high, tuple(shape), dtype

    def __repr__(self):
        return f"Box({self.low}, {self.high}, {self.shape}, {self.dtype})"


class DeviceHistory:
    """Sliding window of the last ``n_history`` images of every env, newest first, on the device: a MIRRORED ring buffer
    ``[n, 2 H, A, A]`` -- every image is written to slots p and p + H, so the window ``buf[:, p : p + H]`` is always one
    contiguous-in-time view.  A push is two slot writes (2 x n x A x A elements); nothing is rolled or concatenated (the
    reference rolls the whole history every step, OOPAOEnv_VPG.py:660-681: 131 MB per step at 1024 envs of the 41 x 41 DM)."""

    def __init__(self, n, n_history, n_act, device, dtype=None):
        torch = _torch()
        self.H = int(n_history)
        self.buf = torch.zeros((n, 2 * self.H, n_act, n_act), device=device, dtype=dtype or torch.float32)
        self.p = 0

    def push(self, img):
        self.p = (self.p - 1) % self.H
        self.buf[:, self.p] = img
        self.buf[:, self.p + self.H] = img

    def window(self):
        """[n, H, A, A] view, newest image at index 0."""
        return self.buf[:, self.p:self.p + self.H]

    def clear(self):
        self.buf.zero_()
        self.p = 0


class HistoryEnv:
    """gymnasium-style facade with the observation history kept on the device
    (MAIN/OOPAOEnv/OOPAOEnv_VPG.py:77-95 spaces, :553-608 step, :660-681 roll_buffer):

    * ``step(action) -> (obs_history, reward, terminated, truncated, info)`` -- no frame index argument; the wrapper
      counts frames itself (and wraps at ``nLoop``, the length of the env's telemetry);
    * ``obs_history`` is ``[n_envs, n_history, nAct, nAct]`` (``[n_history, nAct, nAct]`` for one env), newest image
      at index 0, rolled one slot per step;
    * the reward is the Strehl ratio (``reward = strehl``, :601-603);
    * actions pass through a FIFO of ``delay`` frames (``action_buffer``, :562-566), a 1-D action is first scattered to
      the actuator image (``vec_to_img``, :559-560).

    Nothing leaves the device for a batched env; for the single-env NumPy flavour the history is returned as a NumPy
    array like the reference's ``obs_history.cpu().numpy()``."""

    def __init__(self, env, n_history=20, delay=1):
        if delay < 1:
            raise ValueError("delay must be >= 1 (the reference applies action_buffer[0] after appending the new action)")
        self._env = env
        self.env = env
        self.n_history = int(n_history)
        self.delay = int(delay)
        self.t = 0
        A = env.nActuator
        self.single = getattr(env, "output", "torch") == "numpy"
        lead = () if self.single or env.n_envs == 1 else (env.n_envs,)
        self.observation_space = Box(-float("inf"), float("inf"), lead + (self.n_history, A, A))
        self.action_space = Box(-10.0, 10.0, lead + (A, A))
        self._alloc()

    def __getattr__(self, name):
        return getattr(self._env, name)

    def set_wavefront_basis(self, m2opd=None, opd2m=None, n_modes=None):
        return self._env.set_wavefront_basis(m2opd=m2opd, opd2m=opd2m, n_modes=n_modes)

    def clear_wavefront_basis(self):
        return self._env.clear_wavefront_basis()

    @property
    def n_wavefront_modes(self):
        return self._env.n_wavefront_modes

    def project_wavefront(self, what="residual"):
        return self._env.project_wavefront(what)

    def set_science(self, zero_padding=4, window=None, first_frame=16, log10=False, dft=None):
        return self._env.set_science(zero_padding=zero_padding, window=window, first_frame=first_frame, log10=log10, dft=dft)

    def clear_science(self):
        return self._env.clear_science()

    @property
    def science(self):
        return self._env.science

    def science_psf(self, flat=False):
        return self._env.science_psf(flat)

    def set_science_direction(self, zenith, azimuth=0.0, env_ids=None):
        return self._env.set_science_direction(zenith, azimuth, env_ids)

    def clear_science_direction(self):
        return self._env.clear_science_direction()

    @property
    def science_direction(self):
        return self._env.science_direction

    def set_guide_direction(self, zenith, azimuth=0.0, env_ids=None):
        return self._env.set_guide_direction(zenith, azimuth, env_ids)

    def clear_guide_direction(self):
        return self._env.clear_guide_direction()

    @property
    def guide_direction(self):
        return self._env.guide_direction

    def set_static_aberration(self, wfs=None, science=None, env_ids=None):
        return self._env.set_static_aberration(wfs, science, env_ids)

    def clear_static_aberration(self):
        return self._env.clear_static_aberration()

    def ncpa_map(self, f2=None, coefficients=None, seed=5, basis="zernike"):
        return self._env.ncpa_map(f2, coefficients, seed, basis)

    @property
    def static_aberration(self):
        return self._env.static_aberration

    def set_lgs_per_env(self, Na_profile=None, FWHM_spot_up=None, laser_coordinates=None, env_ids=None):
        return self._env.set_lgs_per_env(Na_profile, FWHM_spot_up, laser_coordinates, env_ids)

    def clear_lgs_per_env(self):
        return self._env.clear_lgs_per_env()

    @property
    def lgs(self):
        return self._env.lgs

    @property
    def src(self):
        return self._env.src

    def science_residual(self):
        return self._env.science_residual()

    def science_atmosphere(self):
        return self._env.science_atmosphere()

    def long_exposure(self):
        return self._env.long_exposure()

    def long_exposure_log10(self):
        return self._env.long_exposure_log10()

    def long_exposure_strehl(self):
        return self._env.long_exposure_strehl()

    def _alloc(self):
        torch = _torch()
        e = self._env
        dev = getattr(e, "device", "cpu")
        n = 1 if self.single else e.n_envs
        A = e.nActuator
        self._hist = DeviceHistory(n, self.n_history, A, dev)
        self.action_buffer = [torch.zeros((n, A, A), device=dev, dtype=torch.float32) for _ in range(self.delay - 1)]

    @property
    def obs_history(self):
        """[n, n_history, nAct, nAct], newest first: a view of the mirrored ring buffer (valid until the next step)."""
        return self._hist.window()

    def _out(self):
        if self.single:
            return self.obs_history[0].cpu().numpy()
        return self.obs_history[0] if self._env.n_envs == 1 else self.obs_history

    def reset(self, seed=None, options=None):
        """New turbulence (``generateNewPhaseScreen(seed)``), flat DM, one measurement, empty histories."""
        e = self._env
        e.atm.generateNewPhaseScreen(seed)
        e.dm.coefs = 0
        e.dm_prev = 0                                           # reset() also clears the integrator state (OOPAOEnv_VPG.py:120-121)
        e.tel * e.dm * e.wfs
        obs = _torch().as_tensor(e.reset_soft(), dtype=_torch().float32)
        self._alloc()
        self.t = 0
        self._push(obs)
        return self._out(), {}

    def set_dm_misregistration(self, *args, **kw):
        return self._env.set_dm_misregistration(*args, **kw)

    def set_dm_tables_per_env(self, gx, gy, env_ids=None):
        return self._env.set_dm_tables_per_env(gx, gy, env_ids)

    def clear_dm_per_env(self):
        return self._env.clear_dm_per_env()

    def set_dm_rotation(self, *args, **kw):
        return self._env.set_dm_rotation(*args, **kw)

    def set_dm_pairs_per_env(self, py, px, env_ids=None):
        return self._env.set_dm_pairs_per_env(py, px, env_ids)

    @property
    def dm_rotation(self):
        return self._env.dm_rotation

    @property
    def dm_misregistration(self):
        return self._env.dm_misregistration

    def set_magnitude_per_env(self, mag, env_ids=None):
        return self._env.set_magnitude_per_env(mag, env_ids)

    def set_threshold_per_env(self, thr, env_ids=None):
        return self._env.set_threshold_per_env(thr, env_ids)

    def clear_star_per_env(self):
        return self._env.clear_star_per_env()

    def change_mag(self, mag):
        return self._env.change_mag(mag)

    @property
    def magnitude(self):
        return self._env.magnitude

    @property
    def threshold_cog(self):
        return self._env.threshold_cog

    def set_r0_per_env(self, r0, env_ids=None):
        """Every env its own Fried parameter (``BatchedAOEnv.set_r0_per_env``); histories and delayed actions go on."""
        return self._env.set_r0_per_env(r0, env_ids)

    def reset_envs(self, env_ids, seed=None, r0=None):
        """``reset()`` for the listed envs only (``BatchedAOEnv.reset_envs``): new turbulence, flat DM and one measurement for them;
        their history rows restart as ``reset()`` starts the whole batch -- empty but for the new observation in the newest slot -- and
        their rows of the delayed actions are cleared.  The other envs' histories, and the frame counter, go on.  Returns the windows
        of the listed envs ``[k, n_history, nAct, nAct]`` in the order of ``env_ids``: a fresh tensor (a NumPy array for the single-env
        flavour), not a view of the ring buffer."""
        torch = _torch()
        h = self._hist
        rows = _env_rows(self._env, env_ids)
        obs = torch.as_tensor(_reset_envs(self._env, env_ids, seed, r0), dtype=torch.float32, device=h.buf.device)
        if obs.dim() == 2:
            obs = obs.unsqueeze(0)
        sel = torch.as_tensor(rows, device=h.buf.device)
        h.buf[sel] = 0
        if len(rows):
            h.buf[sel, h.p] = obs
            h.buf[sel, h.p + h.H] = obs
        self.action_buffer = _with_rows_cleared(self.action_buffer, rows)
        win = h.window()[sel]                                       # (advanced indexing: a copy)
        return win.cpu().numpy() if self.single else win

    def rollout(self, n_steps, sigma, gain=None, seed=None, sigma_env=None):
        """``BatchedAOEnv.rollout`` from this wrapper's frame counter on (no frame index argument, as ``step``; a run that
        reaches ``nLoop`` is cut there and goes on at frame 0, like ``step``'s counter).  Returns the env's trajectory (a list of
        them where the run was cut); the device history is refilled from the tail of the trajectory, so that ``obs_history`` is what
        ``n_steps`` calls of ``step`` with those actions would have left.  Needs ``delay == 1``: the library loop applies action k
        in step k."""
        if self.delay != 1:
            raise NotImplementedError(f"HistoryEnv.rollout: delay is {self.delay}, the library loop applies action k in step k (delay 1)")
        e = self._env
        n_loop = int(e.param.nLoop) if hasattr(e, "param") else 1 << 30
        parts, left = [], int(n_steps)
        while left > 0:
            i = self.t % n_loop
            n = min(left, n_loop - i)
            tr = e.rollout(i, n, sigma, gain=gain, seed=seed, sigma_env=sigma_env)
            seed = None                                             # (the next part continues the stream)
            obs = tr.obs if len(tr.obs.shape) == 4 else tr.obs[:, None]
            for k in range(max(1, n + 1 - self.n_history), n + 1):
                self._push(obs[k])
            self.t += n
            left -= n
            parts.append(tr)
        if not parts:
            return e.rollout(self.t % n_loop, 0, sigma, gain=gain, seed=seed, sigma_env=sigma_env)
        return parts[0] if len(parts) == 1 else parts

    def _push(self, obs):
        torch = _torch()
        obs = torch.as_tensor(obs, dtype=torch.float32, device=self._hist.buf.device)
        if obs.dim() == 2:
            obs = obs.unsqueeze(0)
        self._hist.push(obs)

    def step(self, action):
        torch = _torch()
        e = self._env
        a = torch.as_tensor(action, dtype=torch.float32, device=self._hist.buf.device)
        if a.shape[-1] != e.nActuator or a.dim() == 1 or (a.dim() == 2 and not self.single and e.n_envs > 1):
            a = e.vec_to_img(a, True)                              # command vector(s) -> actuator image(s)
        if a.dim() == 2:
            a = a.unsqueeze(0)
        self.action_buffer.append(a)
        act = self.action_buffer.pop(0)
        n_loop = int(e.param.nLoop) if hasattr(e, "param") else 1 << 30
        i = self.t % n_loop
        self.t += 1
        obs, _, _, strehl, _, info = e.step(i, act[0].cpu().numpy() if self.single else act)
        self._push(obs)
        terminated = truncated = False
        if not self.single and e.n_envs > 1:
            terminated = torch.zeros(e.n_envs, dtype=torch.bool, device=self._hist.buf.device)
            truncated = terminated.clone()
        return self._out(), strehl, terminated, truncated, {"strehl": strehl}
