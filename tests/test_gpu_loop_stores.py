"""GPU: the on-device loop (aoenv_run_integrator) leaves out the residual-phase and camera-frame stores of every step but its last
(StepArgs.store_phase / store_frame, the fused float32 step kernel).  Nothing a caller can see may change: a shard run with
run_integrator(i0, K) is compared BIT FOR BIT (torch.equal / np.array_equal) with a twin that makes
the same K steps through step(), fed the integrator's action gain * obs (gain 0.5: the product is the same float32 in the
kernel and in torch) -- the library's phase and frame buffers, the frame copied out by the last step (the d_frame argument: what
return_frame=True hands out) and the aliasing view (return_frame="view"), obs, reward, Strehl, the slopes, the telemetry of every
step and the checkpoint.

Geometries: the smallest the suite builds on the fused path -- the R = 24 and R = 48 golden geometries and the 10 x 10 lenslet one
of the geometry sweep (R = 60), 2-3 envs.  Winds are chosen so that the ring extrusion (the step kernel's deferred scatter with
its wait for the stores) falls on the last step or on the one before; the accumulators of the twin say where it fell.

The negative control fills the library's phase and frame buffers with a sentinel (aoenv_upload_state takes both) in front of a
K = 5 loop under a camera with read-out noise (every pixel of the frame is then written by a storing step): afterwards they hold
the twin's last step and no sentinel -- the last step of the loop stores.  That the other steps do NOT store cannot be seen from
outside a call (that is the point of the change); the sentinel test pins the half that can.
"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GAIN = 0.5
PS = 3.2 / 48                                                     # pixel size [m] of TINY and SMALL (the sweep's: 0.4 / 6, the same)
TINY = dict(diameter=1.6, nSubaperture=4, nPixelPerSubap=6, r0=0.13, L0=30.0, windSpeed=[10.0], windDirection=[72.0],
            fractionalR0=[1.0], altitude=[0.0], nModes=8, nLoop=16)
TINY3 = dict(TINY, windSpeed=[10.0, 12.0, 11.0], windDirection=[0.0, 72.0, 144.0],
             fractionalR0=[0.6923076923076923, 0.15384615384615385, 0.15384615384615385], altitude=[0.0, 0.0, 0.0])
SMALL = dict(diameter=3.2, nSubaperture=8, nPixelPerSubap=6, r0=0.13, L0=30.0, windSpeed=[10.0], windDirection=[72.0],
             fractionalR0=[1.0], altitude=[0.0], nModes=20, nLoop=16)
SWEEP10 = dict(diameter=4.0, nSubaperture=10, nPixelPerSubap=6, r0=0.13, L0=30.0, windSpeed=[0.45 * PS * 500.0], windDirection=[72.0],
               fractionalR0=[1.0], altitude=[0.0], nModes=30, nLoop=16)


def _along_x(px_per_frame):
    """one layer moving px_per_frame pixels per frame (500 Hz) along one axis: its crossings are at the multiples of 1 / px_per_frame"""
    return dict(windSpeed=[px_per_frame * PS * 500.0], windDirection=[0.0])


SENTINEL = -1.5e30

# geometry, envs, K, camera, per-env winds, store atm.OPD every step, sentinel, the steps that must be crossings (None: not asserted)
CASES = {
    "tiny_k1": dict(geo=TINY, n=2, K=1),
    "small_k1_photon": dict(geo=SMALL, n=2, K=1, cam="photon"),
    "small_k5_crossing_last": dict(geo=dict(SMALL, **_along_x(0.22)), n=2, K=5, crossings=[0, 0, 0, 0, 1]),
    "small_k5_crossing_before_last_readout": dict(geo=dict(SMALL, **_along_x(0.26)), n=2, K=5, cam="readout", sentinel=True,
                                                  crossings=[0, 0, 0, 1, 0]),
    "tiny3_k5_photon": dict(geo=TINY3, n=3, K=5, cam="photon"),
    "sweep10_k5": dict(geo=SWEEP10, n=3, K=5),
    "small_k5_per_env_winds": dict(geo=SMALL, n=3, K=5, winds=(np.array([[0.0], [17.0], [28.0]]), np.array([[0.0], [190.0], [270.0]]))),
    "small_k5_per_env_winds_readout": dict(geo=SMALL, n=3, K=5, cam="readout",
                                           winds=(np.array([[12.0], [24.0], [28.0]]), np.array([[-45.0], [135.0], [270.0]]))),
    "small_k3_store_atm": dict(geo=dict(SMALL, windSpeed=[25.0]), n=2, K=3, store_atm=True),
}


def _make(case, return_frame=True):
    from rlao_amd import _lib as L
    from rlao_amd.env import BatchedAOEnv
    env = BatchedAOEnv(n_envs=case["n"], device=0, dtype="f32", return_frame=return_frame)
    try:
        env.set_params(case["geo"], camera="ideal", wfs_type="shackhartmann", gainCL=GAIN)
        cam = case.get("cam")
        if cam == "photon":
            env.wfs.cam.photonNoise = True
        elif cam == "readout":                                      # the frame's pixels outside the valid lenslets are written too
            env.wfs.cam.configure(photonNoise=True, readoutNoise=3)
        if case.get("store_atm"):
            L.check(env._shard.lib.aoenv_set_option(env._shard.h, L.OPT_STORE_ATM_OPD, 1))
        assert env.fused_step                                       # the kernel this file is about
    except Exception:
        env.close()
        raise
    return env


def _start(env, case, seed=5):
    env.generate_new_phase_screen(seed)
    if case.get("winds") is not None:
        env.set_wind_per_env(case["winds"][0], case["winds"][1], reset=True)
    env.dm.coefs = 0
    env.dm_prev = 0
    env.measure()
    return env.reset_soft()


def _loop(env, i0, K):
    """env.run_integrator(i0, K) with a frame to copy the last step's into (aoenv_run_integrator's d_frame)"""
    import torch
    from rlao_amd import _lib as L
    env._obs = env._obs.clone()
    rew = torch.empty(env.n_envs, device=env.device, dtype=env.tdtype)
    sr = torch.empty_like(rew)
    frame = torch.full((env.n_envs, env.cam_res, env.cam_res), float("nan"), device=env.device, dtype=env.tdtype)
    L.check(env._shard.lib.aoenv_run_integrator(
        env._shard.h, int(i0), int(K), GAIN, C.c_void_p(env._obs.data_ptr()), C.c_void_p(frame.data_ptr()),
        C.c_void_p(rew.data_ptr()), C.c_void_p(sr.data_ptr()), C.c_void_p(env._stream())))
    env._reward, env._strehl = rew, sr
    return env._obs, frame, rew, sr


def _library_side(env, n_steps, store_atm=False):
    """what the library holds after the steps: buffers, telemetry, checkpoint"""
    from rlao_amd import _lib as L
    sh, n = env._shard, env.n_envs
    out = {
        "phase": sh.download(L.B_PHASE, (n, env.R, env.R), env._stream()),
        "frame": sh.download(L.B_FRAME, (n, env.cam_res, env.cam_res), env._stream()),
        "signal": sh.download(L.B_SIGNAL, (n, env.nSignal), env._stream()),
        "total": np.array(env.total[:n_steps]),
        "residual": np.array(env.residual[:n_steps]),
    }
    if store_atm:
        out["opd_atm"] = sh.download(L.B_OPD_ATM, (n, env.R, env.R), env._stream())
    for k, v in env.get_state().items():
        out["state." + k] = v
    return out


def _same(a, b, what):
    if isinstance(a, (tuple, list)):
        assert isinstance(b, (tuple, list)) and len(a) == len(b), what
        for i, (x, y) in enumerate(zip(a, b)):
            _same(x, y, f"{what}[{i}]")
    elif a is None or b is None:
        assert a is None and b is None, what
    else:
        assert np.array_equal(np.asarray(a), np.asarray(b)), what


def _assert_library_side_equal(got, want):
    assert got.keys() == want.keys()
    for k in want:
        _same(got[k], want[k], k)
    assert np.isfinite(want["phase"]).all() and np.abs(want["phase"]).max() > 0 and want["frame"].max() > 0
    assert (want["total"] > 0).all() and (want["residual"] > 0).all()


@pytest.mark.parametrize("name", list(CASES))
def test_loop_equals_stepping_bit_for_bit(name):
    import torch
    from rlao_amd import _lib as L
    case = CASES[name]
    K = case["K"]
    # the twin: K calls of step(), every one of which stores
    twin = _make(case)
    obs = _start(twin, case)
    crossed, before = [], 0.0
    for i in range(K):
        obs, frame, rew, sr, _, _ = twin.step(i, GAIN * obs)
        if case.get("crossings") is not None:                       # the accumulator falls back by one pixel at a crossing
            now = float(np.abs(twin._shard.get_buff(1)).sum())
            crossed.append(int(now < before))
            before = now
    torch.cuda.synchronize()
    if case.get("crossings") is not None:
        assert crossed == case["crossings"]
    want = _library_side(twin, K, case.get("store_atm", False))
    want_out = [t.clone() for t in (obs, frame, rew, sr)]
    twin.close()
    # the loop
    env = _make(case, return_frame="view")
    _start(env, case)
    if case.get("sentinel"):
        for which, shape in ((L.B_PHASE, (env.n_envs, env.R * env.R)), (L.B_FRAME, (env.n_envs, env.cam_res * env.cam_res))):
            env._shard.upload_state(which, np.full(shape, SENTINEL), env._stream())
        assert (env._shard.download(L.B_FRAME, (env.n_envs, env.cam_res, env.cam_res), env._stream()) == np.float32(SENTINEL)).all()
    got_out = _loop(env, 0, K)
    view = env._frame_alias()                                       # return_frame="view": the library's buffer itself
    torch.cuda.synchronize()
    for g, w, what in zip(got_out, want_out, ("obs", "frame (d_frame)", "reward", "strehl")):
        assert torch.equal(g, w), what
    assert torch.equal(view, want_out[1]), "frame (view)"
    got = _library_side(env, K, case.get("store_atm", False))
    env.close()
    _assert_library_side_equal(got, want)
    if case.get("sentinel"):
        assert not (got["phase"] == np.float32(SENTINEL)).any() and not (got["frame"] == np.float32(SENTINEL)).any()


@pytest.mark.parametrize("cam", [None, "readout"])
def test_step_after_two_loops_stores_again(cam):
    """run_integrator(0, 3), run_integrator(3, 2), then one step(): the per-call path stores after the loop path left stores out, and a
    loop that follows a loop starts from buffers the previous one wrote on its last step only."""
    import torch
    case = dict(geo=dict(SMALL, **_along_x(0.26)), n=2, cam=cam)
    twin = _make(case)
    obs = _start(twin, case)
    for i in range(6):
        obs, frame, rew, sr, _, _ = twin.step(i, GAIN * obs)
        if i == 4:
            mid = _library_side(twin, 5)
    torch.cuda.synchronize()
    want = _library_side(twin, 6)
    want_out = [t.clone() for t in (obs, frame, rew, sr)]
    twin.close()
    env = _make(case)
    _start(env, case)
    _loop(env, 0, 3)
    obs2, frame2, _, _ = _loop(env, 3, 2)
    _assert_library_side_equal(_library_side(env, 5), mid)
    assert torch.equal(frame2, torch.as_tensor(mid["frame"], device=frame2.device))
    got_out = env.step(5, GAIN * obs2)[:4]
    torch.cuda.synchronize()
    for g, w, what in zip(got_out, want_out, ("obs", "frame", "reward", "strehl")):
        assert torch.equal(g, w), what
    got = _library_side(env, 6)
    env.close()
    _assert_library_side_equal(got, want)
