"""GPU: the fused step kernel's instantiations specialised on what is constant for a launch (fast trig; the camera off, photon
noise only, or any other camera) and the register-pair form of the 6-pixel lenslet transform, against the general instantiation
and the plain transform that AOENV_PATH_SH_PLAIN forces.  Both compute the same products in the same order, so everything a caller
can see must be the same BIT FOR BIT (torch.equal): obs, reward, Strehl, the frame, the slopes, the residual phase, dm.coefs and
the total / residual telemetry of every step.

Every case runs two float32 shards of 2 envs on the same seeds for 6 steps under a wind that crosses a pixel inside them (the
launch record shows the ring GEMM), one shard as it comes and one with AOENV_PATH_SH_PLAIN; the launch record of both must show
the fused kernel and none of the batched ones.  Geometries are the smallest that reach each instantiation and each edge:

    R = 24, 4 x 4   one wave of lenslets, most lanes idle; pupil-edge pixels with zero amplitude inside valid lenslets
    R = 48, 8 x 8   lenslets over three waves, the last one partial
    R = 36, 6 x 6   R % 16 != 0: lanes past the row end in stage A; four-pixel groups that straddle two lenslets
    R = 42, 7 x 7   outside the fused kernel's envelope (step_fused_supported: R % 4 == 0), so both shards run the batched
                    kernels there -- asserted -- and the case compares k_sh_spots_p6<float> in its two forms at an odd geometry,
                    lenslet rows of which the second wave of a workgroup has none.  (A central obstruction of 0.2 takes the
                    middle lenslet away, 36 valid ones.)  R = 36 is the nearest shape inside the envelope.
    R = 72, 12 x 12 with a second 12 x 12 mirror: 26 actuators across (KS = 8), and a second pass of stage A

each with the camera off, photon noise and the Razor camera where listed; three layers, per-env winds (PE), AOENV_OPT_FAST_TRIG = 0
(the general kernel on both sides) and the batched spots kernel k_sh_spots_p6<float> with and without the bit.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GAIN = 0.5
STEPS = 6
WIND = dict(windSpeed=[50.0], windDirection=[200.0])              # tests/golden/tiny_fastwind.npz: 1.5 pixels per frame
_G = dict(nPixelPerSubap=6, r0=0.13, L0=30.0, fractionalR0=[1.0], altitude=[0.0], nLoop=16, **WIND)
R24 = dict(_G, diameter=1.6, nSubaperture=4, nModes=8)
R48 = dict(_G, diameter=3.2, nSubaperture=8, nModes=20)
R36 = dict(_G, diameter=2.4, nSubaperture=6, nModes=8)
R42 = dict(_G, diameter=2.8, nSubaperture=7, nModes=10, centralObstruction=0.2)
R72 = dict(_G, diameter=4.8, nSubaperture=12, nModes=20)
GEO = {"r24": R24, "r48": R48, "r36": R36, "r42": R42, "r72": R72}
FUSED = {"r24": True, "r48": True, "r36": True, "r42": False, "r72": True}
THREE = dict(windSpeed=[50.0, 12.0, 31.0], windDirection=[200.0, 72.0, 144.0],
             fractionalR0=[0.6923076923076923, 0.15384615384615385, 0.15384615384615385], altitude=[0.0, 0.0, 0.0])
CAMERA = {"off": "ideal", "photon": "papyrus", "razor": "razor"}

# geometry, camera, and: layers = 3, winds = per-env (speed, direction), second_dm, opts on BOTH shards, fused expected
CASES = {f"{g}_{c}": dict(geo=g, cam=c) for g in ("r24", "r48", "r36", "r42") for c in ("off", "photon", "razor")}
CASES.update({
    "r24_photon_three_layers": dict(geo="r24", cam="photon", three=True),
    "r48_razor_three_layers": dict(geo="r48", cam="razor", three=True),
    "r36_off_three_layers": dict(geo="r36", cam="off", three=True),
    "r42_off_three_layers": dict(geo="r42", cam="off", three=True),
    "r48_photon_per_env_winds": dict(geo="r48", cam="photon", winds=(np.array([[12.0], [28.0]]), np.array([[-45.0], [270.0]]))),
    "r72_photon_second_dm": dict(geo="r72", cam="photon", second_dm=dict(nSubaperture=12)),
    "r48_photon_sincosf": dict(geo="r48", cam="photon", opts={"OPT_FAST_TRIG": 0}),
    "r48_photon_batched": dict(geo="r48", cam="photon", path="PATH_GENERIC", fused=False),
    "r24_off_batched": dict(geo="r24", cam="off", path="PATH_GENERIC", fused=False),
})
BATCHED_KERNELS = ("phase", "sh_spots", "sh_centroid", "sh_tail", "gemm_recon", "recon_finish", "detector")


def _run(case, plain):
    """6 closed-loop steps of one shard; per step everything a caller can see, and the launch record of the steps"""
    import torch
    from rlao_amd import _lib as L
    from rlao_amd.env import BatchedAOEnv
    geo = dict(GEO[case["geo"]], **(THREE if case.get("three") else {}))
    env = BatchedAOEnv(n_envs=2, device=0, dtype="f32")
    try:
        env.set_params(geo, camera=CAMERA[case["cam"]], wfs_type="shackhartmann", gainCL=GAIN, second_dm=case.get("second_dm"))
        sh = env._shard
        for k, v in case.get("opts", {}).items():
            L.check(sh.lib.aoenv_set_option(sh.h, getattr(L, k), v))
        path = (getattr(L, case["path"]) if case.get("path") else 0) | (L.PATH_SH_PLAIN if plain else 0)
        L.check(sh.lib.aoenv_set_option(sh.h, L.OPT_FORCE_PATH, path))
        fused = case.get("fused", FUSED[case["geo"]])
        assert env.fused_step == fused, "AOENV_PATH_SH_PLAIN must leave the shard on the path it was on"
        env.generate_new_phase_screen(11)
        if case.get("winds") is not None:
            env.set_wind_per_env(case["winds"][0], case["winds"][1], reset=True)
        env.dm.coefs = 0
        env.dm_prev = 0
        env.measure()
        obs = env.reset_soft()
        rec = [("obs0", obs.clone())]
        sh.profile(True)
        for i in range(STEPS):
            obs, frame, rew, sr, _, _ = env.step(i, GAIN * obs)
            st, n = env._stream(), env.n_envs
            rec += [(f"obs[{i}]", obs.clone()), (f"reward[{i}]", rew.clone()), (f"strehl[{i}]", sr.clone()), (f"frame[{i}]", frame.clone())]
            rec += [(f"{what}[{i}]", torch.from_numpy(sh.download(which, shape, st)))
                    for what, which, shape in (("signal", L.B_SIGNAL, (n, env.nSignal)), ("phase", L.B_PHASE, (n, env.R, env.R)),
                                               ("dm.coefs", L.B_COEFS, (n, env.nValidAct)))]
        torch.cuda.synchronize()
        prof = sh.profile_read(env._stream())
        sh.profile(False)
        rec += [("total", torch.from_numpy(np.array(env.total[:STEPS]))), ("residual", torch.from_numpy(np.array(env.residual[:STEPS])))]
        shape = dict(R=env.R, n_act=env.nActuator, n_valid=env.nSignal // 2, layers=env.param.nLayer)
    finally:
        env.close()
    return rec, prof, shape


@pytest.mark.parametrize("name", list(CASES))
def test_specialised_equals_general_bit_for_bit(name):
    import torch
    case = CASES[name]
    got, prof_got, shape = _run(case, plain=False)
    want, prof_want, _ = _run(case, plain=True)
    # the kernels that ran, on both sides: the fused step (or, in the batched cases, none of it), and a ring crossing among the steps
    for prof in (prof_got, prof_want):
        launches = {k: v[1] for k, v in prof.items()}
        if case.get("fused", FUSED[case["geo"]]):
            assert launches["env_step"] == STEPS, launches
            assert all(launches[k] == 0 for k in BATCHED_KERNELS), launches
        else:
            assert launches["env_step"] == 0 and launches["sh_spots"] == STEPS, launches
        assert launches["gemm_ring"] > 0, launches
    # the shape is the one this case is here for
    assert shape["R"] == {"r24": 24, "r48": 48, "r36": 36, "r42": 42, "r72": 72}[case["geo"]]
    assert shape["layers"] == (3 if case.get("three") else 1)
    assert (shape["n_act"] > 24) == (case["geo"] == "r72")
    assert len(got) == len(want)
    for (what, a), (what_b, b) in zip(got, want):
        assert what == what_b and a.dtype == b.dtype and a.shape == b.shape, what
        assert torch.equal(a, b), (name, what, float((a.double() - b.double()).abs().max()))
    # ... of a loop that did something
    last = dict(got)
    assert torch.isfinite(last[f"phase[{STEPS - 1}]"]).all() and float(last[f"phase[{STEPS - 1}]"].abs().max()) > 0
    assert float(last[f"frame[{STEPS - 1}]"].max()) > 0 and float(last[f"signal[{STEPS - 1}]"].abs().max()) > 0
    assert float(last["total"].min()) > 0 and float(last["residual"].min()) > 0
