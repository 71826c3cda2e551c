"""GPU: the joint reconstruction of a step pair (k_env_step_pair_sh6, AOENV_OPT_STEP_PAIRS) against one launch per step.

In a launch of two steps the first copy ends behind its centre of gravity: it leaves its slopes in LDS words of the pair's own,
forms the next command (which depends on the observation of the step BEFORE it, not on its own) and builds the second step's
Gy C on its last barriers.  The second copy starts at stage A and reconstructs both steps in one pass over the rows of M and
M2C^T: t = M s and o = -M2C t 1e6 twice from the same operand registers, the integrator from the first step's o, and the only
obs / coefs / dm_prev / reward stores of the launch.  No sum changes its operands or its order, so everything a caller can see
must equal one launch per step BIT FOR BIT (torch.equal): what tests/test_gpu_step_pairs.py collects, restated here -- after
every call obs, reward, Strehl, frame and phase; at the end the screens, the clocks, the generator states, dm.coefs, dm_prev, the
slopes, the counters of the noise streams, obs, the telemetry of every step and the return accumulator; and one env.step() behind.

Cases (2 envs each; sizes at which the joint pass takes another path):
    headline     20 x 20 lenslets, R = 120, 50 modes, photon noise, 6 steps from rest at the headline's wind: the only size at
                 which all ten M s turns and all thirteen M2C turns carry data and the pair's LDS words are largest (684)
    r72_m52/m49  12 x 12 lenslets and a second mirror (26 actuators across: KS = 8) with 52 modes (the maximum) and 49 (a rest
                 that is no multiple of 4: the `part + 4 j < n_modes` edge of both reconstructions)
    r24_razor    4 x 4 lenslets, 8 modes, the Razor camera (the CAMERA instantiation): one wave of lenslets, most waves hold no
                 mode and no actuator group; run_integrator(2), an env.step(), run_integrator(2): a pair ends the first call and
                 a pair starts the second, which pins the return accumulator and dm_prev across calls and shows that the only
                 obs / coefs / reward left in memory are the second copy's
Every case must have paired (step_counters: fewer launches than steps).  The headline case builds two 20 x 20 loops: measured
wall time 3.5 s, of which the set-up is nearly all; the others take 0.05 to 0.5 s.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GAIN = 0.5
_G = dict(nPixelPerSubap=6, r0=0.13, L0=30.0, fractionalR0=[1.0], altitude=[0.0], nLoop=16)
# bench.py's GEOMETRY: the headline
HEADLINE = dict(diameter=8.0, nSubaperture=20, nPixelPerSubap=6, r0=0.13, L0=30.0, windSpeed=[10.0], windDirection=[72.0],
                fractionalR0=[1.0], altitude=[0.0], magnitude=8.0, opticalBand="I", mechanicalCoupling=0.35, nModes=50, leak=0.99,
                nLoop=16)
R72 = dict(_G, diameter=4.8, nSubaperture=12, windSpeed=[12.0], windDirection=[0.0])
R24 = dict(_G, diameter=1.6, nSubaperture=4, nModes=8, windSpeed=[12.0], windDirection=[0.0])

# ops: an int n = run_integrator(i, n); "step" = one env.step with GAIN * obs
CASES = {
    "headline": dict(geo=HEADLINE, camera="papyrus", ops=[6], n_act_gt_24=False),
    "r72_m52": dict(geo=dict(R72, nModes=52), camera="papyrus", second_dm=dict(nSubaperture=12), ops=[5], n_act_gt_24=True),
    "r72_m49": dict(geo=dict(R72, nModes=49), camera="razor", second_dm=dict(nSubaperture=12), ops=[5], n_act_gt_24=True),
    "r24_razor": dict(geo=R24, camera="razor", ops=[2, "step", 2], n_act_gt_24=False),
}


def _run(case, pairs):
    import torch
    from rlao_amd import _lib as L
    from rlao_amd.env import BatchedAOEnv
    env = BatchedAOEnv(n_envs=2, device=0, dtype="f32")
    try:
        env.set_params(dict(case["geo"]), camera=case["camera"], wfs_type="shackhartmann", gainCL=GAIN, second_dm=case.get("second_dm"))
        sh, n = env._shard, env.n_envs
        L.check(sh.lib.aoenv_set_option(sh.h, L.OPT_STEP_PAIRS, int(pairs)))
        assert env.fused_step and (env.nActuator > 24) == case["n_act_gt_24"] and env.param.nModes == case["geo"]["nModes"]
        env.generate_new_phase_screen(11)
        env.dm.coefs = 0
        env.dm_prev = 0
        env.measure()
        obs = env.reset_soft()
        ret = torch.zeros(2, device=env.device, dtype=env.tdtype)
        env.accumulate_returns(ret)
        st = env._stream()
        sh.profile(True)
        i, rec = 0, []

        def seen(tag):
            return [(f"{what}@{tag}", torch.from_numpy(sh.download(which, shape, st)))
                    for what, which, shape in (("frame", L.B_FRAME, (n, env.cam_res, env.cam_res)), ("phase", L.B_PHASE, (n, env.R, env.R)))]

        for op in case["ops"]:
            if op == "step":
                obs, frame, rew, sr, _, _ = env.step(i, GAIN * obs)
                i += 1
                rec += [(f"step.frame@{i}", frame.clone())]
            else:
                obs, rew, sr = env.run_integrator(i, op)
                i += op
            rec += [(f"obs@{i}", obs.clone()), (f"reward@{i}", rew.clone()), (f"strehl@{i}", sr.clone()), (f"return@{i}", ret.clone())]
            rec += seen(i)
        torch.cuda.synchronize()
        counters = sh.step_counters()
        sh.profile(False)
        state = env.get_state()
        rec += [(k, torch.from_numpy(np.ascontiguousarray(state[k]).astype(np.int64 if state[k].dtype == np.uint32 else state[k].dtype)))
                for k in ("screen", "buff", "mt", "coefs", "dm_prev", "signal", "counters", "obs")]
        rec += [("total", torch.from_numpy(np.array(env.total[:i]))), ("residual", torch.from_numpy(np.array(env.residual[:i]))),
                ("return", ret.clone())]
        obs, frame, rew, sr, _, _ = env.step(i, GAIN * obs)         # pins the frame counter and the clocks the calls left behind
        rec += [("after.obs", obs.clone()), ("after.frame", frame.clone()), ("after.reward", rew.clone()), ("after.strehl", sr.clone()),
                ("after.return", ret.clone())]
        env.accumulate_returns(None)
        torch.cuda.synchronize()
    finally:
        env.close()
    return rec, counters, i


@pytest.mark.parametrize("name", list(CASES))
def test_joint_pass_equals_one_launch_per_step(name):
    import torch
    case = CASES[name]
    got, c_got, n_steps = _run(case, pairs=1)
    want, c_want, _ = _run(case, pairs=0)
    n_fused = sum(op for op in case["ops"] if op != "step") + case["ops"].count("step")   # env.step runs the fused kernel too
    assert c_want == (n_fused, n_fused), c_want
    assert c_got[1] == n_fused and c_got[0] < c_got[1], ("the case did not pair", c_got)
    if name == "r24_razor":
        assert c_got == (3, 5), c_got                                # pair, step, pair
    assert len(got) == len(want)
    differ = {}
    for (what, a), (what_b, b) in zip(got, want):
        assert what == what_b and a.dtype == b.dtype and a.shape == b.shape, what
        if not torch.equal(a, b):
            differ[what] = float((a.double() - b.double()).abs().max())
    assert not differ, (name, differ)
    last = dict(got)
    fr = last[f"frame@{n_steps}"]
    assert not bool((fr != fr.round()).any()) and float(fr.max()) > 0          # whole-number pixels: a camera that pairs
    assert float(last["total"].min()) > 0 and float(last["residual"].min()) > 0 and float(last["return"].abs().min()) > 0
    assert float(last["coefs"].abs().max()) > 0 and float(last["obs"].abs().max()) > 0 and float(last["signal"].abs().max()) > 0
