"""GPU: aoenv_run_integrator with AOENV_OPT_STEP_PAIRS (a step takes the quiet step behind it along in its launch,
k_env_step_pair_sh6) against the same shard with the option off, and against the general kernel that AOENV_PATH_SH_PLAIN forces
(which never pairs).  The second step of a pair takes the command, the observation, the integrator's state and the return
accumulator from registers, its taps from the host's copy of the clock, and counts the telemetry index and the camera's frame
counter up by one: everything a caller can see afterwards must be the same BIT FOR BIT (torch.equal) -- obs, reward, Strehl, the
last frame and phase, the slopes, dm.coefs, dm_prev, the total / residual telemetry of every step, the return accumulator, the
screens, the generator states, the host clocks, the counters of the noise streams, and one env.step() after the calls.

Which launches are pairs is restated here from the clock's arithmetic (clock_subpixel, common.hpp) and the pixels per frame the
shard itself reports after one step; the library's counters (launches, steps covered) must equal that plan, and every case names the
situations it is here for, which the plan must contain:

    qq            a quiet step takes a quiet step along
    cross_first   a crossing step takes a quiet step along
    single_next   a step runs alone because the step behind it crosses a pixel
    cross_cross   two crossing steps in a row, both alone
    pair_ends     a pair ends the call: the frame and the phase of its second step are stored
    single_ends   the call's last step runs alone (an odd rest, or n_steps = 1)

2 envs; R = 24 (KS = 6) and R = 72 with a second mirror (26 actuators across: KS = 8, two passes of stage A); 1 and 3 layers (one of
them calm, one with negative ratios); the camera off, photon noise and the Razor camera.  Only launches whose camera gives
whole-number pixels pair (photon counts, ADC steps: every product of the centre of gravity is then exact, whichever of its sums of
two products the compiler fuses).  The camera off, read-out noise alone, a quantum efficiency alone and photon noise behind a quantum
efficiency give pixels that are plain floats (the last three run the CAMERA instantiation): there the counters must show one launch
per step -- built as pairs, these cases differed from it in the last bit of the slopes at R = 48 and 72 -- and the results are
compared all the same.  A case that pairs must have whole-number frames.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# the geometries of tests/test_gpu_step_specialised.py: its smallest (one wave of lenslets), and the one with 26 actuators across
GAIN = 0.5
_G = dict(nPixelPerSubap=6, r0=0.13, L0=30.0, fractionalR0=[1.0], altitude=[0.0], nLoop=16)
R24 = dict(_G, diameter=1.6, nSubaperture=4, nModes=8)
R48 = dict(_G, diameter=3.2, nSubaperture=8, nModes=20)
R72 = dict(_G, diameter=4.8, nSubaperture=12, nModes=20)
CAMERA = {"off": "ideal", "photon": "papyrus", "razor": "razor", "readout": "ideal", "qe": "ideal", "photon_qe": "ideal"}
# cameras with non-integer pixels, configured on the ideal one
CAM_FIELDS = {"readout": dict(readoutNoise=3), "qe": dict(QE=0.7), "photon_qe": dict(photonNoise=True, QE=0.7)}

# pixels per frame = speed / 33.33: 12 m/s -> 0.36, 23 m/s -> 0.69 (crosses twice in a row), 28 m/s -> 0.84
ONE_036 = dict(windSpeed=[12.0], windDirection=[0.0])
ONE_069 = dict(windSpeed=[23.0], windDirection=[200.0])
ONE_084 = dict(windSpeed=[28.0], windDirection=[90.0])
THREE = dict(windSpeed=[12.0, 0.0, 9.0], windDirection=[200.0, 0.0, 72.0],
             fractionalR0=[0.6923076923076923, 0.15384615384615385, 0.15384615384615385], altitude=[0.0, 0.0, 0.0])
THREE_FAST = dict(THREE, windSpeed=[23.0, 0.0, 5.0])

CASES = {
    "r24_photon_036_7": dict(geo=R24, cam="photon", wind=ONE_036, calls=[7], tags={"qq", "cross_first", "single_next", "pair_ends"}),
    "r24_razor_036_3_then_2": dict(geo=R24, cam="razor", wind=ONE_036, calls=[3, 2], tags={"qq", "single_ends", "pair_ends"}),
    "r24_off_069_6": dict(geo=R24, cam="off", wind=ONE_069, calls=[6], tags={"cross_cross", "cross_first", "single_next"}),
    "r24_photon_one_step_calls": dict(geo=R24, cam="photon", wind=ONE_036, calls=[1, 1, 2], tags={"single_ends", "cross_first"}),
    "r24_photon_three_layers_5": dict(geo=R24, cam="photon", wind=THREE, calls=[5], tags={"qq", "cross_cross", "pair_ends"}),
    "r24_razor_three_layers_fast_6": dict(geo=R24, cam="razor", wind=THREE_FAST, calls=[6], tags={"cross_cross", "cross_first"}),
    "r24_off_084_5": dict(geo=R24, cam="off", wind=ONE_084, calls=[5], tags={"cross_cross", "single_ends"}),
    "r72_photon_036_5": dict(geo=R72, cam="photon", wind=ONE_036, calls=[5], second_dm=dict(nSubaperture=12),
                             tags={"qq", "cross_first", "single_ends"}),
    "r72_razor_three_layers_4": dict(geo=R72, cam="razor", wind=THREE, calls=[4], second_dm=dict(nSubaperture=12),
                                     tags={"qq", "cross_cross", "single_ends"}),
    "r72_off_069_6": dict(geo=R72, cam="off", wind=ONE_069, calls=[6], second_dm=dict(nSubaperture=12), tags={"cross_cross", "pair_ends"}),
    "r48_off_036_7": dict(geo=R48, cam="off", wind=ONE_036, calls=[7], tags={"qq", "cross_first", "single_next", "pair_ends"}),
    "r48_readout_036_7": dict(geo=R48, cam="readout", wind=ONE_036, calls=[7], tags={"qq", "cross_first", "pair_ends"}),
    "r72_readout_036_5": dict(geo=R72, cam="readout", wind=ONE_036, calls=[5], second_dm=dict(nSubaperture=12), tags={"qq", "cross_first"}),
    "r72_qe_069_6": dict(geo=R72, cam="qe", wind=ONE_069, calls=[6], second_dm=dict(nSubaperture=12), tags={"cross_first", "pair_ends"}),
    "r48_photon_qe_three_layers_5": dict(geo=R48, cam="photon_qe", wind=THREE, calls=[5], tags={"qq", "pair_ends"}),
}


def _make(case, pairs, plain=False, **extra):
    from rlao_amd import _lib as L
    from rlao_amd.env import BatchedAOEnv
    env = BatchedAOEnv(n_envs=2, device=0, dtype="f32")
    env.set_params(dict(case["geo"], **case["wind"]), camera=CAMERA[case["cam"]], wfs_type="shackhartmann", gainCL=GAIN,
                   second_dm=case.get("second_dm"))
    if case["cam"] in CAM_FIELDS:
        env.wfs.cam.configure(**CAM_FIELDS[case["cam"]])
    sh = env._shard
    L.check(sh.lib.aoenv_set_option(sh.h, L.OPT_STEP_PAIRS, int(pairs)))
    if plain:
        L.check(sh.lib.aoenv_set_option(sh.h, L.OPT_FORCE_PATH, L.PATH_SH_PLAIN))
    assert env.fused_step
    env.generate_new_phase_screen(11)
    return env


def _start(env):
    import torch
    env.dm.coefs = 0
    env.dm_prev = 0
    env.measure()
    env.reset_soft()
    ret = torch.zeros(2, device=env.device, dtype=env.tdtype)
    env.accumulate_returns(ret)
    return ret


_RATIO = {}


def _ratio(case):
    """pixels per frame of every layer as the shard's own clock holds them: from rest, one step leaves exactly frac(r) sgn(r) = r
    in the accumulator (every wind here is below one pixel per frame)"""
    key = (case["geo"]["diameter"], tuple(case["wind"]["windSpeed"]), tuple(case["wind"]["windDirection"]))
    if key not in _RATIO:
        env = _make(dict(case, cam="off"), pairs=0)
        try:
            n = env.param.nLayer
            assert not env._shard.get_buff(n).any()
            _start(env)
            env.run_integrator(0, 1)
            _RATIO[key] = env._shard.get_buff(n).copy()
        finally:
            env.close()
        assert np.abs(_RATIO[key]).max() < 1
    return _RATIO[key]


def _plan(ratio, calls):
    """(launches, tags) of the calls from rest: clock_subpixel restated, then the greedy pairing of aoenv_run_integrator"""
    buff = np.zeros_like(ratio)

    def crosses():
        nonlocal buff
        buff = buff + np.fmod(np.abs(ratio), 1.0) * np.sign(ratio)
        c = bool((np.abs(buff) >= 1).any())
        buff = np.fmod(np.abs(buff), 1.0) * np.sign(buff)
        return c

    launches, tags = 0, set()
    for n in calls:
        cross = [crosses() for _ in range(n)]
        k = 0
        while k < n:
            launches += 1
            if k + 1 < n and not cross[k + 1]:
                tags.add("cross_first" if cross[k] else "qq")
                if k + 2 == n:
                    tags.add("pair_ends")
                k += 2
                continue
            if k + 1 == n:
                tags.add("single_ends")
            else:
                tags.add("cross_cross" if cross[k] else "single_next")
            k += 1
    return launches, tags


def _run(case, pairs, plain=False):
    import torch
    from rlao_amd import _lib as L
    env = _make(case, pairs, plain)
    try:
        sh, n, st = env._shard, env.n_envs, env._stream()
        ret = _start(env)
        sh.profile(True)
        i, rec = 0, []
        for c in case["calls"]:
            obs, rew, sr = env.run_integrator(i, c)
            i += c
            rec += [(f"obs@{i}", obs.clone()), (f"reward@{i}", rew.clone()), (f"strehl@{i}", sr.clone())]
            rec += [(f"{what}@{i}", torch.from_numpy(sh.download(which, shape, st)))
                    for what, which, shape in (("frame", L.B_FRAME, (n, env.cam_res, env.cam_res)), ("phase", L.B_PHASE, (n, env.R, env.R)))]
        torch.cuda.synchronize()
        counters = sh.step_counters()
        prof = sh.profile_read(st)
        sh.profile(False)
        state = env.get_state()
        rec += [(k, torch.from_numpy(np.ascontiguousarray(state[k]).astype(np.int64 if state[k].dtype == np.uint32 else state[k].dtype)))
                for k in ("screen", "buff", "mt", "coefs", "dm_prev", "signal", "counters", "obs")]
        rec += [("total", torch.from_numpy(np.array(env.total[:i]))), ("residual", torch.from_numpy(np.array(env.residual[:i]))),
                ("return", ret.clone())]
        obs, frame, rew, sr, _, _ = env.step(i, GAIN * obs)        # pins the frame counter and the clocks the calls left behind
        rec += [("step.obs", obs.clone()), ("step.frame", frame.clone()), ("step.reward", rew.clone()), ("step.strehl", sr.clone())]
        env.accumulate_returns(None)
        torch.cuda.synchronize()
        shape = dict(R=env.R, n_act=env.nActuator, layers=env.param.nLayer)
    finally:
        env.close()
    return rec, counters, prof, shape


@pytest.mark.parametrize("name", list(CASES))
def test_pairs_equal_single_steps_bit_for_bit(name):
    import torch
    case = CASES[name]
    n_steps = sum(case["calls"])
    launches, tags = _plan(_ratio(case), case["calls"])
    assert case["tags"] <= tags, (tags, "the case no longer contains what it is here for")
    if case["cam"] not in ("photon", "razor"):
        launches = n_steps                                          # pixels that are plain floats: these launches do not pair
    got, c_got, p_got, shape = _run(case, pairs=1)
    want, c_want, p_want, _ = _run(case, pairs=0)
    plain, c_plain, _, _ = _run(case, pairs=1, plain=True)
    assert shape["R"] == case["geo"]["nSubaperture"] * 6 and shape["layers"] == len(case["wind"]["windSpeed"])
    assert (shape["n_act"] > 24) == (case["geo"] is R72)
    fr = dict(got)[f"frame@{n_steps}"]
    assert bool((fr != fr.round()).any()) == (case["cam"] not in ("photon", "razor")), "whole-number pixels: exactly the cameras that pair"
    # the launches: the plan with the option on, one per step without it and in the general kernel; the profile counts steps
    assert c_got == (launches, n_steps), (c_got, launches, n_steps)
    assert c_want == (n_steps, n_steps) and c_plain == (n_steps, n_steps), (c_want, c_plain)
    assert p_got["env_step"][1] == n_steps and p_want["env_step"][1] == n_steps, (p_got["env_step"], p_want["env_step"])
    if "cross_first" in tags or "cross_cross" in tags:
        assert p_got["gemm_ring"][1] > 0 and p_got["gemm_ring"][1] == p_want["gemm_ring"][1]
    for other, who in ((want, "one launch per step"), (plain, "AOENV_PATH_SH_PLAIN")):
        assert len(got) == len(other)
        differ = {}
        for (what, a), (what_b, b) in zip(got, other):
            assert what == what_b and a.dtype == b.dtype and a.shape == b.shape, what
            if not torch.equal(a, b):
                differ[what] = float((a.double() - b.double()).abs().max())
        assert not differ, (name, who, differ)
    last = dict(got)
    assert float(last["total"].min()) > 0 and float(last["residual"].min()) > 0 and float(last["return"].abs().min()) > 0
    assert float(last[f"frame@{n_steps}"].max()) > 0 and float(last[f"phase@{n_steps}"].abs().max()) > 0


@pytest.mark.parametrize("what", ["delay", "per_env_winds", "disturbance"])
def test_loops_outside_the_envelope_launch_every_step(what):
    """a control delay, per-env clocks and a disturbance keep aoenv_run_integrator on one launch per step"""
    import torch
    case = CASES["r24_photon_036_7"]
    env = _make(case, pairs=1)
    try:
        if what == "delay":
            env.set_delay(1)
        elif what == "per_env_winds":
            env.set_wind_per_env(np.array([[12.0], [9.0]]), np.array([[0.0], [200.0]]), reset=True)
        else:
            env.set_disturbance(2, np.full((2, 1), 1e-8), np.full((2, 1), 30.0))
        _start(env)
        env._shard.profile(True)
        env.run_integrator(0, 7)
        torch.cuda.synchronize()
        assert env._shard.step_counters() == (7, 7)
        env._shard.profile(False)
        env.accumulate_returns(None)
    finally:
        env.close()
