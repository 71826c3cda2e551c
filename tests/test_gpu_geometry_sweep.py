"""GPU: Shack-Hartmann geometries off the beaten track -- odd lenslet counts (R % 4 == 2: the dword phase kernel as the production
float32 path, a half-empty last block of the register-resident spots kernel, odd n_valid), lenslets of 4, 5, 8 and 10 pixels (the
generic spots / centroid / tail kernels, p > 8: the row-striding branch), the edges of the fused step kernel's envelope (R <= 128,
R % 4, n_valid <= 336, n_modes 52 | 53, the Kp = (n_modes + 3) & ~3 padding) and shards beyond 1024 envs (batched MFMA tail).

Every comparison is against oracle.ao_oracle.OracleEnv (float64 NumPy) built for the same geometry and handed the env's own ring
operators, mode-to-command matrix and modal command matrix: what is left is the device arithmetic.  One oracle run per case is
recorded (three envs, six closed-loop steps, gain 0.5 plus a bounded random perturbation of the action, the float32 actions derived
from the oracle's own observations) and the float64 shard, the float32 shard and every float32 switch combination replay its actions
and are held to it: F64_SAME_OPERATOR_TOL_FULL / F32_TOL / CAL_TOL of tests/test_gpu_parity.py, unchanged.  The maxima measured on
MI355X are in profiles/geometry_sweep_parity_maxima.json (AO_PARITY_REPORT=<file> with this module alone rewrites it).

Centroid threshold: the centre of gravity zeroes the pixels below threshold_cog * max; a pixel ON the cut flips between precisions.
The seed of every case was chosen on the CPU, from the oracle alone, among 1 .. 8 for the largest distance of any pixel from the cut,
and every recorded run asserts -- again from the oracle's frames only -- that the distance is at least 1e-7 of the brightest pixel
(about a hundred float32 roundings of a pixel at the 1 % cut level) at every compared measurement.  No step, env or element is
left out of a comparison.  The reference tree is never read here.

That the sweep bites was checked once with guards weakened in a scratch build (each variant writes or reads less than the real
kernel): the row bound of k_phase_mfma one short -> every float32 odd* / p5 run fails; `active` of k_sh_spots one lenslet short ->
every p4 / p5 / p8 / p10 test and the FAST_WFS=0 runs fail; k_sh_centroid without its row stride -> every p10 test fails; k_sh_tail
dropping the last row of an odd p -> the p5 shards fail; k_sh_spots_p6 skipping the last odd lenslet row -> every odd* / edge21 test
fails.  Unperturbed, all maxima lie below 15 % of their tolerance.
"""
import copy

import numpy as np
import pytest

from test_gpu_parity import CAL_TOL, F32_TOL, F64_SAME_OPERATOR_TOL_FULL, _OBSERVED, _close

pytestmark = pytest.mark.gpu

STEPS = 6
N_ENVS = 3
SEED_STRIDE = 100
MIN_CUT_GAP = 1e-7
# pixels per frame: 0.45 along the wind (72 deg: 0.428 along x -> 2 crossings in 6 frames, 0.139 along y); wind speed = 0.45 pixel / dt
PX_PER_FRAME = 0.45

# case: lenslets across, pixels per lenslet, the oracle's valid lenslets / valid actuators (asserted: a change of the valid-lenslet
# rule must not move a case off the branch it is here for), modes, whether the float32 shard runs the fused step kernel, seed
CASES = {
    "odd7": dict(n_sub=7, ppx=6, n_valid=37, n_valid_act=52, n_modes=10, fused=False, seed=7),
    "odd11": dict(n_sub=11, ppx=6, n_valid=97, n_valid_act=120, n_modes=30, fused=False, seed=7),
    "odd19": dict(n_sub=19, ppx=6, n_valid=293, n_valid_act=332, n_modes=52, fused=False, seed=6),
    "edge21": dict(n_sub=21, ppx=6, n_valid=349, n_valid_act=392, n_modes=40, fused=False, seed=6),
    "p4": dict(n_sub=6, ppx=4, n_valid=32, n_valid_act=45, n_modes=8, fused=False, seed=6),
    "p5": dict(n_sub=6, ppx=5, n_valid=32, n_valid_act=45, n_modes=8, fused=False, seed=8),
    "p8": dict(n_sub=5, ppx=8, n_valid=21, n_valid_act=32, n_modes=8, fused=False, seed=1),
    "p10": dict(n_sub=4, ppx=10, n_valid=12, n_valid_act=21, n_modes=6, fused=False, seed=2),
    "modes1": dict(n_sub=10, ppx=6, n_valid=80, n_valid_act=101, n_modes=1, fused=True, seed=6),
    "modes3": dict(n_sub=10, ppx=6, n_valid=80, n_valid_act=101, n_modes=3, fused=True, seed=8),
    "modes52": dict(n_sub=10, ppx=6, n_valid=80, n_valid_act=101, n_modes=52, fused=True, seed=6),
    "modes53": dict(n_sub=10, ppx=6, n_valid=80, n_valid_act=101, n_modes=53, fused=False, seed=2),
}
M2C_COLUMNS = 53                                                 # the modes* cases truncate ONE 53-column matrix
THREE_LAYERS = dict(windSpeed=[15.0, 12.0, 16.0], windDirection=[72.0, 200.0, 320.0], fractionalR0=[0.6, 0.25, 0.15],
                    altitude=[0.0, 0.0, 0.0], seed=8)


def _geo(name, **kw):
    c = CASES[name]
    ps = 0.4 / c["ppx"]                                          # pixel size [m]: diameter / R
    d = dict(diameter=0.4 * c["n_sub"], nSubaperture=c["n_sub"], nPixelPerSubap=c["ppx"], r0=0.13, L0=30.0,
             windSpeed=[PX_PER_FRAME * ps * 500.0], windDirection=[72.0], fractionalR0=[1.0], altitude=[0.0],
             nModes=c["n_modes"], nLoop=16)
    d.update(kw)
    return d


def _m2c(geo, columns):
    """calib.zernike_m2c for `columns` modes (host code, the matrix set_params would build itself)."""
    from rlao_amd import calib
    p = calib.params_from_args(geo)
    return calib.zernike_m2c(calib.DMTables(p), calib.telescope_pupil(p.resolution), p.diameter, columns)


def _make_env(name, dtype, n_envs=N_ENVS, stride=SEED_STRIDE, opts=None, **geo_kw):
    from rlao_amd import _lib as L
    from rlao_amd.env import BatchedAOEnv
    geo = _geo(name, **geo_kw)
    env = BatchedAOEnv(n_envs=n_envs, device=0, dtype=dtype, env_seed_stride=stride)
    try:
        env.set_params(geo, camera="ideal", wfs_type="shackhartmann",
                       m2c=_m2c(geo, M2C_COLUMNS) if name.startswith("modes") else None)
        for k, v in (opts or {}).items():
            L.check(env._shard.lib.aoenv_set_option(env._shard.h, getattr(L, k), v))
    except Exception:
        env.close()
        raise
    return env


# ---- the oracle side: built once per geometry, run once per case ----------------------------------------------------------
_BASES = {}
_RECORDS = {}


def build_base(geo, m2c, A, B):
    """OracleEnv of the geometry with its OWN interaction matrix (the calibration reference), the ring operators handed over."""
    from oracle import ao_oracle as O
    R = geo["nSubaperture"] * geo["nPixelPerSubap"]
    geom = O.LayerGeometry(R, geo["diameter"], geo["L0"])
    return O.OracleEnv(resolution=R, diameter=geo["diameter"], n_subap=geo["nSubaperture"], r0=geo["r0"], L0=geo["L0"],
                       windSpeed=geo["windSpeed"], windDirection=geo["windDirection"], fractionalR0=geo["fractionalR0"],
                       altitude=geo["altitude"], m2c=m2c, n_modes=m2c.shape[1], nLoop=geo["nLoop"], geom_AB=(geom, A, B))


def cut_gap(frame, thr=0.01):
    """Distance of the closest pixel from the centroid cut thr * max, relative to the brightest pixel (oracle frame: the valid
    lenslets' spots; the pixels of the other lenslets are 0, a whole 1 % away)."""
    mx = float(frame.max())
    return float(np.abs(frame - thr * mx).min() / mx)


def run_oracle(base, m2c, modal_cm, seed, steps=STEPS):
    """Three envs (seeds seed + 100 k) of `base` with the controller (m2c, modal_cm): one closed-loop episode.  The actions come from
    the oracle's own observations and are float32 arrays, as the trainers' wrappers hand them over: NumPy then forms img_to_vec(action) *
    1e-6 in float32, and so does the device for a float32-representable action, whatever the shard's dtype."""
    orcs, rec = [], dict(seed=seed, obs0=[], screen0=[], actions=[], signal=[], obs=[], reward=[], strehl=[], frame=[], gap=[])
    for k in range(N_ENVS):
        o = copy.deepcopy(base, memo={id(x): x for x in (base.dm_modes, base.imat) if x is not None})
        o.M2C = np.asarray(m2c, dtype=np.float64)
        o.modal_cm = np.asarray(modal_cm, dtype=np.float64)
        o.reconstructor = o.M2C @ o.modal_cm
        o.new_episode(seed + SEED_STRIDE * k)
        rec["screen0"].append([lay.mapShift.copy() for lay in o.atm.layers])
        rec["obs0"].append(o.reset_soft())
        rec["gap"].append(cut_gap(o.wfs.frame))
        orcs.append(o)
    rs = np.random.RandomState(9)
    obs = np.stack(rec["obs0"])
    n_layer = len(orcs[0].atm.layers)
    crossings = np.zeros((N_ENVS, n_layer), dtype=int)
    for i in range(steps):
        act = (0.5 * obs + 0.05 * rs.randn(*obs.shape)).astype(np.float32) * orcs[0].dm_mask[None].astype(np.float32)
        row = {q: [] for q in ("signal", "obs", "reward", "strehl", "frame")}
        for k, o in enumerate(orcs):
            b0 = [lay.buff.copy() for lay in o.atm.layers]
            oo, of, orw, osr, _, _ = o.step(i, act[k])
            for l, lay in enumerate(o.atm.layers):               # the sub-pixel accumulator wrapped: the layer crossed a pixel
                assert np.abs(lay.ratio).max() < 1
                crossings[k, l] += int((np.abs(lay.buff) < np.abs(b0[l])).any())
            for q, v in zip(("signal", "obs", "reward", "strehl", "frame"), (o.wfs.signal, oo, orw, osr, of)):
                row[q].append(np.array(v, dtype=np.float64, copy=True))
            rec["gap"].append(cut_gap(of))
        for q, v in row.items():
            rec[q].append(np.stack(v))
        rec["actions"].append(act)
        obs = rec["obs"][-1]
    rec["crossings"] = crossings
    rec["screen"] = [[lay.mapShift.copy() for lay in o.atm.layers] for o in orcs]                # [env][layer][S_l, S_l]
    rec["opd_atm"] = [o.atm.OPD.copy() for o in orcs]
    rec["opd_res"] = [o.tel_OPD.copy() for o in orcs]
    rec["total"] = np.stack([o.total[:steps] for o in orcs], axis=1)
    rec["residual"] = np.stack([o.residual[:steps] for o in orcs], axis=1)
    rec["modal_cm"] = np.asarray(modal_cm, dtype=np.float64).copy()
    rec["min_gap"] = min(rec["gap"])
    return rec


def _base(name, env):
    c = CASES[name]
    key = (c["n_sub"], c["ppx"])
    if key not in _BASES:
        at = env._atm_tables
        geo = _geo(name)
        m2c = _m2c(geo, M2C_COLUMNS) if name.startswith("modes") else env.M2C_CL
        _BASES[key] = build_base(geo, m2c, at.A, at.B)
    return _BASES[key]


def _same_controller(env, rec):
    """The recorded oracle run was made with the modal command matrix of the first env of this case; every env calibrates on the
    GPU in float64 whatever its shard's dtype, so a later env must have come to the same one."""
    scale = float(np.abs(rec["modal_cm"]).max())
    np.testing.assert_allclose(env.modal_CM, rec["modal_cm"], rtol=0, atol=1e-12 * scale)


def _record(name, env):
    if name not in _RECORDS:
        c = CASES[name]
        base = _base(name, env)
        rec = run_oracle(base, env.M2C_CL, env.modal_CM, c["seed"])
        _OBSERVED.setdefault(name + "-oracle", {})["threshold_gap_min"] = rec["min_gap"]
        _RECORDS[name] = rec
    rec = _RECORDS[name]
    _same_controller(env, rec)
    # from the oracle alone: every measurement clear of the centroid cut, the layer crossed a pixel at least twice
    assert rec["min_gap"] >= MIN_CUT_GAP, (name, rec["gap"])
    assert (rec["crossings"] >= 2).all(), rec["crossings"]
    return rec


def _reward(got, want, tol, label):
    rec = _OBSERVED.setdefault(label, {})
    rec["reward_rel"] = max(rec.get("reward_rel", 0.0), float(np.abs((got - want) / want).max()))
    np.testing.assert_allclose(got, want, rtol=tol["reward_rel"], atol=tol["obs"])


def _replay(env, rec, tol, label, steps=STEPS, envs=range(N_ENVS), compare=None, winds=None, screens0=False):
    """A fresh episode of `env` driven by the recorded actions: every step's signal, observation, reward, Strehl and frame, then (a
    full run) the screens, atm.OPD, the residual OPD and the telemetry.  `envs`: which recorded env each env of the shard is;
    `compare`: the envs of the shard held to the oracle (default: all); `screens0`: every layer's whole screen after the reset
    too.  Returns what the shard gave, per step."""
    import torch
    from rlao_amd import _lib as L
    envs = list(envs)
    pairs = [(k, envs[k]) for k in (range(len(envs)) if compare is None else compare)]
    env.generate_new_phase_screen(rec["seed"])
    if winds is not None:
        env.set_wind_per_env(winds[0], winds[1], reset=True)
    env.dm.coefs = 0
    env.dm_prev = 0
    env.measure()
    obs0 = env.reset_soft().cpu().numpy()
    out = [obs0]
    for k, r in pairs:
        _close(obs0[k], rec["obs0"][r], "obs", tol, label, err_msg=f"obs after reset, env {k}")
    if screens0:
        scr = env._download_screens()
        for k, r in pairs:
            for l in range(env.param.nLayer):
                assert scr[l][k].shape == rec["screen0"][r][l].shape
                _close(scr[l][k], rec["screen0"][r][l], "screen", tol, label, err_msg=f"screen after reset, env {k} layer {l}")
    for i in range(steps):
        act = torch.as_tensor(rec["actions"][i][envs])
        obs, frame, rew, sr, _, _ = env.step(i, act)
        obs, frame, rew, sr = obs.cpu().numpy(), frame.cpu().numpy(), rew.cpu().numpy(), sr.cpu().numpy()
        sig = env._shard.download(L.B_SIGNAL, (env.n_envs, env.nSignal))
        out.append((obs, frame, rew, sr, sig))
        for k, r in pairs:
            _close(sig[k], rec["signal"][i][r], "signal", tol, label, err_msg=f"signal step {i} env {k}")
            _close(obs[k], rec["obs"][i][r], "obs", tol, label, err_msg=f"obs step {i} env {k}")
            _reward(rew[k], rec["reward"][i][r], tol, label)
            _close(sr[k], rec["strehl"][i][r], "strehl", tol, label, err_msg=f"strehl step {i} env {k}")
            want = rec["frame"][i][r]
            _close(frame[k], want, "frame_rel", tol, label, scale=float(want.max()), err_msg=f"frame step {i} env {k}")
    if steps == STEPS:
        scr = env._download_screens()                             # [nLayer, n_envs, S, S]
        opd_atm = env._shard.download(L.B_OPD_ATM, (env.n_envs, env.R, env.R))
        phase = env._shard.download(L.B_PHASE, (env.n_envs, env.R, env.R))
        tot, res = env.total[:steps], env.residual[:steps]
        if env.n_envs == 1:                                          # (a one-env shard hands out vectors)
            tot, res = tot[:, None], res[:, None]
        for k, r in pairs:
            for l in range(env.param.nLayer):
                assert scr[l][k].shape == rec["screen"][r][l].shape
                _close(scr[l][k], rec["screen"][r][l], "screen", tol, label, err_msg=f"screen env {k} layer {l}")
            _close(opd_atm[k] * env.pupil, rec["opd_atm"][r], "opd_m", tol, label, err_msg=f"atm.OPD env {k}")
            _close(phase[k] * env.src_wavelength / (2 * np.pi), rec["opd_res"][r], "opd_m", tol, label, err_msg=f"residual OPD env {k}")
            _close(tot[:, k], rec["total"][:, r], "rms_nm", tol, label, err_msg=f"total env {k}")
            _close(res[:, k], rec["residual"][:, r], "rms_nm", tol, label, err_msg=f"residual env {k}")
    return out


def _assert_geometry(name, env, base):
    c = CASES[name]
    assert base.wfs.nValid == c["n_valid"] and base.nValidAct == c["n_valid_act"]          # the oracle's counts: the table of cases
    assert env._sh_tables.nValid == c["n_valid"] and env.nValidAct == c["n_valid_act"]
    assert env.R == c["n_sub"] * c["ppx"] == base.R and env.param.nModes == c["n_modes"]
    assert np.array_equal(env._sh_tables.valid_2d, base.wfs.valid_2d)
    assert np.array_equal(env.dm_mask.astype(bool), base.dm_mask)


# ---- the sweep ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_path_and_calibration_match_oracle(name):
    """The float32 shard of every case sits on the path it is here for (aoenv_fused_step_active), and the calibration -- measured in
    float64 on the GPU, the pokes in groups of nMeasurements = 6 that share the centroid cut (max_group) -- gives the oracle's
    reference centroids, slope units and zonal interaction matrix."""
    c = CASES[name]
    env = _make_env(name, "f32")
    try:
        base = _base(name, env)
        _assert_geometry(name, env, base)
        assert int(env._shard.lib.aoenv_fused_step_active(env._shard.h)) == int(c["fused"])
        assert env.param.nMeasurements == base.n_meas == 6
        label = name + "-cal"
        ns, nv = c["n_sub"], c["n_valid"]
        ref2d, valid = base.wfs.reference_slopes_maps, base.wfs.valid_2d
        _close(env.reference_centroids[:nv], ref2d[:ns][valid], "ref", CAL_TOL, label)
        _close(env.reference_centroids[nv:], ref2d[ns:][valid], "ref", CAL_TOL, label)
        np.testing.assert_allclose(env.slopes_units, base.wfs.slopes_units, rtol=1e-9)
        assert env.imat.shape == base.imat.shape == (2 * nv, c["n_valid_act"])
        _close(env.imat, base.imat, "imat_rel", CAL_TOL, label, scale=float(np.abs(base.imat).max()))
    finally:
        env.close()


@pytest.mark.parametrize("name", list(CASES))
def test_float64_shard_matches_oracle(name):
    """float64 shard (the batched kernels, generic arithmetic) against the oracle that shares its operators: re-ordering noise."""
    env = _make_env(name, "f64")
    try:
        assert not env.fused_step
        _assert_geometry(name, env, _base(name, env))
        _replay(env, _record(name, env), F64_SAME_OPERATOR_TOL_FULL, name + "-f64")
    finally:
        env.close()


@pytest.mark.parametrize("name", list(CASES))
def test_float32_shard_matches_oracle(name):
    """float32 shard, default switches (the production path of the geometry), against the same oracle run."""
    env = _make_env(name, "f32")
    try:
        assert env.fused_step == CASES[name]["fused"]
        _replay(env, _record(name, env), F32_TOL, name + "-f32")
    finally:
        env.close()


SWITCHES = [{"OPT_FAST_WFS": 0}, {"OPT_MFMA_GEMM": 0}, {"OPT_FUSED_TAIL": 0}, {"OPT_FUSED_TAIL": 0, "OPT_FACTORED_RECON": 0},
            {"OPT_COEFS_IMAGE": 1}]
SWITCH_RUNS = [(n, o) for n in ("odd11", "p5", "p10") for o in SWITCHES] + [("modes52", {"OPT_FUSED_STEP": 0})]


@pytest.mark.parametrize("name,opts", SWITCH_RUNS, ids=[n + "-" + "+".join(f"{k[4:]}={v}" for k, v in o.items()) for n, o in SWITCH_RUNS])
def test_float32_switches_match_oracle(name, opts):
    """The other float32 kernels of these geometries (generic spots, VALU contractions, separate centroid / reconstruction kernels,
    dense reconstructor, command images; the 52-mode case outside the fused step kernel): each held to the oracle, not to the
    default run."""
    env = _make_env(name, "f32", opts=opts)
    try:
        assert not env.fused_step
        tag = "+".join(f"{k[4:]}={v}" for k, v in opts.items())
        _replay(env, _record(name, env), F32_TOL, f"{name}-f32-{tag}")
    finally:
        env.close()


def test_odd_geometry_three_layers_and_per_env_wind():
    """odd7 under three ground layers (weights 0.6 / 0.25 / 0.15): the multi-layer dword phase kernel, which has no band variant.
    A float32 shard whose envs are all given the shard's own wind through aoenv_set_wind_env is bit-identical to the shared-clock
    shard, and both match the oracle."""
    tl = {k: v for k, v in THREE_LAYERS.items() if k != "seed"}
    runs = []
    for per_env in (False, True):
        env = _make_env("odd7", "f32", **tl)
        try:
            assert not env.fused_step and env.param.nLayer == 3 and env._atm_tables.uniform
            if "odd7-3layers" not in _RECORDS:
                at = env._atm_tables
                base = build_base(_geo("odd7", **tl), env.M2C_CL, at.A, at.B)
                rec = run_oracle(base, env.M2C_CL, env.modal_CM, THREE_LAYERS["seed"])
                _OBSERVED.setdefault("odd7-3layers-oracle", {})["threshold_gap_min"] = rec["min_gap"]
                _RECORDS["odd7-3layers"] = rec
            rec = _RECORDS["odd7-3layers"]
            _same_controller(env, rec)
            assert rec["min_gap"] >= MIN_CUT_GAP, rec["gap"]
            assert (rec["crossings"] >= 2).all(), rec["crossings"]
            winds = (np.tile(tl["windSpeed"], (N_ENVS, 1)), np.tile(tl["windDirection"], (N_ENVS, 1))) if per_env else None
            runs.append(_replay(env, rec, F32_TOL, "odd7-3layers-f32" + ("-per-env-wind" if per_env else ""), winds=winds))
        finally:
            env.close()
    assert np.array_equal(runs[0][0], runs[1][0])
    for x, y in zip(runs[0][1:], runs[1][1:]):
        assert all(np.array_equal(p, q) for p, q in zip(x, y))


def _kernel_launches(env, fn):
    env._shard.profile(True)
    out = fn()
    prof = env._shard.profile_read(env._stream())
    env._shard.profile(False)
    return out, {k: n for k, (ms, n) in prof.items()}


@pytest.mark.parametrize("n_envs,batched", [(1100, True), (1024, False)])
def test_large_shard_takes_the_batched_tail(n_envs, batched):
    """odd7 in float32, every env the seed of env 0: a shard of more than 1024 envs leaves the one-workgroup-per-env tail
    (k_sh_tail) for the centroid kernel + batched MFMA reconstruction + epilogue; 1024 envs still take k_sh_tail.  After 4
    steps every env equals env 0 bit for bit, and env 0 is held to the oracle run that env 0 of the 3-env shard is held to."""
    steps = 4
    env = _make_env("odd7", "f32", n_envs=n_envs, stride=0)
    try:
        assert not env.fused_step
        rec = _record("odd7", env)
        label = f"odd7-f32-{n_envs}envs"
        out, launches = _kernel_launches(env, lambda: _replay(env, rec, F32_TOL, label, steps=steps, envs=[0] * n_envs, compare=[0]))
        assert launches["env_step"] == 0
        if batched:
            assert launches["sh_tail"] == 0 and launches["sh_centroid"] >= steps and launches["gemm_recon"] >= steps
        else:
            assert launches["sh_tail"] == steps
        assert (out[0] == out[0][:1]).all()
        for arrays in out[1:]:
            for a in arrays:
                assert np.array_equal(a, np.broadcast_to(a[:1], a.shape))
    finally:
        env.close()


def test_envelope_neighbours_agree():
    """52 modes (the last count the fused step kernel takes) and 53 (the batched kernels) on the same seeds, the M2C of both cut
    from one 53-column matrix.  The first step after the reset measures atmosphere + flat DM: its frame, slopes and Strehl do not
    depend on the number of modes, and the two paths agree on them within the float32 tolerances of those quantities."""
    import torch
    from rlao_amd import _lib as L
    got, seed = {}, None
    for name in ("modes52", "modes53"):
        env = _make_env(name, "f32")
        try:
            assert env.fused_step == (name == "modes52")
            if seed is None:
                seed = _record(name, env)["seed"]                   # (its first measurements: clear of the centroid cut)
            env.generate_new_phase_screen(seed)
            env.dm.coefs = 0
            env.dm_prev = 0
            env.measure()
            obs = env.reset_soft()
            _, frame, _, sr, _, _ = env.step(0, 0.5 * obs)
            torch.cuda.synchronize()
            got[name] = (frame.cpu().numpy(), env._shard.download(L.B_SIGNAL, (env.n_envs, env.nSignal)), sr.cpu().numpy())
        finally:
            env.close()
    (f0, s0, r0), (f1, s1, r1) = got["modes52"], got["modes53"]
    label = "modes52-vs-modes53-f32"
    for k in range(N_ENVS):
        _close(f0[k], f1[k], "frame_rel", F32_TOL, label, scale=float(f1[k].max()))
        _close(s0[k], s1[k], "signal", F32_TOL, label)
        _close(r0[k], r1[k], "strehl", F32_TOL, label)
    assert not np.array_equal(f0[0], f0[1])                         # distinct seeds
