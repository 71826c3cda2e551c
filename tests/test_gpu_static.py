"""GPU: static aberration maps per env (aoenv_set_static_opd, rlao_amd/csrc/static_opd.hpp, static_kernels.hip): a map S_w in the
sensor arm, a map S_s in the science arm.

Shapes (tests/test_gpu_dm_env.py, tests/_fov_cases.py), four envs per shard and four closed-loop steps unless noted:
  small      R = 48, 9 actuators across: one full 32-patch of k_dm_static_mfma plus 16
  odd        R = 30, 6 across: R % 4 != 0, the dword stores and loads
  tiny_pyr   R = 24, 5 across, the Pyramid behind it: one partial patch, K below one MFMA K group once padded
  top_first  R = 66, two unequal layers: two full patches plus 2
  wide       R = 144, 37 across, 2 envs: more than one K group (ga_stride 12), two 128-row bands of k_dm_rows
  two_dm     `small` with a second mirror: the composite tables (14 across)
  geo        `two` of tests/_fov_cases.py (R = 42) behind the geometric Shack-Hartmann sensor: the unmasked phase
Modes: "mfma" k_dm_rows + k_dm_static_mfma; "general" k_coefs_image + k_dm_static<float> (AOENV_PATH_DM_STATIC_GENERAL); "f64"
k_dm_static<double>.

1 parity: one tests/_static_ref.py oracle per env (the map on the mirror side of the oracle's sum), replaying its float32 actions;
  after every step, per env, AOENV_B_OPD_ATM (which must not contain the map), the phase, the WFS signal, obs, reward, Strehl and
  the residual rms under the unchanged F32_TOL / F64_SAME_OPERATOR_TOL(_FULL) entries of tests/test_gpu_parity.py that
  tests/test_gpu_guide.py uses; the geometric sensor's unmasked phase carries the map outside the pupil.  AO_PARITY_REPORT=<file>
  with this module alone writes the measured maxima (profiles/static_parity_maxima.json).  tests/test_static_host.py shows on the
  CPU that an oracle which ignores the map misses these inputs by more than 100 tolerances.
2 exact data: integer tables, command and map, every partial sum exact in float32: all three kernels give the float64 product's
  bits at every pixel of every shape (geometric shards: the unmasked phase shows every patch tail).
3 science arm against the restatement: a difference alone, with a direction, S_w alone; S_s == S_w is AOENV_B_PHASE bit for bit.
4 bit-for-bit identities: mixed shard == uniform twins, place and shard size, every loop == per-call stepping, shared == per env,
  env_ids == whole arrays, cleared == untouched (fused again, same launch counts), refused calls leave no trace.
5 composition with per-env mirror tables behind a delay with a disturbance, with actuator pairs, with a guide plus a science
  direction: against per-env oracles under the same tolerances.
No test provokes a fault: the refusals are host-side checks that return before a launch."""
import copy
import json
import os

import numpy as np
import pytest

import _fov_cases as F
import _guide_ref as GR
import _offaxis_ref as X
import _static_ref as ST
import test_gpu_compose as TC
import test_gpu_fov_sweep as V
import test_gpu_geometric as GEOT
import test_gpu_geometry_sweep as G
import test_gpu_guide as GD
import test_gpu_offaxis as OA
import test_gpu_science as S
from test_gpu_dm_env import ODD, SMALL, WIDE
from test_gpu_parity import F32_TOL, F64_SAME_OPERATOR_TOL, F64_SAME_OPERATOR_TOL_FULL, _OBSERVED, _close

pytestmark = pytest.mark.gpu

STEPS = 4
STRIDE = G.SEED_STRIDE
GAIN = 0.5
TINY_PYR = dict(TC.TINY_PYR)
# case: (geometry, set_params keywords, n_envs, seed)
CASES = {
    "small": (dict(SMALL, nLoop=16), {}, 4, 5),
    "odd": (dict(ODD, nLoop=16), {}, 4, 5),
    "tiny_pyr": (dict(TINY_PYR, nLoop=16), dict(wfs_type="pyramid"), 4, 5),
    "top_first": (F.geo("top_first"), {}, 4, 3),
    "wide": (dict(WIDE), {}, 2, 5),
    "two_dm": (dict(SMALL, nLoop=16), dict(second_dm=dict(nSubaperture=4)), 4, 5),
    "geo": (F.geo("two"), dict(is_geometric=True), 4, 5),
}
MODES = ("mfma", "general", "f64")
# aoenv_static_surface_path of a separable mirror per mode: 1 k_dm_rows + k_dm_static_mfma, 2 k_coefs_image + k_dm_static<T> (3: the
# trailing add behind actuator pairs)
SURFACE_PATH = {"mfma": 1, "general": 2, "f64": 2}
TOL = GD.TOL                                                        # tests/test_gpu_guide.py's, unchanged
AMPLITUDE = 100e-9                                                  # rms of env 0's sensor-arm map; env k: (1 + k / 4) times that


def _np(t):
    return t.detach().cpu().numpy()


def maps(R, D, n, arm="wfs"):
    """The module's maps, float64 [n, R, R] metres: per env an f2-law NCPA of its own seed and amplitude (rlao_amd.calib.ncpa_map,
    zero outside the pupil) plus a smooth term over the whole grid, so that the map does not vanish outside the pupil (the unmasked
    phase of the geometric sensor must carry it there).  `arm`: "wfs" S_w, "science" S_s (other modes, other seeds)."""
    from rlao_amd import calib
    pupil = calib.telescope_pupil(R)
    y, x = np.mgrid[0:R, 0:R] / R - 0.5
    out = []
    for k in range(n):
        if arm == "wfs":
            m = calib.ncpa_map(pupil, D, f2=[AMPLITUDE * (1 + 0.25 * k), 2, 12, 1.0], seed=5 + k) + 40e-9 * (x * y + 0.3 * x) * (1 + k)
            m = m + 200e-9 * (1 + 0.5 * k) * ~pupil                  # a step at the pupil's edge: the edge lenslets' gradients see it
        else:
            m = calib.ncpa_map(pupil, D, f2=[0.6 * AMPLITUDE, 4, 16, 2.0], seed=11 + k) - 25e-9 * (x * x - 0.5 * y) * (1 + k)
        out.append(m)
    return np.stack(out)


def _maps_of(env, arm="wfs", ids=None):
    m = maps(env.R, float(env.param.diameter), 4, arm)
    return m[list(range(4))[-env.n_envs:] if ids is None else list(ids)]


def _dtype(mode):
    return "f64" if mode == "f64" else "f32"


def _make(case, mode, n=None, opts=None):
    from rlao_amd import _lib as L
    from rlao_amd.env import BatchedAOEnv
    geo, kw, n_case, _ = CASES[case]
    env = BatchedAOEnv(n_envs=n or n_case, device=0, dtype=_dtype(mode), env_seed_stride=STRIDE)
    try:
        env.set_params(dict(geo), **dict(dict(camera="ideal", wfs_type="shackhartmann", gainCL=GAIN), **kw))
        for k, v in (opts or {}).items():
            L.check(env._shard.lib.aoenv_set_option(env._shard.h, getattr(L, k), v))
        _path(env, mode)
    except Exception:
        env.close()
        raise
    return env


def _path(env, mode):
    from rlao_amd import _lib as L
    L.check(env._shard.lib.aoenv_set_option(env._shard.h, L.OPT_FORCE_PATH, L.PATH_DM_STATIC_GENERAL if mode == "general" else 0))


_ENVS = {}


def _env(case, mode, tag="a"):
    """one shard per (case, dtype, tag) for the module, handed out without maps and with a flat command"""
    key = (case, _dtype(mode), tag)
    if key not in _ENVS:
        _ENVS[key] = _make(case, mode)
    env = _ENVS[key]
    env.clear_static_aberration()
    _path(env, mode)
    env.dm.coefs = 0
    return env


@pytest.fixture(scope="module", autouse=True)
def _close_all():
    yield
    for env in _ENVS.values():
        env.close()
    _ENVS.clear()


def _dump():
    path = os.environ.get("AO_PARITY_REPORT")
    if path:
        with open(path, "w") as f:
            json.dump(_OBSERVED, f, indent=1, sort_keys=True)


_prologue, _buf, _signal = OA._prologue, OA._buf, GD._signal


# ---- 1. parity ------------------------------------------------------------------------------------------------------------------------
_BASES, _RUNS = {}, {}


def _base(case, env):
    """The case's oracle with the env's controller and ring operators (its own calibration is not repeated: the modal command
    matrix is handed over, as for the large geometries of tests/test_gpu_configs.py)."""
    if case not in _BASES:
        from oracle import ao_oracle as O
        geo, kw, _, _ = CASES[case]
        if case == "geo":
            _BASES[case] = GEOT._oracle_for(env, geo)
        elif case == "top_first":
            _BASES[case] = F.build_oracle(geo, env.M2C_CL, V._operators(env), modal_cm=env.modal_CM)
        else:
            at = env._atm_tables
            more = {}
            if kw.get("wfs_type") == "pyramid":
                more = dict(wfs_type="pyramid", modulation=geo["modulation"], psf_centering=geo["psfCentering"])
            if "second_dm" in kw:
                more = dict(second_dm_nsub=kw["second_dm"]["nSubaperture"])
            _BASES[case] = O.OracleEnv(resolution=env.R, diameter=geo["diameter"], n_subap=geo["nSubaperture"], r0=geo["r0"], L0=geo["L0"],
                                       windSpeed=geo["windSpeed"], windDirection=geo["windDirection"], fractionalR0=geo["fractionalR0"],
                                       altitude=geo["altitude"], m2c=env.M2C_CL, n_modes=env.M2C_CL.shape[1], nLoop=geo["nLoop"],
                                       geom_AB=(O.LayerGeometry(env.R, geo["diameter"], geo["L0"]), at.A, at.B), modal_cm=env.modal_CM,
                                       **more)
        assert np.array_equal(env.dm_mask.astype(bool), _BASES[case].dm_mask) and env.nSignal == _BASES[case].wfs.nSignal
    return _BASES[case]


def static_copies(base, s_w, variant=None):
    """one deep copy of `base` per map, the map attached AFTER the copy (tests/_static_ref.py)"""
    out = []
    for m in s_w:
        o = copy.deepcopy(base, memo={id(x): x for x in (base.dm_modes, base.imat) if x is not None})
        out.append(ST.static(o, m, variant=variant))
    return out


MIN_CUT_GAP = G.MIN_CUT_GAP                                         # of the brightest pixel: tests/test_gpu_geometry_sweep.py's, 1e-7


def _oracle_run(case, env):
    """The case's record.  A condition on the inputs, from the oracle alone (tests/test_gpu_geometry_sweep.py): every
    Shack-Hartmann frame of the run keeps every pixel MIN_CUT_GAP away from the 1 % centroid cut -- a pixel on the cut is in or out
    by one rounding, in any implementation.  The seed is the first of seed, seed + 1, ... for which that holds."""
    if case in _RUNS:
        return _RUNS[case]
    seen = []
    for seed in range(CASES[case][3], CASES[case][3] + 4):
        rec = _oracle_run_seed(case, env, seed)
        seen.append(rec["min_gap"])
        if rec["min_gap"] >= MIN_CUT_GAP:
            _OBSERVED.setdefault(f"static-{case}-oracle", {}).update(seed=seed, threshold_gap_min=rec["min_gap"])
            _RUNS[case] = rec
            return rec
    raise AssertionError((case, "no seed keeps the frames clear of the centroid cut", seen))


def _oracle_run_seed(case, env, seed):
    n = CASES[case][2]
    sh = case != "geo" and CASES[case][1].get("wfs_type") != "pyramid"
    gaps = [np.inf]
    s_w = _maps_of(env)
    orcs = static_copies(_base(case, env), s_w)
    keys = ("opd_atm", "opd_res", "signal", "obs", "reward", "strehl", "rms", "total") + (("phase_np",) if case == "geo" else ())
    rec = dict(seed=seed, actions=[], modal_cm=np.array(env.modal_CM), **{q: [] for q in keys})
    for k, o in enumerate(orcs):
        o.new_episode(seed + STRIDE * k)
    obs = np.stack([o.reset_soft() for o in orcs])
    rec["obs0"] = obs
    rs = np.random.RandomState(9)
    for i in range(STEPS):
        act = (GAIN * obs + 0.05 * rs.randn(*obs.shape)).astype(np.float32) * orcs[0].dm_mask[None].astype(np.float32)
        row = {q: [] for q in keys}
        for k, o in enumerate(orcs):
            oo, _, orw, osr, _, _ = o.step(i, act[k])
            if sh:
                gaps.append(G.cut_gap(o.wfs.frame))
            vals = [o.atm.OPD_no_pupil, o.tel_OPD, o.wfs.signal, oo, orw, osr, o.residual[i], o.total[i]]
            if case == "geo":
                vals.append(o.phase_no_pupil)
            for q, v in zip(keys, vals):
                row[q].append(np.array(v, dtype=np.float64, copy=True))
        for q, v in row.items():
            rec[q].append(np.stack(v))
        rec["actions"].append(act)
        obs = rec["obs"][-1]
    assert n == len(orcs)
    rec["min_gap"] = float(min(gaps))
    return rec


PARITY = [("small", "mfma"), ("small", "general"), ("small", "f64"), ("odd", "mfma"), ("odd", "f64"), ("tiny_pyr", "mfma"),
          ("tiny_pyr", "f64"), ("top_first", "mfma"), ("top_first", "f64"), ("wide", "mfma"), ("two_dm", "mfma"), ("two_dm", "f64"),
          ("geo", "mfma"), ("geo", "general"), ("geo", "f64")]


@pytest.mark.parametrize("case,mode", PARITY, ids=[f"{c}-{m}" for c, m in PARITY])
def test_the_sensor_arm_sees_the_map(case, mode):
    import torch
    from rlao_amd import _lib as L
    dtype = _dtype(mode)
    tol, label = dict(TOL[dtype]), f"static-{case}-{mode}"
    env = _env(case, mode)
    n = env.n_envs
    rec = _oracle_run(case, env)
    G._same_controller(env, rec)
    if case == "geo":                                               # (tests/test_gpu_geometric.py: the slopes' bound from the OPD's)
        tol["signal"] = GEOT._sig_bound(env, dtype)
        tol["obs"] = float(np.abs(np.asarray(env.reconstructor)).sum(axis=1).max() * 1e6 * tol["signal"])
    s_w = _maps_of(env)
    assert env._shard.static_surface_path() == 0
    env.set_static_aberration(wfs=s_w)
    assert not env.fused_step and env._shard.static_surface_path() == SURFACE_PATH[mode]
    assert np.array_equal(env.static_aberration["wfs"], s_w) and not env.static_aberration["science"].any()
    obs0 = _np(_prologue(env, rec["seed"]))
    k_opd = env.src_wavelength / (2 * np.pi)
    for k in range(n):
        _close(obs0[k], rec["obs0"][k], "obs", tol, label, err_msg=f"obs after reset env {k}")
    for i in range(STEPS):
        obs, _, rew, sr = (_np(t) for t in env.step(i, torch.as_tensor(rec["actions"][i]))[:4])
        sig, phase, atm = _signal(env), _buf(env, L.B_PHASE), _buf(env, L.B_OPD_ATM)
        res, tot = np.asarray(env.residual)[i], np.asarray(env.total)[i]
        for k in range(n):
            what = f"step {i} env {k}"
            _close(atm[k], rec["opd_atm"][i][k], "opd_m", tol, label, err_msg="AOENV_B_OPD_ATM (no map in it) " + what)
            _close(phase[k] * k_opd, rec["opd_res"][i][k], "opd_m", tol, label, err_msg="phase " + what)
            _close(sig[k], rec["signal"][i][k], "signal", tol, label, err_msg="signal " + what)
            _close(obs[k], rec["obs"][i][k], "obs", tol, label, err_msg="obs " + what)
            G._reward(rew[k], rec["reward"][i][k], tol, label)
            _close(sr[k], rec["strehl"][i][k], "strehl", tol, label, err_msg="strehl " + what)
            _close(res[k], rec["rms"][i][k], "rms_nm", tol, label, err_msg="residual rms " + what)
            _close(tot[k], rec["total"][i][k], "rms_nm", tol, label, err_msg="total (the atmosphere alone) " + what)
        if case == "geo":
            np_phase = np.asarray(env.phase_no_pupil, dtype=np.float64)
            for k in range(n):
                _close(np_phase[k] * k_opd, rec["phase_np"][i][k] * k_opd, "opd_m", tol, label, err_msg=f"unmasked phase step {i} env {k}")
            outside = ~np.asarray(env.pupil, dtype=bool)
            assert np.abs((np_phase[0] * k_opd - atm[0])[outside]).max() > 100 * tol["opd_m"]      # the map (and the mirror) are there
    _dump()
    env.clear_static_aberration()


# ---- 2. exact data --------------------------------------------------------------------------------------------------------------------
EXACT_SHAPES = {"small": SMALL, "odd": ODD, "tiny": TINY_PYR, "top_first": F.geo("top_first"), "wide": WIDE, "two_dm": SMALL}
_EXACT = {}


def _exact_env(shape, dtype):
    """a geometric shard of the shape (its unmasked phase shows the surface at every pixel); two_dm: the composite tables"""
    from rlao_amd.env import BatchedAOEnv
    key = (shape, dtype)
    if key not in _EXACT:
        geo = {k: v for k, v in dict(EXACT_SHAPES[shape], nLoop=16).items() if k not in ("modulation", "psfCentering")}
        env = BatchedAOEnv(n_envs=2, device=0, dtype=dtype, env_seed_stride=STRIDE)
        kw = dict(second_dm=dict(nSubaperture=4)) if shape == "two_dm" else {}
        env.set_params(geo, camera="ideal", wfs_type="shackhartmann", is_geometric=True, **kw)
        _EXACT[key] = env
    return _EXACT[key]


@pytest.fixture(scope="module", autouse=True)
def _close_exact():
    yield
    for env in _EXACT.values():
        env.close()
    _EXACT.clear()


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape", list(EXACT_SHAPES))
def test_integer_data_give_the_float64_products_bits(shape, mode):
    """gx, gy integers in [-3, 3], the command integers in [-4, 4], the map integers in [-50, 50]: every term and every partial sum
    of Gy C Gx^T + S_w is an integer below 36 nAct^2 + 50 < 2^24, exact in float32 in any order.  With a zero atmosphere the
    unmasked phase is (surface + map) * (2 pi / lambda) rounded ONCE, which NumPy forms from the float64 product in the env dtype:
    equal at every pixel of every env -- every patch tail of k_dm_static_mfma, every row tail of k_dm_static<T>.  The tables are
    random, hence asymmetric: a transposed or permuted product cannot pass.  Per-env tables, then one shared pair."""
    from rlao_amd import _lib as L
    env = _exact_env(shape, _dtype(mode))
    _path(env, mode)
    n, R, nA, A = env.n_envs, env.R, env.nActuator, env.nValidAct
    assert 36 * nA * nA + 50 < 2 ** 24
    dt = np.float32 if env.dtype == "f32" else np.float64
    rs = np.random.RandomState(7)
    idx = np.asarray(env._dm_tables.act_idx)
    try:
        for shared in (False, True):
            GX, GY = (rs.randint(-3, 4, (n, R, nA)).astype(np.float64) for _ in range(2))
            c = rs.randint(-4, 5, (n, A)).astype(np.float64)
            s_w = rs.randint(-50, 51, (n, R, R)).astype(np.float64)
            env.clear_static_aberration()
            if shared:
                env.clear_dm_per_env()
                GX[:], GY[:] = GX[0], GY[0]
                env._shard.upload(L.C_DM_GX, GX[0])
                env._shard.upload(L.C_DM_GY, GY[0])
                s_w[:] = s_w[0]
                env.set_static_aberration(wfs=s_w[0])
            else:
                env.set_dm_tables_per_env(GX, GY)
                env.set_static_aberration(wfs=s_w)
            assert not env.fused_step
            before = np.zeros(4, dtype=np.int64)
            assert env._shard.static_surface_path(before) == SURFACE_PATH[mode]      # the kernel this parametrisation is about ...
            env._shard.set_atm_opd(np.zeros((n, R, R)), env._stream())
            env.dm.coefs = c
            env.measure()
            after = np.zeros(4, dtype=np.int64)
            env._shard.static_surface_path(after)
            grew = np.flatnonzero(after - before)
            assert grew.tolist() == [SURFACE_PATH[mode]], (mode, before, after)          # ... and no other formed the surface
            got = np.asarray(env.phase_no_pupil)
            img = np.zeros((n, nA * nA))
            img[:, idx] = c
            want = np.einsum("eyi,eij,exj->eyx", GY, img.reshape(n, nA, nA), GX) + s_w
            assert np.abs(want).max() > 50
            want = (want.astype(dt) * dt(2 * np.pi / env.src_wavelength)).astype(np.float64)
            bad = np.argwhere(got.astype(np.float64) != want)
            assert bad.size == 0, (shape, mode, shared, len(bad), bad[:5], got[tuple(bad[0])], want[tuple(bad[0])])
    finally:
        env.clear_static_aberration()
        env.clear_dm_per_env()
        env._shard.upload(L.C_DM_GX, env._dm_tables.gx)
        env._shard.upload(L.C_DM_GY, env._dm_tables.gy)
        env.dm.coefs = 0
        _path(env, "mfma")


# ---- 3. the science arm -----------------------------------------------------------------------------------------------------------------
def _m2opd(env):
    return OA._m2opd(env)


@pytest.mark.parametrize("mode", ["mfma", "f64"])
@pytest.mark.parametrize("which", ["delta", "wfs_only", "direction"])
def test_science_arm_against_the_restatement(which, mode):
    """`top_first` (a field of view, so a direction can be set).  "delta": S_s alone, no direction -- k_science_static on a shard
    that stays on its path.  "wfs_only": S_w alone -- the science arm must NOT contain it: phase_sci = phase - S_w 2 pi / lambda.
    "direction": both maps and a science direction -- k_science_residual with the difference as one more term.  science_residual()
    against tests/_static_ref.science_phase on the shard's own phase (and, under a direction, its own two atmosphere OPDs): the
    restatement's one expression, within the opd_m / rms_nm / strehl tolerances; science_psf() == the window of that phase_sci and
    project_wavefront("science") == the projection of it, bit for bit (the same kernels on the same buffer)."""
    from rlao_amd import _lib as L
    dtype = _dtype(mode)
    tol, label = TOL[dtype], f"static-science-{which}-{mode}"
    env = _env("top_first", mode, tag="sci")
    n = env.n_envs
    s_w, s_s = _maps_of(env), _maps_of(env, "science")
    try:
        if which == "delta":
            was = env.fused_step
            env.set_static_aberration(science=s_s)
            s_w = np.zeros_like(s_s)
            assert env.fused_step == was                            # a science-arm map alone moves no shard off its path
        elif which == "wfs_only":
            env.set_static_aberration(wfs=s_w)
            s_s = np.zeros_like(s_w)
        else:
            env.set_static_aberration(wfs=s_w, science=s_s)
            d = np.array(GD.DIRS["top_first"])
            env.set_science_direction(d[:, 0], d[:, 1])
        from oracle import ao_oracle as O                          # checker only
        opd2m = np.linalg.pinv(_m2opd(env))
        env.set_wavefront_basis(opd2m=opd2m)
        env.set_science(zero_padding=2, window=8, first_frame=0)
        obs = _prologue(env, 7)
        k_opd = env.src_wavelength / (2 * np.pi)
        for i in range(3):
            obs = env.step(i, GAIN * obs)[0]
            phase_sci, rms, sr = (_np(t) for t in env.science_residual())
            phase = _buf(env, L.B_PHASE)
            sci_atm = _np(env.science_atmosphere()) if which == "direction" else None
            atm = _buf(env, L.B_OPD_ATM) if which == "direction" else None
            for k in range(n):
                want, w_rms, w_sr = ST.science_phase(phase[k], env.pupil, s_w[k], s_s[k], env.src_wavelength,
                                                     None if sci_atm is None else sci_atm[k], None if atm is None else atm[k])
                what = f"step {i} env {k}"
                _close(phase_sci[k] * k_opd, want * k_opd, "opd_m", tol, label, err_msg="phase_sci " + what)
                _close(rms[k], w_rms, "rms_nm", tol, label, err_msg="rms " + what)
                _close(sr[k], w_sr, "strehl", tol, label, err_msg="strehl " + what)
                assert np.abs(phase_sci[k] - phase[k]).max() * k_opd > 100 * tol["opd_m"]
            # the camera and the projection look at that phase: the oracle's render of the restated phase_sci under the science
            # camera's own tolerance (tests/test_gpu_science.py), the projection within sum |row| of the projector times opd_m's
            psf, coef = _np(env.science_psf()).astype(np.float64), _np(env.project_wavefront("science")).astype(np.float64)
            inside = np.asarray(env.pupil, dtype=bool)
            for k in range(n):
                want = ST.science_phase(phase[k], env.pupil, s_w[k], s_s[k], env.src_wavelength,
                                        None if sci_atm is None else sci_atm[k], None if atm is None else atm[k])[0]
                full = O.telescope_psf(inside.astype(float), S._flux(env), want, 2)
                err = float(np.abs(psf[k] - S.S.crop(full[None], 8)[0]).max() / full.max())
                _OBSERVED.setdefault(label, {})["psf_over_peak"] = max(_OBSERVED.get(label, {}).get("psf_over_peak", 0.0), err)
                assert err <= S.TOL[dtype], (i, k, err)
                w_coef = opd2m @ (want * k_opd)[inside]
                bound = np.abs(opd2m).sum(axis=1) * tol["opd_m"]
                assert (np.abs(coef[k] - w_coef) <= bound).all(), (i, k, float((np.abs(coef[k] - w_coef) / bound).max()))
        _dump()
    finally:
        env.clear_static_aberration()
        env.clear_science_direction()
        env.clear_science()
        env.clear_wavefront_basis()


@pytest.mark.parametrize("mode", ["mfma", "f64"])
def test_a_common_path_map_leaves_the_science_arm_on_the_sensors_phase(mode):
    """S_s == S_w, no direction: the difference is zero, the library holds none, and what the science camera and
    project_wavefront look at is AOENV_B_PHASE itself -- bit for bit -- while the sensor arm carries the map."""
    from rlao_amd import _lib as L
    env, plain = _env("small", mode, tag="sci"), _env("small", mode, tag="plain")
    s_w = _maps_of(env)
    try:
        env.set_static_aberration(wfs=s_w, science=s_w)
        for e in (env, plain):
            e.set_science(zero_padding=2, window=8, first_frame=0)
        obs, obs_p = _prologue(env, 7), _prologue(plain, 7)
        env.step(0, GAIN * obs)
        plain.step(0, GAIN * obs_p)
        phase = _buf(env, L.B_PHASE)
        assert not np.array_equal(phase, _buf(plain, L.B_PHASE))
        with pytest.raises(L.AoEnvError, match="no science direction"):
            env.science_residual()                                  # the arms do not differ: there is no phase_sci
        psf = _np(env.science_psf())
        plain._shard.upload_state(L.B_PHASE, phase.astype(np.float64).reshape(plain.n_envs, -1), plain._stream())
        assert np.array_equal(psf, _np(plain.science_psf()))
    finally:
        for e in (env, plain):
            e.clear_static_aberration()
            e.clear_science()


# ---- 4. bit-for-bit identities --------------------------------------------------------------------------------------------------------
def _walk(env, seed, steps=STEPS):
    from rlao_amd import _lib as L
    log, obs = [], _prologue(env, seed)
    for i in range(steps):
        row = []
        obs = V._steps(env, obs, i, 1, row)
        log.append(row[0] + (_buf(env, L.B_PHASE), _buf(env, L.B_OPD_ATM)))
    return log, V._final(env)


TWINS = [("small", "mfma"), ("small", "general"), ("small", "f64"), ("odd", "mfma"), ("tiny_pyr", "mfma"), ("two_dm", "mfma")]


@pytest.mark.parametrize("case,mode", TWINS, ids=[f"{c}-{m}" for c, m in TWINS])
def test_each_env_of_the_mixed_shard_equals_its_uniform_twin(case, mode):
    """Env e of the shard with four different maps == env e of a twin of the same size and seeds whose envs all carry map e, given
    as ONE shared map (stride 0): every step output, buffer, screen, clock and telemetry row, bit for bit."""
    env, twin = _env(case, mode), _env(case, mode, tag="twin")
    s_w = _maps_of(env)
    try:
        env.set_static_aberration(wfs=s_w)
        got, _ = _walk(env, 11)
        for e in range(env.n_envs):
            twin.set_static_aberration(wfs=s_w[e])
            want, _ = _walk(twin, 11)
            V._same_log(got, want, [e], [e])
        assert not np.array_equal(got[-1][0][0], got[-1][0][1])
    finally:
        env.clear_static_aberration()
        twin.clear_static_aberration()


@pytest.mark.parametrize("case", ["small", "top_first"])
def test_an_env_has_the_same_bits_in_any_shard_and_at_any_place(case):
    """float32 (k_dm_static_mfma): env k of the mixed shard == the only env of a one-env shard with its seed and map, and env 0 ==
    env 1 of a two-env shard whose second env has its seed's screens and its map."""
    env = _env(case, "mfma")
    s_w = _maps_of(env)
    try:
        env.set_static_aberration(wfs=s_w)
        whole, _ = _walk(env, 11)
    finally:
        env.clear_static_aberration()
    for k in (1, 3):
        one = _make(case, "mfma", n=1)
        try:
            one.set_static_aberration(wfs=s_w[k:k + 1])
            got, _ = _walk(one, 11 + STRIDE * k)
        finally:
            one.close()
        V._same_log(got, whole, [0], [k])
    both = _make(case, "mfma", n=2)
    try:
        both.set_static_aberration(wfs=s_w[[3, 1]])
        got, _ = _walk(both, 11)
        V._same_log(got, whole, [1], [1])
    finally:
        both.close()


def test_a_shared_map_equals_the_same_map_per_env_and_env_ids_equal_whole_arrays():
    env, twin = _env("small", "mfma"), _env("small", "mfma", tag="twin")
    s_w, s_s = _maps_of(env), _maps_of(env, "science")
    try:
        env.set_static_aberration(wfs=s_w[2], science=s_s[1])                        # one copy, stride 0
        twin.set_static_aberration(wfs=np.tile(s_w[2], (4, 1, 1)), science=np.tile(s_s[1], (4, 1, 1)))
        assert all(np.array_equal(env.static_aberration[k], twin.static_aberration[k]) for k in ("wfs", "science"))
        (la, fa), (lb, fb) = _walk(env, 3), _walk(twin, 3)
        V._same_log(la, lb)
        V._same_final(fa, fb)
        assert np.array_equal(_np(env.science_residual()[0]), _np(twin.science_residual()[0]))
        # a part of the envs at a time, in the caller's order, == the whole arrays at once
        env.clear_static_aberration()
        env.set_static_aberration(wfs=s_w[[3, 0]], env_ids=[3, 0])
        env.set_static_aberration(wfs=s_w[1], science=s_s[1], env_ids=[1])
        env.set_static_aberration(wfs=s_w[2:3], env_ids=[2])
        env.set_static_aberration(science=s_s[[0, 2, 3]], env_ids=[0, 2, 3])
        twin.set_static_aberration(wfs=s_w, science=s_s)
        assert all(np.array_equal(env.static_aberration[k], twin.static_aberration[k]) for k in ("wfs", "science"))
        (la, fa), (lb, fb) = _walk(env, 3), _walk(twin, 3)
        V._same_log(la, lb)
        V._same_final(fa, fb)
        assert np.array_equal(_np(env.science_residual()[0]), _np(twin.science_residual()[0]))
    finally:
        env.clear_static_aberration()
        twin.clear_static_aberration()


LOOPS = ("run_integrator", "run_integrator_delay", "rollout", "policy_rollout", "run_integrator_modal")
LOOP_CASES = [("f32", l) for l in LOOPS] + [("f64", "run_integrator")]
_LOOP_ENVS = {}


def _loop_env(dtype, tag):
    if (dtype, tag) not in _LOOP_ENVS:
        env = GD._make("up70", dtype, gainCL=GAIN)
        env.wfs.cam.photonNoise = True
        _LOOP_ENVS[(dtype, tag)] = env
    env = _LOOP_ENVS[(dtype, tag)]
    env.set_delay(0)
    env.clear_modal()
    env._surface = "zonal"
    return env


@pytest.fixture(scope="module", autouse=True)
def _close_loop_envs():
    yield
    for env in _LOOP_ENVS.values():
        env.close()
    _LOOP_ENVS.clear()


def _attach(env, loop):
    """what both shards of the comparison carry: photon noise, both maps, a wavefront record, a long exposure of the science arm"""
    name = "run_integrator" if loop == "run_integrator_delay" else loop
    S._configure(env, name)
    if loop == "run_integrator_delay":
        env.set_delay(1)
    env.set_static_aberration(wfs=_maps_of(env), science=_maps_of(env, "science"))
    env.set_wavefront_basis(opd2m=np.linalg.pinv(OA._m2opd(env)))
    env.set_science(zero_padding=2, window=8, first_frame=2)
    obs = S._start(env, name)
    env.record_wavefront(0, S.STEPS, what=("residual", "atmosphere"))
    env.start_long_exposure()
    return obs


@pytest.mark.parametrize("dtype,loop", LOOP_CASES, ids=[f"{d}-{l}" for d, l in LOOP_CASES])
def test_every_loop_equals_per_call_stepping(dtype, loop):
    """8 frames of `up70` (fused without maps) under four sensor-arm and four science-arm maps with photon noise, a wavefront record
    (residual and atmosphere) and a long exposure attached: the on-device loop's final outputs, buffers, get_state(), record and long
    exposure are bit for bit those of a twin that takes the same frames through the per-call API."""
    import torch
    name = "run_integrator" if loop == "run_integrator_delay" else loop
    modal = loop == "run_integrator_modal"
    env, twin = _loop_env(dtype, "a"), _loop_env(dtype, "b")
    try:
        assert env.fused_step == (dtype == "f32")
        obs = _attach(env, loop)
        assert not env.fused_step
        handed, actions = S._run_loop(env, name, obs)
        torch.cuda.synchronize()
        got = GD._loop_state(env)
        obs_t = _attach(twin, loop)
        for k in range(S.STEPS):
            if modal:
                last = twin.step_modal(k, GAIN * obs_t)
            elif actions is not None:
                last = twin.step(k, actions[k])
            else:
                last = twin.step(k, GAIN * obs_t)
            obs_t = last[0]
        torch.cuda.synchronize()
        want = GD._loop_state(twin)
        assert got.keys() == want.keys()
        for k in want:
            S._same(got[k], want[k], k)
        assert np.abs(got["wf"]).max() > 0 and np.abs(got["le"][0]).max() > 0
    finally:
        for e in (env, twin):
            e.stop_wavefront_record()
            e.stop_long_exposure()
            e.clear_static_aberration()
            e.clear_science()
            e.clear_wavefront_basis()
            if loop == "policy_rollout":
                e.set_policy(None)


FUSED_LOOPS = ("run_integrator", "rollout", "policy_rollout", "run_integrator_modal")


@pytest.mark.parametrize("loop", FUSED_LOOPS)
def test_a_science_arm_map_alone_in_the_loops_of_a_fused_shard(loop):
    """float32 `up70` with a science-arm map ALONE: the shard stays on the fused step kernel, which stores its phase for the frames
    the science arm reads (sci_reads_step); k_science_static then forms phase_sci inside the loop for the long exposure and for
    the science-direction record.  Against a twin that takes the same frames through the per-call API and calls
    science_residual() after every step: the record (rms, Strehl) bit for bit, and the loop's outputs, buffers, get_state(),
    wavefront record and long exposure bit for bit."""
    import torch
    modal = loop == "run_integrator_modal"
    env, twin = _loop_env("f32", "a"), _loop_env("f32", "b")
    try:
        recs = []
        for e in (env, twin):
            S._configure(e, loop)
            e.set_static_aberration(science=_maps_of(e, "science"))
            assert e.fused_step and e._shard.static_surface_path() == 0
            e.set_wavefront_basis(opd2m=np.linalg.pinv(OA._m2opd(e)))
            e.set_science(zero_padding=2, window=8, first_frame=2)
        obs = S._start(env, loop)
        env.record_wavefront(0, S.STEPS, what=("residual", "atmosphere"))
        env.start_long_exposure()
        rec = env.record_science_direction(0, S.STEPS)
        handed, actions = S._run_loop(env, loop, obs)
        torch.cuda.synchronize()
        assert env.fused_step
        got = GD._loop_state(env)
        obs_t = S._start(twin, loop)
        twin.record_wavefront(0, S.STEPS, what=("residual", "atmosphere"))
        twin.start_long_exposure()
        want_rec = []
        for k in range(S.STEPS):
            if modal:
                last = twin.step_modal(k, GAIN * obs_t)
            elif actions is not None:
                last = twin.step(k, actions[k])
            else:
                last = twin.step(k, GAIN * obs_t)
            obs_t = last[0]
            _, rms, sr = twin.science_residual()
            want_rec.append(np.stack([_np(rms), _np(sr)]))
        torch.cuda.synchronize()
        want = GD._loop_state(twin)
        assert np.array_equal(_np(rec), np.stack(want_rec)) and np.abs(_np(rec)[:, 0]).min() > 0
        assert got.keys() == want.keys()
        for k in want:
            S._same(got[k], want[k], k)
        assert np.abs(got["le"][0]).max() > 0
    finally:
        for e in (env, twin):
            e.stop_science_direction_record()
            e.stop_wavefront_record()
            e.stop_long_exposure()
            e.clear_static_aberration()
            e.clear_science()
            e.clear_wavefront_basis()
            if loop == "policy_rollout":
                e.set_policy(None)


def test_partial_resets_and_new_screens_leave_the_maps_alone():
    """`small`, float32: after reset_envs and generate_new_phase_screen the maps are the ones held before and the shard is still
    on the path of a shard with a map; the episode that follows is bit for bit that of a twin which made the same calls WITHOUT
    maps and was given them only afterwards."""
    from rlao_amd import _lib as L
    env, twin = _make("small", "mfma"), _make("small", "mfma")       # (shards of their own: a partial reset leaves per-env clocks)
    s_w, s_s = _maps_of(env), _maps_of(env, "science")

    def history(e):
        obs = _prologue(e, 11)
        e.step(0, GAIN * obs)
        e.reset_envs([1, 3], seed=900)
        e.step(1, GAIN * e.reset_soft())
        e.generate_new_phase_screen(77)

    def episode(e):
        log, obs = [], _prologue(e, 13)
        for i in range(3):
            row = []
            obs = V._steps(e, obs, i, 1, row)
            log.append(row[0] + (_buf(e, L.B_PHASE), _np(e.science_residual()[0])))
        return log

    try:
        env.set_static_aberration(wfs=s_w, science=s_s)
        history(env)
        held = env.static_aberration
        assert np.array_equal(held["wfs"], s_w) and np.array_equal(held["science"], s_s)
        assert not env.fused_step and env._shard.static_surface_path() == 1
        history(twin)
        twin.set_static_aberration(wfs=s_w, science=s_s)
        V._same_log(episode(env), episode(twin))
    finally:
        env.close()
        twin.close()


def test_a_sensor_arm_of_zeros_stays_held_through_a_partial_assignment():
    """A sensor arm given as zeros is held (the shard takes the path of a shard with a map); assigning the science arm of a part of
    the envs afterwards leaves it held."""
    env = _env("small", "mfma")
    try:
        was = env.fused_step
        env.set_static_aberration(wfs=np.zeros((env.R, env.R)))
        assert not env.fused_step and env._shard.static_surface_path() == 1
        env.set_static_aberration(science=_maps_of(env, "science")[:1], env_ids=[2])
        assert not env.fused_step and env._shard.static_surface_path() == 1 and not env.static_aberration["wfs"].any()
        env.clear_static_aberration()
        assert env.fused_step == was
        env.set_static_aberration(science=_maps_of(env, "science")[:1], env_ids=[2])      # no sensor arm held: it stays absent
        assert env.fused_step == was and env._shard.static_surface_path() == 0
    finally:
        env.clear_static_aberration()


def test_launch_counts_and_the_fused_path():
    """float32 `up70`: without maps -- never set, or set and cleared -- 8 steps of run_integrator launch the same kernels (counted,
    not timed) on the fused path; under a sensor-arm map the fused kernel is not launched and the phase kernel runs once per step;
    under a science-arm map alone the shard stays fused."""
    a, b = _loop_env("f32", "a"), _loop_env("f32", "b")
    counts = []
    for env, mode in ((a, "never"), (b, "cleared"), (b, "set"), (b, "science")):
        assert env.fused_step
        if mode in ("cleared", "set"):
            env.set_static_aberration(wfs=_maps_of(env))
            assert not env.fused_step
        if mode == "science":
            env.set_static_aberration(science=_maps_of(env, "science"))
            assert env.fused_step
        if mode == "cleared":
            env.clear_static_aberration()
            assert env.fused_step and env.static_aberration is None
        _prologue(env, 5)
        env._shard.profile(True)
        env.run_integrator(0, 8)
        prof = env._shard.profile_read(env._stream())
        counts.append(({k: v[1] for k, v in prof.items()}, env._shard.step_counters()))
        env._shard.profile(False)
        env.clear_static_aberration()
    assert counts[0] == counts[1] == counts[3]
    assert counts[0][1][1] == 8 and counts[0][0]["env_step"] >= 1
    assert counts[2][0].get("env_step", 0) == 0 and counts[2][0]["phase"] == 8 and tuple(counts[2][1]) == (0, 0)


def test_refusals_and_cleared_maps_leave_no_trace():
    """`up70`, float32 (fused): what is refused is refused before a launch and changes nothing; a cleared shard and a shard that only
    saw refused calls step on bit-identical to an untouched one, on the fused path."""
    from rlao_amd import _lib as L
    cleared, refused, plain = (GD._make("up70", "f32") for _ in range(3))
    try:
        R = plain.R
        s_w, s_s = _maps_of(cleared), _maps_of(cleared, "science")
        cleared.set_static_aberration(wfs=s_w, science=s_s)
        for env, had in ((cleared, True), (refused, False)):
            for bad in (np.zeros((R, R + 1)), np.zeros((3, R, R)), np.full((R, R), np.nan), np.full((4, R, R), np.inf), "map"):
                with pytest.raises(ValueError):
                    env.set_static_aberration(wfs=bad)
                with pytest.raises(ValueError):
                    env.set_static_aberration(science=bad, env_ids=[1] if np.ndim(bad) != 3 else None)
            with pytest.raises(ValueError):
                env.set_static_aberration()
            nan = s_w.copy()
            nan[1, 3, 2] = np.nan                                    # past the Python layer: the library's own checks
            with pytest.raises(L.AoEnvError, match=r"wfs\[\d+\] is not finite"):
                L.call(env._shard, "aoenv_set_static_opd", nan, None, 4, env._stream())
            with pytest.raises(L.AoEnvError, match=r"science\[\d+\] is not finite"):
                L.call(env._shard, "aoenv_set_static_opd", s_w, nan, 4, env._stream())
            with pytest.raises(L.AoEnvError, match="the shard has 4 envs"):
                L.call(env._shard, "aoenv_set_static_opd", s_w[:3].copy(), None, 3, env._stream())
            huge = np.full_like(s_w, 1e300)                         # finite in float64, not in the float32 shard's dtype
            with pytest.raises(L.AoEnvError, match="not finite in the env dtype"):
                L.call(env._shard, "aoenv_set_static_opd", huge, None, 4, env._stream())
            if had:
                assert np.array_equal(env.static_aberration["wfs"], s_w) and np.array_equal(env.static_aberration["science"], s_s)
                assert not env.fused_step
            else:
                assert env.static_aberration is None and env.fused_step
                with pytest.raises(L.AoEnvError, match="no static map"):
                    L.call(env._shard, "aoenv_get_static_opd", np.zeros((4, R, R)), None)
        cleared.clear_static_aberration()
        assert cleared.static_aberration is None and cleared.fused_step
        logs = []
        for env in (cleared, refused, plain):
            log = []
            V._steps(env, _prologue(env, 13), 0, 4, log)
            logs.append((log, V._final(env)))
        for log, fin in logs[:2]:
            V._same_log(log, logs[2][0])
            V._same_final(fin, logs[2][1])
    finally:
        for env in (cleared, refused, plain):
            env.close()


# ---- 5. composition ---------------------------------------------------------------------------------------------------------------------
COMPOSE_TOL = {"f32": F32_TOL, "f64": F64_SAME_OPERATOR_TOL}


@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_composed_with_per_env_mirrors_behind_a_delay_with_a_disturbance(dtype):
    """tests/test_gpu_compose.py's mixed case, `small`: every env its own mis-registered mirror (per-env tables through their
    stride), vibration line and a two-frame delay, plus its own sensor-arm map: against tests/_compose_ref.py's per-env oracles with
    the map attached (tests/_static_ref.py), through that module's replay and its unchanged tolerances."""
    features = ("mirror", "disturbance", "delay")
    env = TC._shard("sh", dtype, tag="static")
    try:
        TC._apply(env, features=features)
        s_w = maps(env.R, float(env.param.diameter), TC.N)
        env.set_static_aberration(wfs=s_w)
        assert not env.fused_step
        orc = TC.CR.mixed_oracle(TC._base(env), TC.PITCH, m2c=env.M2C_CL, modal_cm=env.modal_CM, off=("r0", "wind", "threshold", "magnitude"))
        for e, o in enumerate(orc.envs):
            ST.static(o, s_w[e])
        rec = TC.CR.drive(orc, TC.STEPS)
        TC._replay(env, rec, COMPOSE_TOL[dtype], f"static-composed-mirror-delay-disturbance-{dtype}")
    finally:
        env.clear_static_aberration()
        TC._clear(env)


@pytest.mark.parametrize("mode", ["mfma", "f64"])
def test_composed_with_actuator_pairs(mode):
    """`small` with tests/_dm_rot_ref.py's four rotated mirrors (actuator pairs: the surface is formed ahead anyway, the map is
    added by one trailing launch) and four maps: against the rotated oracles with the map attached; dm.surface() stays the mirror
    alone."""
    import _dm_rot_ref as REF
    import test_gpu_dm_pairs as DP
    env = TC._shard("sh", _dtype(mode), tag="static")
    env._case_rows, env._case_wind = list(range(TC.N)), False
    try:
        sets = REF.mirrors(env.param.diameter / env.param.nSubaperture)
        env.set_dm_rotation(**{k: np.array([s.get(k, 0.0) for s in sets]) for k in ("rotation_angle", "shift_x", "shift_y", "radial_scaling", "tangential_scaling")})
        PY, PX = DP._pairs(env)
        env.set_dm_pairs_per_env(PY[3:], PX[3:], env_ids=[3])       # mirror 3's dead actuator (tests/test_gpu_dm_pairs.py)
        s_w = maps(env.R, float(env.param.diameter), TC.N)
        before = env.dm.surface()
        env.set_static_aberration(wfs=s_w)
        assert np.array_equal(env.dm.surface(), before) and env._shard.static_surface_path() == 3
        orc = REF.rotated_oracle(TC._base(env), range(TC.N), TC.SEED, DP.STRIDE, n_subap=env.param.nSubaperture,
                                 mech_coupling=env.param.mechanicalCoupling, m2c=env.M2C_CL, modal_cm=env.modal_CM)
        for e, o in enumerate(orc.envs):
            ST.static(o, s_w[e])
        rec = TC.CR.drive(orc, TC.STEPS, rs_seed=DP.ACTION_SEED)
        TC._replay(env, rec, COMPOSE_TOL[_dtype(mode)], f"static-composed-pairs-{mode}")
    finally:
        env.clear_static_aberration()
        TC._clear(env)


@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_composed_with_a_guide_and_a_science_direction(dtype):
    """`top_first`: every env its own guide direction, science direction (zenith 0: classical anisoplanatism), sensor-arm and
    science-arm map.  The sensor's outputs against the guided oracle with the map attached; science_residual() against the
    restatement on the oracle's own layers, mirror and maps."""
    import torch
    from rlao_amd import _lib as L
    tol, label = TOL[dtype], f"static-composed-directions-{dtype}"
    env = _env("top_first", "f64" if dtype == "f64" else "mfma", tag="dir")
    g = CASES["top_first"][0]
    s_w, s_s = _maps_of(env), _maps_of(env, "science")
    try:
        orcs = []
        for k in range(4):
            o = copy.deepcopy(_base("top_first", env), memo={id(x): x for x in (_base("top_first", env).dm_modes,) if x is not None})
            GR.guide(o, g["altitude"], *GD.DIRS["top_first"][k])
            orcs.append(ST.static(o, s_w[k]))
        d = np.array(GD.DIRS["top_first"])
        env.set_guide_direction(d[:, 0], d[:, 1])
        env.set_science_direction(0.0, 0.0)
        env.set_static_aberration(wfs=s_w, science=s_s)
        for k, o in enumerate(orcs):
            o.new_episode(3 + STRIDE * k)
        obs = np.stack([o.reset_soft() for o in orcs])
        got0 = _np(_prologue(env, 3))
        k_opd = env.src_wavelength / (2 * np.pi)
        rs = np.random.RandomState(9)
        for k in range(4):
            _close(got0[k], obs[k], "obs", tol, label, err_msg=f"obs after reset env {k}")
        for i in range(STEPS):
            act = (GAIN * obs + 0.05 * rs.randn(*obs.shape)).astype(np.float32) * orcs[0].dm_mask[None].astype(np.float32)
            got = env.step(i, torch.as_tensor(act))
            phase, atm = _buf(env, L.B_PHASE), _buf(env, L.B_OPD_ATM)
            phase_sci, rms, sr = (_np(t) for t in env.science_residual())
            new = []
            for k, o in enumerate(orcs):
                mirror = o.dm_opd(o.coefs) - s_w[k]                 # the surface this step's measurement sees, the mirror alone
                oo, _, _, osr, _, _ = o.step(i, act[k])
                new.append(oo)
                what = f"step {i} env {k}"
                _close(atm[k], o.atm.OPD_no_pupil, "opd_m", tol, label, err_msg="AOENV_B_OPD_ATM " + what)
                _close(phase[k] * k_opd, o.tel_OPD, "opd_m", tol, label, err_msg="phase " + what)
                _close(_np(got[0])[k], oo, "obs", tol, label, err_msg="obs " + what)
                _close(_np(got[3])[k], osr, "strehl", tol, label, err_msg="strehl " + what)
                axis = X.science_opd(o.atm, g["altitude"], 0.0, 0.0)
                w_opd, _, w_rms, w_sr = X.science_residual(axis + s_s[k], mirror, o.pupil, o.wavelength)
                _close(phase_sci[k] * k_opd, w_opd, "opd_m", tol, label, err_msg="phase_sci " + what)
                _close(rms[k], w_rms, "rms_nm", tol, label, err_msg="science rms " + what)
                _close(sr[k], w_sr, "strehl", tol, label, err_msg="science strehl " + what)
            obs = np.stack(new)
        _dump()
    finally:
        env.clear_static_aberration()
        env.clear_science_direction()
        env.clear_guide_direction()
