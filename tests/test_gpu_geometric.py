"""GPU: the geometric Shack-Hartmann (``set_params(..., is_geometric=True)``, AOENV_WFS_SH_GEOMETRIC) against the float64 restatement
tests/_geometric_ref.py, the reference's golden tests/golden/geometric_sh.npz (scripts/make_geometric_golden.py) and bitwise twins.

Shapes: the golden's three geometries (R = 24 p = 6; R = 20 with 5 x 5 lenslets, p = 4; R = 30 with p = 5 and obstruction 0.3, which
float32 shards run through k_phase_mfma), R = 32 with p = 8 and obstruction 0.3, R = 96 with 16 x 16 lenslets (six phase bands, the
16-byte matrix-core phase kernel), R = 42 with two layers on grids of their own (tests/_fov_cases.py "two"), and once the C2 geometry
(R = 120, 20 x 20) with four envs.

Tolerances, none taken from the code under test: the signal is held to ``geo_signal_bound`` of the OPD tolerance of
tests/test_gpu_parity.py (F64_SAME_OPERATOR_TOL["opd_m"] on float64 shards, F32_TOL["opd_m"] on float32 shards: the sensor is
linear, an OPD error bounds the slope error); the observation to (largest absolute row sum of the env's reconstructor) x 1e6 x that
bound; OPD, Strehl and rms to the two dicts unchanged; slope units and interaction-matrix columns to 1e-10 relative against the
golden (the bound tests/test_gpu_configs.py holds the reference's interaction-matrix columns to).  AO_PARITY_REPORT=<file> writes
the measured maxima (profiles/geometric_parity_maxima.json is such a run)."""
import json
import os

import numpy as np
import pytest

import _fov_cases as F
import _geometric_ref as G
from test_gpu_parity import F32_TOL, F64_SAME_OPERATOR_TOL

pytestmark = pytest.mark.gpu

ATM = dict(r0=0.13, L0=30.0, windSpeed=[10.0], windDirection=[72.0], fractionalR0=[1.0], altitude=[0.0], nLoop=64)
GEO = {
    "r24": dict(ATM, diameter=1.6, nSubaperture=4, nPixelPerSubap=6, nModes=8),
    "r20": dict(ATM, diameter=2.0, nSubaperture=5, nPixelPerSubap=4, nModes=8),
    "r30": dict(ATM, diameter=2.4, nSubaperture=6, nPixelPerSubap=5, nModes=8, centralObstruction=0.3),
    "r32": dict(ATM, diameter=1.6, nSubaperture=4, nPixelPerSubap=8, nModes=8, centralObstruction=0.3),
    "r96": dict(ATM, diameter=6.4, nSubaperture=16, nPixelPerSubap=6, nModes=20),
    "c2": dict(ATM, diameter=8.0, nSubaperture=20, nPixelPerSubap=6, nModes=50),
    # the fused tail takes its 20 lenslet rows in bands of 7, 7 and 6: the partial last band lays its LDS work area out anew, its pupil
    # flags over the totals of the band before (the plan is pinned by tests/test_geometric_host.py)
    "r160": dict(ATM, diameter=8.0, nSubaperture=20, nPixelPerSubap=8, nModes=50),
}
TOL = {"f64": F64_SAME_OPERATOR_TOL, "f32": F32_TOL}
_OBSERVED = {}
_ENVS = {}


@pytest.fixture(scope="module", autouse=True)
def _close_envs():
    yield
    for env in _ENVS.values():
        env.close()
    _ENVS.clear()
    path = os.environ.get("AO_PARITY_REPORT")
    if path:
        with open(path, "w") as f:
            json.dump(_OBSERVED, f, indent=1, sort_keys=True)


def _seen(label, key, value, bound):
    rec = _OBSERVED.setdefault(label, {})
    rec[key] = max(rec.get(key, 0.0), float(value))
    rec[key + "_bound"] = float(bound)
    print(f"{label}: {key} {float(value):.3e} (bound {float(bound):.3e})")


def _new_env(geo, dtype, n_envs, camera="ideal", opts=None, seed_stride=1, geometric=True, **kw):
    """``geometric``: the keyword handed to set_params; None: none (the parameter dict decides)."""
    from rlao_amd import _lib as L
    from rlao_amd.env import BatchedAOEnv
    env = BatchedAOEnv(n_envs=n_envs, device=0, dtype=dtype, env_seed_stride=seed_stride)
    try:
        if geometric is not None:
            kw = dict(kw, is_geometric=geometric)
        env.set_params(dict(geo), camera=camera, wfs_type="shackhartmann", **kw)
        for k, v in (opts or {}).items():
            L.check(env._shard.lib.aoenv_set_option(env._shard.h, getattr(L, k), v))
    except Exception:
        env.close()
        raise
    return env


def _env(name, dtype, n_envs=2, tag="a", **kw):
    key = (name, dtype, n_envs, tag, json.dumps({k: str(v) for k, v in kw.items()}, sort_keys=True))
    if key not in _ENVS:
        _ENVS[key] = _new_env(GEO[name], dtype, n_envs, **kw)
    return _ENVS[key]


def _sig_bound(env, dtype):
    p = env.R // env.param.nSubaperture
    return G.geo_signal_bound(TOL[dtype]["opd_m"], p, env.param.diameter / env.R, env.slopes_units, env.src_wavelength)


def _signal(env):
    from rlao_amd import _lib as L
    return env._shard.download(L.B_SIGNAL, (env.n_envs, env.nSignal), env._stream())


def _phase(env):
    from rlao_amd import _lib as L
    return env._shard.download(L.B_PHASE, (env.n_envs, env.R, env.R), env._stream())


def _frame(env):
    from rlao_amd import _lib as L
    return env._shard.download(L.B_FRAME, (env.n_envs, env.cam_res, env.cam_res), env._stream())


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def _masked_phase_is_the_unmasked_one(env, what):
    """AOENV_B_PHASE == phase_no_pupil inside the pupil, bit for bit; zero outside."""
    ph, pnp = _phase(env), env.phase_no_pupil
    pup = np.broadcast_to(env.pupil, ph.shape)
    assert np.abs(pnp[~pup]).max() > 0, (what, "the unmasked phase is zero outside the pupil")
    assert _same_bits(ph[pup], pnp[pup]), what
    assert not np.any(ph[~pup]), what


def _dm_opd(env, coefs):
    dmt = env._dm_tables
    C = np.zeros((len(coefs), dmt.nAct * dmt.nAct))
    C[:, dmt.act_idx] = coefs
    return np.einsum("yi,nij,xj->nyx", dmt.gy, C.reshape(-1, dmt.nAct, dmt.nAct), dmt.gx)


def _valid2d(env):
    ns = env.param.nSubaperture
    v = np.zeros(ns * ns, dtype=bool)
    v[np.asarray(env._wfs_valid_idx)] = True
    return v.reshape(ns, ns)


# ---- measure: random unmasked OPD and random commands against the restatement ----------------------------------------------------------
MEASURE = [(n, d) for n in ("r24", "r20", "r30", "r32", "r96") for d in ("f64", "f32")]


@pytest.mark.parametrize("name,dtype", MEASURE, ids=[f"{n}-{d}" for n, d in MEASURE])
def test_measure_against_the_restatement(name, dtype):
    env = _env(name, dtype, n_envs=3)
    assert env.is_geometric and env.wfs.is_geometric and env.wfs.tag == "shackHartmann" and not env.fused_step
    assert not np.any(env.reference_centroids)
    rng = np.random.RandomState(11)
    R, n = env.R, env.n_envs
    opd = rng.normal(size=(n, R, R)) * 50e-9                        # not masked
    coefs = rng.normal(size=(n, env.nValidAct)) * 80e-9
    env._shard.set_atm_opd(opd.reshape(n, R * R), env._stream())
    env._shard.set_coefs(coefs, env._stream())
    env._shard.measure(env._stream())
    got = _signal(env).astype(np.float64)
    k = 2 * np.pi / env.src_wavelength
    phi = (opd + _dm_opd(env, coefs)) * k
    valid = _valid2d(env)
    want = np.array([G.geo_signal(x, env.pupil, valid, env.param.diameter / R, env.slopes_units) for x in phi])
    bound = _sig_bound(env, dtype)
    _seen(f"measure-{name}-{dtype}", "signal", np.abs(got - want).max(), bound)
    assert np.abs(want).max() > 0.1 and np.abs(got - want).max() <= bound
    # the unmasked phase: the restatement's within the OPD tolerance, the masked one bit for bit inside the pupil
    pnp = env.phase_no_pupil.astype(np.float64)
    _seen(f"measure-{name}-{dtype}", "opd_m", np.abs(pnp - phi).max() / k, TOL[dtype]["opd_m"])
    assert np.abs(pnp - phi).max() / k <= TOL[dtype]["opd_m"]
    _masked_phase_is_the_unmasked_one(env, (name, dtype))
    assert not np.any(_frame(env)) and not np.any(env.wfs.cam.frame)
    # aoenv_reset_soft reconstructs from that signal
    obs = env.reset_soft().cpu().numpy().astype(np.float64)
    rec = np.asarray(env.reconstructor, dtype=np.float64)
    want_obs = np.zeros_like(obs)
    want_obs[:, env.xvalid, env.yvalid] = -(want @ rec.T) * 1e6
    ob = np.abs(rec).sum(axis=1).max() * 1e6 * bound
    _seen(f"measure-{name}-{dtype}", "obs", np.abs(obs - want_obs).max(), ob)
    assert np.abs(obs - want_obs).max() <= ob


# ---- calibration against the reference's golden ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", list(G.GEOMETRIES))
def test_calibration_matches_the_reference(tag):
    g = np.load(G.GOLDEN)
    env = _env(tag, "f64", n_envs=3)
    # (r30, odd p: the reference cannot select valid lenslets there -- its flux tiling takes 2 (p // 2) pixels -- and the golden's
    #  valid map is the flux rule applied to whole tiles by scripts/make_geometric_golden.py: the project's selection, not pinned by
    #  the reference; units, signals and columns below are the reference's arithmetic ON that map)
    assert np.array_equal(_valid2d(env), g[f"{tag}_valid"]) and np.array_equal(env.pupil, g[f"{tag}_pupil"])
    units = float(g[f"{tag}_slopes_units"])
    _seen(f"calibration-{tag}", "slopes_units_rel", abs(env.slopes_units - units) / units, 1e-10)
    assert abs(env.slopes_units - units) <= 1e-10 * units
    want = g[f"{tag}_poke_cols"]
    got = env.imat[:, g[f"{tag}_poke_idx"]]
    rel = (np.abs(got - want).max(axis=0) / np.abs(want).max(axis=0)).max()
    _seen(f"calibration-{tag}", "imat_col_rel", rel, 1e-10)
    assert (np.abs(got - want).max(axis=0) <= 1e-10 * np.abs(want).max(axis=0)).all()
    # ... and the reference's own signals of its random DM commands, through the library
    coefs = g[f"{tag}_coefs"][:3]
    env._shard.set_atm_opd(np.zeros((3, env.R * env.R)), env._stream())
    env._shard.set_coefs(coefs, env._stream())
    env._shard.measure(env._stream())
    want = g[f"{tag}_sig_dm"][:3]
    _seen(f"calibration-{tag}", "signal_of_reference_commands", np.abs(_signal(env) - want).max(), _sig_bound(env, "f64"))
    assert np.abs(_signal(env) - want).max() <= _sig_bound(env, "f64")


# ---- closed loop against the GeometricOracle --------------------------------------------------------------------------------------------
def _oracle_for(env, geo):
    at = env._atm_tables
    geoms = F.layer_geometries(dict(geo, fov=geo.get("fov", 0.0)))
    ops = [(at.A, at.B)] * len(geoms) if at.uniform else [(t.A, t.B) for t in at.layers]
    return G.GeometricOracle(resolution=env.R, diameter=geo["diameter"], n_subap=geo["nSubaperture"], r0=geo["r0"], L0=geo["L0"],
                             windSpeed=geo["windSpeed"], windDirection=geo["windDirection"], fractionalR0=geo["fractionalR0"],
                             altitude=geo["altitude"], m2c=env.M2C_CL, n_modes=env.M2C_CL.shape[1], nLoop=geo["nLoop"],
                             fov_arcsec=geo.get("fov", 0.0), geom_AB=[(q, A, B) for q, (A, B) in zip(geoms, ops)],
                             modal_cm=env.modal_CM)


def _oracle_run(orc, seed, steps, gain=0.5):
    """The oracle's episode on its own float32 actions, handed over AS float32 arrays: the increment ``action * 1e-6`` is then the
    float32 product the reference forms (array * python float), which the library restates on every dtype (k_recon_finish)."""
    orc.new_episode(seed)
    obs = orc.reset_soft()
    rec = dict(obs0=obs, actions=[], obs=[], signal=[], opd=[], strehl=[], phase_np=[])
    for i in range(steps):
        act = (gain * obs).astype(np.float32)
        obs, _, _, sr, _, _ = orc.step(i, act)
        rec["actions"].append(act)
        rec["obs"].append(obs)
        rec["signal"].append(orc.wfs.signal.copy())
        rec["opd"].append(orc.tel_OPD.copy())
        rec["strehl"].append(sr)
    rec["total"], rec["residual"] = orc.total[:steps].copy(), orc.residual[:steps].copy()
    return rec


def _replay(env, geo, dtype, label, seed=17, steps=8):
    import torch
    orc = _oracle_for(env, geo)
    assert abs(orc.wfs.slopes_units - env.slopes_units) <= 1e-10 * env.slopes_units and orc.wfs.nSignal == env.nSignal
    rec = _oracle_run(orc, seed, steps)
    tol, sb = TOL[dtype], _sig_bound(env, dtype)
    ob = np.abs(np.asarray(env.reconstructor)).sum(axis=1).max() * 1e6 * sb
    env.env_seed_stride = 0                                         # every env the same episode
    env.generate_new_phase_screen(seed)
    env.dm.coefs = 0
    env.dm_prev = 0
    env.measure()
    obs0 = env.reset_soft().cpu().numpy()
    bad = []

    def close(got, want, key, bound, what):
        err = float(np.abs(np.asarray(got, dtype=np.float64) - want).max())
        _seen(label, key, err, bound)
        if not err <= bound:
            bad.append(f"{what}: {key} off by {err:.3e} (bound {bound:.3e})")

    k = env.src_wavelength / (2 * np.pi)
    for e in range(env.n_envs):
        close(obs0[e], rec["obs0"], "obs", ob, "reset")
    for i in range(steps):
        act = torch.as_tensor(np.stack([rec["actions"][i]] * env.n_envs))
        obs, frame, rew, sr, _, _ = env.step(i, act)
        sig, ph = _signal(env), _phase(env)
        assert not np.any(frame.cpu().numpy())
        for e in range(env.n_envs):
            close(sig[e], rec["signal"][i], "signal", sb, f"step {i}")
            close(obs[e].cpu().numpy(), rec["obs"][i], "obs", ob, f"step {i}")
            close(ph[e] * k, rec["opd"][i], "opd_m", tol["opd_m"], f"step {i}")
            close(float(sr[e]), rec["strehl"][i], "strehl", tol["strehl"], f"step {i}")
        _masked_phase_is_the_unmasked_one(env, (label, i))
    for e in range(env.n_envs):
        close(env.total[:steps, e] if np.ndim(env.total) == 2 else env.total[:steps], rec["total"], "rms_nm", tol["rms_nm"], "total")
        close(env.residual[:steps, e] if np.ndim(env.residual) == 2 else env.residual[:steps], rec["residual"], "rms_nm", tol["rms_nm"], "residual")
    assert not bad, (label, bad[:10])
    return orc


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("fused_tail", [1, 0])
def test_closed_loop_against_the_geometric_oracle(dtype, fused_tail):
    """Eight steps at R = 24 (0.3 pixel per frame: two ring extrusions).  The env is handed the oracle's ring operators."""
    from oracle import ao_oracle as O
    geo = GEO["r24"]
    geom = O.LayerGeometry(24, geo["diameter"], geo["L0"])
    A, B = geom.AB(geo["r0"])
    env = _env("r24", dtype, n_envs=2, tag="AB", atm_AB=(A, B), opts=dict(OPT_FUSED_TAIL=fused_tail))
    orc = _replay(env, geo, dtype, f"closed-loop-r24-{dtype}-tail{fused_tail}")
    assert max(l.buff.max() for l in orc.atm.layers) < 1 and orc.residual[7] < 0.6 * orc.total[7]


def test_two_layers_on_grids_of_their_own():
    """tests/_fov_cases.py "two" (R = 42: k_phase_mfma, grids of 46 and 61 pixels) against the oracle handed the env's operators."""
    geo = F.geo("two")
    key = ("two", "f32")
    if key not in _ENVS:
        _ENVS[key] = _new_env(geo, "f32", 2)
    env = _ENVS[key]
    assert not env._atm_tables.uniform
    _replay(env, geo, "f32", "closed-loop-two-layers-f32", seed=F.CASES["two"]["seed"], steps=6)


# ---- exact properties ---------------------------------------------------------------------------------------------------------------
def _actions(seeds, step, a):
    """Fixed actions [len(seeds), a, a] in micrometres, a function of (env seed, step) alone."""
    return np.stack([np.random.RandomState(1000 * int(s) + step).normal(size=(a, a)) * 0.05 for s in seeds]).astype(np.float32)


def _episode(env, seed, steps, seeds=None, hold_prev=False):
    """A fresh episode on the fixed actions of the envs' seeds; per step the signal, the observation, the Strehl ratio and the
    unmasked phase.  ``hold_prev``: dm_prev is zeroed before every step, so that the command is the increment alone -- the same bits
    from the fused tail and from the epilogue kernel, whose ``dm_prev * leak + inc`` the compiler contracts differently (a property
    of the two tails that diffractive shards share; shards that are to agree bit for bit across the two must not carry it)."""
    import torch
    seeds = [seed + e * env.env_seed_stride for e in range(env.n_envs)] if seeds is None else seeds
    env.generate_new_phase_screen(seed)
    env.dm.coefs = 0
    env.dm_prev = 0
    env.measure()
    out = [dict(signal=_signal(env), obs=env.reset_soft().cpu().numpy())]
    for i in range(steps):
        if hold_prev:
            env.dm_prev = 0
        obs, frame, rew, sr, _, _ = env.step(i, torch.as_tensor(_actions(seeds, i, env.nActuator)))
        out.append(dict(signal=_signal(env), obs=obs.cpu().numpy(), strehl=sr.cpu().numpy(), phase_np=env.phase_no_pupil))
    return out


@pytest.mark.parametrize("name,dtype", [("r24", "f32"), ("r24", "f64"), ("r30", "f32"), ("r96", "f32")])
def test_every_phase_path_stores_the_same_unmasked_phase(name, dtype):
    """phase_no_pupil x pupil == AOENV_B_PHASE bit for bit on every phase path the shard can take (the default, the dword matrix-core
    kernel, k_phase<T> with the matrix cores off), from the screens (one layer: the band variant) and from a user OPD; the paths
    agree with one another on the signal's bound."""
    from rlao_amd import _lib as L
    env = _env(name, dtype, n_envs=2, tag="paths")
    lib, h = env._shard.lib, env._shard.h
    rng = np.random.RandomState(3)
    coefs = rng.normal(size=(2, env.nValidAct)) * 80e-9
    opd = rng.normal(size=(2, env.R * env.R)) * 50e-9
    sigs = []
    try:
        for path, mfma in ((0, 1), (L.PATH_PHASE_DWORD, 1), (L.PATH_GENERIC, 1), (0, 0)):
            L.check(lib.aoenv_set_option(h, L.OPT_FORCE_PATH, path))
            L.check(lib.aoenv_set_option(h, L.OPT_MFMA_GEMM, mfma))
            env.generate_new_phase_screen(5)
            env._shard.set_coefs(coefs, env._stream())
            env._shard.measure(env._stream())
            _masked_phase_is_the_unmasked_one(env, (name, dtype, path, mfma, "screens"))
            env._shard.set_atm_opd(opd, env._stream())
            env._shard.measure(env._stream())
            _masked_phase_is_the_unmasked_one(env, (name, dtype, path, mfma, "user OPD"))
            sigs.append(_signal(env).astype(np.float64))
    finally:
        L.check(lib.aoenv_set_option(h, L.OPT_FORCE_PATH, 0))
        L.check(lib.aoenv_set_option(h, L.OPT_MFMA_GEMM, 1))
    for s in sigs[1:]:
        assert np.abs(s - sigs[0]).max() <= 2 * _sig_bound(env, dtype)


@pytest.mark.parametrize("name,dtype", [("r24", "f32"), ("r24", "f64"), ("r30", "f32"), ("r96", "f32"), ("c2", "f32"), ("c2", "f64"),
                                        ("r160", "f32")])
def test_fused_tail_signal_is_the_stand_alone_kernels(name, dtype):
    """AOENV_OPT_FUSED_TAIL at 1 and at 0: the same signal and unmasked phase bit for bit over five steps (both kernels call one
    slope function); the launches are phase + tail, against phase + slopes + reconstruction + epilogue.  The tail of c2 runs two
    bands (12 + 8 lenslet rows in float32, 6 + 6 + 6 + 2 in float64), that of r160 three (7 + 7 + 6) with a last band whose work area
    overlaps the totals of the band before it; the other shapes are one band."""
    a = _env(name, dtype, n_envs=2, tag="tail1")
    b = _env(name, dtype, n_envs=2, tag="tail0", opts=dict(OPT_FUSED_TAIL=0))
    a._shard.profile(True)
    b._shard.profile(True)
    ra, rb = _episode(a, 21, 5, hold_prev=True), _episode(b, 21, 5, hold_prev=True)
    pa, pb = a._shard.profile_read(a._stream()), b._shard.profile_read(b._stream())
    a._shard.profile(False)
    b._shard.profile(False)
    for i, (x, y) in enumerate(zip(ra, rb)):
        assert _same_bits(x["signal"], y["signal"]), (name, dtype, i)
        if i:
            assert _same_bits(x["phase_np"], y["phase_np"]), (name, dtype, i)
            # (observation and Strehl ratio come from two epilogues, tail_from_slopes and k_recon_finish, whose sums and exp differ in
            #  the last bits as they do on diffractive shards: held to the parity tolerances, not to the bit)
            assert np.abs(x["obs"].astype(np.float64) - y["obs"]).max() <= TOL[dtype]["obs"]
            assert np.abs(x["strehl"].astype(np.float64) - y["strehl"]).max() <= TOL[dtype]["strehl"]
    assert np.abs(ra[5]["signal"]).max() > 0.05
    n = {k: v[1] for k, v in pa.items()}
    assert n["sh_tail"] == 5 and n["sh_spots"] == 0 and n["detector"] == 0 and n["env_step"] == 0 and n["gemm_recon"] == 1, n
    assert n["sh_centroid"] == 1                                    # the prologue's measure: the stand-alone kernel
    n = {k: v[1] for k, v in pb.items()}
    assert n["sh_tail"] == 0 and n["sh_centroid"] == 6 and n["sh_spots"] == 0 and n["gemm_recon"] >= 6, n
    assert a._shard.step_counters() == (0, 0)


def test_an_env_has_the_same_bits_in_any_shard_and_at_any_place():
    """Env seed 20: row 3 of a 5-env shard, row 1 of another, and alone."""
    five = _env("r24", "f32", n_envs=5, tag="five")
    other = _env("r24", "f32", n_envs=5, tag="five-b")
    alone = _env("r24", "f32", n_envs=1, tag="alone")
    r5, ro, r1 = _episode(five, 17, 6), _episode(other, 19, 6), _episode(alone, 20, 6)
    for i in range(7):
        for key in r5[i]:
            assert _same_bits(r5[i][key][3], ro[i][key][1]) and _same_bits(r5[i][key][3], r1[i][key][0]), (i, key)
    assert not _same_bits(r5[6]["signal"][3], r5[6]["signal"][2])


def test_a_shard_above_1024_envs_equals_its_envs_in_a_small_shard():
    """1030 envs at R = 24 (no fused tail above 1024: the stand-alone kernel and the batched reconstruction) on fixed actions: the
    signal and the phase of the first, an inner and the last env are those of the env stepped alone through the fused tail."""
    big = _env("r24", "f32", n_envs=1030, tag="big")
    rb = _episode(big, 100, 3, hold_prev=True)
    for e in (0, 517, 1029):
        alone = _env("r24", "f32", n_envs=1, tag="alone")
        ra = _episode(alone, 100 + e, 3, hold_prev=True)
        for i in range(4):
            assert _same_bits(rb[i]["signal"][e], ra[i]["signal"][0]), (e, i)
            if i:
                assert _same_bits(rb[i]["phase_np"][e], ra[i]["phase_np"][0])
                assert abs(float(rb[i]["strehl"][e]) - float(ra[i]["strehl"][0])) <= F32_TOL["strehl"]      # (two epilogues)
                assert np.abs(rb[i]["obs"][e].astype(np.float64) - ra[i]["obs"][0]).max() <= F32_TOL["obs"]


@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_device_loops_equal_stepping(dtype):
    """run_integrator and rollout (sigma 0: the same actions) against step() on gain * obs, bit for bit, eight frames."""
    import torch
    a, b, c = (_env("r24", dtype, n_envs=2, tag=t) for t in ("loop-a", "loop-b", "loop-c"))
    for env in (a, b, c):
        env.generate_new_phase_screen(31)
        env.dm.coefs = 0
        env.dm_prev = 0
        env.measure()
    obs = a.reset_soft()
    for i in range(8):
        obs, _, rew, sr, _, _ = a.step(i, 0.5 * obs)
    b.reset_soft()
    ob, rb, sb = b.run_integrator(0, 3, gain=0.5)
    ob, rb, sb = b.run_integrator(3, 5, gain=0.5)
    assert torch.equal(ob, obs) and torch.equal(rb, rew) and torch.equal(sb, sr)
    assert _same_bits(_signal(a), _signal(b)) and _same_bits(a.phase_no_pupil, b.phase_no_pupil)
    c.reset_soft()
    ro = c.rollout(0, 8, sigma=0.0, gain=0.5, seed=1)
    assert torch.equal(ro.obs[8], obs) and torch.equal(ro.strehl[7], sr) and _same_bits(_signal(a), _signal(c))


def test_noise_settings_change_no_bit_and_count_no_frame():
    """The camera flavours are accepted: the frame stays zero, the noise frame counter does not advance, the signal is unchanged."""
    from rlao_amd import _lib as L
    ideal = _env("r24", "f32", n_envs=2, tag="ideal")
    razor = _env("r24", "f32", n_envs=2, tag="razor", camera="razor")
    papyrus = _env("r24", "f32", n_envs=2, tag="papyrus", camera="papyrus")
    papyrus.wfs.cam.configure(readoutNoise=2.0)
    assert papyrus.wfs.cam.photonNoise and razor.wfs.cam.readoutNoise
    want = _episode(ideal, 9, 4)
    for env in (razor, papyrus):
        got = _episode(env, 9, 4)
        for x, y in zip(got, want):
            for key in x:
                assert _same_bits(x[key], y[key]), key
        assert not np.any(_frame(env)) and not np.any(env.wfs.cam.frame)
        assert int(env._shard.download(L.B_COUNTERS, (4,), env._stream(), dtype=np.uint32)[0]) == 0


# ---- composition ----------------------------------------------------------------------------------------------------------------------
def _composed(env, rows):
    """CASE_MIXED of tests/_compose_ref.py without its stars: every env its own wind (one above a pixel per frame), r0, mis-registered
    mirror, one vibration line, and a delay of 1.  ``rows``: which case env each env of the shard is."""
    import _compose_ref as CR
    case, n = CR.CASE_MIXED, env.n_envs
    col = lambda key: np.array([case[key][e] for e in rows], dtype=np.float64)
    env.set_r0_per_env(col("r0"))
    m = [CR.mixed_misreg(e, 0.4) for e in rows]
    env.set_dm_misregistration(**{k: np.array([x.get(k, 0.0) for x in m]) for k in CR.MISREG_KEYS})
    dt = env.param.samplingTime
    freq = np.array([0.0 if case["dist_period"][e] is None else 1.0 / (case["dist_period"][e] * dt) for e in rows])
    env.set_disturbance(1, col("dist_amp").reshape(n, 1, 1), freq.reshape(n, 1, 1), t0=case["t0"])
    env.set_delay(case["delay"])
    env.generate_new_phase_screen(case["seed"])
    env.set_wind_per_env(np.array([[case["wind_speed"][e]] for e in rows]), np.array([[case["wind_dir"][e]] for e in rows]), reset=True,
                         max_pixels=case["wind_ceiling"])
    env.dm.coefs = 0
    env.dm_prev = 0
    env.measure()
    return env.reset_soft()


def test_composed_per_env_features_equal_their_uniform_twins():
    import _compose_ref as CR
    import torch
    case = CR.CASE_MIXED
    assert case["n_envs"] == 4 and case["delay"] == 1
    mixed = _new_env(GEO["r24"], "f32", 4, seed_stride=case["seed_stride"])
    twin = _new_env(GEO["r24"], "f32", 4, seed_stride=case["seed_stride"])
    try:
        obs = _composed(mixed, [0, 1, 2, 3])
        acts, rec = [], []
        for i in range(8):
            acts.append((0.5 * obs).clone())
            obs, _, rew, sr, _, _ = mixed.step(i, acts[-1])
            rec.append((_signal(mixed), obs.clone(), sr.clone()))
        assert not _same_bits(rec[7][0][0], rec[7][0][1])
        for e in range(4):
            _composed(twin, [e] * 4)
            for i in range(8):
                a = acts[i][e:e + 1].repeat(4, 1, 1)
                obs, _, rew, sr, _, _ = twin.step(i, a)
                # (row e of the twin: the same seed, the same place in the shard's streams)
                assert _same_bits(_signal(twin)[e], rec[i][0][e]), (e, i)
                assert torch.equal(obs[e], rec[i][1][e]) and torch.equal(sr[e], rec[i][2][e]), (e, i)
    finally:
        mixed.close()
        twin.close()


@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_modal_surface_projects_the_geometric_signal(dtype):
    """step_modal's observation is -1e6 cm @ signal of the step, within the projection bound of tests/_modal_ref.py."""
    import _modal_ref as MR
    import torch
    env = _env("r24", dtype, n_envs=2, tag="modal")
    env.set_modal(4)
    try:
        env.generate_new_phase_screen(12)
        env.dm.coefs = 0
        env.dm_prev = 0
        env.measure()
        obs = env.reset_soft_modal()
        for i in range(4):
            obs, _, rew, sr, _, _ = env.step_modal(i, 0.4 * obs)
            sig = _signal(env).astype(np.float64)
            cm = env._modal["cm"]
            o64 = -1e6 * sig @ cm.T
            bound = MR.projection_bound(env.dtype, cm, sig)
            assert (np.abs(obs.cpu().numpy().astype(np.float64) - o64) <= bound).all(), i
        assert np.abs(o64).max() > 1e-3
    finally:
        env.clear_modal()


# ---- the C2 geometry, once ---------------------------------------------------------------------------------------------------------------
def test_c2_geometry_calibrates_and_steps():
    """R = 120, 20 x 20 lenslets, four envs: the calibration against the restatement, two steps (the fused tail in bands of 12 and
    8 lenslet rows) against the restatement of the shard's own unmasked phase, a measurement through the stand-alone kernel against
    the same.  (Tail against stand-alone kernel bit for bit at this size: test_fused_tail_signal_is_the_stand_alone_kernels.)"""
    env = _env("c2", "f32", n_envs=4)
    valid = _valid2d(env)
    ps = env.param.diameter / env.R
    units = G.slopes_units_of(env.pupil, valid, ps, env.src_wavelength)
    assert abs(env.slopes_units - units) <= 1e-10 * units and not env.fused_step
    out = _episode(env, 40, 2)
    sb = _sig_bound(env, "f32")
    for i in (1, 2):
        want = np.array([G.geo_signal(x, env.pupil, valid, ps, env.slopes_units) for x in out[i]["phase_np"].astype(np.float64)])
        err = np.abs(out[i]["signal"] - want).max()
        _seen("c2-f32", "signal_of_own_phase", err, sb)
        assert err <= sb and np.abs(want).max() > 0.1
    _masked_phase_is_the_unmasked_one(env, "c2")
    env._shard.measure(env._stream())                               # the stand-alone kernel at this size, on the commands as they stand
    want = np.array([G.geo_signal(x, env.pupil, valid, ps, env.slopes_units) for x in env.phase_no_pupil.astype(np.float64)])
    err = np.abs(_signal(env) - want).max()
    _seen("c2-f32", "signal_of_own_phase", err, sb)
    assert err <= sb and np.abs(want).max() > 0.1
    assert np.isfinite(out[2]["obs"]).all() and (out[2]["strehl"] > 0).all()


# ---- refusals, and the diffractive shards ----------------------------------------------------------------------------------------------
def test_refusals():
    from rlao_amd import _lib as L
    from rlao_amd.env import BatchedAOEnv
    env = _env("r24", "f32", n_envs=2, tag="ideal")
    before = _episode(env, 9, 2)
    for call in (lambda: env.set_magnitude_per_env(7.0), lambda: env.change_mag(7.0), lambda: env.set_threshold_per_env(0.1)):
        with pytest.raises(L.AoEnvError, match="neither photons nor a threshold"):
            call()
    with pytest.raises(AttributeError, match="set_params"):
        env.wfs.is_geometric = False
    assert env.wfs.is_geometric and L.invoke(env._shard, "aoenv_fused_step_active") == 0 and not env.fused_step
    env.clear_star_per_env()                                        # (clearing what was never set stays a no-op)
    after = _episode(env, 9, 2)
    assert all(_same_bits(x["signal"], y["signal"]) for x, y in zip(before, after))
    pyr = BatchedAOEnv(n_envs=1, device=0, dtype="f32")
    try:
        with pytest.raises(ValueError, match="geometric"):
            pyr.set_params(dict(GEO["r24"], modulation=0.0), wfs_type="pyramid", is_geometric=True)
        with pytest.raises(ValueError, match="geometric"):
            pyr.set_params(dict(GEO["r24"], modulation=0.0, is_geometric=True), wfs_type="pyramid")
    finally:
        pyr.close()
    # the parameter-file key alone switches the mode on
    key = _new_env(dict(GEO["r24"], is_geometric=True), "f32", 1, geometric=None)
    try:
        assert key.is_geometric and key.slopes_units == env.slopes_units
    finally:
        key.close()


def test_diffractive_shards_are_untouched():
    """A diffractive C2-shape shard launches what it launched: one fused step kernel per step, or with AOENV_OPT_FUSED_STEP 0 the
    phase, spots and tail kernels; it keeps no unmasked phase."""
    from rlao_amd import _lib as L
    env = _new_env(GEO["c2"], "f32", 4, geometric=False)
    try:
        assert not env.is_geometric and not env.wfs.is_geometric and env.fused_step
        with pytest.raises(L.AoEnvError, match="geometric shards only"):
            env.phase_no_pupil
        env._shard.profile(True)
        _episode_plain(env, 4)
        n = {k: v[1] for k, v in env._shard.profile_read(env._stream()).items()}
        assert env._shard.step_counters() == (4, 4) and n["env_step"] == 4 and n["sh_tail"] == 0 and n["sh_spots"] == 1, n
        assert n["phase"] <= 2 and n["sh_centroid"] == 1                # the new screens and the prologue's measure
        env._shard.profile(False)
        L.check(env._shard.lib.aoenv_set_option(env._shard.h, L.OPT_FUSED_STEP, 0))
        env._shard.profile(True)
        _episode_plain(env, 4)
        n = {k: v[1] for k, v in env._shard.profile_read(env._stream()).items()}
        assert n["env_step"] == 0 and 5 <= n["phase"] <= 6 and n["sh_spots"] == 5 and n["sh_tail"] == 4 and n["sh_centroid"] == 1, n
        env._shard.profile(False)
        assert np.any(_frame(env))
    finally:
        env.close()


def _episode_plain(env, steps):
    env.generate_new_phase_screen(3)
    env.dm.coefs = 0
    env.measure()
    obs = env.reset_soft()
    for i in range(steps):
        obs = env.step(i, 0.5 * obs)[0]
