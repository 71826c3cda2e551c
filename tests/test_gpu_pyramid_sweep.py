"""GPU: Pyramid geometries off the two reference sizes -- every FFT radix of fft.hpp (16 / 4 / 2 with no odd factor, 3, 5 once and
twice, the two-sweep stage for the primes 17 / 19 / 23), lenslets of 2, 4, 8, 10, 12, 16 and 24 pixels (the nb binned rows per camera
row of k_pyr_rows_inv and its sub-batching), the row remainder of k_pyr_rows, the padded grid of k_pyr_cols, and the register-resident
float32 kernels of nRes 288 / 528 at geometries other than the reference ones.

Every comparison is against oracle.ao_oracle.OracleEnv (float64 NumPy, wfs_type="pyramid") built for the same geometry and handed
the env's own ring operators and mode-to-command matrix; it computes its own valid pixels, reference signal and interaction matrix.
One oracle run per case is recorded (three envs with seed stride 100, six closed-loop steps, action = 0.5 obs + 0.05 randn, masked,
float32, from the oracle's own observations; wind 0.45 pixel per frame at 72 deg: two pixel crossings, asserted) and the float64
shard, the float32 shard and every float32 switch replay its actions and are held to it: F64_SAME_OPERATOR_TOL_FULL / F32_TOL /
CAL_TOL of tests/test_gpu_parity.py.  The maxima measured on MI355X are in profiles/pyramid_sweep_parity_maxima.json
(AO_PARITY_REPORT=<file> with this module alone rewrites it).  No step, env or element is left out of a comparison; the reference
tree is never read here.

Valid-pixel cut: the Pyramid has no cut per measurement, only validI4Q = I4Q >= 0.1 I4Q.max() at calibration; a pixel ON the cut
would flip the valid set between the oracle and the device.  Every case asserts from the oracle alone that no pixel of I4Q is
closer to the cut than 1e-4 of the maximum (the smallest gap of the cases below is 1.5e-3) and that the env's valid set is the
oracle's.

Even sizes only: the reference's support[c - R//2 : c + R//2] cannot hold an odd R, and Pyramid.py:210 refuses a telescope whose
pixels per sub-aperture are odd; calib.PyramidTables refuses them the same way (test_odd_pixels_per_subaperture_are_refused).
nb = 5 binned rows per camera row therefore cannot be built through set_params; radix 5 twice runs at 21 x 2 (nRes 100) instead.

FAST_TRIG, FAST_WFS, FUSED_TAIL and FUSED_STEP are read by the Shack-Hartmann kernels only; the Pyramid step reads MFMA_GEMM,
FACTORED_RECON, COEFS_IMAGE and the PATH_* bits of FORCE_PATH (env.hip: run_phase, recon_product, run_wfs).

That the sweep bites was checked once with the kernels weakened in a scratch build, one change at a time (each variant reads or
writes less or differently, always in bounds), the float64 / float32 / forced-path replays run against each:
  nrow of k_pyr_rows one short                        -> every float64 case, every float32 case on the Stockham passes (all but
                                                         f288a) and the three PATH_GENERIC runs fail
  fft_stage_any: the qr >= R wrap off by one          -> r17, r17m, r19, r23 fail in float64 and float32
  fft_stage_any: the r > 0 twiddle sweep skipped      -> r17, r17m, r19, r23 fail in float64 and float32
  radix-5 stage: C / S swapped for q = 2              -> r5x5 and p10 fail in float64 and float32
  k_pyr_cols: per_xcd from N / CB, not the padded grid -> r5x5, r17, r17m, r19, r23, p8 (both dtypes), p10 (float32) and the three
                                                         PATH_GENERIC runs fail
  k_pyr_rows_inv: acc without the last row of a camera row -> the same runs as for nrow fail
  off one pixel off where ppx != 6                    -> every case but r17 and r19 (6 pixels) fails in both dtypes, all four forced runs
(The block remap of k_pyr_cols replaced by blockIdx.x alone computes the same frame -- the remap is a bijection of the padded grid
and the blk >= nblk bound stays -- so the grid variant above stands in for it.)  Unperturbed, every float32 maximum lies below
9 % of its tolerance, every float64 one below 10 % but the frame (2.3e-14 of the peak at nRes 228: 45 %).
"""
import copy

import numpy as np
import pytest

from test_gpu_geometry_sweep import PX_PER_FRAME, STEPS, N_ENVS, SEED_STRIDE, _replay, _same_controller
from test_gpu_parity import CAL_TOL, F32_TOL, F64_SAME_OPERATOR_TOL_FULL, _OBSERVED, _close

pytestmark = pytest.mark.gpu

MIN_CUT_GAP = 1e-4
SEED = 5

# case: sub-apertures across, pixels per sub-aperture, nRes and its radix list (make_fft_plan's rule, asserted), mask centring
# (True: on 4 pixels, the phasor; False: on one pixel, fftshift), modulation [lambda / D], the oracle's nSignal / nValidAct, modes
CASES = {
    "r5x5": dict(n_sub=21, ppx=2, n_res=100, plan=[4, 5, 5], centering=True, mod=0.0, n_signal=786, n_valid_act=392, n_modes=8),
    "r17": dict(n_sub=13, ppx=6, n_res=204, plan=[4, 3, 17], centering=True, mod=0.0, n_signal=298, n_valid_act=164, n_modes=8),
    "r17m": dict(n_sub=13, ppx=4, n_res=136, plan=[4, 2, 17], centering=False, mod=2.0, n_signal=298, n_valid_act=164, n_modes=8),
    "r19": dict(n_sub=15, ppx=6, n_res=228, plan=[4, 3, 19], centering=True, mod=0.0, n_signal=402, n_valid_act=208, n_modes=8),
    "r23": dict(n_sub=19, ppx=4, n_res=184, plan=[4, 2, 23], centering=True, mod=0.0, n_signal=626, n_valid_act=332, n_modes=8),
    "pow64": dict(n_sub=4, ppx=4, n_res=64, plan=[16, 4], centering=True, mod=0.0, n_signal=32, n_valid_act=21, n_modes=6),
    "pow128": dict(n_sub=12, ppx=4, n_res=128, plan=[16, 4, 2], centering=False, mod=0.0, n_signal=264, n_valid_act=137, n_modes=8),
    "p8": dict(n_sub=5, ppx=8, n_res=144, plan=[16, 3, 3], centering=True, mod=2.0, n_signal=50, n_valid_act=32, n_modes=8),
    "p10": dict(n_sub=4, ppx=10, n_res=160, plan=[16, 2, 5], centering=False, mod=0.0, n_signal=32, n_valid_act=21, n_modes=6),
    "f288a": dict(n_sub=5, ppx=16, n_res=288, plan=[16, 2, 3, 3], centering=False, mod=0.0, n_signal=50, n_valid_act=32, n_modes=8),
    "f288b": dict(n_sub=8, ppx=12, n_res=288, plan=[16, 2, 3, 3], centering=True, mod=2.0, n_signal=120, n_valid_act=69, n_modes=8),
    "f528a": dict(n_sub=7, ppx=24, n_res=528, plan=[16, 3, 11], centering=True, mod=0.0, n_signal=90, n_valid_act=52, n_modes=8),
}


def fft_plan(n):
    """The radix list of make_fft_plan (pyr_kernels.hip): 16s, 4s, 2s, 3s, 5s, then the remaining primes in rising order."""
    fac = []
    for r in (16, 4, 2, 3, 5):
        while n % r == 0:
            fac.append(r)
            n //= r
    p = 7
    while n > 1:
        while n % p == 0:
            fac.append(p)
            n //= p
        p += 2
    return fac


def _geo(name, **kw):
    c = CASES[name]
    ps = 0.4 / c["ppx"]                                          # pixel size [m]
    d = dict(diameter=0.4 * c["n_sub"], nSubaperture=c["n_sub"], nPixelPerSubap=c["ppx"], r0=0.13, L0=30.0,
             windSpeed=[PX_PER_FRAME * ps * 500.0], windDirection=[72.0], fractionalR0=[1.0], altitude=[0.0],
             nModes=c["n_modes"], nLoop=16, psfCentering=c["centering"], modulation=c["mod"])
    d.update(kw)
    return d


def _make_env(name, dtype, n_envs=N_ENVS, stride=SEED_STRIDE, opts=None):
    from rlao_amd import _lib as L
    from rlao_amd.env import BatchedAOEnv
    env = BatchedAOEnv(n_envs=n_envs, device=0, dtype=dtype, env_seed_stride=stride)
    try:
        env.set_params(_geo(name), camera="ideal", wfs_type="pyramid")
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
    """OracleEnv of the geometry with its OWN valid pixels, reference signal and interaction matrix, the ring operators handed over."""
    from oracle import ao_oracle as O
    R = geo["nSubaperture"] * geo["nPixelPerSubap"]
    geom = O.LayerGeometry(R, geo["diameter"], geo["L0"])
    return O.OracleEnv(resolution=R, diameter=geo["diameter"], n_subap=geo["nSubaperture"], r0=geo["r0"], L0=geo["L0"],
                       windSpeed=geo["windSpeed"], windDirection=geo["windDirection"], fractionalR0=geo["fractionalR0"],
                       altitude=geo["altitude"], m2c=m2c, n_modes=m2c.shape[1], nLoop=geo["nLoop"], wfs_type="pyramid",
                       modulation=geo["modulation"], psf_centering=geo["psfCentering"], geom_AB=(geom, A, B))


def valid_cut_gap(base, light_ratio=0.1):
    """Distance of the closest pixel of I4Q from the valid-pixel cut light_ratio * max, relative to the maximum."""
    i4q = base.wfs.I4Q
    return float(np.abs(i4q - light_ratio * i4q.max()).min() / i4q.max())


def run_oracle(base, m2c, modal_cm, seed, steps=STEPS):
    """Three envs (seeds seed + 100 k) of `base` with the controller (m2c, modal_cm): one closed-loop episode, as the
    Shack-Hartmann sweep records it (float32 actions from the oracle's own observations)."""
    w = base.wfs
    shared = [x for x in (base.dm_modes, base.imat, w.phasor, w.mask, w.m, w.tt_buffer, w.Tip, w.Tilt) if x is not None]
    orcs, rec = [], dict(seed=seed, obs0=[], screen0=[], actions=[], signal=[], obs=[], reward=[], strehl=[], frame=[])
    for k in range(N_ENVS):
        o = copy.deepcopy(base, memo={id(x): x for x in shared})
        o.M2C = np.asarray(m2c, dtype=np.float64)
        o.modal_cm = np.asarray(modal_cm, dtype=np.float64)
        o.reconstructor = o.M2C @ o.modal_cm
        o.new_episode(seed + SEED_STRIDE * k)
        rec["screen0"].append([lay.mapShift.copy() for lay in o.atm.layers])
        rec["obs0"].append(o.reset_soft())
        orcs.append(o)
    rs = np.random.RandomState(9)
    obs = np.stack(rec["obs0"])
    crossings = np.zeros((N_ENVS, len(orcs[0].atm.layers)), dtype=int)
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
    return rec


def _base(name, env):
    c = CASES[name]
    key = (c["n_sub"], c["ppx"], c["centering"], c["mod"])
    if key not in _BASES:
        at = env._atm_tables
        base = build_base(_geo(name), env.M2C_CL, at.A, at.B)
        _OBSERVED.setdefault(name + "-oracle", {})["valid_cut_gap"] = valid_cut_gap(base)
        _BASES[key] = base
    return _BASES[key]


def _record(name, env):
    base = _base(name, env)
    if name not in _RECORDS:
        _RECORDS[name] = run_oracle(base, env.M2C_CL, env.modal_CM, SEED)
    rec = _RECORDS[name]
    _same_controller(env, rec)
    # from the oracle alone: every pixel clear of the valid-pixel cut, the layer crossed a pixel at least twice
    assert valid_cut_gap(base) >= MIN_CUT_GAP
    assert (rec["crossings"] >= 2).all(), rec["crossings"]
    return rec


def _assert_geometry(name, env, base):
    c = CASES[name]
    w = base.wfs
    assert w.nSignal == c["n_signal"] and base.nValidAct == c["n_valid_act"]               # the oracle's counts: the table of cases
    assert env.nSignal == c["n_signal"] and env.nValidAct == c["n_valid_act"]
    assert env.R == c["n_sub"] * c["ppx"] == base.R and env.param.nModes == c["n_modes"]
    pt = env._pyr_tables
    assert pt.nRes == c["n_res"] == w.nRes == c["ppx"] * (2 * c["n_sub"] + 8) and fft_plan(pt.nRes) == c["plan"]
    assert env.cam_res == w.cam_res == 2 * c["n_sub"] + 8 and pt.psf_centering == c["centering"] == w.psfCentering
    assert env._wfs_n_theta == w.nTheta == (16 if c["mod"] else 1)
    assert valid_cut_gap(base) >= MIN_CUT_GAP
    assert np.array_equal(env.validI4Q, w.validI4Q)
    assert np.array_equal(env.dm_mask.astype(bool), base.dm_mask)


# ---- the sweep ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_calibration_matches_oracle(name):
    """The calibration -- measured in float64 on the GPU whatever the shard's dtype -- gives the oracle's valid pixels, reference
    signal, slope units (1) and zonal interaction matrix."""
    c = CASES[name]
    env = _make_env(name, "f64")
    try:
        base = _base(name, env)
        _assert_geometry(name, env, base)
        label = name + "-cal"
        ns, nv = c["n_sub"], c["n_signal"] // 2
        ref2d, valid = base.wfs.referenceSignal_2D, base.wfs.validI4Q
        _close(env.reference_centroids[:nv], ref2d[:ns][valid], "ref", CAL_TOL, label)
        _close(env.reference_centroids[nv:], ref2d[ns:][valid], "ref", CAL_TOL, label)
        assert env.slopes_units == base.wfs.slopesUnits == 1
        assert env.imat.shape == base.imat.shape == (c["n_signal"], c["n_valid_act"])
        _close(env.imat, base.imat, "imat_rel", CAL_TOL, label, scale=float(np.abs(base.imat).max()))
    finally:
        env.close()


@pytest.mark.parametrize("name", list(CASES))
def test_float64_shard_matches_oracle(name):
    """float64 shard (run-time-plan Stockham passes at every length) against the oracle that shares its operators."""
    env = _make_env(name, "f64")
    try:
        _assert_geometry(name, env, _base(name, env))
        _replay(env, _record(name, env), F64_SAME_OPERATOR_TOL_FULL, name + "-f64")
    finally:
        env.close()


@pytest.mark.parametrize("name", list(CASES))
def test_float32_shard_matches_oracle(name):
    """float32 shard, default switches (the production path of the geometry: the run-time plan off nRes 288 / 528, the
    register-resident kernels of pyr528_kernels.hip on them), against the same oracle run."""
    env = _make_env(name, "f32")
    try:
        assert not env.fused_step
        _assert_geometry(name, env, _base(name, env))
        _replay(env, _record(name, env), F32_TOL, name + "-f32")
    finally:
        env.close()


def _tag(opts):
    return "+".join(f"{k[4:]}={v}" for k, v in opts.items())


# PATH_GENERIC = 512: the float32 Stockham passes with the compile-time plans (288: all three passes, 528: the inverse row pass);
# PATH_PYR_ROUND_ROBIN = 1024: the register-resident column pass with its blocks dealt round-robin over the XCDs
FORCED_RUNS = [("f288a", 512), ("f288b", 512), ("f528a", 512), ("f288a", 1024)]


@pytest.mark.parametrize("name,path", FORCED_RUNS, ids=[f"{n}-{p}" for n, p in FORCED_RUNS])
def test_float32_forced_path_matches_oracle(name, path):
    """nRes 288 / 528 off the reference geometries through the other float32 kernels: held to the oracle, not to their sibling."""
    from rlao_amd import _lib as L
    assert (L.PATH_GENERIC, L.PATH_PYR_ROUND_ROBIN) == (512, 1024)
    env = _make_env(name, "f32", opts={"OPT_FORCE_PATH": path})
    try:
        _replay(env, _record(name, env), F32_TOL, f"{name}-f32-FORCE_PATH={path}")
    finally:
        env.close()


# PATH_PHASE_DWORD = 256 / PATH_GENERIC = 512: the other float32 phase kernels in front of the Pyramid
SWITCHES = [{"OPT_MFMA_GEMM": 0}, {"OPT_FACTORED_RECON": 0}, {"OPT_COEFS_IMAGE": 1}, {"OPT_FORCE_PATH": 256}, {"OPT_FORCE_PATH": 512}]
SWITCH_RUNS = [(n, o) for n in ("r17", "p10") for o in SWITCHES]


@pytest.mark.parametrize("name,opts", SWITCH_RUNS, ids=[n + "-" + _tag(o) for n, o in SWITCH_RUNS])
def test_float32_switches_match_oracle(name, opts):
    """Every option the Pyramid step reads (VALU contractions, dense reconstructor, command images, the dword and the tiled phase
    kernel), one at a time: each run held to the oracle, not to the default run."""
    env = _make_env(name, "f32", opts=opts)
    try:
        _replay(env, _record(name, env), F32_TOL, f"{name}-f32-{_tag(opts)}")
    finally:
        env.close()


def test_batch_invariance_70_envs():
    """r17m in float32, 70 envs (no multiple of anything in the launch grids), every env the seed of env 0: after 3 steps every
    env equals env 0 bit for bit, and env 0 is held to the oracle run that env 0 of the 3-env shard is held to."""
    n_envs, steps = 70, 3
    env = _make_env("r17m", "f32", n_envs=n_envs, stride=0)
    try:
        rec = _record("r17m", env)
        out = _replay(env, rec, F32_TOL, "r17m-f32-70envs", steps=steps, envs=[0] * n_envs, compare=[0])
        assert len(out) == steps + 1 and out[0].shape[0] == n_envs
        assert (out[0] == out[0][:1]).all()
        for arrays in out[1:]:
            for a in arrays:
                assert a.shape[0] == n_envs and np.array_equal(a, np.broadcast_to(a[:1], a.shape))
    finally:
        env.close()


def test_odd_pixels_per_subaperture_are_refused():
    """6 x 5 pixels (nRes 100, nb = 5): the reference's Pyramid refuses an odd number of pixels per sub-aperture (Pyramid.py:210)
    and so does set_params, before anything is launched."""
    from rlao_amd.env import BatchedAOEnv
    env = BatchedAOEnv(n_envs=1, device=0, dtype="f32")
    try:
        geo = dict(_geo("p10"), diameter=2.4, nSubaperture=6, nPixelPerSubap=5)
        with pytest.raises(ValueError, match="even number"):
            env.set_params(geo, camera="ideal", wfs_type="pyramid")
    finally:
        env.close()
