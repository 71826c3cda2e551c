"""GPU: every kernel path of the WFS camera (k_detector<float / double> in both quad layouts, k_detector_sh6 with one and with
several chunks, the camera blocks of the fused step kernel) against tests/_camera_ref.py, count for count.

The camera's random numbers are Philox4x32-7 words of (quad id, global env index, frame number, purpose) under the detector seed: a
noisy frame is a pure function of the ideal frame and a handful of integers, and the restatement reproduces it.  Recipe of every
case: the env is built with the ideal camera and measured -- B_FRAME is then the photon input the camera kernel will read (a float64
shard: cast to float32, as the kernel casts it); the camera is configured; two more measurements give two noisy frames of the SAME
input at consecutive frame numbers (word 0 of B_COUNTERS, read after each: the counter is advanced before the launch).

Pass condition (_camera_ref.assert_flips): the device differs from the float32 restatement on at most 2e-3 of the pixels -- the cap
tests/test_gpu_detector.py grants the camera -- and by at most one count (one ADC step with the ADC on) on a pixel that did not go
through PTRS.  A PTRS pixel (at and above the env's hand-over, _camera_ref.env_lmax: 832 photons for 8 x 8 lenslets of 6 pixels, 992
for 20 x 20, 1024 elsewhere; every pixel under a dark current of 10 e or more) may flip an accept / reject
decision, which moves its count by more than one: those are held to the share and, pooled over the case, to the Poisson law (PIT).
Before the device's counts are looked at every case asserts, from the ideal frame alone, that its pixels fall into the brightness
classes it is about, and that the float32 and the float64 restatement differ on at most 1e-3 of the pixels (so the reference alone
stays inside the cap).  The shares measured on MI355X are in profiles/camera_stream_parity.json (AO_PARITY_REPORT=<file> with this
module alone rewrites it).

Why each case reaches its kernel (launch_detector, detector_kernels.hip): sh6 = valid2d && cam == 6 n_subap.
  sh6-f32           float32 && sh6 -> k_detector_sh6; n_runs = cdiv(3 * 64, 512) = 1, chunks = max(1, 1 * 4 / 2048) = 1
  sh6-chunks2       20 x 20 lenslets, 1400 envs: n_runs = cdiv(1200, 512) = 3, chunks = 3 * 1400 / 2048 = 2, grid.x = cdiv(3, 2) = 2:
                    workgroup 1 runs c = 0 (tasks 1024 .. 1199: a ragged run) and leaves at c = 1 (task0 = 1536 >= 1200); both
                    workgroups pass the barrier at c == 0 only and read the table copied once
  sh6-f64           sizeof(T) == 8 -> k_detector<double> with sh6 = 1
  sh4-*, sh8-*      valid2d, cam = 4 n_subap / 8 n_subap: sh6 = 0, (cam / n_subap) % 4 == 0 -> k_detector<T>, generic quads, `lit`
  pyr7-*, pyr5-*    valid2d == nullptr, cam = 2 n + 8 = 22 / 18: generic quads with a 2-pixel tail quad per row
  pyr8-f32          cam = 24: no tail
  fused             env.fused_step asserted; step() on a noisy env and on an ideal twin driven by the same actions: the twin's frames
                    are the photon input; lit lenslets go through camera_sh6_lane, the others through detector_quad<false>

That the comparison bites was checked once with three scratch builds, arithmetic only (the counts measured then are in the pull
request that added this module): the purposes of the fine and the remainder draw swapped; the EMCCD gain applied after the
read-out noise; the sin branch for slot 0."""
import json
import os

import numpy as np
import pytest

import _camera_ref as R
from test_gpu_parity import F32_TOL, F64_SAME_OPERATOR_TOL_FULL

pytestmark = pytest.mark.gpu

MEASURED = {}
SEED = 7
FAINT, BRIGHT = 8.0, 6.0                   # Shack-Hartmann: brightest pixel ~860 photons at magnitude 8, ~5400 at 6
PYR_FAINT, PYR_BRIGHT = 9.0, 6.0           # Pyramid (2 pixels per sub-aperture): ~900 at magnitude 9, ~14000 at 6
DEFAULTS = dict(photonNoise=False, readoutNoise=0, QE=1, darkCurrent=0, integrationTime=None, FWC=None, bits=None, gain=1, sensor="CCD")

# path: wfs, sub-apertures, pixels per sub-aperture, dtype, envs, env_index_offset, the envs restated
PATHS = {
    "sh6-f32": dict(wfs="shackhartmann", n_sub=8, ppx=6, dtype="f32", n_envs=4, offset=100),
    "sh6-chunks2": dict(wfs="shackhartmann", n_sub=20, ppx=6, dtype="f32", n_envs=1400, offset=0, restate=[0, 1, 699, 1398, 1399]),
    "sh6-f64": dict(wfs="shackhartmann", n_sub=8, ppx=6, dtype="f64", n_envs=3, offset=0),
    "sh4-f32": dict(wfs="shackhartmann", n_sub=8, ppx=4, dtype="f32", n_envs=3, offset=100),
    "sh4-f64": dict(wfs="shackhartmann", n_sub=8, ppx=4, dtype="f64", n_envs=3, offset=0),
    "sh8-f32": dict(wfs="shackhartmann", n_sub=8, ppx=8, dtype="f32", n_envs=3, offset=0),
    "sh8-f64": dict(wfs="shackhartmann", n_sub=8, ppx=8, dtype="f64", n_envs=3, offset=100),
    "pyr7-f32": dict(wfs="pyramid", n_sub=7, ppx=2, dtype="f32", n_envs=4, offset=100),
    "pyr7-f64": dict(wfs="pyramid", n_sub=7, ppx=2, dtype="f64", n_envs=3, offset=0),
    "pyr5-f32": dict(wfs="pyramid", n_sub=5, ppx=2, dtype="f32", n_envs=3, offset=0),
    "pyr5-f64": dict(wfs="pyramid", n_sub=5, ppx=2, dtype="f64", n_envs=3, offset=100),
    "pyr8-f32": dict(wfs="pyramid", n_sub=8, ppx=2, dtype="f32", n_envs=3, offset=0),
    "fused": dict(wfs="shackhartmann", n_sub=8, ppx=6, dtype="f32", n_envs=4, offset=100),
}
ALL_SETTINGS = list(R.SETTINGS) + ["everything", "photon-bright", "everything-bright"]
FULL = ("sh6-f32", "fused", "pyr7-f32")
RUNS = [(p, s) for p in PATHS for s in (ALL_SETTINGS if p in FULL else ["photon", "everything"])] + [("sh4-f64", "photon-bright"),
                                                                                                      ("pyr5-f32", "photon-bright")]


def _fields(setting):
    name = setting[:-len("-bright")] if setting.endswith("-bright") else setting
    return R.EVERYTHING if name == "everything" else R.SETTINGS[name]


def _geo(p, bright):
    pyr = p["wfs"] == "pyramid"
    mag = (PYR_BRIGHT if bright else PYR_FAINT) if pyr else (BRIGHT if bright else FAINT)
    return dict(diameter=0.4 * p["n_sub"], nSubaperture=p["n_sub"], nPixelPerSubap=p["ppx"], r0=0.13, L0=30.0, windSpeed=[10.0],
                windDirection=[72.0], fractionalR0=[1.0], altitude=[0.0], nModes=20 if p["n_sub"] == 20 else 8, nLoop=16, magnitude=mag)


def _make(path, bright, n_envs=None, ppx=None):
    from rlao_amd.env import BatchedAOEnv
    p = dict(PATHS[path], **({"ppx": ppx} if ppx else {}))
    env = BatchedAOEnv(n_envs=n_envs or p["n_envs"], device=0, dtype=p["dtype"], env_index_offset=p["offset"])
    try:
        env.set_params(_geo(p, bright), camera="ideal", wfs_type=p["wfs"])
        env.generate_new_phase_screen(SEED)
        env.dm.coefs = 0
        env.dm_prev = 0
    except Exception:
        env.close()
        raise
    return env


@pytest.fixture(scope="module")
def shards():
    made = {}

    def get(path, bright, twin=False):
        key = (path, bright, twin)
        if key not in made:
            made[key] = _make(path, bright)
        return made[key]

    yield get
    for e in made.values():
        e.close()
    out = os.environ.get("AO_PARITY_REPORT")
    if out and MEASURED:
        with open(out, "w") as f:
            f.write(json.dumps(MEASURED, indent=1, sort_keys=True) + "\n")


@pytest.fixture(scope="module")
def table():
    import ctypes as C
    from rlao_amd import _lib as L
    lib = L.load()
    n = C.c_size_t()
    L.check(lib.aoenv_test_poisson_table(None, 0, C.byref(n)))
    t = np.zeros(n.value, dtype=np.uint32)
    L.check(lib.aoenv_test_poisson_table(t.ctypes.data_as(C.c_void_p), t.size, C.byref(n)))
    return t


def _frame(env):
    from rlao_amd import _lib as L
    return env._shard.download(L.B_FRAME, (env.n_envs, env.cam_res, env.cam_res))


def _frame_number(env):
    from rlao_amd import _lib as L
    return int(env._shard.download(L.B_COUNTERS, (4,), env._stream(), dtype=np.uint32)[0])


def _cfg(env, fields):
    return R.CameraCfg.from_fields(env.param.samplingTime, seed=env.detector_seed, **fields)


def _layout(env, path):
    sh = PATHS[path]["wfs"] == "shackhartmann"
    return R.layout_for(env.cam_res, PATHS[path]["n_sub"], sh)


def _assert_classes(ideal, setting, label):
    """From the ideal frame alone: pixels in every brightness class the case is about (8 of each at the least)."""
    n = dict(below_quarter=int((ideal < 0.25).sum()), quarter_to_32=int(((ideal >= 0.25) & (ideal < 32)).sum()),
             to_1024=int(((ideal >= 32) & (ideal < 1024)).sum()), ptrs=int((ideal >= 1024).sum()))
    assert min(n["below_quarter"], n["quarter_to_32"], n["to_1024"]) >= 8, (label, n)
    if setting.endswith("-bright"):
        assert n["ptrs"] >= 8, (label, n)
    return n


def _lmax(env, path, table):
    p = PATHS[path]
    return R.env_lmax(table, p["wfs"] == "shackhartmann", env.cam_res // p["n_sub"], env.R, env.nActuator)


def _compare(label, ideal32, noisy, cfg, layout, env_ids, frame_number, table, setting, valid2d=None, lmax=None):
    """One noisy frame [E, cam, cam] of the envs with the global indices env_ids against its restatement."""
    ideal32 = np.ascontiguousarray(ideal32, dtype=np.float32)
    want, ptrs = R.noisy_frame(ideal32, cfg, layout, env_ids, frame_number, table, valid2d=valid2d, lmax=lmax)
    want64, ptrs64 = R.noisy_frame(ideal32, cfg, layout, env_ids, frame_number, table, valid2d=valid2d, exact=True, lmax=lmax)
    assert np.array_equal(ptrs, ptrs64)
    ref_share, _ = R.assert_flips(want, want64, ptrs, cfg, R.REFERENCE_FLIP_CAP, label + " float32 vs float64 restatement")
    got = np.asarray(noisy, dtype=np.float64)
    assert np.isfinite(got).all()
    share, worst = R.flip_figures(got, want, ptrs, cfg)
    rec = MEASURED.setdefault(label.rsplit(" frame", 1)[0], {})
    rec["flip_share"] = max(rec.get("flip_share", 0.0), share)
    rec["largest_alias_pixel_difference_steps"] = max(rec.get("largest_alias_pixel_difference_steps", 0.0), worst)
    rec["reference_flip_share"] = max(rec.get("reference_flip_share", 0.0), ref_share)
    rec["ptrs_share"] = float(ptrs.mean())
    R.assert_flips(got, want, ptrs, cfg, R.DEVICE_FLIP_CAP, label)
    return got, want, ptrs


def _assert_ptrs_law(label, setting, cfg, triples):
    """PTRS pixels, pooled over the (ideal, counts, PTRS mask) triples of a case, follow the Poisson law (randomised PIT; photon
    noise alone: the counts are the draws.  Dark current of 10 e or more: the pixels without light hold the dark draw alone).
    640 samples and more: chi-square over 64 bins and Kolmogorov-Smirnov; fewer: Kolmogorov-Smirnov alone."""
    from scipy import stats
    if setting not in ("photon-bright", "dark40"):
        return
    rs = np.random.RandomState(12)
    x, lam = [], []
    for ideal32, got, ptrs in triples:
        sel = ptrs if setting == "photon-bright" else (ideal32 == 0)
        x.append(got[sel])
        lam.append(ideal32[sel].astype(np.float64) if setting == "photon-bright" else np.full(int(sel.sum()), float(cfg.dark_e)))
    x, lam = np.concatenate(x), np.concatenate(lam)
    MEASURED.setdefault(label, {})["ptrs_pixels_in_law_test"] = int(lam.size)
    if lam.size < 100:
        assert setting == "dark40", (label, lam.size)             # the Pyramid has no pixel without light
        return
    u = R.pit(x, lam, rs)
    if lam.size >= 640:
        R.assert_uniform(u, label + " PTRS pixels")
    else:
        assert float(stats.kstest(u, "uniform").statistic) * np.sqrt(u.size) < 2.2, label


# ---- the stand-alone kernels ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path,setting", [r for r in RUNS if r[0] != "fused"], ids=[f"{p}-{s}" for p, s in RUNS if p != "fused"])
def test_measured_frame_equals_its_restatement(shards, table, path, setting):
    p = PATHS[path]
    env = shards(path, setting.endswith("-bright"))
    label = f"{path} {setting}"
    sh = p["wfs"] == "shackhartmann"
    assert not env.wfs.cam.photonNoise and env.cam_res == (p["n_sub"] * p["ppx"] if sh else 2 * p["n_sub"] + 8)
    if path == "sh6-chunks2":                                      # launch_detector's arithmetic, restated
        n_runs = -(-3 * p["n_sub"] ** 2 // 512)
        assert n_runs == 3 and (n_runs * env.n_envs) // 2048 == 2 and 3 * p["n_sub"] ** 2 % 512 != 0
    if not sh:
        assert env.cam_res % 4 == (0 if p["n_sub"] == 8 else 2)
    ids = np.asarray(p.get("restate", range(env.n_envs)))
    env.measure()
    ideal = _frame(env)[ids]
    assert ideal.dtype == (np.float32 if p["dtype"] == "f32" else np.float64)
    ideal32 = ideal.astype(np.float32)
    _assert_classes(ideal32, setting, label)
    valid2d = env._sh_tables.valid_2d if sh else None
    if sh:                                                         # no light outside the valid lenslets
        assert (ideal32[:, ~np.asarray(valid2d, dtype=bool).repeat(p["ppx"], 0).repeat(p["ppx"], 1)] == 0).all()
    fields = _fields(setting)
    cfg, layout = _cfg(env, fields), _layout(env, path)
    try:
        env.wfs.cam.configure(**fields)
        frames, numbers, triples = [], [], []
        for k in range(2):
            env.measure()
            noisy = _frame(env)[ids]
            numbers.append(_frame_number(env))
            got, want, ptrs = _compare(f"{label} frame {k}", ideal32, noisy, cfg, layout, ids + p["offset"], numbers[-1], table, setting,
                                       lmax=_lmax(env, path, table))
            frames.append(got)
            triples.append((ideal32, got, ptrs))
        assert numbers[1] == numbers[0] + 1
        assert (frames[0] != frames[1]).mean() > 0.05              # a new frame number is a new draw
        _assert_ptrs_law(label, setting, cfg, triples)
        if "readout" in setting:                                   # negative counts survive the ADC (trunc toward zero, clipped from above only)
            assert min(f.min() for f in frames) < 0
    finally:
        env.wfs.cam.configure(**DEFAULTS)


def test_emccd_and_ccd_frames_differ(shards, table):
    """The same numbers (gain 3.7, read-out 14) as EMCCD and as CCD at ONE frame number: each equals its restatement (the two runs of
    test_measured_frame_equals_its_restatement), and the two restatements -- hence the two cameras -- differ on most pixels."""
    env = shards("sh6-f32", False)
    env.measure()
    ideal32 = _frame(env).astype(np.float32)
    lay = _layout(env, "sh6-f32")
    lmax = _lmax(env, "sh6-f32", table)
    a, _ = R.noisy_frame(ideal32, _cfg(env, R.SETTINGS["emccd"]), lay, 100 + np.arange(env.n_envs), 5, table, lmax=lmax)
    b, _ = R.noisy_frame(ideal32, _cfg(env, R.SETTINGS["ccd"]), lay, 100 + np.arange(env.n_envs), 5, table, lmax=lmax)
    assert (a != b).mean() > 0.5
    got = {}
    for name in ("emccd", "ccd"):
        try:
            env.wfs.cam.configure(**R.SETTINGS[name])
            env.measure()
            n = _frame_number(env)
            got[name] = (_frame(env).astype(np.float64), n)
        finally:
            env.wfs.cam.configure(**DEFAULTS)
    assert (got["emccd"][0] != got["ccd"][0]).mean() > 0.5
    for name in got:
        want, ptrs = R.noisy_frame(ideal32, _cfg(env, R.SETTINGS[name]), lay, 100 + np.arange(env.n_envs), got[name][1], table, lmax=lmax)
        R.assert_flips(got[name][0], want, ptrs, _cfg(env, R.SETTINGS[name]), R.DEVICE_FLIP_CAP, name)


# ---- the fused step kernel -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("setting", ALL_SETTINGS)
def test_fused_step_frames_equal_their_restatement(shards, table, setting):
    """step(i, a_i) with prescribed actions on a noisy env and on an ideal twin (same seeds, same actions: the same atmosphere and
    mirror): the twin's frame of step i is the photon input of the noisy env's.  Lit lenslets: camera_sh6_lane; the others:
    detector_quad<false>, dark and read-out noise only (valid2d handed to the restatement)."""
    import torch
    bright = setting.endswith("-bright")
    env, twin = shards("fused", bright), shards("fused", bright, twin=True)
    assert env is not twin and env.fused_step and twin.fused_step
    label = f"fused {setting}"
    p = PATHS["fused"]
    fields = _fields(setting)
    cfg, layout = _cfg(env, fields), _layout(env, "fused")
    valid2d = env._sh_tables.valid_2d
    lit = np.asarray(valid2d, dtype=bool).repeat(6, 0).repeat(6, 1)
    rs = np.random.RandomState(21)
    actions = [torch.as_tensor((0.05 * rs.randn(env.n_envs, env.nActuator, env.nActuator) * env.dm_mask[None]).astype(np.float32)) for _ in range(2)]
    try:
        env.wfs.cam.configure(**fields)
        for e in (env, twin):
            e.generate_new_phase_screen(SEED)
            e.dm.coefs = 0
            e.dm_prev = 0
            e.measure()
            e.reset_soft()
        ideals, triples = [], []
        for i, a in enumerate(actions):
            _, ideal, _, _, _, _ = twin.step(i, a)
            _, noisy, _, _, _, _ = env.step(i, a)
            number = _frame_number(env)
            ideal32 = ideal.cpu().numpy()
            assert ideal32.dtype == np.float32 and (ideal32[:, ~lit] == 0).all()
            _assert_classes(ideal32, setting, label)
            got, want, ptrs = _compare(f"{label} frame {i}", ideal32, noisy.cpu().numpy(), cfg, layout, p["offset"] + np.arange(env.n_envs),
                                       number, table, setting, valid2d=valid2d, lmax=_lmax(env, "fused", table))
            ideals.append(ideal32)
            triples.append((ideal32, got, ptrs))
            if cfg.dark_e > 0 or cfg.readout_noise != 0:           # the lenslets without light are read out too
                assert got[:, ~lit].std() > 0
                assert np.abs(got - want)[:, ~lit].max() <= cfg.step * (1 + 1e-5) or ptrs.all()
            else:
                assert (got[:, ~lit] == 0).all()
        assert not np.array_equal(ideals[0], ideals[1])            # the atmosphere moved: another input, another frame number
        _assert_ptrs_law(label, setting, cfg, triples)
    finally:
        env.wfs.cam.configure(**DEFAULTS)


# ---- slopes from a noisy frame: wfs_max after the noise, `lit` ------------------------------------------------------------------------
def _oracle_sh_signal(env, noisy):
    """oracle.ao_oracle.OracleSH.measure (split_camera_frame, threshold at threshold_cog * max over the valid lenslets, centre of
    gravity, reference, units) on a given camera frame."""
    from oracle import ao_oracle as O

    class _Given:
        def integrate(self, frame):
            return np.asarray(noisy, dtype=np.float64)

    t = env._sh_tables
    w = object.__new__(O.OracleSH)
    ns, nv = t.valid_2d.shape[0], int(t.valid_2d.sum())
    w.nSubap, w.p, w.cam_res, w.thr = ns, env.cam_res // ns, env.cam_res, float(env.param.threshold_cog)
    w.valid_2d = np.asarray(t.valid_2d, dtype=bool)
    w.valid_1d = w.valid_2d.ravel()
    w.valid_slopes_maps = np.concatenate((w.valid_2d, w.valid_2d))
    w.vx, w.vy = np.where(w.valid_2d)
    w.SX, w.SY = np.zeros((ns, ns)), np.zeros((ns, ns))
    w.reference_slopes_maps = np.zeros((2 * ns, ns))
    w.reference_slopes_maps[:ns][w.valid_2d] = env.reference_centroids[:nv]
    w.reference_slopes_maps[ns:][w.valid_2d] = env.reference_centroids[nv:]
    w.slopes_units = float(env.slopes_units)
    w.cam = _Given()
    w.spots = lambda phase: np.zeros((ns * ns, w.p, w.p))
    sig = np.array(w.measure(None), dtype=np.float64)
    return sig, w.last_max


def _oracle_pyramid_signal(env, noisy, ns):
    """oracle.ao_oracle.OraclePyramid.signal_processing (quadrants, valid pixels, normalisation by the frame's mean, reference) on
    a given camera frame."""
    from oracle import ao_oracle as O
    w = object.__new__(O.OraclePyramid)
    w.nSubap, w.R, w.cam_res, w.n_pix_separation = ns, env.R, env.cam_res, 4
    w.postProcessing, w.slopesUnits = "slopesMaps_incidence_flux", 1
    w.validI4Q = np.asarray(env.validI4Q, dtype=bool)
    w.validSignal = np.concatenate((w.validI4Q, w.validI4Q))
    nv = int(w.validI4Q.sum())
    w.referenceSignal_2D = np.zeros((2 * ns, ns))
    w.referenceSignal_2D[:ns][w.validI4Q] = env.reference_centroids[:nv]
    w.referenceSignal_2D[ns:][w.validI4Q] = env.reference_centroids[nv:]
    w.frame = np.asarray(noisy, dtype=np.float64)
    return np.array(w.signal_processing()[1], dtype=np.float64)


# the Razor camera with a full well of 1000 e: the brightest pixel is some 500 ADC steps, the centroid cut some 5 -- above most of the
# read-out noise (14 e = 14 steps), so the cut removes pixels that hold counts
SLOPES_CAMERA = dict(R.RAZOR, FWC=1000)


@pytest.mark.parametrize("path", ["sh6-f32", "sh4-f32", "sh4-f64", "pyr7-f32"])
def test_slopes_of_a_noisy_frame_match_the_oracle(shards, path):
    """The oracle's centroiding / Pyramid slopes run on the DEVICE's noisy frame (SLOPES_CAMERA: photon, dark and read-out noise,
    10-bit ADC, negative counts) against the device's B_SIGNAL, at the tolerance the geometry sweeps hold the signal to.  The
    Shack-Hartmann cut is threshold_cog * max over the VALID lenslets' pixels after the noise: wfs_max of the camera kernels and
    the `lit` lookup of the generic layout."""
    from rlao_amd import _lib as L
    p = PATHS[path]
    env = shards(path, False)
    tol = F32_TOL if p["dtype"] == "f32" else F64_SAME_OPERATOR_TOL_FULL
    sh = p["wfs"] == "shackhartmann"
    try:
        env.wfs.cam.configure(**SLOPES_CAMERA)
        env.measure()
        noisy = _frame(env).astype(np.float64)
        sig = env._shard.download(L.B_SIGNAL, (env.n_envs, env.nSignal)).astype(np.float64)
        assert noisy.min() < 0
        for e in range(env.n_envs):
            if sh:
                assert float(env.param.threshold_cog) > 0
                want, mx = _oracle_sh_signal(env, noisy[e])
                cut = float(env.param.threshold_cog) * mx
                # counts are whole numbers: a pixel is on the cut or a hundredth of a count away from it; on it (max a multiple of
                # 100) float32 0.01f * max and float64 0.01 * max are the same number for every max up to 1000, and < keeps the pixel
                assert cut > 2 and ((noisy[e] > 0) & (noisy[e] < cut)).sum() >= 8                # the cut removes pixels that hold counts
            else:
                want = _oracle_pyramid_signal(env, noisy[e], p["n_sub"])
            err = float(np.abs(sig[e] - want).max())
            rec = MEASURED.setdefault(f"{path} razor slopes", {})
            rec["signal"] = max(rec.get("signal", 0.0), err)
            np.testing.assert_allclose(sig[e], want, rtol=0, atol=tol["signal"], err_msg=f"{path} env {e}")
    finally:
        env.wfs.cam.configure(**DEFAULTS)


# ---- the refusal -----------------------------------------------------------------------------------------------------------------
def test_five_pixel_lenslets_refuse_a_noisy_camera_and_recover():
    """8 x 8 lenslets of 5 pixels: neither the sh6 nor the generic layout fits (a quad would straddle two lenslets).  measure()
    raises; the refused frame is no frame of the noise streams (the counter stays); back on the default camera the shard measures
    what a twin that never had the camera measures."""
    from rlao_amd import _lib as L
    env, twin = _make("sh4-f32", False, ppx=5), _make("sh4-f32", False, ppx=5)
    try:
        assert env.cam_res == 40
        with pytest.raises(ValueError, match="6 or a multiple of 4"):
            R.layout_for(env.cam_res, 8, True)
        for e in (env, twin):
            e.measure()
        n0 = _frame_number(env)
        env.wfs.cam.configure(photonNoise=True)
        with pytest.raises(L.AoEnvError, match="camera noise on a Shack-Hartmann frame needs 6 or a multiple of 4 pixels per lenslet"):
            env.measure()
        assert _frame_number(env) == n0
        env.wfs.cam.configure(**DEFAULTS)
        for e in (env, twin):
            e.measure()
        np.testing.assert_array_equal(_frame(env), _frame(twin))
        np.testing.assert_array_equal(env._shard.download(L.B_SIGNAL, (env.n_envs, env.nSignal)),
                                      twin._shard.download(L.B_SIGNAL, (twin.n_envs, twin.nSignal)))
        assert np.abs(_frame(env)).max() > 0
        # ... and a closed-loop step of the two still agrees
        o1, o2 = env.reset_soft(), twin.reset_soft()
        a, b = env.step(0, 0.4 * o1), twin.step(0, 0.4 * o2)
        for x, y in zip(a[:4], b[:4]):
            assert np.array_equal(x.cpu().numpy(), y.cpu().numpy())
    finally:
        env.close()
        twin.close()


# ---- checkpoint ------------------------------------------------------------------------------------------------------------------
def test_checkpoint_resumes_the_generic_layout_streams(shards, table):
    """Razor camera on 4-pixel lenslets (k_detector, generic quads): get_state() after step k, one more step; set_state() and the
    same step again gives the same counts -- the frame number is part of the state -- and they equal the restatement of an ideal
    twin's frame."""
    import torch
    env = shards("sh4-f32", False)
    assert not env.fused_step
    try:
        env.wfs.cam.configure(**R.RAZOR)
        env.generate_new_phase_screen(SEED)
        env.dm.coefs = 0
        env.dm_prev = 0
        env.measure()
        obs = env.reset_soft()
        for i in range(2):
            obs = env.step(i, 0.4 * obs)[0]
        snap = env.get_state()
        n_snap = _frame_number(env)
        act = (0.4 * obs).clone()
        out_a = [t.cpu().numpy().copy() for t in env.step(2, act)[:4]]
        assert _frame_number(env) == n_snap + 1
        extra = env.step(3, act)[1].cpu().numpy()                  # the streams move on ...
        assert _frame_number(env) == n_snap + 2 and not np.array_equal(extra, out_a[1])
        env.set_state(snap)                                        # ... and come back
        assert _frame_number(env) == n_snap
        out_b = [t.cpu().numpy().copy() for t in env.step(2, act)[:4]]
        for x, y in zip(out_a, out_b):
            np.testing.assert_array_equal(x, y)
        assert (out_a[1] != np.floor(out_a[1])).sum() == 0 and out_a[1].max() <= 1023
        torch.cuda.synchronize()
    finally:
        env.wfs.cam.configure(**DEFAULTS)
        env.generate_new_phase_screen(SEED)
        env.dm.coefs = 0
        env.dm_prev = 0
