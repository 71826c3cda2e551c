"""CPU: the NumPy restatement of the WFS camera (tests/_camera_ref.py) that tests/test_gpu_camera_streams.py holds the device to count
for count.  Here the restatement itself is held to what it restates: the quad layouts are bijections onto the frame and agree with
sh6_quad_pixels written as the loop it is; every sampler follows its law (the bounds of tests/test_poisson_alias.py and of
_explore_ref.assert_law); the deterministic part equals oracle.ao_oracle.Detector exactly and the noisy moments equal the oracle's
within sampling error (EMCCD and CMOS: the order of gain and read-out noise); and float32 against float64 arithmetic moves at most
REFERENCE_FLIP_CAP of the pixels, by one count, on frames with the brightness classes and camera settings of the GPU tests."""
import ctypes as C
import itertools

import numpy as np
import pytest

import _camera_ref as R
import _explore_ref as X


@pytest.fixture(scope="module")
def table():
    import __graft_entry__ as g
    g.build()
    from rlao_amd import _lib as L
    lib = L.load()
    n = C.c_size_t()
    L.check(lib.aoenv_test_poisson_table(None, 0, C.byref(n)))
    t = np.zeros(n.value, dtype=np.uint32)
    L.check(lib.aoenv_test_poisson_table(t.ctypes.data_as(C.c_void_p), t.size, C.byref(n)))
    return t


# ---- layouts -------------------------------------------------------------------------------------------------------------------
def _assert_bijection(layout, cam):
    quad, slot = layout
    assert quad.shape == slot.shape == (cam * cam,) and slot.min() == 0 and slot.max() == 3
    key = quad.astype(np.int64) * 4 + slot
    assert np.unique(key).size == cam * cam                     # no two pixels share a (quad, slot)
    first = np.nonzero(slot == 0)[0]
    assert np.array_equal(quad[first].astype(np.int64), first)  # a quad is named by its slot-0 pixel ...
    assert np.isin(quad.astype(np.int64), first).all()          # ... and every pixel's quad has one


@pytest.mark.parametrize("cam", [18, 22, 24, 32, 48])
def test_generic_layout_is_a_bijection(cam):
    lay = R.generic_layout(cam)
    _assert_bijection(lay, cam)
    quad, slot = lay
    # k_detector: quad q of row r starts at column 4 (q mod qpr); the last one of a row holds cam % 4 pixels (or 4)
    qpr = (cam + 3) // 4
    seen = np.zeros(cam * cam, dtype=int)
    for q in range(cam * qpr):
        r, c4 = q // qpr, 4 * (q % qpr)
        for s in range(4):
            if c4 + s < cam:
                p = r * cam + c4 + s
                assert (int(quad[p]), int(slot[p])) == (r * cam + c4, s)
                seen[p] += 1
    assert (seen == 1).all()
    assert np.bincount(np.unique(quad, return_inverse=True)[1]).min() == (cam % 4 or 4)


@pytest.mark.parametrize("n_sub", [3, 8])
def test_sh6_layout_is_a_bijection_and_is_sh6_quad_pixels(n_sub):
    cam = 6 * n_sub
    lay = R.sh6_layout(cam, n_sub)
    _assert_bijection(lay, cam)
    quad, slot = lay
    seen = np.zeros(cam * cam, dtype=int)
    for k in range(n_sub * n_sub):
        y0, x0 = 6 * (k // n_sub), 6 * (k % n_sub)
        for j in range(9):
            if j < 6:
                pix = [(y0 + s) * cam + x0 + j for s in range(4)]
            else:
                c = j - 6
                pix = [(y0 + 4) * cam + x0 + c, (y0 + 5) * cam + x0 + c, (y0 + 4) * cam + x0 + c + 3, (y0 + 5) * cam + x0 + c + 3]
            for s, p in enumerate(pix):
                assert (int(quad[p]), int(slot[p])) == (pix[0], s)
                seen[p] += 1
    assert (seen == 1).all()
    assert R.layout_for(cam, n_sub, True)[0].tolist() == quad.tolist()
    assert R.layout_for(cam, n_sub, False)[0].tolist() == R.generic_layout(cam)[0].tolist()


def test_layout_refusal():
    with pytest.raises(ValueError, match="6 or a multiple of 4"):
        R.layout_for(30, 6, True)
    assert R.layout_for(24, 6, True)[0].tolist() == R.generic_layout(24)[0].tolist()


# ---- laws ----------------------------------------------------------------------------------------------------------------------
CAM = 256                                                          # 8 envs x 65536 pixels = 2^19 draws per law


def _cfg(**fields):
    return R.CameraCfg.from_fields(1 / 500, seed=0x1234567890ABCDEF, **fields)


@pytest.mark.parametrize("dark_e", [0.5, 3, 9.9, 10, 40])
def test_dark_current_follows_the_poisson_law(table, dark_e):
    """Inversion below 10 electrons, PTRS (its own streams: purposes 1 and 5, pixel | 0x80000000) from 10 on."""
    cfg = _cfg(darkCurrent=dark_e * 500, integrationTime=1 / 500)
    assert cfg.dark_e == np.float32(dark_e)
    x, ptrs = R.noisy_frame(np.zeros((8, CAM, CAM), np.float32), cfg, R.generic_layout(CAM), 100 + np.arange(8), 7, table)
    assert ptrs.all() == (dark_e >= 10) and ptrs.any() == (dark_e >= 10)
    assert (x == np.floor(x)).all() and x.min() >= 0
    rs = np.random.RandomState(2)
    lam = np.float64(np.float32(dark_e))
    R.assert_uniform(R.pit(x, lam, rs), dark_e)
    assert abs(x.mean() - lam) < 5 * np.sqrt(lam / x.size)
    # another frame number, another env: other draws
    y, _ = R.noisy_frame(np.zeros((1, CAM, CAM), np.float32), cfg, R.generic_layout(CAM), [100], 8, table)
    assert (y[0] != x[0]).mean() > 0.3 and (x[0] != x[1]).mean() > 0.3


@pytest.mark.parametrize("layout", ["generic", "sh6"])
def test_readout_normals_follow_the_normal_law(layout):
    """64 envs x 64 frames x 64 pixels (a 8 x 8 frame ... of the generic layout, the first 64 pixels of a 2-lenslet sh6 frame):
    mean, variance, kurtosis, Kolmogorov distance and the lag-1 correlations along env, frame number and pixel -- the last one is
    between the cos and the sin branch of a pair, and between pairs."""
    lay = R.generic_layout(8) if layout == "generic" else R.sh6_layout(12, 2)
    z = np.stack([R.readout_normals(lay, np.arange(64, dtype=np.uint64)[:, None], c, X.SEED)[:, :64] for c in range(1, 65)], axis=1)
    assert z.shape == (64, 64, 64) and z.dtype == np.float32
    X.assert_law(z, "camera read-out " + layout)
    z64 = np.stack([R.readout_normals(lay, np.arange(64, dtype=np.uint64)[:, None], c, X.SEED, exact=True)[:, :64] for c in (1, 2)], axis=1)
    assert np.abs(z64 - z[:, :2]).max() < X.STREAM_ATOL


def test_photon_counts_follow_the_poisson_law_across_the_hand_over(table):
    """A continuum of lambdas over every class, and lambdas on both sides of the table's end (1024 photons: alias below, PTRS from
    there on), through noisy_frame with the sh6 layout."""
    cfg = _cfg(photonNoise=True)
    rs = np.random.RandomState(4)
    n_sub = 40                                                    # 240 x 240 pixels x 8 envs
    lay = R.sh6_layout(6 * n_sub, n_sub)
    shape = (8, 6 * n_sub, 6 * n_sub)
    for name, lam in (("continuum", np.exp(rs.uniform(np.log(0.02), np.log(4000), size=shape))), ("hand-over", rs.uniform(960, 1090, size=shape))):
        lam = lam.astype(np.float32)
        x, ptrs = R.noisy_frame(lam, cfg, lay, np.arange(8), 3, table)
        assert np.array_equal(ptrs, lam >= 1024) and 0.05 < ptrs.mean() < 0.6
        R.assert_uniform(R.pit(x, lam.astype(np.float64), rs), name)
        R.assert_uniform(R.pit(x[ptrs], lam[ptrs].astype(np.float64), rs), name + " PTRS")
        R.assert_uniform(R.pit(x[~ptrs], lam[~ptrs].astype(np.float64), rs), name + " alias")


def test_hand_over_follows_the_table_prefix(table):
    """PoissonAliasHost::prefix restated: a budget that just holds the coarse rows 0 .. c - 1 reaches 32 c photons, one word less 32
    (c - 1); an env of a geometry the fused step kernel can take keeps what fits in that kernel's LDS, for every kernel; and
    noisy_frame hands the pixels at and above that count to PTRS."""
    t = table
    nf, nc = int(t[0]), int(t[1])
    assert R.table_lmax(t) == 1024.0 and (nf, nc) == (128, 32)
    for c in range(1, nc + 1):
        upto = int(t[R.HEADER + 2 * (nf + c)]) if c < nc else t.size
        need = (upto + 3) & ~3
        assert R.table_lmax(t, need) == 32.0 * c and R.table_lmax(t, need - 1) == 32.0 * (c - 1)
    assert R.step_alias_capacity(9) == 84 + 128 * 13 + 10944 and R.step_alias_capacity(21) == 444 + 128 * 25 + 10944
    small, large = R.env_lmax(t, True, 6, 48, 9), R.env_lmax(t, True, 6, 120, 21)
    assert 32 <= small <= large <= 1024 and small == R.table_lmax(t, R.step_alias_capacity(9))
    assert R.env_lmax(t, True, 4, 32, 9) == R.env_lmax(t, False, 6, 48, 9) == R.env_lmax(t, True, 6, 132, 23) == 1024.0
    lam = np.linspace(small - 40, small + 40, 36 * 36, dtype=np.float32).reshape(36, 36)
    x, ptrs = R.noisy_frame(lam, _cfg(photonNoise=True), R.sh6_layout(36, 6), 0, 1, t, lmax=small)
    assert np.array_equal(ptrs, lam >= small) and 0.3 < ptrs.mean() < 0.7
    assert np.abs(x - lam).max() < 8 * np.sqrt(small)


# ---- the deterministic part against the oracle -----------------------------------------------------------------------------------
def test_deterministic_part_equals_the_oracle(table):
    """QE, saturation, gain, ADC with every noise off: the float64 restatement equals oracle.ao_oracle.Detector exactly (the oracle
    given the float32 values of the settings, as the library holds them); the float32 one differs from it at a truncation boundary
    only.  Input: 0 .. 2.5 FWC, whole and fractional values, negative ones (clipped where there is an FWC)."""
    from oracle import ao_oracle as O
    rs = np.random.RandomState(6)
    fwc = 5000.0
    ideal = np.concatenate([rs.uniform(-3, 2.5 * fwc, size=20000), np.arange(0, 6000, 1.0), [0.0, fwc, 2 * fwc]]).astype(np.float32)
    ideal = ideal[:160 * 160].reshape(160, 160)
    assert (ideal > fwc).mean() > 0.3 and (ideal < 0).any()
    lay = R.generic_layout(160)
    f32 = lambda v: float(np.float32(v))
    n = 0
    for sensor, gain, bits, FWC, QE in itertools.product(("CCD", "CMOS", "EMCCD"), (0.5, 1, 3.7), (None, 8, 10, 16), (None, fwc), (1, 0.56)):
        if bits is not None and FWC is None:
            continue                                              # not a camera the library builds (aoenv_set_detector refuses it)
        cfg = _cfg(sensor=sensor, gain=gain, bits=bits, FWC=FWC, QE=QE)
        want = O.Detector(QE=f32(QE), FWC=FWC, bits=bits, gain=f32(gain), sensor=sensor).integrate(ideal)
        got64, ptrs = R.noisy_frame(ideal, cfg, lay, 0, 1, table, exact=True)
        assert not ptrs.any()
        np.testing.assert_array_equal(got64, want, err_msg=str((sensor, gain, bits, FWC, QE)))
        got32, _ = R.noisy_frame(ideal, cfg, lay, 0, 1, table)
        R.assert_flips(got32, want, ptrs, cfg, R.REFERENCE_FLIP_CAP, f"deterministic {sensor} gain {gain} bits {bits} FWC {FWC} QE {QE}")
        if bits is not None:
            assert got64.max() == min(int(f32(gain) * (2 ** bits - 1)), 2 ** bits - 1) and got64.min() == 0   # saturated; clipped from above
        n += 1
    assert n == 3 * 3 * (1 + 4) * 2


@pytest.mark.parametrize("sensor", ["EMCCD", "CMOS"])
def test_noisy_moments_equal_the_oracle(table, sensor):
    """Photon + dark + read-out noise, QE, gain 3.7, FWC, 12 bits: per-pixel mean and variance over N restated frames against N
    frames of the oracle's Detector (its own RandomStates), each within 5 sigma of the sampling error of the difference.  The gain
    multiplies the read-out noise for CCD / CMOS and not for EMCCD: the variances of the two differ by a factor of 3 at these
    settings, so a swapped order fails."""
    from oracle import ao_oracle as O
    N = 4000
    fields = dict(sensor=sensor, gain=3.7, readoutNoise=14, photonNoise=True, QE=0.8, darkCurrent=1500, integrationTime=1 / 500,
                  FWC=20000, bits=12)
    cfg = _cfg(**fields)
    rs = np.random.RandomState(8)
    ideal = np.exp(rs.uniform(np.log(0.1), np.log(1500), size=(12, 12))).astype(np.float32)
    got, _ = R.noisy_frame(np.broadcast_to(ideal, (N, 12, 12)), cfg, R.sh6_layout(12, 2), np.arange(N), 5, table)
    det = O.Detector(seed=3, **fields)
    want = np.stack([det.integrate(ideal) for _ in range(N)])
    gm, wm, gv, wv = got.mean(0), want.mean(0), got.var(0), want.var(0)
    z_mean = (gm - wm) / np.sqrt((gv + wv) / N)
    # variance of a sample variance: (m4 - var^2) / N, m4 from the oracle's sample
    m4 = ((want - wm) ** 4).mean(0)
    z_var = (gv - wv) / np.sqrt(2 * (m4 - wv ** 2) / N)
    print(sensor, "largest |z| of the means", np.abs(z_mean).max(), "of the variances", np.abs(z_var).max())
    assert np.abs(z_mean).max() < 5 and np.abs(z_var).max() < 5
    other = O.Detector(seed=3, **dict(fields, sensor="CMOS" if sensor == "EMCCD" else "EMCCD"))
    ov = np.stack([other.integrate(ideal) for _ in range(400)]).var(0)
    assert np.median(np.maximum(ov, wv) / np.minimum(ov, wv)) > 2  # the other order is another camera (but on the brightest pixels)


# ---- float32 against float64 ----------------------------------------------------------------------------------------------------------
def synthetic_frame(n_sub, p, peak, rs):
    """A Shack-Hartmann-like frame: one Gaussian spot per lenslet with a random centre and flux, so that pixels fall into every
    brightness class up to `peak` photons."""
    cam = n_sub * p
    y, x = np.mgrid[:cam, :cam]
    cy = (y // p) * p + p / 2 - 0.5 + rs.uniform(-1, 1, size=(n_sub, n_sub)).repeat(p, 0).repeat(p, 1)
    cx = (x // p) * p + p / 2 - 0.5 + rs.uniform(-1, 1, size=(n_sub, n_sub)).repeat(p, 0).repeat(p, 1)
    amp = np.exp(rs.uniform(np.log(peak / 30), np.log(peak), size=(n_sub, n_sub))).repeat(p, 0).repeat(p, 1)
    return (amp * np.exp(-((y - cy) ** 2 + (x - cx) ** 2) / (2 * 0.9 ** 2))).astype(np.float32)


@pytest.mark.parametrize("name", list(R.SETTINGS) + ["everything", "photon-bright"])
def test_float32_and_float64_restatements_agree_within_the_flip_cap(table, name):
    """The cap the GPU tests lean on: on frames with pixels in every brightness class and under every camera setting they run, the
    float32 restatement differs from the float64 one on at most REFERENCE_FLIP_CAP of the pixels, by one count there (PTRS pixels:
    the share only).  (The GPU tests assert the same on the device's own frames before they look at the device's counts.)"""
    fields = R.EVERYTHING if name == "everything" else R.SETTINGS["photon" if name == "photon-bright" else name]
    cfg = _cfg(**fields)
    rs = np.random.RandomState(10)
    peak = 6000.0 if name == "photon-bright" else 900.0
    ideal = np.stack([synthetic_frame(16, 6, peak, rs) for _ in range(4)])
    classes = [(ideal < 0.25).mean(), ((ideal >= 0.25) & (ideal < 32)).mean(), ((ideal >= 32) & (ideal < 1024)).mean()]
    assert min(classes) > 0.02 and ((ideal >= 1024).mean() > 0.01) == (name == "photon-bright")
    for lay in (R.sh6_layout(96, 16), R.generic_layout(96)):
        a, ptrs = R.noisy_frame(ideal, cfg, lay, 100 + np.arange(4), 2, table)
        b, ptrs_b = R.noisy_frame(ideal, cfg, lay, 100 + np.arange(4), 2, table, exact=True)
        assert np.array_equal(ptrs, ptrs_b)
        R.assert_flips(a, b, ptrs, cfg, R.REFERENCE_FLIP_CAP, name)
    if name != "dark40":
        assert ptrs.any() == (name == "photon-bright")
