"""CPU: the geometric Shack-Hartmann's restatement (tests/_geometric_ref.py) against tests/golden/geometric_sh.npz, which
scripts/make_geometric_golden.py wrote from the reference's own ``ShackHartmann(..., is_geometric=True)``; five convention errors
that each move a golden signal far beyond the tolerance; the OPD-to-slope bound the GPU tests hold the library to; the
``GeometricOracle`` in closed loop; the launch plan of the fused tail (rlao_amd/csrc/sh_geometric.hpp) through
tests/native/geometric_driver.cpp."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import _geometric_ref as G

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TAGS = list(G.GEOMETRIES)
REL = 1e-12                                                         # of the array's maximum; measured 0.0 for the OPD cases


@pytest.fixture(scope="module")
def gold():
    return np.load(G.GOLDEN)


def _geo(gold, tag):
    R, ns, D, ob = G.GEOMETRIES[tag]
    return dict(R=R, ns=ns, D=D, ob=ob, ps=D / R, pupil=gold[f"{tag}_pupil"], valid=gold[f"{tag}_valid"],
                units=float(gold[f"{tag}_slopes_units"]), wl=float(gold[f"{tag}_wavelength"]))


def _dm_opd(g, coefs):
    """dm.OPD of the project's own tables (Gy C Gx^T), [n, R, R]."""
    from rlao_amd import calib
    p = calib.params_from_args(dict(diameter=g["D"], nSubaperture=g["ns"], nPixelPerSubap=g["R"] // g["ns"], centralObstruction=g["ob"]))
    dmt = calib.DMTables(p)
    C = np.zeros((len(coefs), dmt.nAct * dmt.nAct))
    C[:, dmt.act_idx] = coefs
    return np.einsum("yi,nij,xj->nyx", dmt.gy, C.reshape(-1, dmt.nAct, dmt.nAct), dmt.gx), dmt


@pytest.mark.parametrize("tag", TAGS)
def test_restatement_matches_every_array_of_the_golden(gold, tag):
    g = _geo(gold, tag)
    from rlao_amd import calib
    # (r30, odd p: the golden's valid map is the flux rule applied to whole tiles by scripts/make_geometric_golden.py, because the
    #  reference's own flux tiling cannot build an odd-p sensor: that selection is the project's, not pinned by the reference)
    assert np.array_equal(calib.telescope_pupil(g["R"], g["ob"]), g["pupil"])
    k = 2 * np.pi / g["wl"]
    assert int(gold[f"{tag}_params"][1]) == g["ns"] and gold[f"{tag}_sig_opd"].shape == (4, 2 * g["valid"].sum())
    units = G.slopes_units_of(g["pupil"], g["valid"], g["ps"], g["wl"])
    print(f"{tag}: slopes_units {units!r} golden {g['units']!r}")
    assert abs(units - g["units"]) <= REL * g["units"]
    want = gold[f"{tag}_sig_opd"]
    got = np.array([G.geo_signal(o * k, g["pupil"], g["valid"], g["ps"], g["units"]) for o in gold[f"{tag}_opd"]])
    print(f"{tag}: opd signals max |diff| {np.abs(got - want).max():.3e} of {np.abs(want).max():.3e}")
    assert np.abs(got - want).max() <= REL * np.abs(want).max()
    assert np.abs(gold[f"{tag}_opd"][:, ~g["pupil"]]).min() > 0         # the inputs are not masked
    opd, dmt = _dm_opd(g, gold[f"{tag}_coefs"])
    assert np.array_equal(dmt.validAct.reshape(-1), gold[f"{tag}_validAct"].reshape(-1))
    want = gold[f"{tag}_sig_dm"]
    got = np.array([G.geo_signal(o * k, g["pupil"], g["valid"], g["ps"], g["units"]) for o in opd])
    print(f"{tag}: dm signals max |diff| {np.abs(got - want).max():.3e} of {np.abs(want).max():.3e}")
    assert np.abs(got - want).max() <= REL * np.abs(want).max()
    stroke = g["wl"] / 16
    idx = gold[f"{tag}_poke_idx"]
    pokes = np.zeros((6, dmt.nValidAct))
    pokes[np.arange(6), idx] = stroke
    opd, _ = _dm_opd(g, pokes)
    got = np.array([G.geo_signal(o * k, g["pupil"], g["valid"], g["ps"], g["units"]) for o in opd]).T / stroke
    want = gold[f"{tag}_poke_cols"]
    print(f"{tag}: poke columns max |diff| {np.abs(got - want).max():.3e} of {np.abs(want).max():.3e}")
    assert np.abs(got - want).max() <= REL * np.abs(want).max()


def _variant(name, phi, g, ref_diffractive):
    """The signal of one convention error."""
    pupil = g["pupil"].astype(np.float64)
    ns, ps, units = g["ns"], g["ps"], g["units"]
    maps = np.concatenate((g["valid"], g["valid"]))
    grad = lambda a, ax: np.gradient(a, axis=ax)
    if name == "blocks_swapped":
        s = G.geo_signal_2d(phi, pupil, ns, ps, units)
        return np.concatenate((s[ns:], s[:ns]))[maps]
    if name == "masked_first":
        return G.geo_signal_2d(phi * pupil, pupil, ns, ps, units)[maps]
    if name == "forward":
        def grad(a, ax):
            d = np.diff(a, axis=ax)
            last = np.take(d, [-1], axis=ax)
            return np.concatenate((d, last), axis=ax)
    elif name == "wrapped":
        grad = lambda a, ax: (np.roll(a, -1, axis=ax) - np.roll(a, 1, axis=ax)) / 2
    elif name == "clamped":
        def grad(a, ax):
            n = a.shape[ax]
            hi, lo = np.minimum(np.arange(n) + 1, n - 1), np.maximum(np.arange(n) - 1, 0)
            return (np.take(a, hi, axis=ax) - np.take(a, lo, axis=ax)) / 2
    elif name == "reference_subtracted":
        return G.geo_signal(phi, pupil, g["valid"], ps, units) - ref_diffractive
    gx = grad(phi, 0) / ps * pupil
    gy = grad(phi, 1) / ps * pupil
    return (np.concatenate((G.bin_sum(gy, ns), G.bin_sum(gx, ns))) / units)[maps]


@pytest.mark.parametrize("name", ["blocks_swapped", "masked_first", "forward", "wrapped", "clamped", "reference_subtracted"])
def test_every_convention_error_moves_a_golden_signal(gold, name):
    """Swapped blocks, masking before differentiating, forward for central differences, central differences wrapped or clamped at
    the first / last row, a (diffractive) reference subtracted: each is more than 100 tolerances away on every geometry."""
    from oracle import ao_oracle as O
    for tag in TAGS:
        g = _geo(gold, tag)
        flux = g["pupil"].astype(float)
        sh = O.OracleSH(g["ns"], g["R"], g["D"], g["pupil"], g["wl"], flux, 0.5, 0.01)
        assert np.array_equal(sh.valid_2d, g["valid"])
        ref = sh.reference_slopes_maps[np.concatenate((g["valid"], g["valid"]))] / g["units"]
        want = gold[f"{tag}_sig_opd"]
        moved = max(np.abs(_variant(name, o * 2 * np.pi / g["wl"], g, ref) - w).max() for o, w in zip(gold[f"{tag}_opd"], want))
        print(f"{tag} {name}: moves the signal by {moved:.3e}, tolerance {REL * np.abs(want).max():.3e}")
        assert moved > 100 * REL * np.abs(want).max()


@pytest.mark.parametrize("tag", TAGS)
def test_signal_bound_holds_for_random_phase_perturbations(gold, tag):
    g = _geo(gold, tag)
    p = g["R"] // g["ns"]
    rng = np.random.RandomState(5)
    worst = 0.0
    for tol in (1e-12, 2e-9):
        bound = G.geo_signal_bound(tol, p, g["ps"], g["units"], g["wl"])
        for o in gold[f"{tag}_opd"]:
            for _ in range(8):
                d = rng.uniform(-tol, tol, o.shape)
                a = G.geo_signal(o * 2 * np.pi / g["wl"], g["pupil"], g["valid"], g["ps"], g["units"])
                b = G.geo_signal((o + d) * 2 * np.pi / g["wl"], g["pupil"], g["valid"], g["ps"], g["units"])
                worst = max(worst, np.abs(a - b).max() / bound)
    print(f"{tag}: largest |d signal| / bound = {worst:.3f}")
    assert 0 < worst <= 1


def _closed_loop(steps=8):
    o = G.GeometricOracle(resolution=24, diameter=1.6, n_subap=4, r0=0.13, L0=30.0, windSpeed=[10.0], windDirection=[72.0],
                          fractionalR0=[1.0], altitude=[0.0], n_modes=8)
    o.new_episode(17)
    obs = o.reset_soft()
    out = [obs]
    for i in range(steps):
        obs, frame, rew, sr, _, _ = o.step(i, 0.5 * obs)
        assert not np.any(frame)
        out.append(obs)
    return o, np.array(out)


def test_geometric_oracle_closed_loop_is_deterministic_and_corrects(gold):
    a, obs_a = _closed_loop()
    b, obs_b = _closed_loop()
    assert np.array_equal(obs_a, obs_b) and np.array_equal(a.residual[:8], b.residual[:8])
    g = _geo(gold, "r24")
    assert abs(a.wfs.slopes_units - g["units"]) <= REL * g["units"] and np.array_equal(a.wfs.valid_2d, g["valid"])
    assert not np.any(a.wfs.reference_slopes_maps)
    # its interaction matrix is the golden's at the six poked columns
    want = gold["r24_poke_cols"]
    assert np.abs(a.imat[:, gold["r24_poke_idx"]] - want).max() <= 1e-10 * np.abs(want).max()
    print("residual nm", a.residual[:8], "total nm", a.total[:8])
    assert np.isfinite(obs_a).all() and a.residual[7] < 0.6 * a.total[7]      # the integrator closes the loop on these slopes


# ---- the fused tail's launch plan: rlao_amd/csrc/sh_geometric.hpp through tests/native/geometric_driver.cpp -------------------------
def _plan(R, ns, nv, na, nm, esz):
    p = R // ns
    base = 2 * nv + na * na + nm
    band = lambda g: (g * p + 2) * R + 2 * g * R + 2 * g * ns + (g * p * R + esz - 1) // esz
    g = 0
    while g < ns and esz * (base + band(g + 1)) <= 64 * 1024 - 128:      # (the kernel's 128 B of static LDS beside it)
        g += 1
    return g, base, band(max(g, 1)), esz * band(1)


def test_tail_plan_of_the_header_is_the_restated_one(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = tmp_path / "geometric_driver"
    subprocess.run([cxx, "-std=c++17", "-O1", f"-I{os.path.join(REPO, 'rlao_amd', 'csrc')}",
                    os.path.join(REPO, "tests", "native", "geometric_driver.cpp"), "-o", str(exe)], check=True)
    cases = [(R, ns, nv, ns + 1, nm, esz)
             for R, ns in [(24, 4), (20, 5), (30, 6), (32, 4), (96, 16), (120, 20), (480, 80), (480, 20), (48, 2), (46, 23)]
             for nv in sorted({max(1, ns * ns // 2), ns * ns}) for nm in (1, 50, 300) for esz in (4, 8)]
    text = "".join("%d %d %d %d %d %d\n" % c for c in cases)
    out = subprocess.run([str(exe)], input=text, capture_output=True, text=True, check=True).stdout.split("\n")
    got = [tuple(int(v) for v in line.split()) for line in out if line]
    assert got == [_plan(*c) for c in cases]
    # literal pins: the C2 shape in float32 takes its 20 lenslet rows in bands of 12; the C4 shape leaves the fused tail (the tail's
    # own arrays are above 64 KB there, as k_sh_tail's are); p = 24 in float64 stages 117 KB a lenslet row in the stand-alone kernel
    assert _plan(120, 20, 316, 21, 50, 4)[0] == 12 and _plan(120, 20, 316, 21, 50, 8)[0] == 6
    assert _plan(480, 80, 5024, 81, 300, 4)[0] == 0
    # a partial last band whose work area is laid out anew over the previous band's totals (tests/test_gpu_geometric.py "r160"):
    # 20 lenslet rows of p = 8 in bands of 7, 7 and 6
    assert _plan(160, 20, 316, 21, 50, 4)[0] == 7
    assert _plan(24, 4, 12, 5, 8, 8)[0] == 4
    assert _plan(480, 20, 316, 21, 50, 8)[3] == 8 * (26 * 480 + 2 * 480 + 40 + 24 * 480 // 8) <= 160 * 1024
