"""CPU: layers on grids of their own (a telescope with a field of view), host side.  The table of tests/_fov_cases.py -- grids,
footprint offsets, ring sizes -- from calib.AtmosphereTables and from oracle.LayerGeometry; the oracle handed one (geometry, A, B)
per layer; BatchedAOEnv's own check of per-layer operators.  The reference tree is never read here."""
import os

import numpy as np
import pytest

from _fov_cases import CASES, PYR, atmosphere, build_oracle, geo, layer_geometries
from oracle import ao_oracle as O


@pytest.mark.parametrize("name", list(CASES))
def test_grid_table(name):
    """N_l, foot_l = N_l // 2 - R // 2 + 1 and K_l = n_inner + n_outer of every case, from calib and from the oracle's geometry."""
    from rlao_amd import calib
    c, g = CASES[name], geo(name)
    p = calib.params_from_args(g)
    at = calib.AtmosphereTables(p)
    R = c["n_sub"] * c["ppx"]
    assert p.resolution == R and R % 2 == 0
    assert at.layer_res == c["grids"] and at.uniform == c["uniform"] == (len(set(c["grids"])) == 1)
    assert [t.foot + 1 for t in at.layers] == c["foot"] == [n // 2 - R // 2 + 1 for n in c["grids"]]
    assert [t.n_inner + t.n_outer for t in at.layers] == c["K"] == [12 * n - 12 for n in c["grids"]]
    assert [t.AB.shape for t in at.layers] == [(4 * n + 4, 12 * n - 12) for n in c["grids"]]
    geoms = layer_geometries(g)
    assert [q.resolution for q in geoms] == c["grids"]
    assert [q.foot[0].start + 1 for q in geoms] == c["foot"] and all(q.foot[0].stop - q.foot[0].start == R for q in geoms)
    assert [q.innerZ.size + q.outerZ.size for q in geoms] == c["K"]
    for t, q in zip(at.layers, geoms):                              # one ordering of the ring on both sides
        assert np.array_equal(t.outer_mask, q.outerMask) and np.array_equal(t.inner_mask, q.innerMask)
    # the winds: below a pixel per frame on both axes, a pixel crossed within six frames
    ratio = at.wind_ratio(p.windSpeed, p.windDirection, p.samplingTime)
    assert (np.abs(ratio).max(axis=1) < 1).all() and (6 * np.abs(ratio).max(axis=1) >= 1).all()
    np.testing.assert_allclose(np.hypot(ratio[:, 0], ratio[:, 1]), c["px"], rtol=1e-12)


def test_pyramid_case_has_unequal_layers():
    from rlao_amd import calib
    p = calib.params_from_args(dict(diameter=1.6, nSubaperture=4, nPixelPerSubap=4, r0=0.13, L0=30.0, **atmosphere(PYR, 4)))
    at = calib.AtmosphereTables(p)
    assert not at.uniform and at.layer_res[0] == p.resolution + 4 and at.layer_res[1] > at.layer_res[0]


def _small(fov=12.0):
    """4 x 6 pixels, layers at 0 / 6000 / 6000 m: grids of 28 / 34 / 34."""
    return dict(diameter=1.6, nSubaperture=4, nPixelPerSubap=6, r0=0.13, L0=30.0, nModes=6, nLoop=16,
                windSpeed=[15.0, 12.0, 16.0], windDirection=[72.0, 200.0, 320.0], fractionalR0=[0.5, 0.3, 0.2],
                altitude=[0.0, 6000.0, 6000.0], fov=fov)


def _oracle_kw(g):
    return dict(resolution=g["nSubaperture"] * g["nPixelPerSubap"], diameter=g["diameter"], n_subap=g["nSubaperture"], r0=g["r0"],
                L0=g["L0"], windSpeed=g["windSpeed"], windDirection=g["windDirection"], fractionalR0=g["fractionalR0"],
                altitude=g["altitude"], n_modes=g["nModes"], nLoop=g["nLoop"], fov_arcsec=g["fov"])


def _episode(o, seed, steps=5):
    o.new_episode(seed)
    obs = o.reset_soft()
    out = [obs.copy()] + [lay.mapShift.copy() for lay in o.atm.layers]
    for i in range(steps):
        obs, frame, rew, sr, _, _ = o.step(i, (0.5 * obs).astype(np.float32))
        out += [obs.copy(), frame.copy(), np.float64(rew), np.float64(sr), o.atm.OPD.copy()]
    return out + [lay.mapShift.copy() for lay in o.atm.layers]


def test_oracle_with_its_own_operators_per_layer_reproduces_itself():
    """OracleEnv(geom_AB=[(geometry, A, B) per layer]) under a field of view is the oracle that computed them, bit for bit; a list
    of the wrong length, a geometry of the wrong grid and operators of the wrong shape are refused."""
    g = _small()
    own = O.OracleEnv(**_oracle_kw(g))
    assert [lay.g.resolution for lay in own.atm.layers] == [28, 34, 34]
    triples = [(lay.g, lay.A.copy(), lay.B.copy()) for lay in own.atm.layers]
    given = O.OracleEnv(m2c=own.M2C, geom_AB=triples, **_oracle_kw(g))
    assert all(np.array_equal(a.A, t[1]) and np.array_equal(a.B, t[2]) for a, t in zip(given.atm.layers, triples))
    assert np.array_equal(given.imat, own.imat)
    for x, y in zip(_episode(own, 3), _episode(given, 3)):
        assert np.array_equal(x, y)
    # ... and the operators are USED: the second layer's B doubled changes the screens from its first ring on
    other = [(q, A, 2 * B if l == 1 else B) for l, (q, A, B) in enumerate(triples)]
    changed = O.OracleEnv(m2c=own.M2C, geom_AB=other, **_oracle_kw(g))
    changed.new_episode(3)
    own.new_episode(3)
    assert np.array_equal(changed.atm.layers[0].mapShift, own.atm.layers[0].mapShift)
    assert not np.array_equal(changed.atm.layers[1].mapShift, own.atm.layers[1].mapShift)
    with pytest.raises(ValueError, match="triples"):
        O.OracleEnv(m2c=own.M2C, geom_AB=triples[:2], **_oracle_kw(g))
    with pytest.raises(ValueError, match="grid"):
        O.OracleEnv(m2c=own.M2C, geom_AB=[triples[1], triples[1], triples[2]], **_oracle_kw(g))
    with pytest.raises(ValueError, match="shapes"):
        O.OracleEnv(m2c=own.M2C, geom_AB=[triples[0], (triples[1][0], triples[0][1], triples[0][2]), triples[2]], **_oracle_kw(g))


def test_single_triple_keeps_its_meaning():
    """fov = 0: the one (geometry, A, B) for every layer, as before; under a field of view a single triple is still not used."""
    g = _small(fov=0.0)
    own = O.OracleEnv(**_oracle_kw(g))
    lay = own.atm.layers[0]
    given = O.OracleEnv(m2c=own.M2C, geom_AB=(lay.g, lay.A, 2 * lay.B), **_oracle_kw(g))
    assert all(x.B is given.atm.layers[0].B for x in given.atm.layers) and np.array_equal(given.atm.layers[2].B, 2 * lay.B)
    g = _small()
    fov = O.OracleEnv(m2c=own.M2C, geom_AB=(lay.g, lay.A, 2 * lay.B), **_oracle_kw(g))
    assert [x.g.resolution for x in fov.atm.layers] == [28, 34, 34] and np.array_equal(fov.atm.layers[0].B, lay.B)


def test_oracle_replays_fov_fixture_with_injected_operators(golden_dir):
    """tiny_3layer_fov1 (grids 28 / 29 / 29) replayed by the oracle that is handed the fixture's A, B, A_l1, B_l1, A_l2, B_l2: the
    tolerances of tests/test_oracle_golden.py::test_closed_loop_replay."""
    from test_oracle_golden import _env_from_golden
    g = np.load(os.path.join(golden_dir, "tiny_3layer_fov1.npz"))
    R, D, fov_rad = int(g["cfg_R"]), float(g["cfg_D"]), float(g["cfg_fov"]) / 206265.0
    geoms = [O.LayerGeometry(R, D, float(g["cfg_L0"]), altitude=float(h), fov_rad=fov_rad) for h in g["cfg_alt"]]
    ops = [(g["A"], g["B"])] + [(g[f"A_l{l}"], g[f"B_l{l}"]) for l in range(1, len(geoms))]
    env = _env_from_golden(g, geom_AB=[(q, A, B) for q, (A, B) in zip(geoms, ops)])
    assert [lay.mapShift.shape[0] for lay in env.atm.layers] == list(g["cfg_layer_S"])
    for lay, (A, B) in zip(env.atm.layers, ops):
        assert np.array_equal(lay.A, A) and np.array_equal(lay.B, B)
    np.testing.assert_allclose(env.imat, g["imat"], atol=1e-12 * np.abs(g["imat"]).max())
    for seed in g["cfg_seeds"]:
        p = f"s{int(seed)}_"
        env.dm_prev[:] = 0
        env.new_episode(int(seed))
        for l, lay in enumerate(env.atm.layers):
            S = lay.mapShift.shape[0]
            np.testing.assert_allclose(lay.mapShift, g[p + "mapShift0"][l][:S, :S], atol=1e-12)
        np.testing.assert_allclose(env.reset_soft(), g[p + "obs0"], atol=1e-11)
        full = {int(s): k for k, s in enumerate(g[p + "full_steps"])}
        for i, act in enumerate(g[p + "actions"]):
            obs, frame, rew, sr, _, _ = env.step(i, act)
            np.testing.assert_allclose(obs, g[p + "obs"][i], atol=1e-10)
            np.testing.assert_allclose(rew, g[p + "reward"][i], atol=1e-10)
            np.testing.assert_allclose(sr, g[p + "strehl"][i], atol=1e-12)
            np.testing.assert_allclose(env.total[i], g[p + "total"][i], atol=1e-9)
            np.testing.assert_allclose(env.residual[i], g[p + "residual"][i], atol=1e-9)
            np.testing.assert_allclose(env.wfs.signal, g[p + "signal"][i], atol=1e-11)
            np.testing.assert_allclose(env.coefs, g[p + "coefs"][i], atol=1e-18)
            for l, lay in enumerate(env.atm.layers):
                np.testing.assert_allclose(lay.buff, g[p + "buff"][i, l], atol=1e-13)
            if i in full:
                k = full[i]
                np.testing.assert_allclose(env.atm.OPD, g[p + "opd_atm"][k], atol=1e-18)
                np.testing.assert_allclose(env.tel_OPD, g[p + "opd_res"][k], atol=1e-18)
                np.testing.assert_allclose(frame, g[p + "frame"][k], atol=1e-8 * g[p + "frame"][k].max())


def test_env_checks_operators_per_layer():
    """BatchedAOEnv._atmosphere_tables (what set_params validates atm_AB with, before it touches the env): one pair per layer for
    layers on grids of their own -- every layer then owns its table, the two layers of one grid size too; the single pair keeps
    its meaning and refuses such an atmosphere; a list refuses a shared grid, a wrong length and a wrong shape."""
    from rlao_amd import calib
    from rlao_amd.env import BatchedAOEnv
    g = _small()
    p = calib.params_from_args(g)
    plain = BatchedAOEnv._atmosphere_tables(p)
    assert plain.layer_res == [28, 34, 34] and plain.layers[1] is plain.layers[2]
    pairs = [(t.A + l, t.B - l) for l, t in enumerate(plain.layers)]
    at = BatchedAOEnv._atmosphere_tables(p, pairs)
    assert len({id(t) for t in at.layers}) == 3
    for t, (A, B) in zip(at.layers, pairs):
        assert np.array_equal(t.A, A) and np.array_equal(t.B, B) and np.array_equal(t.AB, np.concatenate([A, B], axis=1))
        assert t.AB.flags.c_contiguous
    assert at.A is at.layers[0].A and at.AB is at.layers[0].AB
    assert np.array_equal(at.layers[1].inner_idx, plain.layers[1].inner_idx)
    at.set_r0(p.r0)                                                 # a new r0 recomputes every layer's operators
    for t, q in zip(at.layers, plain.layers):
        assert np.array_equal(t.AB, q.AB)
    with pytest.raises(ValueError, match="one pair per layer"):
        BatchedAOEnv._atmosphere_tables(p, (plain.A, plain.B))
    with pytest.raises(ValueError, match="2 pairs for 3 layers"):
        BatchedAOEnv._atmosphere_tables(p, pairs[:2])
    with pytest.raises(ValueError, match=r"atm_AB\[1\]"):
        BatchedAOEnv._atmosphere_tables(p, [pairs[0], pairs[0], pairs[2]])
    p0 = calib.params_from_args(_small(fov=0.0))
    with pytest.raises(ValueError, match="share one grid"):
        BatchedAOEnv._atmosphere_tables(p0, [(plain.A, plain.B)] * 3)
    one = BatchedAOEnv._atmosphere_tables(p0, (plain.A + 1, plain.B))
    assert one.uniform and np.array_equal(one.layers[2].A, plain.A + 1)


def test_build_oracle_takes_the_hosts_operators():
    """_fov_cases.build_oracle (what the GPU sweep builds its reference with) on the smallest case: the oracle's layers carry the
    operators calib computed, on the grids of the table."""
    from rlao_amd import calib
    g = geo("p5_shared")
    p = calib.params_from_args(g)
    at = calib.AtmosphereTables(p)
    m2c = calib.zernike_m2c(calib.DMTables(p), calib.telescope_pupil(p.resolution), p.diameter, p.nModes)
    o = build_oracle(g, m2c, [(t.A, t.B) for t in at.layers])
    assert [lay.g.resolution for lay in o.atm.layers] == CASES["p5_shared"]["grids"]
    for lay, t in zip(o.atm.layers, at.layers):
        assert np.array_equal(lay.A, t.A) and np.array_equal(lay.B, t.B)
        np.testing.assert_allclose(lay.g.AB(p.r0)[0], t.A, atol=1e-9)       # (the oracle's own operators: the same to the pinv's noise)
