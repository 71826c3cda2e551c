"""The cases of the field-of-view sweep (tests/test_gpu_fov_sweep.py, tests/test_fov_host.py): Shack-Hartmann geometries with
D = 0.4 n_sub, r0 = 0.13, L0 = 30 whose layers sit at an altitude under a telescope with a field of view.  A layer at altitude h then
has a grid of N = ceil(R / D (D + 2 tan(fov / 2) h)) + 4 pixels (OOPAO/Atmosphere.py:216-218), the on-axis R x R footprint starts at
foot = N // 2 - R // 2 + 1 of its (N + 2)^2 screen, and its ring operator [A | B] has K = n_inner + n_outer = 12 N - 12 columns.
Every number of the table is asserted from calib and from the oracle: a change of the grid rule must not move a case off its branch.

Winds: 0.40 .. 0.48 pixel per frame (every layer of every env crosses a pixel in six steps: asserted from the oracle's clocks);
directions 72 / 200 / 320 / 144 deg: (+x +y), (-x -y), (-x +y), (+x -y).  The seeds: chosen on the CPU from the oracle alone, among
1 .. 8, for the largest distance of any pixel from the 1 % centroid cut over three envs and six steps (see the sweep's docstring).
"""
import numpy as np

R0, L0_M = 0.13, 30.0
FRAME_RATE = 500.0

CASES = {
    # R % 4 == 2 (k_phase_mfma); a prime N; very unequal footprint offsets
    "two": dict(n_sub=7, ppx=6, altitude=[0.0, 10000.0], fov=20.0, grids=[46, 61], foot=[3, 10], K=[540, 720],
                px=[0.45, 0.40], wd=[144.0, 320.0], frac=[0.65, 0.35], n_modes=10, uniform=False, seed=5),
    # k_phase_mfma4, not its band variant; three distinct grids, K and slab sizes
    "three": dict(n_sub=10, ppx=6, altitude=[0.0, 5000.0, 12000.0], fov=10.0, grids=[64, 68, 73], foot=[3, 5, 7],
                  K=[756, 804, 864], px=[0.45, 0.40, 0.48], wd=[72.0, 200.0, 320.0], frac=[0.5, 0.3, 0.2], n_modes=20,
                  uniform=False, seed=6),
    # layer 0 is the larger grid (whatever is taken "from layer 0")
    "top_first": dict(n_sub=11, ppx=6, altitude=[3000.0, 0.0], fov=30.0, grids=[77, 70], foot=[6, 3], K=[912, 828],
                      px=[0.48, 0.42], wd=[200.0, 144.0], frac=[0.4, 0.6], n_modes=30, uniform=False, seed=3),
    # generic spots / centroid / tail kernels; two layers that share one host table but own device tables and streams
    "p5_shared": dict(n_sub=6, ppx=5, altitude=[0.0, 9000.0, 9000.0], fov=15.0, grids=[34, 43, 43], foot=[3, 7, 7],
                      K=[396, 504, 504], px=[0.45, 0.40, 0.48], wd=[72.0, 200.0, 320.0], frac=[0.5, 0.3, 0.2], n_modes=8,
                      uniform=False, seed=6),
    # one elevated layer: uniform, the fused step kernel with S = 72, foot 6 (FUSED_STEP=0: k_phase_mfma4<BAND>)
    "up70": dict(n_sub=10, ppx=6, altitude=[8000.0], fov=10.0, grids=[70], foot=[6], K=[828],
                 px=[0.45], wd=[200.0], frac=[1.0], n_modes=20, uniform=True, seed=5),
    # two elevated layers on one odd prime grid: uniform, the fused kernel, shared tables
    "up71x2": dict(n_sub=10, ppx=6, altitude=[9000.0, 9000.0], fov=10.0, grids=[71, 71], foot=[6, 6], K=[840, 840],
                   px=[0.45, 0.42], wd=[320.0, 144.0], frac=[0.6, 0.4], n_modes=20, uniform=True, seed=3),
}

# the Pyramid behind unequal layers: the smallest geometry of tests/test_gpu_pyramid_sweep.py
PYR = dict(base="pow64", altitude=[0.0, 10000.0], fov=20.0, px=[0.45, 0.40], wd=[144.0, 320.0], frac=[0.65, 0.35])


def atmosphere(c, ppx):
    """The atmosphere keys of a case: winds of c["px"] pixels per frame (pixel size 0.4 / ppx m, 500 frames per second)."""
    ps = 0.4 / ppx
    return dict(windSpeed=[x * ps * FRAME_RATE for x in c["px"]], windDirection=list(c["wd"]), fractionalR0=list(c["frac"]),
                altitude=list(c["altitude"]), fov=c["fov"])


def geo(name, **kw):
    c = CASES[name]
    d = dict(diameter=0.4 * c["n_sub"], nSubaperture=c["n_sub"], nPixelPerSubap=c["ppx"], r0=R0, L0=L0_M, nModes=c["n_modes"],
             nLoop=16, **atmosphere(c, c["ppx"]))
    d.update(kw)
    return d


def layer_geometries(g):
    """oracle.LayerGeometry of every layer of the parameter dict `g` (layers of one grid size share one)."""
    from oracle import ao_oracle as O
    R = g["nSubaperture"] * g["nPixelPerSubap"]
    fov_rad = g.get("fov", 0.0) / 206265.0
    made, out = {}, []
    for h in g["altitude"]:
        n = O.LayerGeometry.grid(R, g["diameter"], h, fov_rad)
        if n not in made:
            made[n] = O.LayerGeometry(R, g["diameter"], g["L0"], altitude=h, fov_rad=fov_rad)
        out.append(made[n])
    return out


def build_oracle(g, m2c, operators, **kw):
    """OracleEnv of the parameter dict `g` with its OWN calibration, handed one (A, B) per layer (the env's own ring operators)."""
    from oracle import ao_oracle as O
    geoms = layer_geometries(g)
    assert len(operators) == len(geoms)
    return O.OracleEnv(resolution=g["nSubaperture"] * g["nPixelPerSubap"], diameter=g["diameter"], n_subap=g["nSubaperture"],
                       r0=g["r0"], L0=g["L0"], windSpeed=g["windSpeed"], windDirection=g["windDirection"],
                       fractionalR0=g["fractionalR0"], altitude=g["altitude"], m2c=m2c, n_modes=np.shape(m2c)[1], nLoop=g["nLoop"],
                       fov_arcsec=g.get("fov", 0.0), geom_AB=[(q, A, B) for q, (A, B) in zip(geoms, operators)], **kw)
