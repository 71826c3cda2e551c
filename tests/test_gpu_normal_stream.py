"""GPU: the one-pass Gaussian draw (mt_normal_body, ring_device.hpp) is numpy.random.RandomState(seed).normal -- the values
through aoenv_test_normal (k_mt_normal<double>), the stored stream (state block and word position) through the checkpoint of a
small env whose crossings are counted on the host clock.

The (seed, n, calls) tuples move the start position of a request through every residue of the 156 attempts of a state block and
make a request span from a fraction of a block (n = 2, 6) over the two or three blocks of a C2 ring (n = 500) to the ~99 blocks
of a whole screen at reset (n = 30 752: the draw goes round many times).  The bound is that of
test_gpu_parity.test_mt19937_legacy_normal_stream: 4e-15 = a few ulp of the largest deviate (the device's log / sqrt against
libm's); a stream that is one word off gives errors of order 1.

Measured on MI355X: 4.4e-16 on every tuple.  The draw before the one-pass form formed r2 = x1^2 + x2^2 with one fused multiply-add,
which NumPy does not: it passed the four tuples of test_gpu_parity (3.9e-15 at the worst) but gave 1.1e-14 on (3, 6, 3000) and
5.6e-15 on (9, 30752, 2) -- an ulp of r2 is magnified by 1 / (1 - r2) in log(r2) -- so mt_polar is compiled without contraction."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SMALL = dict(diameter=3.2, nSubaperture=8, nPixelPerSubap=6, r0=0.13, L0=30.0, windSpeed=[15.0], windDirection=[72.0],
             fractionalR0=[1.0], altitude=[0.0], nModes=20, nLoop=64)


@pytest.mark.parametrize("seed,n,calls", [(3, 6, 3000), (11, 250, 60), (17, 500, 40), (5, 1248, 8), (9, 30752, 2),
                                          (2**32 - 1, 2, 2000)])
def test_normal_stream_matches_numpy(seed, n, calls):
    from rlao_amd import _lib
    lib = _lib.load()
    out = np.zeros(n * calls)
    rc = lib.aoenv_test_normal(0, seed, n, calls, out.ctypes.data_as(C.c_void_p))
    assert rc == 0, lib.aoenv_last_error()
    rs = np.random.RandomState(seed)
    want = np.concatenate([rs.normal(size=n) for _ in range(calls)])
    err = float(np.abs(out - want).max())
    print(f"seed {seed} n {n} calls {calls}: max |device - numpy| = {err:.3e}")
    np.testing.assert_allclose(out, want, rtol=0, atol=4e-15)


@pytest.mark.parametrize("lookahead", [1, 0])
def test_stored_stream_position_matches_numpy(lookahead):
    """aoenv_test_normal does not return the stream, so the stored state is read where the library exposes it: AOENV_B_MT_STATE
    of a SMALL env (624 state words + the word position per env).  Start: the checkpoint after the episode reset, loaded into a
    RandomState.  After k crossings -- counted from the host clock: a step crossed iff the sub-pixel accumulator did not simply
    grow by the wind ratio -- the device's block and position must be NumPy's after k calls of normal(size=n_outer), with the
    draw-ahead of the ring pipeline (the out-of-place form: committed at the next crossing) and without it."""
    from rlao_amd import _lib as L
    from rlao_amd.env import BatchedAOEnv
    n_env, steps = 3, 40
    env = BatchedAOEnv(n_envs=n_env, device=0, dtype="f32")
    env.set_params(SMALL, camera="ideal", wfs_type="shackhartmann")
    L.check(env._shard.lib.aoenv_set_option(env._shard.h, L.OPT_RING_LOOKAHEAD, lookahead))
    env.generate_new_phase_screen(23)
    env.dm.coefs = 0
    env.measure()
    obs = env.reset_soft()
    mt0 = env.get_state()["mt"]                                 # [1][n_env][625]
    n_outer = env._atm_tables.n_outer
    ratio = env._atm_tables.wind_ratio(env.param.windSpeed, env.param.windDirection, env.param.samplingTime)
    streams = []
    for e in range(n_env):
        rs = np.random.RandomState(0)
        rs.set_state(("MT19937", mt0[0, e, :624], int(mt0[0, e, 624]), 0, 0.0))
        streams.append(rs)
    crossings, checked = 0, 0
    for i in range(steps):
        before = env._shard.get_buff(1)
        obs = env.step(i, 0.5 * obs)[0]
        after = env._shard.get_buff(1)
        if np.abs(after - (before + ratio)).max() > 0.5:
            crossings += 1
            for rs in streams:
                rs.normal(size=n_outer)
        if i % 5 == 4 or i == steps - 1:
            mt = env.get_state()["mt"]
            for e, rs in enumerate(streams):
                _, key, pos, has_gauss, _ = rs.get_state()
                assert has_gauss == 0
                assert int(mt[0, e, 624]) == pos, (i, e, crossings, int(mt[0, e, 624]), pos)
                np.testing.assert_array_equal(mt[0, e, :624], key)
            checked += 1
    env.close()
    assert crossings >= 12 and checked >= 8, (crossings, checked)     # 0.45 px per frame over 40 steps
