"""CPU: the LDS layout of a launch of two steps (step_pair_lds_layout, rlao_amd/csrc/step_kernel.hip) through the host hook
aoenv_test_step_lds.  A pair has words of its own for the first step's slopes (2 n_valid, rounded up to 4) and modal coefficients
(n_modes, rounded up to 4) behind everything a launch of one step has, whose total and offsets do not move; the headline's
geometry fits the workgroup's LDS; and a geometry whose single-step layout fits but whose pair layout does not is not pairable
(env_step_pairable: it runs one launch per step)."""
import ctypes as C

import numpy as np
import pytest


@pytest.fixture(scope="module")
def lds():
    from rlao_amd import _lib as L
    lib = L.load()

    def f(n_act, n_subap, n_valid, n_modes):
        out = np.zeros(6, dtype=np.int32)
        L.check(lib.aoenv_test_step_lds(n_act, n_subap, n_valid, n_modes, out.ctypes.data_as(C.c_void_p)))
        return dict(zip(("single", "pair", "at", "tm_at", "limit_bytes", "pairable"), (int(x) for x in out)))
    return f


def _up4(n):
    return (n + 3) & ~3


# (actuators across, lenslets across, valid lenslets, modes): the headline, the smallest loop of the suite, the second mirror at 12 x 12,
# odd counts that need the rounding
GEOMETRIES = [(21, 20, 316, 50), (5, 4, 12, 8), (26, 12, 112, 52), (26, 12, 112, 49), (9, 8, 52, 20), (17, 16, 194, 33)]


@pytest.mark.parametrize("geo", GEOMETRIES)
def test_pair_layout_is_the_single_layout_plus_its_own_words(lds, geo):
    n_act, n_subap, n_valid, n_modes = geo
    r = lds(*geo)
    extra = _up4(2 * n_valid) + _up4(n_modes)
    assert r["pair"] == r["single"] + extra
    assert r["at"] == r["single"] and r["tm_at"] == r["at"] + _up4(2 * n_valid)      # behind everything else, 16-byte aligned
    assert r["at"] % 4 == 0 and r["tm_at"] % 4 == 0
    assert r["limit_bytes"] == 160 * 1024 - 1024
    assert 4 * r["pair"] <= r["limit_bytes"] and r["pairable"] == 1


def test_headline_geometry_fits(lds):
    r = lds(21, 20, 316, 50)
    assert r["pair"] - r["single"] == 632 + 52                      # 2 736 bytes
    assert 4 * r["single"] == 152688 and 4 * r["pair"] == 155424 and r["pairable"] == 1


def test_a_layout_that_does_not_fit_is_not_pairable(lds):
    """Every (actuators, valid lenslets) at the edge: pairable exactly where the pair's total fits, and at least one geometry
    whose launch of one step fits while its pair does not"""
    edge = 0
    for n_act in range(21, 33):
        for n_valid in range(300, 337, 2):                           # (2 n_valid is a multiple of 4, at most 16 x 21 lenslets)
            r = lds(n_act, 21, n_valid, 52)
            fits_one, fits_two = 4 * r["single"] <= r["limit_bytes"], 4 * r["pair"] <= r["limit_bytes"]
            assert r["pairable"] == int(fits_two), (n_act, n_valid, r)
            edge += fits_one and not fits_two
    assert edge > 0
