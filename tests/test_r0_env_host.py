"""CPU: the host side of the per-env Fried parameter (aoenv_set_r0_env / BatchedAOEnv.set_r0_per_env).  The design rests on one
fact -- LayerTables.set_r0 gives an r0-invariant A and a B that goes as r0^(-5/6) -- which is pinned here, next to the sigma
formula, the argument handling of the Python layer and the refusals of the C ABI that need no device.  No GPU."""
import ctypes as C

import numpy as np
import pytest
import torch

from rlao_amd import _lib as L
from rlao_amd.calib import LayerTables
from rlao_amd.env import resolve_r0_per_env
from rlao_amd.wrappers import HistoryEnv, TimeDelayEnv, TorchWrapper

R0_TABLES = 0.13


def _sigma(r0_tables, r0):
    return (r0_tables / np.asarray(r0, dtype=np.float64)) ** (5.0 / 6)


def test_sigma_is_exactly_one_at_the_table_r0():
    for r in (0.13, 0.05, 0.2, 0.15, 1.0 / 3):
        assert _sigma(r, r) == 1.0
        assert pow(r / r, 5.0 / 6) == 1.0
    assert _sigma(0.13, 0.05) > 1.0 > _sigma(0.13, 0.2)
    np.testing.assert_allclose(_sigma(0.13, [0.08, 0.2]) ** 1.2, [0.13 / 0.08, 0.13 / 0.2], rtol=1e-14)


@pytest.mark.parametrize("N", [28, 52])
def test_A_does_not_depend_on_r0_and_B_scales_with_sigma(N):
    """The premise: B(r0) = sigma B(r0_tables) to the rounding of the host's Cholesky factorisation (1e-10 ..
    6e-9 of max |B|), A the same at every r0 (to 1.2e-12).  Bounds: 1e-8 and 1e-11."""
    t = LayerTables(N, N - 4, 3.2, 30.0)
    t.set_r0(R0_TABLES)
    A0, B0 = t.A.copy(), t.B.copy()
    for r in (0.05, 0.08, 0.2):
        t.set_r0(r)
        dB = np.abs(t.B - _sigma(R0_TABLES, r) * B0).max() / np.abs(B0).max()
        dA = np.abs(t.A - A0).max()
        print(f"N={N} r0={r}: |B - sigma B0| / max|B0| = {dB:.2e}, |A - A0| = {dA:.2e}")
        assert dB < 1e-8
        assert dA < 1e-11


def test_values_for_every_env_or_for_a_list_or_a_mask():
    full = resolve_r0_per_env([0.13, 0.08, 0.2, 0.05], None, 4, 0.13)
    assert full.dtype == np.float64 and full.tolist() == [0.13, 0.08, 0.2, 0.05]
    assert resolve_r0_per_env(torch.tensor([0.1, 0.2]), None, 2, 0.13).tolist() == pytest.approx([0.1, 0.2])
    # a list: the caller's order pairs values with ids; the others keep the uniform value, or the value they had
    assert resolve_r0_per_env([0.2, 0.1], [3, 1], 4, 0.13).tolist() == [0.13, 0.1, 0.13, 0.2]
    assert resolve_r0_per_env([0.2, 0.1], [3, 1], 4, full).tolist() == [0.13, 0.1, 0.2, 0.2]
    assert resolve_r0_per_env(0.3, [0, 2], 4, full).tolist() == [0.3, 0.08, 0.3, 0.05]
    # a mask: ascending
    assert resolve_r0_per_env([0.2, 0.1], np.array([False, True, False, True]), 4, 0.13).tolist() == [0.13, 0.2, 0.13, 0.1]
    assert resolve_r0_per_env([], [], 4, full).tolist() == full.tolist()
    # the result is the caller's to keep: not a view of `current`
    out = resolve_r0_per_env([0.3], [0], 4, full)
    assert full[0] == 0.13 and out is not full


@pytest.mark.parametrize("r0, ids, what", [
    ([0.1, 0.2, 0.3], None, "shape"), (0.1, None, "shape"), ([[0.1, 0.2, 0.3, 0.4]], None, "shape"),
    ([0.1, 0.2], [1], "one value per listed env"), ([0.1], [1, 2], "one value per listed env"),
    ([0.1, 0.0, 0.2, 0.3], None, "finite and positive"), ([0.1, -0.2, 0.2, 0.3], None, "finite and positive"),
    ([0.1, np.nan, 0.2, 0.3], None, "finite and positive"), ([0.1, np.inf, 0.2, 0.3], None, "finite and positive"),
    (np.nan, [1], "finite and positive"), (0.0, [1, 2], "finite and positive"),
    ([0.1], [4], "outside"), ([0.1, 0.2], [1, 1], "twice"), ([0.1], [True, False], "length"), (["a", "b", "c", "d"], None, "numeric"),
])
def test_bad_values_raise(r0, ids, what):
    with pytest.raises(ValueError, match=what):
        resolve_r0_per_env(r0, ids, 4, 0.13)


def test_the_library_refuses_a_null_env():
    lib = L.load()
    r0 = np.array([0.1, 0.2])
    assert lib.aoenv_set_r0_env(None, r0.ctypes.data_as(C.c_void_p), 0.13, None) != 0
    assert b"null" in lib.aoenv_last_error()
    assert lib.aoenv_set_r0_env(None, None, 0.13, None) != 0
    assert lib.aoenv_get_r0_env(None, r0.ctypes.data_as(C.c_void_p)) != 0
    assert L.ABI_VERSION == 7 and lib.aoenv_abi_version() == 7


class _StubEnv:
    """The batched env's surface as far as the wrappers use it: records what reaches it."""
    output = "torch"
    nActuator = 3
    n_envs = 4
    device = "cpu"
    tdtype = torch.float64

    def __init__(self):
        self.r0_calls, self.resets = [], []
        self.param = type("P", (), {"nLoop": 50})()

    def set_r0_per_env(self, r0, env_ids=None):
        self.r0_calls.append((r0, env_ids))

    def reset_envs(self, env_ids, seed=None, r0=None):
        self.resets.append((list(env_ids), seed, r0))
        return torch.zeros((len(env_ids), 3, 3), dtype=torch.float64)

    def step(self, i, action):
        return torch.zeros((4, 3, 3)), None, torch.zeros(4), torch.ones(4), torch.zeros(4, dtype=torch.bool), {}


@pytest.mark.parametrize("wrap", [TorchWrapper, lambda e: TimeDelayEnv(e, 2), lambda e: HistoryEnv(e, n_history=3, delay=2)])
def test_wrappers_forward_the_per_env_r0(wrap):
    inner = _StubEnv()
    env = wrap(inner)
    assert "set_r0_per_env" in type(env).__dict__                   # a method of the wrapper, not attribute forwarding
    env.set_r0_per_env([0.1, 0.2, 0.3, 0.4])
    env.set_r0_per_env([0.2], env_ids=[3])
    assert inner.r0_calls == [([0.1, 0.2, 0.3, 0.4], None), ([0.2], [3])]
    env.reset_envs([2, 0], seed=5, r0=[0.2, 0.1])
    env.reset_envs([1], seed=6)
    assert inner.resets == [([2, 0], 5, [0.2, 0.1]), ([1], 6, None)]
