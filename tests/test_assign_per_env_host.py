"""rlao_amd.env.assign_per_env / as_float64: the rule every per-env setter shares, over the forms of ``env_ids`` and of the value
(pure host code)."""
import numpy as np
import pytest
import torch

from rlao_amd.env import as_float64, assign_per_env

N_ = 4
ENV_IDS = {                                                         # name: (env_ids, the rows written, in the order of the value's rows)
    "none": (None, [0, 1, 2, 3]),
    "unsorted list": ([3, 1], [3, 1]),
    "mask": (np.array([True, False, True, True]), [0, 2, 3]),       # ascending
    "range": (range(1, 3), [1, 2]),
    "tensor": (torch.tensor([2, 0]), [2, 0]),
}
TAILS = [(), (3,)]


def _current(tail):
    return 100.0 + np.arange(N_ * int(np.prod(tail, dtype=int)), dtype=np.float64).reshape((N_,) + tail)


def _rows(k, tail):
    """k distinct rows: row j holds values starting at 10 (j + 1)."""
    return np.stack([10.0 * (j + 1) + np.arange(int(np.prod(tail, dtype=int)), dtype=np.float64).reshape(tail) for j in range(k)])


@pytest.mark.parametrize("tail", TAILS, ids=["tail()", "tail(3,)"])
@pytest.mark.parametrize("ids", list(ENV_IDS))
def test_row_k_of_the_value_goes_to_env_ids_k(ids, tail):
    env_ids, rows = ENV_IDS[ids]
    cur = _current(tail)
    before = cur.copy()
    value = _rows(len(rows), tail)
    for v in (value, value.tolist(), torch.tensor(value)):
        full = assign_per_env(v, env_ids, N_, cur, "thing", tail=tail)
        assert full.shape == (N_,) + tail and full.dtype == np.float64 and full.flags["C_CONTIGUOUS"]
        for k, e in enumerate(rows):                                # the caller's order, not the k-th smallest id
            assert np.array_equal(full[e], value[k]), (ids, k, e)
        for e in set(range(N_)) - set(rows):
            assert np.array_equal(full[e], before[e])               # the others keep theirs
        assert np.array_equal(cur, before) and not np.shares_memory(full, cur)     # `current` is not written


@pytest.mark.parametrize("tail", TAILS, ids=["tail()", "tail(3,)"])
@pytest.mark.parametrize("ids", list(ENV_IDS))
def test_a_scalar_goes_to_every_written_env(ids, tail):
    env_ids, rows = ENV_IDS[ids]
    cur = _current(tail)
    full = assign_per_env(0.25, env_ids, N_, cur, "thing", tail=tail)
    assert full.shape == (N_,) + tail
    for e in range(N_):
        assert (full[e] == 0.25).all() if e in rows else np.array_equal(full[e], cur[e])
    none_yet = assign_per_env(0.25, env_ids, N_, None, "thing", tail=tail)          # nothing in force: zeros
    assert all((none_yet[e] == (0.25 if e in rows else 0.0)).all() for e in range(N_))
    with pytest.raises(ValueError, match="thing must"):
        assign_per_env(0.25, env_ids, N_, cur, "thing", tail=tail, scalar=False)


@pytest.mark.parametrize("tail", TAILS, ids=["tail()", "tail(3,)"])
@pytest.mark.parametrize("ids", list(ENV_IDS))
def test_bad_values_raise_with_the_name_and_write_nothing(ids, tail):
    env_ids, rows = ENV_IDS[ids]
    cur = _current(tail)
    before = cur.copy()
    k = len(rows)
    nan_rows = _rows(k, tail)
    nan_rows[-1] = np.nan
    for bad, what in ((_rows(k + 1, tail), "thing must .*shape"), (_rows(k, tail)[..., None], "thing must .*shape"),
                      (np.nan, "thing must be finite"), (nan_rows, "thing must be finite"), (np.inf, "thing must be finite"),
                      ("abc", "thing must be numeric"), ([object()] * k, "thing must be numeric")):
        with pytest.raises(ValueError, match=what):
            assign_per_env(bad, env_ids, N_, cur, "thing", tail=tail)
    assert np.array_equal(cur, before)
    assert np.isnan(assign_per_env(np.nan, env_ids, N_, cur, "thing", tail=tail, finite=False)[rows[0]]).all()   # the caller checks


def test_a_shared_row_a_free_dimension_and_the_tail_in_force():
    cur = _current((3,))
    row = np.array([1.0, 2.0, 3.0])
    full = assign_per_env(row, [2, 0], N_, cur, "gains", tail=(3,), row=True)
    assert np.array_equal(full[2], row) and np.array_equal(full[0], row) and np.array_equal(full[[1, 3]], cur[[1, 3]])
    with pytest.raises(ValueError, match="gains must"):
        assign_per_env(row, [2, 0], N_, cur, "gains", tail=(3,))    # not unless the caller allows it
    shared = assign_per_env(5.0, [1], N_, row, "gains", tail=(3,))  # a `current` of one row: every env's
    assert np.array_equal(shared[0], row) and (shared[1] == 5.0).all()
    free = assign_per_env(np.ones((2, 5)), None, N_, None, "amp", tail=(2, None), scalar=False, row=True)
    assert free.shape == (N_, 2, 5) and (free == 1.0).all()
    with pytest.raises(ValueError, match="amp must have shape"):
        assign_per_env(np.ones((3, 5)), None, N_, None, "amp", tail=(2, None), scalar=False, row=True)
    with pytest.raises(ValueError, match="in force"):
        assign_per_env(np.ones((2, 5)), [1], N_, np.zeros((N_, 2, 4)), "amp", tail=(2, None), scalar=False, row=True)
    with pytest.raises(ValueError, match="in force"):
        assign_per_env(0.5, [1], N_, np.zeros((N_, 2)), "gains", tail=(3,))


def test_bad_env_ids_are_normalize_env_ids_refusals():
    for bad, what in (([4], "outside"), ([1, 1], "twice"), ([True, False], "length"), ([0.5], "integers")):
        with pytest.raises(ValueError, match=what):
            assign_per_env(1.0, bad, N_, np.zeros(N_), "thing")


def test_coercion():
    t = torch.tensor([1.5, 2.5], dtype=torch.float32, requires_grad=True)
    a = as_float64(t, "x")
    assert a.dtype == np.float64 and a.tolist() == [1.5, 2.5]
    assert as_float64(np.float32(0.2), "x") == np.float64(np.float32(0.2)) and as_float64(3, "x").shape == ()
    b = np.arange(3.0)
    assert as_float64(b, "x") is b                                  # float64 already: no copy
    for bad in ("abc", [1.0, "b"], {"a": 1}, [[1.0], [2.0, 3.0]]):
        with pytest.raises(ValueError, match="quantity must be numeric"):
            as_float64(bad, "quantity")
