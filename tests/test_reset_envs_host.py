"""CPU: the host side of the partial reset (BatchedAOEnv.reset_envs) -- the helper that normalises the env list, and the wrappers'
forwarding and row clearing against a stub env.  No GPU."""
import numpy as np
import pytest
import torch

from rlao_amd.env import normalize_env_ids
from rlao_amd.wrappers import HistoryEnv, TimeDelayEnv, TorchWrapper


def test_ids_from_lists_arrays_tensors_ranges_and_masks():
    for given in ([4, 1], (4, 1), np.array([4, 1]), np.array([4, 1], dtype=np.uint8), torch.tensor([4, 1]),
                  torch.tensor([4, 1], dtype=torch.int32)):
        ids = normalize_env_ids(given, 6)
        assert ids.dtype == np.int32 and ids.tolist() == [1, 4]
    assert normalize_env_ids(range(3), 3).tolist() == [0, 1, 2]
    assert normalize_env_ids([5], 6).tolist() == [5] and normalize_env_ids([0], 1).tolist() == [0]
    for mask in ([False, True, False, False, True, False], np.array([0, 1, 0, 0, 1, 0], dtype=bool),
                 torch.tensor([False, True, False, False, True, False])):
        ids = normalize_env_ids(mask, 6)
        assert ids.dtype == np.int32 and ids.tolist() == [1, 4]
    assert normalize_env_ids(np.zeros(6, dtype=bool), 6).size == 0
    assert normalize_env_ids(np.ones(3, dtype=bool), 3).tolist() == [0, 1, 2]
    # the caller's order, to pair per-env seeds and returned rows with the ids
    ids, given = normalize_env_ids([4, 1, 2], 6, return_order=True)
    assert ids.tolist() == [1, 2, 4] and given.tolist() == [4, 1, 2] and given.dtype == np.int32


def test_the_empty_list_is_a_list():
    for given in ([], (), np.zeros(0, dtype=np.int64), np.zeros(0), torch.zeros(0, dtype=torch.long), range(0)):
        ids = normalize_env_ids(given, 4)
        assert ids.dtype == np.int32 and ids.shape == (0,)


@pytest.mark.parametrize("given, n, what", [
    ([6], 6, "outside"), ([-1], 6, "outside"), ([0, 7, 1], 6, "outside"), (torch.tensor([2, 9]), 6, "outside"),
    ([1, 4, 1], 6, "twice"), (np.array([3, 3]), 6, "twice"),
    ([True, False], 6, "length"), (np.ones(7, dtype=bool), 6, "length"), (np.zeros(0, dtype=bool), 6, "length"),
    ([[1, 2]], 6, "1-D"), (3, 6, "1-D"), (np.zeros((2, 3), dtype=bool), 6, "1-D"), (torch.zeros((1, 1), dtype=torch.long), 6, "1-D"),
    ([1.0, 2.0], 6, "integers"), (["a"], 6, "integers"),
])
def test_bad_ids_raise(given, n, what):
    with pytest.raises(ValueError, match=what):
        normalize_env_ids(given, n)


class _StubEnv:
    """The batched env's surface as far as the wrappers use it, on the CPU: obs of env e at call c is 100 c + e everywhere."""
    output = "torch"
    nActuator = 3
    n_envs = 4
    device = "cpu"
    tdtype = torch.float64

    def __init__(self):
        self.seen, self.resets, self.calls = [], [], 0
        self.param = type("P", (), {"nLoop": 50})()

    def _obs(self):
        self.calls += 1
        return (100.0 * self.calls + torch.arange(4, dtype=torch.float64)).reshape(4, 1, 1).expand(4, 3, 3).clone()

    def reset_soft(self):
        return self._obs()

    def step(self, i, action):
        self.seen.append((i, action.clone()))
        return self._obs(), None, torch.zeros(4), torch.ones(4), torch.zeros(4, dtype=torch.bool), {}

    def reset_envs(self, env_ids, seed=None):
        from rlao_amd.env import normalize_env_ids as norm
        given = norm(env_ids, self.n_envs, return_order=True)[1]
        self.resets.append((given.tolist(), seed))
        return self._obs()[torch.as_tensor(given.astype(np.int64))]


def test_torch_wrapper_forwards_reset_envs():
    inner = _StubEnv()
    env = TorchWrapper(inner)
    obs = env.reset_envs([2, 0], seed=5)
    assert inner.resets == [([2, 0], 5)]
    assert obs.dtype == torch.float32 and obs.shape == (2, 3, 3) and obs[:, 0, 0].tolist() == [102.0, 100.0]
    env.reset_envs(torch.tensor([False, True, False, False]))
    assert inner.resets[-1] == ([1], None)


def test_time_delay_env_clears_the_rows_of_the_listed_envs():
    inner = _StubEnv()
    env = TimeDelayEnv(inner, 2)
    env.reset_soft()
    acts = [torch.full((4, 3, 3), float(i + 1), dtype=torch.float64) for i in range(3)]
    for i, a in enumerate(acts):
        env.step(i, a)                                              # the FIFO now holds actions 2 and 3
    obs = env.reset_envs([3, 1], seed=9)
    assert inner.resets == [([3, 1], 9)] and obs.shape == (2, 3, 3) and obs[:, 0, 0].tolist() == [503.0, 501.0]
    assert all(bool((a == float(i + 1)).all()) for i, a in enumerate(acts))      # the caller's own tensors are not written to
    env.step(3, torch.full((4, 3, 3), 4.0, dtype=torch.float64))
    env.step(4, torch.full((4, 3, 3), 5.0, dtype=torch.float64))
    env.step(5, torch.full((4, 3, 3), 6.0, dtype=torch.float64))
    got = [a[:, 0, 0].tolist() for _, a in inner.seen[3:]]
    assert got == [[2.0, 0.0, 2.0, 0.0], [3.0, 0.0, 3.0, 0.0], [4.0, 4.0, 4.0, 4.0]]
    with pytest.raises(ValueError):
        env.reset_envs([1, 1])
    assert len(inner.resets) == 1                                   # refused before the env was touched


def test_history_env_restarts_the_rows_of_the_listed_envs():
    inner = _StubEnv()
    env = HistoryEnv(inner, n_history=3, delay=2)
    for k in range(4):
        env.step(torch.full((4, 3, 3), float(k + 1)))
    before = env.obs_history.clone()
    assert before[:, :, 0, 0].tolist() == [[400.0 + e, 300.0 + e, 200.0 + e] for e in range(4)]
    win = env.reset_envs([2, 0], seed=3)
    assert inner.resets == [([2, 0], 3)]
    assert win.shape == (2, 3, 3, 3) and win.dtype == torch.float32
    assert win[:, :, 0, 0].tolist() == [[502.0, 0.0, 0.0], [500.0, 0.0, 0.0]]           # as reset() starts a history: the new obs, then nothing
    now = env.obs_history
    assert torch.equal(now[[1, 3]], before[[1, 3]])                 # the other envs' histories go on
    assert torch.equal(now[[2, 0]], win)
    # fresh tensors, not views of the ring buffer: the next push does not reach them
    kept = win.clone()
    env.step(torch.full((4, 3, 3), 5.0))
    assert torch.equal(win, kept)
    assert env.obs_history[:, :, 0, 0].tolist() == [[600.0, 500.0, 0.0], [601.0, 401.0, 301.0], [602.0, 502.0, 0.0], [603.0, 403.0, 303.0]]
    # the delayed action of a listed env is cleared (delay 2: one action waits), the others' is kept; the frame counter goes on
    i, a = inner.seen[-1]
    assert i == 4 and a[:, 0, 0].tolist() == [0.0, 4.0, 0.0, 4.0]
    # a mask, and the empty list
    assert env.reset_envs(torch.tensor([False, False, False, True])).shape == (1, 3, 3, 3)
    assert env.reset_envs([]).shape == (0, 3, 3, 3)
    assert inner.resets[-1][0] == []
