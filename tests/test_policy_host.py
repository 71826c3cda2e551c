"""CPU: the host side of the on-device policy (aoenv_set_policy / aoenv_policy_forward / aoenv_run_policy_rollout): the ctypes
mirror of AoPolicy against the compiled header, the float64 restatement of tests/_policy_ref.py against a torch module of the
reference's shape, the weight extraction of rlao_amd.env.policy_arrays, and the history roll against the literal lines of
MAIN/PO4AO/mbrl.py:80-81."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import _policy_ref as P

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "aoenv.h")


@pytest.fixture(scope="module")
def built_lib():
    sys.path.insert(0, REPO)
    import __graft_entry__ as g
    g.build()
    from rlao_amd import _lib
    return _lib


def test_policy_struct_matches_header_and_abi_is_7(built_lib, tmp_path):
    L = built_lib
    prog = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', "int main(void){",
            'printf("size %zu\\n", sizeof(AoPolicy));']
    prog += [f'printf("{f[0]} %zu\\n", offsetof(AoPolicy, {f[0]}));' for f in L.AoPolicy._fields_]
    prog += ['printf("abi %d\\n", (int)AOENV_ABI_VERSION);', "return 0;}"]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(prog))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-o", str(exe), str(src)], check=True)
    out = dict(l.split() for l in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(out["size"]) == C.sizeof(L.AoPolicy)
    for f in L.AoPolicy._fields_:
        assert int(out[f[0]]) == getattr(L.AoPolicy, f[0]).offset, f[0]
    assert int(out["abi"]) == L.ABI_VERSION == 7
    lib = L.load()
    assert lib.aoenv_abi_version() == 7
    for name in ("aoenv_set_policy", "aoenv_policy_forward", "aoenv_run_policy_rollout"):
        assert hasattr(lib, name) and name in L.EXPORTS
    # no env: every entry point refuses a null handle
    assert lib.aoenv_set_policy(None, None, None) != 0
    assert lib.aoenv_policy_forward(None, None, None, None, None, None) != 0
    assert lib.aoenv_run_policy_rollout(None, None, None, None, None, None, None, None, None, None) != 0


def _inputs(n, H, a, seed):
    rng = np.random.RandomState(seed)
    return rng.normal(0, 1, (n, a, a)), rng.normal(0, 1, (n, H - 1, a, a)), rng.normal(0, 1, (n, H - 1, a, a))


@pytest.mark.parametrize("H,n_filt,proj", [(1, 16, False), (3, 24, True), (5, 8, True)])
def test_restatement_equals_the_torch_module_in_float64(H, n_filt, proj):
    a, n = 7, 3
    rng = np.random.RandomState(3)
    act_idx = np.sort(rng.choice(a * a, 37, replace=False))
    xv, yv = np.divmod(act_idx, a)
    F = rng.normal(0, 0.3, (37, 37)) if proj else None
    w = P.make_weights(H, n_filt, seed=11, scale=(1.0, 2.0, 3.0))
    obs, po, pa = _inputs(n, H, a, 5)
    ours = P.policy(w, obs, po, pa, act_idx, F)
    theirs = P.torch_eval(w, obs, po, pa, xv, yv, F)
    inner = np.abs(P.network(w, obs, po, pa).reshape(n, -1)[:, act_idx])
    assert 0.1 < (inner < 1).mean() < 0.9                           # the clamp takes part
    assert np.abs(ours - theirs).max() <= 1e-12
    mask = np.ones(a * a, dtype=bool)
    mask[act_idx] = False
    assert (ours.reshape(n, -1)[:, mask] == 0).all()


def test_weight_extraction_from_module_sequential_and_dict():
    import torch
    from rlao_amd.env import policy_arrays
    w = P.make_weights(3, 16, seed=2)
    w["negative_slope"] = 0.02
    mod = P.torch_module(w, np.arange(3), np.arange(3))
    got = [policy_arrays(mod), policy_arrays(mod.net), policy_arrays({k: w[k] for k in ("w1", "b1", "w2", "b2", "w3", "b3", "negative_slope")}),
           policy_arrays(dict(mod.state_dict(), negative_slope=0.02)), policy_arrays(dict(mod.net.state_dict(), negative_slope=0.02))]
    for g in got:
        assert g["n_history"] == 3 and g["n_filt"] == 16 and g["negative_slope"] == 0.02
        for k in ("w1", "b1", "w2", "b2", "w3", "b3"):
            assert g[k].dtype == np.float64 and g[k].flags["C_CONTIGUOUS"] and np.array_equal(g[k], w[k]), k
    # a float32 module: the arrays are the float32 values, widened
    m32 = P.torch_module(w, np.arange(3), np.arange(3), dtype=torch.float32)
    assert np.array_equal(policy_arrays(m32)["w2"], w["w2"].astype(np.float32).astype(np.float64))
    with pytest.raises(ValueError):
        policy_arrays(dict(w, w2=w["w2"][:, :-1]))
    with pytest.raises(ValueError):
        policy_arrays(dict(w, w1=w["w1"][:, :-1]))                  # an even channel count is no 2H - 1
    with pytest.raises(ValueError):
        policy_arrays(mod.net[:3])


@pytest.mark.parametrize("n_steps", [0, 1, 2, 3, 4, 9])
def test_history_roll_equals_the_trainer_loop(n_steps):
    """H = 4: n_steps below, at and above H - 1 = 3.  The literal lines of mbrl.py:80-81 on torch tensors against the index
    arithmetic of the library (restated in _policy_ref.window / roll), and every step's window on the way."""
    import torch
    H, n, a = 4, 2, 3
    rng = np.random.RandomState(n_steps)
    past0 = rng.normal(0, 1, (n, H - 1, a, a))
    traj = rng.normal(0, 1, (max(n_steps, 1), n, a, a))
    past = torch.as_tensor(past0)
    for k in range(n_steps):
        assert np.array_equal(P.window(past0, traj, k), past.numpy()), k
        new = torch.as_tensor(traj[k])
        past = torch.cat([past[:, 1:, :, :], new.unsqueeze(1)], dim=1)          # mbrl.py:80 with a leading env dimension
    assert np.array_equal(P.roll(past0, traj, n_steps), past.numpy())
