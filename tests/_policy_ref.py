"""Float64 restatement of the PO4AO policy function (ConvPolicy, MAIN/PO4AO/conv_models_simple.py:56-111) and of the history roll
of the trainer loop (MAIN/PO4AO/mbrl.py:80-81), for tests/test_policy_host.py, tests/test_gpu_policy.py and
tests/test_gpu_policy_sweep.py.  NumPy only; the torch module of the same shape (``RefPolicy``) is the second opinion the
restatement is pinned against on the CPU and the float32 yardstick of the GPU tolerances.  Further down: the host model of the MFMA
convolution (rlao_amd/csrc/policy.hpp) restated, the stand-alone driver that answers for the library's own, the cases of the
sweep and its exact integer data."""
import os
import shutil
import subprocess

import numpy as np


def conv3x3(x, w, b):
    """x [N, C, a, a], w [F, C, 3, 3], b [F] -> [N, F, a, a]: cross-correlation with padding 1 (torch.nn.Conv2d)"""
    a = x.shape[-1]
    xp = np.pad(x, ((0, 0), (0, 0), (1, 1), (1, 1)))
    out = np.zeros((x.shape[0], w.shape[0], a, a), dtype=np.float64)
    for ky in range(3):
        for kx in range(3):
            out += np.einsum("ncyx,fc->nfyx", xp[:, :, ky:ky + a, kx:kx + a], w[:, :, ky, kx])
    return out + b[None, :, None, None]


def leaky(x, slope):
    return np.where(x > 0, x, x * slope)


def network(w, obs, past_obs, past_act):
    """net(cat([obs, past_obs, past_act])) before the clamp: [N, a, a].  Windows oldest first, [N, H-1, a, a]."""
    x = np.concatenate([obs[:, None], past_obs, past_act], axis=1).astype(np.float64)
    h = leaky(conv3x3(x, w["w1"], w["b1"]), w["negative_slope"])
    h = leaky(conv3x3(h, w["w2"], w["b2"]), w["negative_slope"])
    return conv3x3(h, w["w3"], w["b3"])[:, 0]


def policy(w, obs, past_obs, past_act, act_idx, F=None, clamp=1.0):
    """The action images [N, a, a]: vec_to_img(F @ clamp(net(x))[valid]), zero off the valid actuators.  act_idx: flat indices of
    the valid actuators; F [A, A] or None."""
    out = np.clip(network(w, obs, past_obs, past_act), -clamp, clamp)
    n, a = out.shape[0], out.shape[-1]
    vec = out.reshape(n, -1)[:, act_idx]
    if F is not None:
        vec = vec @ np.asarray(F, dtype=np.float64).T
    img = np.zeros((n, a * a), dtype=np.float64)
    img[:, act_idx] = vec
    return img.reshape(n, a, a)


def window(past, traj, k):
    """The window [N, H-1, a, a] in front of step k by the library's index arithmetic: channel c is trajectory slot k - (H-1) + c
    when that is >= 0, and row k + c of the caller's window otherwise.  past [N, H-1, a, a], traj [>= k, N, a, a]."""
    hm1 = past.shape[1]
    rows = []
    for c in range(hm1):
        s = k - hm1 + c
        rows.append(traj[s] if s >= 0 else past[:, k + c])
    return np.stack(rows, axis=1) if rows else past.copy()


def roll(past, traj, n_steps):
    """What n_steps iterations of mbrl.py:80-81 leave of `past` when traj[k] is appended in step k"""
    return window(past, traj, n_steps)


def make_weights(H, n_filt, seed, scale=(1.0, 1.0, 1.0), bias=0.05):
    """Seeded normal weights in torch's Conv2d layout, std = scale_l / sqrt(fan-in) per layer"""
    rng = np.random.RandomState(seed)
    c1 = 2 * H - 1
    return dict(w1=rng.normal(0, scale[0] / np.sqrt(9 * c1), (n_filt, c1, 3, 3)), b1=rng.normal(0, bias, n_filt),
                w2=rng.normal(0, scale[1] / np.sqrt(9 * n_filt), (n_filt, n_filt, 3, 3)), b2=rng.normal(0, bias, n_filt),
                w3=rng.normal(0, scale[2] / np.sqrt(9 * n_filt), (1, n_filt, 3, 3)), b3=rng.normal(0, bias, 1),
                negative_slope=0.01, n_history=H, n_filt=n_filt)


def torch_module(w, xvalid, yvalid, F=None, clamp=1.0, dtype=None):
    """A torch module of the reference's shape (``.net`` = Conv2d, LeakyReLU, Conv2d, LeakyReLU, Conv2d; clamp; F; scatter) carrying
    the weights ``w``; ``forward(state [N, a, a], history [N, 2(H-1), a, a])`` as ConvPolicy.forward."""
    import torch
    import torch.nn as nn
    dtype = dtype or torch.float64

    class RefPolicy(nn.Module):
        def __init__(self):
            super().__init__()
            c1, f = w["w1"].shape[1], w["w1"].shape[0]
            self.net = nn.Sequential(nn.Conv2d(c1, f, 3, padding=1), nn.LeakyReLU(w["negative_slope"]), nn.Conv2d(f, f, 3, padding=1),
                                     nn.LeakyReLU(w["negative_slope"]), nn.Conv2d(f, 1, 3, padding=1)).to(dtype)
            with torch.no_grad():
                for i, n in ((0, "1"), (2, "2"), (4, "3")):
                    self.net[i].weight.copy_(torch.as_tensor(w["w" + n]))
                    self.net[i].bias.copy_(torch.as_tensor(w["b" + n]))
            self.F = None if F is None else torch.as_tensor(np.asarray(F)).to(dtype)

        def forward(self, state, history=None):
            feats = state.unsqueeze(1) if history is None else torch.cat([state.unsqueeze(1), history], dim=1)
            out = self.net(feats).clamp(-clamp, clamp)
            vec = out[:, 0, xvalid, yvalid]
            if self.F is not None:
                vec = torch.matmul(self.F.unsqueeze(0), vec.unsqueeze(2)).squeeze(-1)
            ret = torch.zeros_like(out[:, 0])
            ret[:, xvalid, yvalid] = vec
            return ret

    return RefPolicy().eval()


def torch_eval(w, obs, past_obs, past_act, xvalid, yvalid, F=None, clamp=1.0, dtype=None):
    """The torch-CPU evaluation of the module in `dtype` (float64 default), as a float64 array"""
    import torch
    dtype = dtype or torch.float64
    m = torch_module(w, xvalid, yvalid, F, clamp, dtype)
    t = lambda x: torch.as_tensor(np.asarray(x)).to(dtype)
    with torch.no_grad():
        hist = torch.cat([t(past_obs), t(past_act)], dim=1) if past_obs.shape[1] else None
        return m(t(obs), hist).double().numpy()


# ---- the host model of the MFMA convolution (rlao_amd/csrc/policy.hpp), restated ----------------------------------------------
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LDS_MAX = 160 * 1024                                                # kPolicyLdsMax
BAND_PIXELS = 256                                                   # kPolicyBandPixels


def ksteps(c_in):
    return -(-9 * c_in // 4)


def conv_lds_rows(a, c_in, rows):
    """bytes: the padded band [C][rows + 2][a + 2], the tap offsets [4 ksteps], 8-byte aligned the source pointers [C]"""
    words = c_in * (rows + 2) * (a + 2) + 4 * ksteps(c_in)
    return (words + (words & 1)) * 4 + c_in * 8


def bands(a, c_in):
    """(rows, bands) of policy_bands: the tallest band of at most 256 pixels of which two fit a CU's LDS -- where not even one
    row does, the tallest that fits at all -- and the rows then spread evenly"""
    r = max(1, min(a, BAND_PIXELS // a))
    limit = LDS_MAX // 2 if conv_lds_rows(a, c_in, 1) <= LDS_MAX // 2 else LDS_MAX
    while r > 1 and conv_lds_rows(a, c_in, r) > limit:
        r -= 1
    n = -(-a // r)
    return -(-a // n), n


def conv_lds(a, c_in):
    return conv_lds_rows(a, c_in, bands(a, c_in)[0])


def mfma_fits(a, c_in):
    return 2 <= a <= BAND_PIXELS and conv_lds(a, c_in) <= LDS_MAX


def band_rows(a, c_in):
    """the rows of every band, top to bottom (the last one may be shorter)"""
    rows, n = bands(a, c_in)
    return [min(rows, a - b * rows) for b in range(n)]


def wave_tiles(npx):
    """live 16-pixel tiles of the four waves of a band of npx pixels: wave w owns the tiles w, w + 4, .."""
    return [max(0, (-(-npx // 16) - w + 3) // 4) for w in range(4)]


# The policy sweep (tests/test_gpu_policy_sweep.py; the selection test of tests/test_policy_host.py): actuators across -> (H, n_filt)
SWEEP_CASES = {5: [(1, 16), (3, 48), (32, 128)], 9: [(2, 32), (6, 96), (32, 128)], 16: [(3, 16), (20, 64), (2, 48)],
               17: [(2, 32), (32, 64), (6, 96)], 21: [(3, 48), (32, 128)], 41: [(3, 16), (20, 64), (4, 128)],
               53: [(1, 16), (4, 128), (32, 64)]}


def build_driver(out_dir, sanitize=False):
    """Compiles tests/native/policy_driver.cpp for the host; None when there is no hipcc."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        return None
    exe = os.path.join(str(out_dir), "policy_driver" + ("_san" if sanitize else ""))
    flags = ["-O1", "-g", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-omit-frame-pointer"] if sanitize else ["-O2"]
    subprocess.run([hipcc, *flags, "-std=c++17", "-x", "hip", "--cuda-host-only", f"-I{REPO}/include", f"-I{REPO}/rlao_amd/csrc",
                    os.path.join(REPO, "tests", "native", "policy_driver.cpp"), "-o", exe], check=True, capture_output=True)
    return exe


def ask(exe, lines, env=None):
    """-> the driver's answer lines (one per request), its stderr"""
    r = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, env=env)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    return r.stdout.splitlines(), r.stderr


def host_plans(exe, pairs, env=None):
    """[(a, C)] -> int array [n, 6]: rows, bands, lds, lds of one row, fits, ksteps"""
    out, err = ask(exe, [f"plan {a} {c}" for a, c in pairs], env)
    return np.array([[int(v) for v in l.split()] for l in out], dtype=np.int64).reshape(len(pairs), 6), err


def host_select(exe, cases, env=None):
    """[(esz, path, F, a, C1)] -> list of bool"""
    out, err = ask(exe, ["select %d %d %d %d %d" % c for c in cases], env)
    return [l.strip() == "1" for l in out], err


def host_relayout(exe, w, env=None):
    """w [F][C][3][3] -> float32 [ksteps][F / 16][64]"""
    f, c = w.shape[:2]
    out, err = ask(exe, [f"relayout {f} {c}", " ".join(repr(float(v)) for v in w.ravel())], env)
    return np.array(out[0].split(), dtype=np.float64).astype(np.float32).reshape(ksteps(c), f // 16, 64), err


def host_channels(exe, H, k, E, e, env=None):
    """-> [(kind, index)] for c = 0 .. 2H - 2, kind in O, A (trajectory slot), PO, PA (window row)"""
    out, err = ask(exe, [f"channel {H} {k} {E} {e}"], env)
    t = out[0].split()
    return [(t[i], int(t[i + 1])) for i in range(0, len(t), 2)], err


# ---- exact data: integers whose every partial sum is a float32 -------------------------------------------------------------------
QUANTA = (1.0, 0.5, 0.25, 0.25)                                     # layer 1, 2, 3 and the projection at negative_slope = 0.5


def conv3x3_gemm(x, w, b):
    """conv3x3 as nine matrix products: another order of the same sum, so the same values wherever the sum is exact"""
    n, c, a = x.shape[0], x.shape[1], x.shape[-1]
    xp = np.pad(np.asarray(x, dtype=np.float64), ((0, 0), (0, 0), (1, 1), (1, 1)))
    out = np.zeros((n, w.shape[0], a * a))
    for ky in range(3):
        for kx in range(3):
            out += np.matmul(w[None, :, :, ky, kx], np.ascontiguousarray(xp[:, :, ky:ky + a, kx:kx + a]).reshape(n, c, a * a))
    return out.reshape(n, w.shape[0], a, a) + b[None, :, None, None]


def layers(w, obs, past_obs, past_act, conv=conv3x3_gemm):
    """-> (hidden 1, hidden 2 before the LeakyReLU, net before the clamp [N, a, a])"""
    x = np.concatenate([obs[:, None], past_obs, past_act], axis=1).astype(np.float64)
    p1 = conv(x, w["w1"], w["b1"])
    p2 = conv(leaky(p1, w["negative_slope"]), w["w2"], w["b2"])
    return p1, p2, conv(leaky(p2, w["negative_slope"]), w["w3"], w["b3"])[:, 0]


def _ternary_filters(rng, n_filt, c_in, nnz):
    """[F][C][3][3] in {-1, 0, 1}: every tap (ci, ky, kx) non-zero in some filter (tap t of a shuffled order goes to filter t % F),
    then every filter topped up to nnz non-zeros"""
    K = 9 * c_in
    w = np.zeros((n_filt, K))
    sign = lambda n: rng.choice([-1.0, 1.0], n)
    order = rng.permutation(K)
    w[np.arange(K) % n_filt, order] = sign(K)
    for f in range(n_filt):
        free = np.flatnonzero(w[f] == 0)
        more = nnz - (K - free.size)
        if more > 0:
            pick = rng.choice(free, min(more, free.size), replace=False)
            w[f, pick] = sign(pick.size)
    return w.reshape(n_filt, c_in, 3, 3)


def exact_weights(H, n_filt, seed, nnz=16):
    rng = np.random.RandomState(seed)
    c1 = 2 * H - 1
    bias = lambda n: rng.randint(-1, 2, n).astype(np.float64)
    return dict(w1=_ternary_filters(rng, n_filt, c1, nnz), b1=bias(n_filt), w2=_ternary_filters(rng, n_filt, n_filt, nnz), b2=bias(n_filt),
                w3=rng.choice([-1.0, 1.0], (1, n_filt, 3, 3)), b3=bias(1), negative_slope=0.5, n_history=H, n_filt=n_filt)


def exact_inputs(n, H, a, seed, amp=2):
    rng = np.random.RandomState(seed)
    return tuple(rng.randint(-amp, amp + 1, s).astype(np.float64) for s in ((n, a, a), (n, H - 1, a, a), (n, H - 1, a, a)))


def exact_factors(n_valid, seed, rank=4, nnz=8):
    """(Fr [rank, A], Fl [A, rank]) ternary, at most nnz non-zeros per row of Fr"""
    rng = np.random.RandomState(seed)
    fr = np.zeros((rank, n_valid))
    for k in range(rank):
        pick = rng.choice(n_valid, min(nnz, n_valid), replace=False)
        fr[k, pick] = rng.choice([-1.0, 1.0], pick.size)
    return fr, rng.randint(-1, 2, (n_valid, rank)).astype(np.float64)


def exact_case(w, x, act_idx, factors):
    """The float64 reference of an exact case and the conditions that make it one, asserted on the reference alone.
    -> dict(clamp, plain [N, a, a], proj [N, a, a], quanta: the largest sum of absolute values per stage, in its quanta)"""
    n = x[0].shape[0]
    for name in ("w1", "w2", "w3"):                                 # every tap of every layer is non-zero in some filter
        assert (np.abs(w[name]).reshape(w[name].shape[0], -1).max(axis=0) > 0).all(), name
    assert all(np.array_equal(t, np.round(t)) for t in x) and w["negative_slope"] == 0.5
    assert all(not np.array_equal(x[0][i], x[0][j]) for i in range(n) for j in range(i))   # the envs have different inputs
    p1, p2, net = layers(w, *x)
    for p, lo in ((p1, "hidden 1"), (p2, "hidden 2")):
        neg = float((p < 0).mean())
        assert 0.3 <= neg <= 0.7, (lo, neg)                         # both branches of the LeakyReLU take part
    inner = np.abs(net.reshape(n, -1)[:, act_idx])
    clamp = float(2.0 ** np.round(np.log2(np.median(inner))))       # the power of two nearest to the median
    unclamped = float((inner < clamp).mean())
    assert 0.1 <= unclamped <= 0.9, unclamped
    # the network of absolute values bounds every partial sum of every summation order
    aw = dict(w, **{k: np.abs(w[k]) for k in ("w1", "b1", "w2", "b2", "w3", "b3")})
    a1, a2, a3 = layers(aw, *(np.abs(t) for t in x))
    fr, fl = factors
    q_last = min(QUANTA[3], clamp)
    vec = np.minimum(a3.reshape(n, -1)[:, act_idx], clamp)
    aproj = (vec @ np.abs(fr).T) @ np.abs(fl).T
    quanta = [float(a1.max() / QUANTA[0]), float(a2.max() / QUANTA[1]), float(a3.max() / min(QUANTA[2], q_last)), float(aproj.max() / q_last)]
    assert max(quanta) < 2.0 ** 24, quanta
    for t, q in ((p1, QUANTA[0]), (p2, QUANTA[1]), (net, QUANTA[2])):
        assert np.array_equal(t / q, np.round(t / q))
    a = net.shape[-1]
    clamped = np.clip(net, -clamp, clamp).reshape(n, -1)[:, act_idx]
    plain, proj = np.zeros((n, a * a)), np.zeros((n, a * a))
    plain[:, act_idx] = clamped
    proj[:, act_idx] = (clamped @ fr.T) @ fl.T
    return dict(clamp=clamp, plain=plain.reshape(n, a, a), proj=proj.reshape(n, a, a), quanta=quanta, unclamped=unclamped)
