"""Float64 restatement of the PO4AO policy function (ConvPolicy, MAIN/PO4AO/conv_models_simple.py:56-111) and of the history roll
of the trainer loop (MAIN/PO4AO/mbrl.py:80-81), for tests/test_policy_host.py and tests/test_gpu_policy.py.  NumPy only; the torch
module of the same shape (``RefPolicy``) is the second opinion the restatement is pinned against on the CPU and the float32
yardstick of the GPU tolerances."""
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
