#!/usr/bin/env python3
"""Host model of the bookkeeping of mt_normal_body (rlao_amd/csrc/ring_device.hpp): the ring of kMtSlots state blocks, how many
successors a pass produces, the attempts of a pass in stream order, the attempt that completes the request, and the block and word
position that are stored -- in NumPy, one attempt after the other, against numpy.random.RandomState itself.  No GPU.

It shows (a) that the scheme consumes exactly NumPy's words: after every request the deviates, the state block and the position are
RandomState's, and (b) how many passes a request takes, which is where DESIGN.md section 4.2 has its figures from: one pass for a
ring (n = 6 .. 500), 2 for n = 1248, 42 for the 30 752 normals of a screen.
    python scripts/draw_model.py            # the tuples of tests/test_gpu_normal_stream.py
"""
import numpy as np

N, SLOTS, TRY, LANE_TRY = 624, 4, 156, 512         # kMtN, kMtSlots, kMtTry, kMtLaneTry


def mix(a, b, far):
    y = (a & np.uint32(0x80000000)) | (b & np.uint32(0x7fffffff))
    return far ^ (y >> np.uint32(1)) ^ np.where(y & np.uint32(1), np.uint32(0x9908b0df), np.uint32(0))


def twist_next(s):
    """mt_twist_next: the successor block out of place, three phases"""
    n = np.zeros(N, np.uint32)
    t = np.arange(227)
    n[t] = mix(s[t], s[t + 1], s[t + 397])
    n[t + 227] = mix(s[t + 227], s[t + 228], n[t])
    t = np.arange(169)
    n[t + 454] = mix(s[t + 454], s[t + 455], n[t + 227])
    n[623] = mix(s[623:624], n[0:1], n[396:397])[0]
    return n


def temper(y):
    y = y ^ (y >> np.uint32(11))
    y = y ^ ((y << np.uint32(7)) & np.uint32(0x9d2c5680))
    y = y ^ ((y << np.uint32(15)) & np.uint32(0xefc60000))
    return y ^ (y >> np.uint32(18))


def polar(w):
    """mt_polar: one attempt from 4 words"""
    w = temper(w.astype(np.uint32))
    d1 = ((w[0] >> 5) * 67108864.0 + (w[1] >> 6)) / 9007199254740992.0
    d2 = ((w[2] >> 5) * 67108864.0 + (w[3] >> 6)) / 9007199254740992.0
    x1, x2 = 2.0 * d1 - 1.0, 2.0 * d2 - 1.0
    r2 = x1 * x1 + x2 * x2
    if not (r2 < 1.0 and r2 != 0.0):
        return False, 0.0, 0.0
    f = np.sqrt(-2.0 * np.log(r2) / r2)
    return True, f * x2, f * x1


def slot(b):
    return b - SLOTS if b >= SLOTS else b


def draw(state, pos, n_outer):
    """one request: (stored block, stored position, deviates, passes)"""
    s = np.zeros((SLOTS, N), np.uint32)
    s[0] = state
    got, cur, need, passes = 0, 0, n_outer // 2, 0
    out = np.zeros(n_outer)
    while got < need:
        passes += 1
        remaining = need - got
        avail0 = (N - pos) // 4
        want = remaining + remaining // 3 + 16 - avail0
        nt = 0 if want <= 0 else min((LANE_TRY - avail0) // TRY, (want + TRY - 1) // TRY)
        for j in range(nt):
            s[slot(cur + j + 1)] = twist_next(s[slot(cur + j)])
        n_try = avail0 + TRY * nt
        assert n_try <= LANE_TRY and nt <= SLOTS - 1
        incl, stop = 0, -1
        for a in range(n_try):
            a2 = a - avail0
            w = s[cur, pos + 4 * a: pos + 4 * a + 4] if a2 < 0 else s[slot(cur + 1 + a2 // TRY), 4 * (a2 % TRY): 4 * (a2 % TRY) + 4]
            ok, n0, n1 = polar(w)
            if ok:
                incl += 1
                if incl <= remaining:
                    j = got + incl - 1
                    out[2 * j], out[2 * j + 1] = n0, n1
                    if incl == remaining:
                        stop = a
        if stop >= 0:
            a2 = stop - avail0
            if a2 < 0:
                pos += 4 * (stop + 1)
            else:
                cur = slot(cur + 1 + a2 // TRY)
                pos = 4 * (a2 % TRY + 1)
            got = need
        else:
            cur = slot(cur + nt)
            pos = N
            got += incl
    return s[cur].copy(), pos, out, passes


if __name__ == "__main__":
    for seed, n, calls in [(3, 6, 3000), (11, 250, 60), (17, 500, 40), (5, 1248, 8), (9, 30752, 2), (2**32 - 1, 2, 2000)]:
        rs = np.random.RandomState(seed)
        st = rs.get_state()
        state, pos = st[1].copy(), int(st[2])
        worst, passes = 0.0, 0
        for c in range(calls):
            state, pos, out, p = draw(state, pos, n)
            passes += p
            worst = max(worst, float(np.abs(out - rs.normal(size=n)).max()))
            g = rs.get_state()
            assert g[3] == 0 and pos == g[2] and (state == g[1]).all(), (seed, c, pos, g[2])
        print(f"seed {seed} n {n} calls {calls}: max |model - numpy| {worst:.1e}, stream equal after every call, {passes / calls:.2f} passes per call")
