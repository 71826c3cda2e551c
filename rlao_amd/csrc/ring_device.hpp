// Device functions of the ring extrusion shared by several kernels: the torus addressing of the screens, the Z gather, and NumPy's
// legacy Gaussian stream (MT19937 + polar Box-Muller) -- used by k_ring_prepare* (atm_kernels.hip), by the ring GEMM launch that
// draws the NEXT crossing's innovations in workgroups of its own (gemm_kernels.hip) and by the fused step kernel, which gathers
// the next crossing's Z right after it has written a ring (step_kernel.hip).
#pragma once
#include "common.hpp"

namespace ao {

// ---------------------------------------------------------------------------------------------------
// add_row, part 1: onePixelShiftedPhaseScreen = warp(map_full, translate(sx, sy))[1:-1, 1:-1]  and
// Z = shifted[innerMask].  A one-pixel translation through the cubic interpolator returns the source
// pixel exactly: new[r][c] = old[r - sy][c - sx] on the N x N interior, and no interior pixel reads
// outside the (N+2)^2 map.  The screen is therefore kept as a TORUS: logical pixel (r, c) lives at
// physical ((r + oy) mod S, (c + ox) mod S), and the shift only moves the origin (oy, ox) -> (oy - sy,
// ox - sx); the old border row / column that wraps around becomes the new border, which the ring
// extrusion overwrites anyway.  No pixel is copied (the copy was as much HBM traffic as the step itself).
// Here only Z = old_logical[r_k - sy][c_k - sx] is gathered, through the OLD origin.
// ---------------------------------------------------------------------------------------------------
__device__ inline int torus(int r, int c, int oy, int ox, int S) {
    int pr = r + oy, pc = c + ox;
    pr = pr >= S ? pr - S : pr;
    pc = pc >= S ? pc - S : pc;
    return pr * S + pc;
}

template <typename T>
__device__ inline void gather_ring(const T* __restrict__ map, T* __restrict__ zx, const int* __restrict__ inner_idx, int S,
                                   int n_inner, int K, int sx, int sy, int oy, int ox, int e, int t0, int nt) {
    const T* src = map + (size_t)e * S * S;
    for (int k = t0; k < n_inner; k += nt) {
        const int idx = inner_idx[k];
        const int r = idx / S - sy, c = idx % S - sx;            // interior pixel: 0 <= r, c < S
        zx[(size_t)e * K + k] = src[torus(r, c, oy, ox, S)];
    }
}

// ---------------------------------------------------------------------------------------------------
// layer.randomState.normal(size=n_outer)  (OOPAO/Atmosphere.py:308): NumPy's legacy generator =
// MT19937 + polar Box-Muller with a cached second deviate.  One workgroup per stream (env, layer).
//   * 53-bit double = ((w0 >> 5) * 2^26 + (w1 >> 6)) / 2^53 ; one polar attempt consumes 4 words
//   * attempt accepted iff 0 < r2 < 1; the call returns f*x2 first, then the cached f*x1
//   * n_outer = 4N+4 is even, so every call leaves the cache empty and the word position a multiple
//     of 4; 624 = 4*156, so an attempt never straddles a state regeneration ("twist").
// Parallel form, one pass per request: only the twists depend on each other, so the state blocks the request is expected to
// need (the rest of the current one and up to kMtSlots - 1 successors) are produced one behind the other into LDS first; then
// ALL their polar attempts are evaluated at once, two consecutive ones per lane, one exclusive scan of the accept flags assigns
// the output slots in stream order, and the attempt that completes the request decides the block and the word position that are
// stored -- bit-identical to NumPy's serial walk.  A request the blocks at hand do not complete (a whole screen at reset; a
// ring with bad luck) goes round again from the last block.
// ---------------------------------------------------------------------------------------------------
__device__ inline uint32_t mt_temper(uint32_t y) {
    y ^= (y >> 11);
    y ^= (y << 7) & 0x9d2c5680u;
    y ^= (y << 15) & 0xefc60000u;
    y ^= (y >> 18);
    return y;
}

__device__ inline uint32_t mt_mix(uint32_t a, uint32_t b, uint32_t far) {
    uint32_t y = (a & 0x80000000u) | (b & 0x7fffffffu);
    return far ^ (y >> 1) ^ ((y & 1u) ? 0x9908b0dfu : 0u);
}

constexpr int kMtTry = kMtN / 4;             // polar attempts per state block
constexpr int kMtSlots = 4;                  // state blocks in LDS (10 KB): the current one and up to 3 successors per pass
constexpr int kMtLaneTry = 2 * 256;          // attempts of a pass: two per lane, so 3 successors only behind a nearly spent block

// the successor of the 624-word state `s` into `n` (another block of LDS): three dependency-free phases, the wrap-around word
// in the third (its operands n[0] and n[396] are complete after the second)
__device__ inline void mt_twist_next(const uint32_t* s, uint32_t* n) {
    const int t = threadIdx.x;
    if (t < 227) n[t] = mt_mix(s[t], s[t + 1], s[t + 397]);
    __syncthreads();
    if (t < 227) n[t + 227] = mt_mix(s[t + 227], s[t + 228], n[t]);          // i = t + 227 in [227, 454)
    __syncthreads();
    if (t < 169) n[t + 454] = mt_mix(s[t + 454], s[t + 455], n[t + 227]);    // i in [454, 623)
    if (t == 192) n[623] = mt_mix(s[623], n[0], n[396]);                     // (a lane of the wave that is idle in this phase)
    __syncthreads();
}

// one polar attempt from 4 words of the stream: accepted?  n0 is returned first, n1 is the cached deviate returned next
// Not contracted: NumPy rounds both squares of r2 = x1^2 + x2^2.  One of them kept exact inside an fma moves r2 by an ulp, and
// log(r2) -- hence both deviates -- by 1.1e-16 / (1 - r2) relative: measured 1.1e-14 absolute on one pair of small deviates among the
// first 18 000 of RandomState(3), three times the 4e-15 the stream is held to (tests/test_gpu_normal_stream.py).
__device__ inline bool mt_polar(const uint32_t* w, double& n0, double& n1) {
#pragma clang fp contract(off)
    const double d1 = ((double)(mt_temper(w[0]) >> 5) * 67108864.0 + (double)(mt_temper(w[1]) >> 6)) /
                      9007199254740992.0;
    const double d2 = ((double)(mt_temper(w[2]) >> 5) * 67108864.0 + (double)(mt_temper(w[3]) >> 6)) /
                      9007199254740992.0;
    const double x1 = 2.0 * d1 - 1.0, x2 = 2.0 * d2 - 1.0;
    const double r2 = x1 * x1 + x2 * x2;
    if (!(r2 < 1.0 && r2 != 0.0)) return false;
    const double f = sqrt(-2.0 * log(r2) / r2);
    n0 = f * x2;
    n1 = f * x1;
    return true;
}

// mt_state_out / mt_pos_out: where the advanced stream is stored (== the inputs: in place; another buffer: the draw is
// speculative -- the ring look-ahead of env.hip -- and the caller commits it by swapping the buffers)
// xi_scale: per-env Fried parameter (aoenv_set_r0_env): [n_env] float64 sigma_e = (r0_tables / r0_e)^(5/6); the deviates of env e
// are multiplied by it in float64, before the conversion to T -- X = A Z + B(r0_e) xi = A Z + B(r0_tables) (sigma_e xi).  The
// stream itself is the same either way.  Null: one r0 for the shard, the deviates are stored as drawn.
template <typename T>
__device__ inline void mt_normal_body(const uint32_t* mt_state, const int* mt_pos, uint32_t* mt_state_out, int* mt_pos_out,
                                      T* __restrict__ zx, int K, int n_inner, int n_outer, int e, const double* xi_scale) {
    __shared__ uint32_t s[kMtSlots * kMtN];                      // a ring of state blocks: block `cur` is the stream's current one
    __shared__ int scan[4];
    __shared__ int sh_stop;
    const int t = threadIdx.x;
    const int lane = t & (kWave - 1), wv = t / kWave;
    const uint32_t* gs = mt_state + (size_t)e * kMtN;
    uint32_t* gso = mt_state_out + (size_t)e * kMtN;
    for (int i = t; i < kMtN; i += 256) s[i] = gs[i];
    // pos, got and cur are the same on every lane: each is a function of the loaded position, scan[] and sh_stop
    int pos = mt_pos[e], got = 0, cur = 0;
    const double sg = xi_scale ? xi_scale[e] : 1.0;
    __syncthreads();
    const int need_pairs = n_outer / 2;
    T* out = zx + (size_t)e * K + n_inner;
    auto slot = [](int b) { return b >= kMtSlots ? b - kMtSlots : b; };
    while (got < need_pairs) {
        const int remaining = need_pairs - got;
        const int avail0 = (kMtN - pos) / 4;                     // attempts left in the current block
        // blocks to produce: pi/4 of the attempts are accepted, so 4/3 per pair and 16 to spare (3 sigma at a 250-pair ring)
        const int want = remaining + remaining / 3 + 16 - avail0;
        const int nt = want <= 0 ? 0 : min((kMtLaneTry - avail0) / kMtTry, (want + kMtTry - 1) / kMtTry);   // 2 or 3 at the most
        for (int j = 0; j < nt; ++j) mt_twist_next(s + slot(cur + j) * kMtN, s + slot(cur + j + 1) * kMtN);
        const int n_try = avail0 + kMtTry * nt;                  // <= 512 attempts, in stream order: lane t has 2t, 2t + 1
        bool acc[2];
        double n0[2], n1[2];
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int a = 2 * t + u;
            acc[u] = false;
            n0[u] = n1[u] = 0.0;
            if (a < n_try) {
                const int a2 = a - avail0;                       // an attempt never straddles a block
                const uint32_t* w = a2 < 0 ? s + cur * kMtN + pos + 4 * a
                                           : s + slot(cur + 1 + a2 / kMtTry) * kMtN + 4 * (a2 % kMtTry);
                acc[u] = mt_polar(w, n0[u], n1[u]);
                if (acc[u] && xi_scale) {
                    n0[u] *= sg;
                    n1[u] *= sg;
                }
            }
        }
        // exclusive scan of the accept flags over the workgroup: ballots + popcounts inside a wave, 4 wave totals in LDS
        const unsigned long long bal0 = __ballot(acc[0]), bal1 = __ballot(acc[1]);
        const unsigned long long below = (1ull << lane) - 1ull;
        const int in_wave = __popcll(bal0 & below) + __popcll(bal1 & below);
        if (lane == 0) scan[wv] = __popcll(bal0) + __popcll(bal1);
        if (t == 0) sh_stop = -1;
        __syncthreads();
        int before = in_wave;
        for (int q = 0; q < wv; ++q) before += scan[q];
        const int total_acc = scan[0] + scan[1] + scan[2] + scan[3];
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            before += acc[u] ? 1 : 0;                            // inclusive count at this attempt
            if (acc[u] && before <= remaining) {
                const int j = got + before - 1;
                out[2 * j] = (T)n0[u];
                out[2 * j + 1] = (T)n1[u];
                if (before == remaining) sh_stop = 2 * t + u;    // the attempt that completes the request
            }
        }
        __syncthreads();
        const int stop = sh_stop;
        if (stop >= 0) {
            const int a2 = stop - avail0;
            if (a2 < 0) pos += 4 * (stop + 1);
            else {
                cur = slot(cur + 1 + a2 / kMtTry);
                pos = 4 * (a2 % kMtTry + 1);
            }
            got = need_pairs;
        } else {
            cur = slot(cur + nt);                                // every block at hand consumed: go on from the last one
            pos = kMtN;
            got += total_acc;
        }
        __syncthreads();                                         // scan[] and sh_stop are rewritten by the next pass
    }
    for (int i = t; i < kMtN; i += 256) gso[i] = s[cur * kMtN + i];
    if (t == 0) mt_pos_out[e] = pos;
}

}  // namespace ao
