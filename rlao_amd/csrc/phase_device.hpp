// Device-side pieces of the residual phase shared by phase_kernel.hip (k_phase, k_phase_mfma, k_phase_mfma4) and stage A of the
// fused step kernel (step_kernel_body.hpp): one definition of the tile load, the warp, the clip, the pixel, the pupil sums and
// the batched prologue, so that the kernels agree because they run the same function.  Every piece is forced inline and takes
// arrays by reference: a caller's registers stay where they were.  The forms below are the ones that leave the callers'
// machine code what it was ("phase_device.hpp: what the phase kernels share"): check there before changing one.
#pragma once
#include "common.hpp"

namespace ao {

typedef float f32x4 __attribute__((ext_vector_type(4)));

// Four consecutive elements of a staged layer tile: logical (rr, cc) .. (rr, cc + 3) of the screen `map` (S x S, stored as a
// torus with origin (oy, ox); its rows are only 4-byte aligned) as one 16-byte load.  `need`: the element is inside the caller's
// tile and inside the screen; otherwise the result is zero, from an unconditional load of a clamped address.
__device__ __forceinline__ f32x4 torus_tile4(const float* map, int S, int oy, int ox, int rr, int cc, bool need) {
    int pr = rr + oy, pc = cc + ox;                         // torus: physical = (logical + origin) mod S
    pr = pr >= S ? pr - S : pr;
    pc = pc >= S ? pc - S : pc;
    const bool ok = need && cc + 3 < S && pc + 3 < S;        // the 4 columns are contiguous in memory
    f32x4 t;
    __builtin_memcpy(&t, map + (ok ? (size_t)pr * S + pc : 0), 16);
    f32x4 v = ok ? t : f32x4{0.f, 0.f, 0.f, 0.f};
    if (need && !ok) {
        // a float4 that straddles the wrap of the torus or the edge of the screen: element by element
#pragma unroll
        for (int d = 0; d < 4; ++d) {
            int pd = pc + d;
            pd = pd >= S ? pd - S : pd;
            if (cc + d < S) v[d] = map[(size_t)pr * S + pd];
        }
    }
    return v;
}

// skimage clip=True: clamp to the input range, keep exact zeros when 0 is outside it
template <typename T>
__device__ __forceinline__ T clip_to_range(T v, T lo, T hi, bool zero_outside) {
    if (!(zero_outside && v == (T)0)) v = v < lo ? lo : (v > hi ? hi : v);
    return v;
}

// Separable Catmull-Rom of a lane's row of 4 consecutive pixels from an LDS tile: element (row, col) of `tile` is the first tap
// of the first pixel, the 4 rows x 8 columns of taps (7 used) are read as 16-byte LDS reads; horizontal pass per row, then
// vertical, the clip to the screen's range [lo, hi] (zero_outside = lo > 0 || hi < 0), and sup += v * wl.
__device__ __forceinline__ void warp_row4(const float* tile, int row_stride, int row, int col, const float (&wx)[4],
                                          const float (&wy)[4], float lo, float hi, bool zero_outside, float wl, f32x4& sup) {
    float h[4][4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const float* m = tile + (row + q) * row_stride + col;
        const f32x4 m0 = *reinterpret_cast<const f32x4*>(m), m1 = *reinterpret_cast<const f32x4*>(m + 4);
        const float t[7] = {m0[0], m0[1], m0[2], m0[3], m1[0], m1[1], m1[2]};
#pragma unroll
        for (int r = 0; r < 4; ++r) h[q][r] = ((wx[0] * t[r] + wx[1] * t[r + 1]) + wx[2] * t[r + 2]) + wx[3] * t[r + 3];
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const float v = ((wy[0] * h[0][r] + wy[1] * h[1][r]) + wy[2] * h[2][r]) + wy[3] * h[3][r];
        sup[r] += clip_to_range(v, lo, hi, zero_outside) * wl;
    }
}

// Sum x, Sum x^2 of the atmosphere and of the residual OPD over the pupil, in float64
struct PupilSums {
    double s_atm = 0.0, q_atm = 0.0, s_res = 0.0, q_res = 0.0;
    template <typename T>
    __device__ __forceinline__ void add(T atm, T res) {
        const double da = (double)atm, dr = (double)res;
        s_atm += da;
        q_atm += da * da;
        s_res += dr;
        q_res += dr * dr;
    }
    __device__ __forceinline__ void wave_reduce() {
        s_atm = wave_sum_f64(s_atm);
        q_atm = wave_sum_f64(q_atm);
        s_res = wave_sum_f64(s_res);
        q_res = wave_sum_f64(q_res);
    }
};

// the four sums over the wave into red[c][wave]; the caller puts its barrier behind it and adds the waves in a fixed order
template <int NW>
__device__ __forceinline__ void reduce_pupil_sums(PupilSums& s, double (&red)[4][NW], int lane, int wave) {
    s.wave_reduce();
    if (lane == 0) {
        red[0][wave] = s.s_atm;
        red[1][wave] = s.q_atm;
        red[2][wave] = s.s_res;
        red[3][wave] = s.q_res;
    }
}

// One pixel: residual OPD = (atmosphere + DM surface) inside the pupil, 0 outside; returns the phase at the source's wavelength
template <typename T>
__device__ __forceinline__ T residual_pixel(T atm, T dm, bool in, T src_scale, PupilSums& sums) {
    const T res = in ? (atm + dm) : (T)0;
    const T phi = res * src_scale;
    if (in) sums.add(atm, res);
    return phi;
}
// ... and a lane's 4 consecutive pixels; update_atm = 0: `atm` holds the caller's OPD and is left as it is
__device__ __forceinline__ void residual_pixel4(int update_atm, const f32x4& sup, f32x4 dmv, const bool (&in)[4], float atm_scale,
                                                float src_scale, f32x4& atm, f32x4& phi, PupilSums& sums) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        if (update_atm) atm[r] = sup[r] * atm_scale;
        const float res = in[r] ? (atm[r] + dmv[r]) : 0.f;
        phi[r] = res * src_scale;
        if (in[r]) sums.add(atm[r], res);
    }
}

// s1[y][ix] = sum_iy gy[y0 + y][iy] C[iy][ix] of one 16-row tile on the matrix cores: 16 x 16 output tiles over the command
// columns, wave w takes the tiles w, w + 4, ...; the A operands (the tile's 16 rows of gy) are the same for every column tile
// and are loaded once, all loads in flight together.  (As a per-output dot product through LDS this was 2/3 of the kernel at
// 81 actuators across: a chain of nA LDS latencies per output.)  KS = k steps held in registers (n_act <= 4 KS).  Every load is
// unconditional from a clamped index: a predicated load compiles to a branch, and a run of them to a chain of latencies.
template <int KS>
__device__ inline void s1_tiles_mfma(const float* __restrict__ gya, int ga_stride, const float* cimg, float* s1, int y0, int nA,
                                     int nAp, int SS, int lc, int lq, int wave) {
    float av[KS];
    {
        const f32x4* src = reinterpret_cast<const f32x4*>(gya) + (size_t)(y0 >> 4) * (ga_stride >> 2) * 64 + (lq * 16 + lc);
#pragma unroll
        for (int q4 = 0; q4 < KS / 4; ++q4) {
            const f32x4 t = src[4 * q4 < ga_stride ? 64 * q4 : 0];
#pragma unroll
            for (int d = 0; d < 4; ++d) av[4 * q4 + d] = 4 * q4 < ga_stride ? t[d] : 0.f;     // A[i = lane & 15 -> row][k = lane >> 4]
        }
    }
    for (int ct = wave; 16 * ct < nA; ct += 4) {
        const int ix = 16 * ct + lc;
        float bv[KS];
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            const int iy = lq + 4 * ks;
            const bool ok = iy < nA && ix < nA;
            const float t = cimg[ok ? iy * nA + ix : 0];
            bv[ks] = ok ? t : 0.f;                           // B[k = lane >> 4][j = lane & 15]
        }
        f32x4 d = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ks = 0; ks < KS; ++ks)
            if (4 * ks < nAp) d = __builtin_amdgcn_mfma_f32_16x16x4f32(av[ks], bv[ks], d, 0, 0, 0);
        if (ix < nA) {
#pragma unroll
            for (int r = 0; r < 4; ++r) s1[(4 * lq + r) * SS + ix] = d[r];
        }
    }
}

// Prologue of the batched matrix-core kernels (256 lanes, 16-row tile at y0 of env e): the command image into LDS -- from the
// actuator images (coefs_img), or zeroed and scattered from the command vector -- then s1 = Gy[tile rows] C.  Nothing to do
// where Gy C is already in HBM (rows_given: s1a, k_dm_rows).  The caller's next barrier completes s1.  (The caller hands over
// the values it has already formed -- nA, nAp, SS, the lane decomposition: re-derived here, k_phase_mfma4 compiled to other code.)
__device__ __forceinline__ void stage_command_and_rows(const KArgs<float>& a, float* cimg, float* s1, const float* gya, bool rows_given,
                                                       int e, int y0, int tid, int nA, int nAp, int SS, int lc, int lq, int wave) {
    if (rows_given) {
    } else if (a.pb.coefs_img) {
        for (int i = tid; i < 16 * SS; i += 256) s1[i] = 0.f;
        // batches of 8 independent loads per lane (a load-then-store loop pays one memory latency per iteration)
        const float* ci = a.pb.coefs_img + (size_t)e * nA * nA;
        for (int i0 = tid; i0 < nA * nA; i0 += 8 * 256) {
            float v[8];
#pragma unroll
            for (int q = 0; q < 8; ++q) v[q] = ci[i0 + 256 * q < nA * nA ? i0 + 256 * q : i0];
#pragma unroll
            for (int q = 0; q < 8; ++q) if (i0 + 256 * q < nA * nA) cimg[i0 + 256 * q] = v[q];
        }
    } else {
        for (int i = tid; i < 16 * SS; i += 256) s1[i] = 0.f;
        for (int i = tid; i < nA * nA; i += 256) cimg[i] = 0.f;
        __syncthreads();
        const float* cf = a.pb.coefs + (size_t)e * a.n_valid_act;
        for (int k = tid; k < a.n_valid_act; k += 256) cimg[a.pb.act_idx[k]] = cf[k];
    }
    __syncthreads();
    if (!rows_given) {
        if (nAp <= 32) s1_tiles_mfma<8>(gya, a.pb.ga_stride, cimg, s1, y0, nA, nAp, SS, lc, lq, wave);
        else s1_tiles_mfma<32>(gya, a.pb.ga_stride, cimg, s1, y0, nA, nAp, SS, lc, lq, wave);
    }
}

}  // namespace ao
