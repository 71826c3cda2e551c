// The surface of a mirror given as per-env actuator factor pairs (aoenv_set_dm_pairs; layouts: dm_pairs.hpp):
//   S_e[y][x] = sum_k c_e[k] py_e[y][k] px_e[x][k]  =  ((Py_e diag(c_e)) Px_e^T)[y][x],   k over the A valid actuators
// written to dm_opd [E][R*R], which k_phase<T> reads.  Both kernels form t = c[k] * py[y][k] (one rounding) and add t * px[x][k] by one
// fma per k in ASCENDING k: the order of the sum depends on (R, A) alone, there are no atomics, and an env has the same bits in any
// shard and at any place in it.
//
// k_dm_pairs_mfma (float32): one wave per workgroup and per 32 x 32 patch of the surface, grid (ceil(R / 32), ceil(R / 32), E).
//   The patch is 2 x 2 tiles of v_mfma_f32_16x16x4_f32 -- four independent accumulators of 4 registers, which covers the
//   instruction's dependent latency from a single wave -- and K runs in steps of 4.  The product is formed TRANSPOSED (A operand:
//   px rows, B operand: c py rows), because the accumulator of a lane holds 4 consecutive ROWS of D at one column: with x on the
//   rows a lane owns S[y][x0 .. x0 + 3] and stores it as one float4.
//   Operands: the tables are in the operand layout of the separable mirror (ga_index()): the 64 lanes' float4s of one (16-row tile,
//   4 k steps) are 1 KB contiguous, so each of the 4 operand loads per 16 MFMAs is one coalesced 16-byte-per-lane access.  Rows
//   R .. R pad 128 and actuators A .. 4 ga_stride of the table are zero: the padding rows and the K tail multiply zeros, no load is
//   guarded.  The command is staged in LDS 1024 actuators at a time, permuted so that a lane's 4 steps are one 16-byte read
//   (4 distinct addresses per wave), zero beyond A.
//   Stores: float4 per lane where R % 4 == 0 (a float4 is then inside the surface or outside it as a whole, and 16-byte aligned);
//   dwords otherwise.
// k_dm_pairs<T> (float64 shards; float32 under AOENV_PATH_DM_PAIRS_GENERAL): one lane per pixel, 64 x 4 pixels per workgroup, the
//   transposed env-dtype tables [A][R] so that a wave reads 64 consecutive px per k (py and c are wave-uniform per row).
#include "common.hpp"
#include "dm_pairs.hpp"

namespace ao {

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kPairsChunk = 1024;                                  // actuators of the command held in LDS at a time (64 step quads)

__global__ __launch_bounds__(64) void k_dm_pairs_mfma(PairsArgs<float> a) {
    __shared__ float4 cs[kPairsChunk / 4];                         // [step quad][lq] -> c[16 sq + 4 j + lq], j = 0 .. 3
    const int lane = threadIdx.x, lc = lane & 15, lq = lane >> 4;
    const int e = blockIdx.z, tx0 = 2 * blockIdx.x, ty0 = 2 * blockIdx.y;
    const int R = a.R, A = a.A, nq = a.ga_stride >> 2;
    const float* cf = a.coefs + (size_t)e * A;
    const float4* pxa = reinterpret_cast<const float4*>(a.pxa + (size_t)e * a.ga_env) + lane;
    const float4* pya = reinterpret_cast<const float4*>(a.pya + (size_t)e * a.ga_env) + lane;
    const float4* x0p = pxa + (size_t)tx0 * nq * 64;
    const float4* x1p = x0p + (size_t)nq * 64;
    const float4* y0p = pya + (size_t)ty0 * nq * 64;
    const float4* y1p = y0p + (size_t)nq * 64;
    f32x4 acc00 = {0.f, 0.f, 0.f, 0.f}, acc01 = acc00, acc10 = acc00, acc11 = acc00;   // acc<y tile><x tile>
    float* csf = reinterpret_cast<float*>(cs);
    for (int q0 = 0; q0 < nq; q0 += kPairsChunk / 16) {
        const int nqc = min(kPairsChunk / 16, nq - q0);
        __syncthreads();                                           // (the chunk before this one has been read)
        for (int i = lane; i < nqc * 16; i += 64) {
            const int k = q0 * 16 + i;                             // i = 16 sq + 4 j + q  ->  slot (sq, q, j)
            csf[((i >> 4) * 4 + (i & 3)) * 4 + ((i >> 2) & 3)] = k < A ? cf[k] : 0.f;
        }
        __syncthreads();
        for (int s = 0; s < nqc; ++s) {
            const size_t o = (size_t)(q0 + s) * 64;
            const float4 x0 = x0p[o], x1 = x1p[o];
            float4 y0 = y0p[o], y1 = y1p[o];
            const float4 c = cs[s * 4 + lq];
            y0.x *= c.x; y0.y *= c.y; y0.z *= c.z; y0.w *= c.w;
            y1.x *= c.x; y1.y *= c.y; y1.z *= c.z; y1.w *= c.w;
#define AO_PAIRS_STEP(m)                                                                \
    acc00 = __builtin_amdgcn_mfma_f32_16x16x4f32(x0.m, y0.m, acc00, 0, 0, 0);           \
    acc01 = __builtin_amdgcn_mfma_f32_16x16x4f32(x1.m, y0.m, acc01, 0, 0, 0);           \
    acc10 = __builtin_amdgcn_mfma_f32_16x16x4f32(x0.m, y1.m, acc10, 0, 0, 0);           \
    acc11 = __builtin_amdgcn_mfma_f32_16x16x4f32(x1.m, y1.m, acc11, 0, 0, 0)
            AO_PAIRS_STEP(x);
            AO_PAIRS_STEP(y);
            AO_PAIRS_STEP(z);
            AO_PAIRS_STEP(w);
#undef AO_PAIRS_STEP
        }
    }
    // D[i][j]: i = the A operand's row = x within the tile, j = the B operand's column = y; lane (lc, lq) holds j = lc, i = 4 lq + reg
    float* out = a.out + (size_t)e * R * R;
    const bool vec = (R & 3) == 0;
    auto store = [&](const f32x4& v, int ty, int tx) {
        const int y = 16 * ty + lc, x = 16 * tx + 4 * lq;
        if (y >= R || x >= R) return;
        float* p = out + (size_t)y * R + x;
        if (vec) {
            *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
        } else {
            p[0] = v[0];
            if (x + 1 < R) p[1] = v[1];
            if (x + 2 < R) p[2] = v[2];
            if (x + 3 < R) p[3] = v[3];
        }
    };
    store(acc00, ty0, tx0);
    store(acc01, ty0, tx0 + 1);
    store(acc10, ty0 + 1, tx0);
    store(acc11, ty0 + 1, tx0 + 1);
}

template <typename T>
__global__ __launch_bounds__(256) void k_dm_pairs(PairsArgs<T> a) {
    const int e = blockIdx.z, R = a.R, A = a.A;
    const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y;
    if (x >= R || y >= R) return;
    const T* cf = a.coefs + (size_t)e * A;
    const T* py = a.pyt + (size_t)e * a.t_env + y;
    const T* px = a.pxt + (size_t)e * a.t_env + x;
    T acc = (T)0;
    for (int k = 0; k < A; ++k) {
        const T t = cf[k] * py[(size_t)k * R];
        acc = fma(t, px[(size_t)k * R], acc);
    }
    a.out[(size_t)e * R * R + (size_t)y * R + x] = acc;
}

}  // namespace

template <typename T>
int launch_dm_pairs(const PairsArgs<T>& a, int n_env, bool general, hipStream_t st) {
    if (a.R < 1 || a.A < 1 || n_env < 1) return fail("dm pairs: R = %d, A = %d, %d envs", a.R, a.A, n_env);
    if constexpr (std::is_same<T, float>::value) {
        if (!general) {
            PairsLayout L;
            L.R = a.R;
            L.A = a.A;
            // what the kernel's unguarded loads rely on: the table covers every tile of the grid and every k step
            if (a.ga_stride != L.ga_stride() || a.ga_env != L.ga_elems() || 32 * cdiv(a.R, 32) > L.r_pad() || 4 * a.ga_stride < a.A)
                return fail("dm pairs: operand table of stride %d / %zu floats per env does not fit R = %d, A = %d", a.ga_stride, a.ga_env, a.R, a.A);
            const int t = cdiv(a.R, 32);
            hipLaunchKernelGGL(k_dm_pairs_mfma, dim3(t, t, n_env), dim3(64), 0, st, a);
            AO_HIP(hipGetLastError());
            return 0;
        }
    }
    hipLaunchKernelGGL(k_dm_pairs<T>, dim3(cdiv(a.R, 64), cdiv(a.R, 4), n_env), dim3(64, 4), 0, st, a);
    AO_HIP(hipGetLastError());
    return 0;
}
template int launch_dm_pairs<float>(const PairsArgs<float>&, int, bool, hipStream_t);
template int launch_dm_pairs<double>(const PairsArgs<double>&, int, bool, hipStream_t);

}  // namespace ao
