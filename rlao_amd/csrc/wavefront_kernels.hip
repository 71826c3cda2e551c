// Wavefront modes on the device (aoenv_project_wavefront, aoenv_set_wavefront_record; the model, the slices and the order of the
// sum are wavefront.hpp): c[w][e][m] = s_w sum_q P[m][q] X_w[e][q], a skinny product with a long reduction -- [n_env][R^2] . [R^2][K],
// K from 1 to 1024 -- that reads X once from HBM.  Two launches:
//   k_wf_project_mfma   float32 shards.  A wave takes one tile of 16 envs x 16 NB modes over one slice of [0, R^2) on
//                       v_mfma_f32_16x16x4_f32, operands from global memory straight into registers (no LDS: nothing is shared
//                       between waves).  Lane (r = l & 15, g = l >> 4) loads X[e0 + r][k .. k + 3] and P[m0 + 16 b + r][k .. k + 3] at
//                       k = k0 + 4 g as 16 bytes each (element by element, every element guarded, when R^2 % 4 != 0: the rows of X
//                       are then not 16-byte aligned; the choice is uniform per launch) and issues four matrix-core steps, one per
//                       component: step c contracts over k0 + 4 g' + c, g' = 0 .. 3, on BOTH operands -- a permutation of k that is
//                       the same for X and P, so the sum is that of the slice.  The loads of four rounds (64 elements of a
//                       row) are issued together; rounds of 16 elements alternate between two
//                       accumulators per (operand, mode block) (the 16x16x4 form needs two independent chains to reach its issue
//                       rate), added at the end: even rounds + odd rounds.  With both operands in a launch the P registers are
//                       loaded once and used for the residual and the atmosphere rows.
//                       Guards: a lane whose env is >= n_env, whose mode is >= K or whose k is >= the slice's end loads NOTHING and
//                       contributes zeros; with 16-byte loads k and the slice ends are multiples of 4, so a load never straddles the
//                       end of a row.  Only results with env < n_env and mode < K are stored.
//                       D layout (16x16x4 f32): lane l, register v holds D[row 4 (l >> 4) + v][col l & 15]: row = env, col = mode.
//                       Grid (env tiles, mode tiles, slices / 4): the 4 waves of a workgroup take 4 consecutive slices.
//   k_wf_project<T>     the general kernel: float64 shards and AOENV_PATH_WF_GENERAL.  One lane per (env, mode, slice): the plain
//                       fma chain of wf_chain in T.
//   k_wf_finish<T>      adds the slices in slice order, applies s, writes [n_w][E][K] (d_out, or the slot of the record).
#include "common.hpp"
#include "wavefront.hpp"

namespace ao {

namespace {

using wf_f32x4 = __attribute__((ext_vector_type(4))) float;
constexpr int kWfUnroll = 4;           // rounds of 16 elements whose loads are in flight together (even: the rounds alternate accumulators)
constexpr int kWfFinishBatch = 8;      // slabs the finish kernel loads before it adds them, in order

// the four elements k .. k + 3 of a row, zero where the row is not the lane's to read or k is past `hi`
template <bool VEC>
__device__ __forceinline__ wf_f32x4 wf_load4(const float* row, bool ok, int k, int hi) {
    wf_f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (!ok || k >= hi) return v;
    if (VEC) return *reinterpret_cast<const wf_f32x4*>(row + k);   // (k % 4 == 0 and hi % 4 == 0: k + 3 < hi)
#pragma unroll
    for (int c = 0; c < 4; ++c)
        if (k + c < hi) v[c] = row[k + c];
    return v;
}

template <int NB, int W, bool VEC>
__global__ void __launch_bounds__(256) k_wf_project_mfma(const WfArgs<float> a) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int z = blockIdx.z * 4 + wave;
    if (z >= a.n_slices) return;                                   // (wave-uniform; the kernel has no barrier)
    const int r = lane & 15, g = lane >> 4;
    const int e0 = blockIdx.x * 16, m0 = blockIdx.y * 16 * NB;
    const int lo = z * a.slice_len, hi = min(a.r2, lo + a.slice_len);
    const bool e_ok = e0 + r < a.n_env;
    const float* xr[W];
#pragma unroll
    for (int w = 0; w < W; ++w) xr[w] = a.x[w] + (size_t)(e_ok ? e0 + r : 0) * a.r2;
    const float* pr[NB];
    bool m_ok[NB];
#pragma unroll
    for (int b = 0; b < NB; ++b) {
        m_ok[b] = m0 + 16 * b + r < a.n_modes;
        pr[b] = a.p + (size_t)(m_ok[b] ? m0 + 16 * b + r : 0) * a.ld;
    }
    wf_f32x4 acc[2][W][NB];
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
        for (int w = 0; w < W; ++w)
#pragma unroll
            for (int b = 0; b < NB; ++b) acc[u][w][b] = wf_f32x4{0.f, 0.f, 0.f, 0.f};
    for (int k0 = lo; k0 < hi; k0 += kWfUnroll * kWfRound) {
        wf_f32x4 xv[kWfUnroll][W], pv[kWfUnroll][NB];
#pragma unroll
        for (int u = 0; u < kWfUnroll; ++u) {
            const int k = k0 + u * kWfRound + 4 * g;
#pragma unroll
            for (int w = 0; w < W; ++w) xv[u][w] = wf_load4<VEC>(xr[w], e_ok, k, hi);
#pragma unroll
            for (int b = 0; b < NB; ++b) pv[u][b] = wf_load4<VEC>(pr[b], m_ok[b], k, hi);
        }
#pragma unroll
        for (int u = 0; u < kWfUnroll; ++u)
#pragma unroll
            for (int c = 0; c < 4; ++c)
#pragma unroll
                for (int w = 0; w < W; ++w)
#pragma unroll
                    for (int b = 0; b < NB; ++b)
                        acc[u & 1][w][b] = __builtin_amdgcn_mfma_f32_16x16x4f32(xv[u][w][c], pv[u][b][c], acc[u & 1][w][b], 0, 0, 0);
    }
    const int m_lane = m0 + r;                                     // + 16 b: the lane's column of D
#pragma unroll
    for (int w = 0; w < W; ++w) {
        float* slab = a.slabs + ((size_t)z * W + w) * a.n_env * a.n_modes;
#pragma unroll
        for (int b = 0; b < NB; ++b) {
            const wf_f32x4 s = acc[0][w][b] + acc[1][w][b];
            const int m = m_lane + 16 * b;
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                const int e = e0 + 4 * g + v;                      // the register's row of D
                if (e < a.n_env && m < a.n_modes) slab[(size_t)e * a.n_modes + m] = s[v];
            }
        }
    }
}

template <typename T>
__global__ void __launch_bounds__(64) k_wf_project(const WfArgs<T> a) {
    const int m = blockIdx.x * 64 + threadIdx.x, e = blockIdx.y, z = blockIdx.z;
    if (m >= a.n_modes) return;
    const int lo = z * a.slice_len, hi = min(a.r2, lo + a.slice_len);
    const T* pr = a.p + (size_t)m * a.ld;
    for (int w = 0; w < a.n_w; ++w)
        a.slabs[(((size_t)z * a.n_w + w) * a.n_env + e) * a.n_modes + m] = wf_chain<T>(pr, a.x[w] + (size_t)e * a.r2, lo, hi);
}

template <typename T>
__global__ void __launch_bounds__(256) k_wf_finish(const WfArgs<T> a) {
    const size_t per = (size_t)a.n_env * a.n_modes, n = per * a.n_w;
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    T acc = a.slabs[i];
    for (int z0 = 1; z0 < a.n_slices; z0 += kWfFinishBatch) {                      // slice order; the loads of a batch are independent
        T v[kWfFinishBatch];
#pragma unroll
        for (int j = 0; j < kWfFinishBatch; ++j) v[j] = z0 + j < a.n_slices ? a.slabs[(size_t)(z0 + j) * n + i] : (T)0;
#pragma unroll
        for (int j = 0; j < kWfFinishBatch; ++j)
            if (z0 + j < a.n_slices) acc += v[j];
    }
    const int w = i >= per ? 1 : 0;
    a.out[i] = a.use_scale[w] ? wf_scale<T>(acc, a.scale[w]) : acc;
}

template <int NB, int W>
void wf_launch_mfma(const WfArgs<float>& a, hipStream_t st) {
    const dim3 grid(cdiv(a.n_env, 16), cdiv(a.n_modes, 16 * NB), cdiv(a.n_slices, 4));
    if (a.r2 % 4 == 0) hipLaunchKernelGGL((k_wf_project_mfma<NB, W, true>), grid, dim3(256), 0, st, a);
    else hipLaunchKernelGGL((k_wf_project_mfma<NB, W, false>), grid, dim3(256), 0, st, a);
}

template <typename T>
int wf_project_dispatch(const WfArgs<T>& a, bool, hipStream_t st) {
    hipLaunchKernelGGL(k_wf_project<T>, dim3(cdiv(a.n_modes, 64), a.n_env, a.n_slices), dim3(64), 0, st, a);
    return 0;
}
template <>
int wf_project_dispatch<float>(const WfArgs<float>& a, bool general, hipStream_t st) {
    if (general) {
        hipLaunchKernelGGL(k_wf_project<float>, dim3(cdiv(a.n_modes, 64), a.n_env, a.n_slices), dim3(64), 0, st, a);
        return 0;
    }
    // mode blocks per wave: the X registers of a round are used NB times
    const int nb = a.n_modes <= 16 ? 1 : a.n_modes <= 32 ? 2 : 4;
    if (a.n_w == 1) {
        if (nb == 1) wf_launch_mfma<1, 1>(a, st);
        else if (nb == 2) wf_launch_mfma<2, 1>(a, st);
        else wf_launch_mfma<4, 1>(a, st);
    } else {
        if (nb == 1) wf_launch_mfma<1, 2>(a, st);
        else if (nb == 2) wf_launch_mfma<2, 2>(a, st);
        else wf_launch_mfma<4, 2>(a, st);
    }
    return 0;
}

}  // namespace

template <typename T>
int launch_wf_project(const WfArgs<T>& a, bool general, hipStream_t st) {
    const WfPlan pl = wf_plan(a.r2, a.n_modes);
    if (a.n_w < 1 || a.n_w > 2 || a.n_env < 1 || a.n_env > 65535 || a.n_modes < 1 || a.n_modes > kWfMaxModes || a.r2 < 1 ||
        a.ld != wf_row_stride(a.r2) || a.n_slices != pl.n_slices || a.slice_len != pl.slice_len)
        return fail("wavefront projection: %d operands, %d envs, %d modes, %d pixels (stride %d), %d slices of %d", a.n_w, a.n_env,
                    a.n_modes, a.r2, a.ld, a.n_slices, a.slice_len);
    AO_TRY(wf_project_dispatch<T>(a, general, st));
    AO_HIP(hipGetLastError());
    return launch_wf_finish<T>(a, st);
}

template <typename T>
int launch_wf_finish(const WfArgs<T>& a, hipStream_t st) {
    if (a.n_w < 1 || a.n_w > 2 || a.n_env < 1 || a.n_modes < 1 || a.n_slices < 1)
        return fail("wavefront finish: %d operands, %d envs, %d modes, %d slices", a.n_w, a.n_env, a.n_modes, a.n_slices);
    const size_t n = (size_t)a.n_w * a.n_env * a.n_modes;
    hipLaunchKernelGGL(k_wf_finish<T>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, a);
    AO_HIP(hipGetLastError());
    return 0;
}

#define AO_INST_WF(T)                                                              \
    template int launch_wf_project<T>(const WfArgs<T>&, bool, hipStream_t);       \
    template int launch_wf_finish<T>(const WfArgs<T>&, hipStream_t);
AO_INST_WF(float)
AO_INST_WF(double)
#undef AO_INST_WF

}  // namespace ao
