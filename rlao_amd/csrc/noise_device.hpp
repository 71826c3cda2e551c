// Device pieces shared by the last stage of the two on-device rollouts (k_rollout_action, rollout_kernels.hip, and
// k_policy_action, policy_kernels.hip): the N(0,1)^A draw of explore.hpp into LDS and the factored projection n = Fl (Fr z).
// One source, so that the exploration noise of a policy episode is the noise of a warm-up episode bit for bit.
// NTH = lanes of the workgroup (a multiple of the wave); every lane of the workgroup calls, the functions hold the barriers.
#pragma once
#include "common.hpp"
#include "explore.hpp"

namespace ao {

// zs[4q .. 4q + 3] = the four normals of quad q (the tail of the last quad lands in the padding: zs holds A rounded up to 4)
template <typename T, int NTH>
__device__ inline void explore_draw_lds(T* zs, int A, uint32_t seed_lo, uint32_t seed_hi, uint32_t env, uint32_t counter) {
    for (int q = threadIdx.x; 4 * q < A; q += NTH) {
        float z4[4];
        explore_normals(seed_lo, seed_hi, (uint32_t)q, env, counter, z4);
#pragma unroll
        for (int j = 0; j < 4; ++j) zs[4 * q + j] = (T)z4[j];
    }
    __syncthreads();
}

// zs <- Fl (Fr zs) in place, ts [K] scratch.  fr [K][A]; fl_t [K][A] (Fl transposed).
//   t = Fr z: wave w takes the rows k = w, w + NTH/64, ...; the lanes read row k of Fr contiguously (a = lane, lane + 64, ...),
//      each sums its terms in the order of a, then the 64 partial sums meet in the xor butterfly 32, 16, .. 1.
//   n = Fl t: lane a sums over k in order; a wave reads 64 consecutive elements of Fl^T per k.
// Each row k belongs to one wave and each element to one lane whatever NTH is, so both sums have one order whatever the workgroup
// size, n_env, e or the number of idle lanes.  zs must be complete (a barrier behind its last write) on entry; it is on return.
template <typename T, int NTH>
__device__ inline void apply_factored_lds(const T* fr, const T* fl_t, T* zs, T* ts, int A, int K) {
    const int tid = threadIdx.x, lane = tid & (kWave - 1), w = tid / kWave;
    for (int k = w; k < K; k += NTH / kWave) {
        const T* row = fr + (size_t)k * A;
        T acc = 0;
        for (int i = lane; i < A; i += kWave) acc += row[i] * zs[i];
#pragma unroll
        for (int off = kWave / 2; off > 0; off >>= 1) acc += __shfl_xor(acc, off, kWave);
        if (lane == 0) ts[k] = acc;
    }
    __syncthreads();
    for (int i = tid; i < A; i += NTH) {                           // (zs[i] has no reader left: the products ended at the barrier)
        T acc = 0;
        for (int k = 0; k < K; ++k) acc += fl_t[(size_t)k * A + i] * ts[k];
        zs[i] = acc;
    }
    __syncthreads();
}

}  // namespace ao
