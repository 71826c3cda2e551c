// The action of one exploration step of aoenv_run_rollout (MAIN/PO4AO/mbrl.py:64-89):
//   action = gain * obs + sample_noise(sigma),  sample_noise = vec_to_img(F @ (sigma N(0,1)^A))   (MAIN/OOPAOEnv/OOPAOEnv.py:566-570)
// as ONE launch in front of the step: the normals come from the counter-based stream of explore.hpp, the filter F = Fl Fr
// (A x K times K x A: M2C_CL and its pseudo-inverse, OOPAOEnv.py:383) is applied in factored form, 2 A K multiply-adds per env
// instead of the A^2 of the dense F.
//
// One workgroup per env, 256 lanes; workgroup e touches nothing of another env.  LDS: z [A] (later n [A]) and t [K].
//   1. lane q draws quad q: z[4q .. 4q + 3]
//   2. t = Fr z: wave w takes the rows k = w, w + 4, ...; the lanes read row k of Fr contiguously (a = lane, lane + 64, ...),
//      each sums its terms in the order of a, then the 64 partial sums meet in the xor butterfly 32, 16, .. 1.
//   3. n = Fl t: lane a sums over k in order; Fl is stored TRANSPOSED ([K][A]) so that a wave reads 64 consecutive elements per k.
//      Both sums have one order whatever n_env, e or the number of idle lanes (an idle lane adds an exact zero).
//   4. the image: every pixel gain * obs (one multiply in the env dtype, not contracted), plus sigma_e n[slot] at the valid actuators
//      (slot = the inverse of AOENV_C_ACT_IDX, -1 elsewhere): pixels are read and written contiguously, once.
// Steps 1 - 3 are explore_draw_lds and apply_factored_lds of noise_device.hpp, which the policy rollout's last stage shares.
// The factors are shared by all envs and come from L2 (K A elements each: 2 x 64 KB at the 8 m geometry in float32).
#include "common.hpp"
#include "noise_device.hpp"

namespace ao {

namespace {

template <typename T>
__global__ __launch_bounds__(256) void k_rollout_action(RolloutActionArgs<T> a) {
    extern __shared__ __attribute__((aligned(16))) char rollout_smem[];
    const int A = a.n_valid_act, K = a.n_filter;
    T* zs = reinterpret_cast<T*>(rollout_smem);                    // [A rounded up to 4]: z, then n
    T* ts = zs + ((A + 3) & ~3);                                   // [K]
    const int e = blockIdx.x, tid = threadIdx.x;
    explore_draw_lds<T, 256>(zs, A, a.seed_lo, a.seed_hi, a.env_offset + (uint32_t)e, a.counter);
    if (K > 0) apply_factored_lds<T, 256>(a.fr, a.fl_t, zs, ts, A, K);
    const int img = a.n_act * a.n_act;
    const T g = a.gain, sigma = a.sigma_env ? a.sigma_env[e] : a.sigma;
    const T* ob = a.obs + (size_t)e * img;
    T* ac = a.action + (size_t)e * img;
    for (int p = tid; p < img; p += 256) {
#pragma clang fp contract(off)
        T v = g * ob[p];
        const int s = a.act_slot[p];
        if (s >= 0 && sigma != (T)0) v = v + sigma * zs[s];        // sigma == 0: the bits of gain * obs, the sign of a zero included
        ac[p] = v;
    }
}

}  // namespace

size_t rollout_action_lds(int n_valid_act, int n_filter, size_t esz) { return ((size_t)((n_valid_act + 3) & ~3) + n_filter) * esz; }

template <typename T>
int launch_rollout_action(const RolloutActionArgs<T>& a, int n_env, hipStream_t st) {
    const size_t lds = rollout_action_lds(a.n_valid_act, a.n_filter, sizeof(T));
    if (lds > kRolloutLdsMax) return fail("rollout action: %zu bytes of LDS for %d actuators and filter rank %d, %zu at the most", lds, a.n_valid_act, a.n_filter, kRolloutLdsMax);
    static size_t attr_set = 0;                                    // (per instantiation)
    if (lds > 64 * 1024 && lds > attr_set) {
        AO_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(k_rollout_action<T>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        attr_set = lds;
    }
    hipLaunchKernelGGL(k_rollout_action<T>, dim3(n_env), dim3(256), lds, st, a);
    AO_HIP(hipGetLastError());
    return 0;
}
template int launch_rollout_action<float>(const RolloutActionArgs<float>&, int, hipStream_t);
template int launch_rollout_action<double>(const RolloutActionArgs<double>&, int, hipStream_t);

}  // namespace ao
