// The modal control surface on the device (aoenv_set_modal; the model and every summation order are modal.hpp): the two launches
// that aoenv_step_modal / aoenv_run_integrator_modal put around the explicit-action step of aoenv_step.
//   k_modal_action<T>   in front of the step: img[e][act_px[k]] = sum_m m2c[k][m] a[e][m], the action image the step integrates
//                       (MAIN/OOPAOEnv/modalAOEnv.py:150-157, M2C_tt @ a).  One workgroup per env.  a[e][:] is staged in LDS -- with
//                       gains it is g[e][m] * o_prev[e][m], the modal integrator -- and so is the image, zeroed first (vec_to_img).
//                       Lanes run over the actuators: m2c is stored TRANSPOSED ([K][A]) so that a wave reads 64 consecutive elements
//                       per mode, each lane one fma chain over m.  The whole image, zeros included, then leaves LDS in 16-byte stores
//                       where the env's row of the destination is 16-byte aligned (the last nAct^2 mod 4 or 2 elements one by one),
//                       element by element otherwise; the choice is uniform over a workgroup.
//                       Bytes per env: K (or 2 K) of coefficients in, nAct^2 of image out; m2c (K A elements) comes from L2.
//   k_modal_obs<T>      behind the step, small shapes: o[e][m] = -1e6 sum_j cm[m][j] signal[e][j] and reward[e] = -sum_m o^2
//                       (modalAOEnv.py:165-171, 190).  One workgroup per env, the signal row staged in LDS once; wave w of 4 .. 16
//                       (one per mode while they last: the workgroup has a CU to itself at 256 envs, and the chain of a mode is
//                       latency, not bandwidth) takes the modes w, w + waves, ...: every lane the fma chain over its terms
//                       j = lane, lane + 64, ... (a wave reads 64 consecutive elements of cm per round), then the shuffle tree of
//                       modal.hpp.  Wave 0 then sums the squares of the K observations from LDS in float64 in the same
//                       lane-strided order.  [Measured and dropped: four modes per wave as four interleaved chains -- fewer
//                       waves, four loads per lane and round -- was slower at every K (K = 5 at C2: 7.0 us against 3.4).]
//                       Bytes per env: n_signal in, K out; cm (K n_signal elements) is re-read by every env from L2, which is what
//                       the GEMM path below avoids at large shapes.
//   k_modal_finish<T>   behind the step, large shapes: the products come from the batched GEMM (launch_gemm_nt_mfma with split-K
//                       slabs, or launch_gemm_nt) as [splits][E][K]; this kernel adds the slabs in slab order, scales, stores and
//                       forms the reward exactly as k_modal_obs does.
// All LDS is dynamic, every carve offset a multiple of 16 bytes.
#include "common.hpp"
#include "modal.hpp"

namespace ao {

namespace {

template <typename T> struct ModalVec16;
template <> struct ModalVec16<float> { using type = float4; static constexpr int N = 4; };
template <> struct ModalVec16<double> { using type = double2; static constexpr int N = 2; };

constexpr size_t kLdsDefault = 64 * 1024, kLdsMax = 160 * 1024;

inline size_t pad16(size_t bytes) { return (bytes + 15) & ~(size_t)15; }

template <typename T>
__global__ void __launch_bounds__(1024) k_modal_action(const ModalActionArgs<T> a, int img_pad) {
    extern __shared__ __align__(16) unsigned char lds_raw[];
    T* img_s = reinterpret_cast<T*>(lds_raw);                      // [img_pad]: the image, zero at non-actuators
    T* as = img_s + img_pad;                                       // [K]: the coefficients this env applies
    const int e = blockIdx.x, tid = threadIdx.x, nt = blockDim.x;
    const int K = a.n_modes, A = a.n_valid_act, n = a.img;
    for (int q = tid; q < n; q += nt) img_s[q] = (T)0;
    const T* av = a.coef + (size_t)e * K;
    if (a.gain) {
        const T* g = a.gain + (size_t)e * a.gain_env;
        for (int m = tid; m < K; m += nt) as[m] = modal_gain<T>(g[m], av[m]);
    } else {
        for (int m = tid; m < K; m += nt) as[m] = av[m];
    }
    __syncthreads();
    for (int k = tid; k < A; k += nt) img_s[a.act_idx[k]] = modal_expand<T>(a.m2c_t + k, (size_t)A, as, K);
    __syncthreads();
    T* dst = a.image + (size_t)e * n;
    constexpr int V = ModalVec16<T>::N;
    using vec = typename ModalVec16<T>::type;
    if ((reinterpret_cast<uintptr_t>(dst) & 15) == 0) {
        const int nv = n / V;
        for (int i = tid; i < nv; i += nt) reinterpret_cast<vec*>(dst)[i] = reinterpret_cast<const vec*>(img_s)[i];
        for (int i = nv * V + tid; i < n; i += nt) dst[i] = img_s[i];
    } else {
        for (int i = tid; i < n; i += nt) dst[i] = img_s[i];
    }
}

// the cross-lane tree of modal.hpp: lane 0 ends with the sum
template <typename S>
__device__ __forceinline__ S modal_tree_wave(S p) {
    for (int off = kModalLanes / 2; off > 0; off >>= 1) p = p + __shfl_down(p, off);
    return p;
}

// reward[e] = -sum_m o[m]^2 by wave 0 of the workgroup, o_s complete (the caller's barrier)
template <typename T>
__device__ __forceinline__ void modal_reward(const T* o_s, int K, T* reward, T* ret, int e) {
    if (threadIdx.x >= kModalLanes) return;
    const double q = modal_tree_wave<double>(modal_lane_sq<T>(o_s, K, (int)threadIdx.x));
    if (threadIdx.x == 0) {
        const T r = (T)(-q);
        if (reward) reward[e] = r;
        if (ret) ret[e] += r;
    }
}

template <typename T>
__global__ void __launch_bounds__(1024) k_modal_obs(const ModalObsArgs<T> a, int sig_pad) {
    extern __shared__ __align__(16) unsigned char lds_raw[];
    T* sig_s = reinterpret_cast<T*>(lds_raw);                      // [sig_pad]
    T* o_s = sig_s + sig_pad;                                      // [K]
    const int e = blockIdx.x, tid = threadIdx.x, nt = blockDim.x;
    const int K = a.n_modes, nS = a.n_signal;
    const T* sg = a.signal + (size_t)e * nS;
    for (int j = tid; j < nS; j += nt) sig_s[j] = sg[j];
    __syncthreads();
    const int wave = tid / kModalLanes, lane = tid & (kModalLanes - 1);
    T* ob = a.obs + (size_t)e * K;
    for (int m = wave; m < K; m += nt / kModalLanes) {
        const T s = modal_tree_wave<T>(modal_lane_dot<T>(a.cm + (size_t)m * nS, sig_s, nS, lane));
        if (lane == 0) {
            const T o = modal_scale<T>(s);
            o_s[m] = o;
            ob[m] = o;
        }
    }
    __syncthreads();
    modal_reward<T>(o_s, K, a.reward, a.ret, e);
}

template <typename T>
__global__ void __launch_bounds__(256) k_modal_finish(const ModalObsArgs<T> a, int n_env) {
    extern __shared__ __align__(16) unsigned char lds_raw[];
    T* o_s = reinterpret_cast<T*>(lds_raw);                        // [K]
    const int e = blockIdx.x, K = a.n_modes;
    const size_t slab = (size_t)n_env * K;
    const T* pv = a.slabs + (size_t)e * K;
    T* ob = a.obs + (size_t)e * K;
    for (int m = threadIdx.x; m < K; m += 256) {
        T acc = pv[m];
        for (int z = 1; z < a.splits; ++z) acc += pv[(size_t)z * slab + m];      // split-K slabs, fixed order
        const T o = modal_scale<T>(acc);
        o_s[m] = o;
        ob[m] = o;
    }
    __syncthreads();
    modal_reward<T>(o_s, K, a.reward, a.ret, e);
}

// dynamic LDS above 64 KB is opted into once per kernel and size reached (`granted`: a static of the launcher's instantiation)
template <typename K>
int allow_lds(K kern, size_t lds, size_t* granted) {
    if (lds > kLdsDefault && lds > *granted) {
        AO_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        *granted = lds;
    }
    return 0;
}

}  // namespace

bool modal_obs_fits(int n_modes, int n_signal, size_t esz) { return pad16((size_t)n_signal * esz) + (size_t)n_modes * esz <= kLdsDefault; }

template <typename T>
int launch_modal_action(const ModalActionArgs<T>& a, int n_env, hipStream_t st) {
    if (a.n_modes < 1 || a.n_modes > a.n_valid_act || a.n_valid_act > a.img)
        return fail("modal action: %d modes, %d actuators, %d pixels", a.n_modes, a.n_valid_act, a.img);
    const size_t img_bytes = pad16((size_t)a.img * sizeof(T)), lds = img_bytes + (size_t)a.n_modes * sizeof(T);
    if (lds > kLdsMax) return fail("modal action: %zu bytes of LDS for a %d-pixel image and %d modes", lds, a.img, a.n_modes);
    static size_t granted = 0;
    AO_TRY(allow_lds(k_modal_action<T>, lds, &granted));
    // a lane per actuator in one round up to 1024 lanes
    const int lanes = a.n_valid_act > 1024 ? 1024 : a.n_valid_act < 256 ? 256 : cdiv(a.n_valid_act, kModalLanes) * kModalLanes;
    hipLaunchKernelGGL(k_modal_action<T>, dim3(n_env), dim3(lanes), lds, st, a, (int)(img_bytes / sizeof(T)));
    AO_HIP(hipGetLastError());
    return 0;
}

template <typename T>
int launch_modal_obs(const ModalObsArgs<T>& a, int n_env, hipStream_t st) {
    if (a.n_modes < 1 || a.n_signal < 1 || !modal_obs_fits(a.n_modes, a.n_signal, sizeof(T)))
        return fail("modal projection: %d modes x %d slopes do not fit the per-env kernel", a.n_modes, a.n_signal);
    const size_t sig_bytes = pad16((size_t)a.n_signal * sizeof(T));
    // a wave per mode up to 16 waves (a mode's order of summation does not depend on the wave that takes it)
    const int waves = a.n_modes < 4 ? 4 : a.n_modes > 16 ? 16 : a.n_modes;
    hipLaunchKernelGGL(k_modal_obs<T>, dim3(n_env), dim3(waves * kModalLanes), sig_bytes + (size_t)a.n_modes * sizeof(T), st, a,
                       (int)(sig_bytes / sizeof(T)));
    AO_HIP(hipGetLastError());
    return 0;
}

template <typename T>
int launch_modal_finish(const ModalObsArgs<T>& a, int n_env, hipStream_t st) {
    const size_t lds = (size_t)a.n_modes * sizeof(T);
    if (a.n_modes < 1 || a.splits < 1 || lds > kLdsMax) return fail("modal finish: %d modes, %d slabs", a.n_modes, a.splits);
    static size_t granted = 0;
    AO_TRY(allow_lds(k_modal_finish<T>, lds, &granted));
    hipLaunchKernelGGL(k_modal_finish<T>, dim3(n_env), dim3(256), lds, st, a, n_env);
    AO_HIP(hipGetLastError());
    return 0;
}

#define AO_INST_MODAL(T)                                                                   \
    template int launch_modal_action<T>(const ModalActionArgs<T>&, int, hipStream_t);     \
    template int launch_modal_obs<T>(const ModalObsArgs<T>&, int, hipStream_t);           \
    template int launch_modal_finish<T>(const ModalObsArgs<T>&, int, hipStream_t);
AO_INST_MODAL(float)
AO_INST_MODAL(double)
#undef AO_INST_MODAL

}  // namespace ao
