// Modal control surface of the stepped loops (aoenv_set_modal): the action and the observation of the reference's modal envs
// (MAIN/OOPAOEnv/modalAOEnv.py:150-157, 165-171, 190: dm.coefs = dm_prev * leak + (M2C_tt @ a) * 1e-6,
// obs = -(reconstructor_tt @ wfs.signal) * 1e6, reward = -||obs||^2) as a second surface beside the actuator images of aoenv_step.
// ONE host/device source: modal_kernels.hip compiles it for the device, tests/native/modal_driver.cpp for the host.
//   env e, K modes, A valid actuators, n_signal slopes, T the env dtype:
//     action     a[e][m] as given, or g[e][m] * o_prev[e][m] (the modal integrator): one multiply in T, not contracted
//     expansion  img[e][act_px[k]] = fma chain over m = 0 .. K - 1, in index order, from 0, of m2c[k][m] * a[e][m]           (T)
//                micrometres of command; pixels that are no actuator are 0 (vec_to_img)
//     projection s[e][m] = sum over j < n_signal of cm[m][j] * signal[e][j]                                                  (T)
//                o[e][m] = (T)(-1e6) * s[e][m]                        one multiply in T
//     reward     r[e] = -sum over m of (double)o[e][m]^2              float64, converted to T once
// Order of the projection on the per-env kernel path (k_modal_obs), and of the reward on every path: "lane-strided, then the tree".
// Lane l of 64 takes the terms l, l + 64, l + 128, ... in that order (the projection as an fma chain from 0, the reward as multiply
// then add); the 64 partial sums are then folded by p[l] += p[l + off] for off = 32, 16, 8, 4, 2, 1, lanes l < off, and p[0] is the
// sum.  The order depends on nothing but the number of terms, so an env has the same bits in a shard of 1 and of 1000, whichever wave
// or workgroup took it.  The split-K GEMM path of the projection has its own order (gemm_kernels.hip) and only the bound of any
// summation order in common with this one.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define AO_MODAL_HD __host__ __device__
#else
#define AO_MODAL_HD
#endif

namespace ao {

constexpr int kModalLanes = 64;        // the lanes of the fixed order: one wave

AO_MODAL_HD inline float modal_fma(float a, float b, float c) { return __builtin_fmaf(a, b, c); }
AO_MODAL_HD inline double modal_fma(double a, double b, double c) { return __builtin_fma(a, b, c); }

// the modal integrator's action: one multiply in the env dtype
template <typename T>
AO_MODAL_HD inline T modal_gain(T g, T o_prev) {
#pragma clang fp contract(off)
    return g * o_prev;
}

// the command of one actuator: m2c_t points at column k of the transposed table [K][A] (stride A), a at the K coefficients
template <typename T>
AO_MODAL_HD inline T modal_expand(const T* m2c_t, size_t stride, const T* a, int n_modes) {
    T v = (T)0;
    for (int m = 0; m < n_modes; ++m) v = modal_fma(m2c_t[(size_t)m * stride], a[m], v);
    return v;
}

// lane l's part of one projection: the terms l, l + 64, ... of cm[m][:] . signal[e][:]
template <typename T>
AO_MODAL_HD inline T modal_lane_dot(const T* cm_row, const T* signal, int n_signal, int lane) {
    T p = (T)0;
    for (int j = lane; j < n_signal; j += kModalLanes) p = modal_fma(cm_row[j], signal[j], p);
    return p;
}

// lane l's part of the reward sum: o[l]^2 + o[l + 64]^2 + ... in float64
template <typename T>
AO_MODAL_HD inline double modal_lane_sq(const T* o, int n_modes, int lane) {
#pragma clang fp contract(off)
    double p = 0.0;
    for (int m = lane; m < n_modes; m += kModalLanes) p = p + (double)o[m] * (double)o[m];
    return p;
}

// the scale of the observation: one multiply in T
template <typename T>
AO_MODAL_HD inline T modal_scale(T s) {
#pragma clang fp contract(off)
    return (T)(-1e6) * s;
}

#if !defined(__HIP_DEVICE_COMPILE__)
// ---- the host's restatement of the device's cross-lane tree (a wave does it with shuffles: modal_kernels.hip) --------------------
template <typename S>
inline S modal_tree(S* p) {            // p[kModalLanes], destroyed
    for (int off = kModalLanes / 2; off > 0; off >>= 1)
        for (int l = 0; l < off; ++l) p[l] = p[l] + p[l + off];
    return p[0];
}

// o[e][:] and the reward of one env as k_modal_obs forms them
template <typename T>
inline double modal_project_env(const T* cm, const T* signal, int n_modes, int n_signal, T* o) {
    for (int m = 0; m < n_modes; ++m) {
        T p[kModalLanes];
        for (int l = 0; l < kModalLanes; ++l) p[l] = modal_lane_dot<T>(cm + (size_t)m * n_signal, signal, n_signal, l);
        o[m] = modal_scale<T>(modal_tree<T>(p));
    }
    double q[kModalLanes];
    for (int l = 0; l < kModalLanes; ++l) q[l] = modal_lane_sq<T>(o, n_modes, l);
    return -modal_tree<double>(q);
}
#endif

}  // namespace ao
