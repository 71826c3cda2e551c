// The PO4AO policy inside the library (aoenv_set_policy / aoenv_policy_forward / aoenv_run_policy_rollout): ConvPolicy of
// MAIN/PO4AO/conv_models_simple.py:56-111, three 3x3 convolutions (2H - 1 -> F -> F -> 1 channels, padding 1, LeakyReLU between
// them), clamp, the projection on the controlled modes, scatter to the actuator image.  Kernels: policy_kernels.hip.
#pragma once
#include <algorithm>

#include "common.hpp"

namespace ao {

constexpr int kPolicyMaxHistory = 32;                              // AoPolicy.n_history
constexpr int kPolicyMaxFilt = 128;                                // AoPolicy.n_filt
constexpr size_t kPolicyLdsMax = 160 * 1024;                       // LDS of a CU
constexpr int kPolicyBandPixels = 256;                             // output pixels of one workgroup of the MFMA convolution: 16 tiles of 16

// Where a convolution finds its input channels.  plain != null: [E][C][img], a hidden image.  plain == null: the first layer,
// whose 2H - 1 channels [obs, past_obs (oldest first), past_act] (conv_models_simple.py:89, mbrl.py:73) are gathered by index
// arithmetic over the trajectory buffers and the caller's windows: at step k past channel j (of H - 1) is trajectory slot
// s = k - (H - 1) + j when s >= 0 and row H - 1 + s = k + j of the caller's window otherwise.
template <typename T>
struct ConvIn {
    const T* plain;
    const T* obs;            // [slot][E][img] observations, slot k = the current one
    const T* act;            // [slot][E][img] actions
    const T* past_obs;       // [E][H-1][img]
    const T* past_act;       // [E][H-1][img]
    int k, H, C, E, img;
};

template <typename T>
__host__ __device__ inline const T* conv_channel(const ConvIn<T>& s, int c, int e) {
    if (s.plain) return s.plain + ((size_t)e * s.C + c) * s.img;
    if (c == 0) return s.obs + ((size_t)s.k * s.E + e) * s.img;
    const bool is_act = c >= s.H;
    const int j = is_act ? c - s.H : c - 1;
    const int slot = s.k - (s.H - 1) + j;
    if (slot >= 0) return (is_act ? s.act : s.obs) + ((size_t)slot * s.E + e) * s.img;
    return (is_act ? s.past_act : s.past_obs) + ((size_t)e * (s.H - 1) + (s.H - 1 + slot)) * s.img;
}

inline int policy_ksteps(int c_in) { return cdiv(9 * c_in, 4); }
// LDS of the MFMA convolution with bands of `rows` image rows: the padded input band [C][rows + 2][n_act + 2], the tap offsets
// [4 ksteps] and, 8-byte aligned, the channels' source pointers [C]
inline size_t policy_conv_lds_rows(int n_act, int c_in, int rows) {
    const size_t words = (size_t)c_in * (rows + 2) * (n_act + 2) + 4 * (size_t)policy_ksteps(c_in);
    return (words + (words & 1)) * 4 + (size_t)c_in * 8;
}
// rows of one band of the MFMA convolution and the number of bands: a function of the image size and the channel count alone.
// The tallest band of at most kPolicyBandPixels pixels whose LDS lets two workgroups share a CU (one stages while the other
// multiplies); where not even one row does, the tallest that fits a CU at all.  The rows are then spread evenly over the bands.
inline void policy_bands(int n_act, int c_in, int* rows, int* bands) {
    int r = std::max(1, std::min(n_act, kPolicyBandPixels / n_act));
    const size_t half = kPolicyLdsMax / 2;
    const size_t limit = policy_conv_lds_rows(n_act, c_in, 1) <= half ? half : kPolicyLdsMax;
    while (r > 1 && policy_conv_lds_rows(n_act, c_in, r) > limit) --r;
    *bands = cdiv(n_act, r);
    *rows = cdiv(n_act, *bands);
}
inline size_t policy_conv_lds(int n_act, int c_in) {
    int rows, bands;
    policy_bands(n_act, c_in, &rows, &bands);
    return policy_conv_lds_rows(n_act, c_in, rows);
}
// (n_act >= 2: the staging loop divides by multiplication, whose constants need divisors above 1)
inline bool policy_mfma_fits(int n_act, int c_in) { return n_act >= 2 && n_act <= kPolicyBandPixels && policy_conv_lds(n_act, c_in) <= kPolicyLdsMax; }
// which convolution kernel a policy gets (aoenv_set_policy): the MFMA kernel on a float32 shard unless path = 1 asks for the
// general one, the filters are no whole N tiles, or a band of either wide layer (c1 = 2H - 1 and n_filt input channels) does not fit
inline bool policy_uses_mfma(size_t esz, int path, int n_filt, int n_act, int c1) {
    return esz == 4 && path == 0 && n_filt % 16 == 0 && policy_mfma_fits(n_act, c1) && policy_mfma_fits(n_act, n_filt);
}

// y = leaky(conv3x3(x) + b) on the matrix cores, float32.  wt: the weights in operand order [kstep][F / 16][64] (policy_relayout)
int launch_policy_conv_mfma(const ConvIn<float>& in, const float* wt, const float* bias, float* out, int n_act, int n_filt,
                            float slope, int n_env, hipStream_t st);
// the same on the VALU, one output element per lane, summing in (ci, ky, kx) order.  w: torch layout [F][C][3][3]
template <typename T>
int launch_policy_conv_general(const ConvIn<T>& in, const T* w, const T* bias, T* out, int n_act, int n_filt, T slope, int n_env,
                               hipStream_t st);
// host: torch layout [F][C][3][3] (float64) -> operand order, float32, zero in the K padding
inline void policy_relayout(const double* w, int n_filt, int c_in, std::vector<float>& out) {
    const int K = 9 * c_in, ksteps = policy_ksteps(c_in), nt = n_filt / 16;
    out.assign((size_t)ksteps * nt * 64, 0.0f);
    for (int ks = 0; ks < ksteps; ++ks)
        for (int t = 0; t < nt; ++t)
            for (int lane = 0; lane < 64; ++lane) {
                const int k = 4 * ks + (lane >> 4), f = 16 * t + (lane & 15);
                if (k < K) out[((size_t)ks * nt + t) * 64 + lane] = (float)w[(size_t)f * K + k];
            }
}

// last stage: conv3 + bias + clamp at the valid actuators, the factored projection, exploration noise, scatter
template <typename T>
struct PolicyActionArgs {
    const T* hidden;         // [E][F][img]
    const T* w3;             // [F][3][3]
    T b3, clamp_abs;
    const T* proj_fr;        // [Kp][A] or null with proj_rank == 0
    const T* proj_fl_t;      // [Kp][A]
    T* action;               // [E][img]
    const int* act_slot;     // [img] pixel -> index among the valid actuators, -1 = not an actuator
    // exploration noise, as RolloutActionArgs
    const T* fr;
    const T* fl_t;
    const T* sigma_env;
    T sigma;
    int n_act, n_valid_act, n_filt, proj_rank, n_filter;
    uint32_t seed_lo, seed_hi, counter, env_offset;
};
// LDS of the last stage: two vectors over the valid actuators (padded to 4) and the inner vector of the wider factor pair
inline size_t policy_action_lds(int n_valid_act, int proj_rank, int n_filter, size_t esz) {
    return ((size_t)2 * ((n_valid_act + 3) & ~3) + std::max(proj_rank, n_filter)) * esz;
}
template <typename T>
int launch_policy_action(const PolicyActionArgs<T>& a, int n_env, hipStream_t st);

// past [E][H-1][img] <- the window n_steps iterations of mbrl.py:80-81 leave: row c = trajectory slot n - (H-1) + c, or the old row c + n
template <typename T>
int launch_policy_roll(T* past, const T* traj, int n_steps, int H, int n_env, int img, hipStream_t st);

}  // namespace ao
