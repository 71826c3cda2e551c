// Static aberrations per env (aoenv_set_static_opd): a fixed optical-path map in the sensor arm, S_w, and the difference of the
// science arm's map against it, D = S_s - S_w (the reference's OPD_map / NCPA objects, OOPAO/OPD_map.py, OOPAO/NCPA.py; applied as
// tel.OPD += obj.OPD, tel.OPD_no_pupil += obj.OPD, OOPAO/Telescope.py:502-512).  Both are [R][R] in metres, unmasked, in the env
// dtype; a per-env set is E maps one after the other, a shared map is ONE copy read with stride 0.
//
// Sensor arm: S_w is added on the MIRROR side of the phase kernel's sum.  While it is set the shard forms its surface ahead of the
// phase kernel (AoEnv::dm_surface_ahead, refresh_dense_dm) and k_phase<T> reads surface + S_w through PhaseBuffers::dm_opd: the
// pupil masks it with the mirror, the unmasked phase of a geometric shard carries it unmasked, and the atmosphere's own sums and
// AOENV_B_OPD_ATM never see it.  No phase kernel and no step kernel changes.
// Science arm: phase_sci = phase + D 2 pi / lambda_src inside the pupil (k_science_static), or D as one more term of
// k_science_residual's final accumulate while a science direction is set.
// This header only declares what the kernels of static_kernels.hip are handed; there is no layout logic in it.
#pragma once
#include <cstddef>
#include <cstdint>

#include "common.hpp"

namespace ao {

template <typename T>
struct StaticDmArgs {
    // k_dm_static_mfma (float32)
    const float* s1a;        // [E] x operand table: Gy C (k_dm_rows)
    const float* gxa;        // gx operand table, env e at + e * ga_env
    size_t ga_env;
    int ga_stride;
    // k_dm_static<T>
    const T* coefs_img;      // [E][n_act^2] the command as an actuator image (k_coefs_image)
    const T* gx;             // [R][n_act], env e at + e * g_env
    const T* gy;
    size_t g_env;
    // k_static_add<T>: the surface of a mirror that is formed ahead anyway (actuator pairs, a dense mirror)
    const T* base;           // [E][R*R]
    // all three
    const T* map;            // S_w, env e at + e * map_env (0: one map for the shard)
    size_t map_env;
    T* out;                  // [E][R*R] what k_phase<T> reads
    int R, n_act;
};
int launch_dm_static_mfma(const StaticDmArgs<float>& a, int n_env, hipStream_t st);
template <typename T>
int launch_dm_static(const StaticDmArgs<T>& a, int n_env, hipStream_t st);
template <typename T>
int launch_static_add(const StaticDmArgs<T>& a, int n_env, hipStream_t st);

template <typename T>
struct SciStaticArgs {
    const uint8_t* pupil;    // [R*R]
    const T* phase;          // [E][R*R] AOENV_B_PHASE
    const T* delta;          // D = S_s - S_w, env e at + e * delta_env
    size_t delta_env;
    T* phase_sci;            // [E][R*R], or null
    T* rms_nm;               // [E], or null
    T* strehl;               // [E], or null
    int R, n_pupil;
    T src_scale;             // 2 pi / lambda_src
    double src_scale_d;
};
template <typename T>
int launch_science_static(const SciStaticArgs<T>& a, int n_env, hipStream_t st);

}  // namespace ao
