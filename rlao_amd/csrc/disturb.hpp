// Command-space disturbance of the stepped loops (aoenv_set_disturbance): the vibration lines of the reference's vibration envs
// (MAIN/OOPAOEnv/vibrationEnv.py:119-123, 146-167, 197-202: three sine lines each on tip and tilt, dm.coefs = vibration_state +
// correction_state), every env with its own frequencies, amplitudes and phases.  ONE host/device source: k_disturb_apply compiles
// it for the device, tests/native/disturb_driver.cpp for the host.
//   env e, mode m < M, line j < J, measurement time tau (an integer frame count):
//     x       = fma(f[e][m][j], (double)tau, phi[e][m][j])                      cycles; float64 whatever the env dtype
//     v[e][m] = sum over j, in index order, of amp[e][m][j] * sin(2 pi (x - floor(x)))               float64, multiply then add
//     d[e][a] = fma chain over m, in index order, from 0, of B[a][m] * (T)v[e][m]                    env dtype T
//     seen[e][a] = coefs[e][a] + d[e][a]                                                             one add, env dtype
//   f in cycles per frame, phi in cycles, amp in metres of command (the unit of dm.coefs), B dimensionless.
// The phase is reduced in cycles BEFORE the multiplication by 2 pi, so that a vibration that runs on across episodes (tau in the
// billions) loses the rounding of one fma and nothing to the argument reduction of sin.  Every sum has one order whatever the
// shard size, the env or the number of idle lanes (the rule of explore.hpp / noise_device.hpp).  With every amp == 0, v and d are
// +0 and seen equals coefs in value.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define AO_DISTURB_HD __host__ __device__
#else
#define AO_DISTURB_HD
#endif

namespace ao {

constexpr int kDisturbMaxModes = 64;   // M in [1, 64]
constexpr int kDisturbMaxLines = 8;    // J in [1, 8]

// v of one (env, mode): amp, freq, phase point at its J lines
AO_DISTURB_HD inline double disturb_mode(const double* amp, const double* freq, const double* phase, int n_lines, int64_t tau) {
#pragma clang fp contract(off)
    double v = 0.0;
    for (int j = 0; j < n_lines; ++j) {
        const double x = __builtin_fma(freq[j], (double)tau, phase[j]);
        const double s = sin(6.283185307179586476925286766559 * (x - floor(x)));
        v = v + amp[j] * s;
    }
    return v;
}

AO_DISTURB_HD inline float disturb_fma(float a, float b, float c) { return __builtin_fmaf(a, b, c); }
AO_DISTURB_HD inline double disturb_fma(double a, double b, double c) { return __builtin_fma(a, b, c); }

// d of one actuator: b points at B[0][a] of the transposed table [M][A] (stride A), v at the M modal values in the env dtype
template <typename T>
AO_DISTURB_HD inline T disturb_command(const T* b, size_t stride, const T* v, int n_modes) {
    T d = (T)0;
    for (int m = 0; m < n_modes; ++m) d = disturb_fma(b[(size_t)m * stride], v[m], d);
    return d;
}

}  // namespace ao
