// Every env its own guide star: validation and the host arithmetic of aoenv_set_flux_env / aoenv_set_threshold_env (host only,
// plain C++: the library and the stand-alone driver tests/native/star_env_driver.cpp share it).
//
// The model (OOPAO/Source.py:109, 151; OOPAO/ShackHartmann.py:327-338, 515-517): fluxMap is linear in nPhoton and the WFS field
// amplitude is sqrt(fluxMap), so an env whose star has `scale` times the flux of the calibrated one is the calibrated shard with
// every WFS amplitude multiplied by a = sqrt(scale).  The valid lenslets are chosen relative to the maximum and the reference
// slopes and slope units are measured on ideal intensities: neither moves with the flux.  The env's threshold takes the place of
// AoCfg.threshold_cog in  I < thr * max -> 0  (ShackHartmann.py:314-324).
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdio>

namespace ao {

// h_scale [n]: flux relative to the uploaded AOENV_C_WFS_AMP, finite and > 0.  0, or 1 with the reason in msg.
inline int star_flux_check(const double* h_scale, int n, char* msg, size_t cap) {
    for (int e = 0; e < n; ++e) {
        if (!std::isfinite(h_scale[e])) { std::snprintf(msg, cap, "scale[%d] is not finite", e); return 1; }
        if (!(h_scale[e] > 0.0)) { std::snprintf(msg, cap, "scale[%d] = %g is not above 0", e, h_scale[e]); return 1; }
    }
    return 0;
}

// a_e = sqrt(scale_e) in float64, rounded once to the env dtype; scale 1 gives exactly 1
template <typename T>
inline void star_amp_factors(const double* h_scale, int n, T* out) {
    for (int e = 0; e < n; ++e) out[e] = (T)std::sqrt(h_scale[e]);
}

// h_thr [n]: finite and >= 0.  0, or 1 with the reason in msg.
inline int star_threshold_check(const double* h_thr, int n, char* msg, size_t cap) {
    for (int e = 0; e < n; ++e) {
        if (!std::isfinite(h_thr[e])) { std::snprintf(msg, cap, "threshold[%d] is not finite", e); return 1; }
        if (h_thr[e] < 0.0) { std::snprintf(msg, cap, "threshold[%d] = %g is below 0", e, h_thr[e]); return 1; }
    }
    return 0;
}

template <typename T>
inline void star_thresholds(const double* h_thr, int n, T* out) {
    for (int e = 0; e < n; ++e) out[e] = (T)h_thr[e];
}

// the shards that have no per-env threshold: null, or the reason
inline const char* star_threshold_refusal(bool pyramid, int max_group) {
    if (pyramid) return "a Pyramid shard has no centre of gravity to threshold";
    if (max_group > 1) return "envs of one measurement batch share the threshold maximum (max_group > 1, the interaction-matrix emulation)";
    return nullptr;
}

}  // namespace ao
