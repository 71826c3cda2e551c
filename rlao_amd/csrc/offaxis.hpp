// Off-axis science target per env (aoenv_set_science_direction, aoenv_science_residual, aoenv_set_science_direction_record): a
// second line of sight through the layers, the reference's `src.coordinates = [zenith arcsec, azimuth deg]` with `atm * src`
// (OOPAO/Atmosphere.py:313-334 set_pupil_footprint, :439-450 fill_phase_support; MAIN_CODE/OOPAOEnv/OOPAOEnv.py:140-146, 303-304).
// ONE host/device source: offaxis_kernels.hip compiles it for the device, env.hip and tests/native/offaxis_driver.cpp for the host.
//   a layer at altitude h on its N x N grid, the telescope R pixels across D metres:
//     [x_z, y_z] = pol2cart(h tan(zenith / 206265) N / (N D / R), deg2rad(azimuth))              pixels
//     ix, iy = int(x_z), int(y_z) (towards zero);  extra_sx, extra_sy = ix - x_z, iy - y_z      in (-1, 1)
//     footprint = rows iy + N//2 - R//2 .. + R, columns ix + N//2 - R//2 .. + R                 (y_z moves ROWS, x_z columns)
//     _im = layer.phase, the wind's clipped bicubic warp; where extra_sx != 0 or extra_sy != 0 it is translated bilinearly:
//     out[r][c] = _im[r - extra_sy][c - extra_sx];  phase_support += _im[footprint] sqrt(fractionalR0)
//   so pixel (r, c) of the pupil reads layer.phase at (r + N//2 - R//2 + y_z, c + N//2 - R//2 + x_z).  For the device the offset is
//   normalised to floor + fraction: f = floor(z), t = z - f in [0, 1), and
//     v = (1 - ty) ((1 - tx) P[f_y][f_x] + tx P[f_y][f_x + 1]) + ty ((1 - tx) P[f_y + 1][f_x] + tx P[f_y + 1][f_x + 1])      (oa_blend)
//   in the env dtype, skipped -- v = P[f_y][f_x] -- exactly where the reference skips it: both fractions zero.
// The plan of a launch (oa_plan_layer): with blend the patch of P is (R + 1)^2, and every row and column of it must lie in
// [1, N - 2] of layer.phase, so that every Catmull-Rom tap lies inside the (N + 2)^2 screen and the zero fill of neither warp is
// reached.  The grid rule N = ceil(R + 2 s_max) + 4 gives that for every zenith <= fov / 2; the host asserts it and refuses what
// breaks it, the kernel has no branch for it.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define AO_OA_HD __host__ __device__
#else
#define AO_OA_HD
#endif

namespace ao {

// the footprint of (layer, env) toward the target, as the device reads it
struct OaShift {
    int fy, fx;            // floor(y_z), floor(x_z): whole pixels (rows, columns)
    double ty, tx;         // y_z - fy, x_z - fx in [0, 1)
};

// ... and as the reference states it (the golden's corners and fractions)
struct OaRefShift {
    double x_z, y_z;
    int ix, iy;            // int(): truncation toward zero
    double extra_sx, extra_sy;
    int row0, col0;        // first row / column of the footprint in layer.phase
};

enum OaRefusal {
    kOaOk = 0,
    kOaNoLayers,
    kOaNull,
    kOaZenith,             // negative, not finite or above fov / 2
    kOaAzimuth,            // not finite
    kOaGeometry,           // diameter / fov / an altitude that is not finite or negative
    kOaPlan                // a footprint whose taps would leave the screen
};

inline OaRefShift oa_ref_shift(double altitude, double zenith_arcsec, double azimuth_deg, int R, double D, int N) {
#pragma clang fp contract(off)
    OaRefShift s;
    const double layer_D = (double)N * D / (double)R;               // layer.D (Atmosphere.py:219)
    const double rho = altitude * tan(zenith_arcsec / 206265.0) * (double)N / layer_D;
    const double phi = azimuth_deg * (3.14159265358979323846 / 180.0);   // np.deg2rad
    s.x_z = rho * cos(phi);
    s.y_z = rho * sin(phi);
    s.ix = (int)s.x_z;
    s.iy = (int)s.y_z;
    s.extra_sx = (double)s.ix - s.x_z;
    s.extra_sy = (double)s.iy - s.y_z;
    s.row0 = s.iy + N / 2 - R / 2;
    s.col0 = s.ix + N / 2 - R / 2;
    return s;
}

inline OaShift oa_shift(const OaRefShift& r) {
#pragma clang fp contract(off)
    OaShift s;
    const double ky = floor(r.y_z), kx = floor(r.x_z);
    s.fy = (int)ky;
    s.fx = (int)kx;
    s.ty = r.y_z - ky;
    s.tx = r.x_z - kx;
    return s;
}

AO_OA_HD inline bool oa_blends(double ty, double tx) { return ty != 0.0 || tx != 0.0; }

// the in-range assertion of one (layer, env): rows and columns [lo, hi] of layer.phase the patch takes
inline bool oa_plan_layer(const OaShift& s, int R, int N, int* lo, int* hi) {
    const int foot0 = N / 2 - R / 2, more = oa_blends(s.ty, s.tx) ? 1 : 0;
    const int lo_y = foot0 + s.fy, lo_x = foot0 + s.fx;
    const int hi_y = lo_y + R - 1 + more, hi_x = lo_x + R - 1 + more;
    if (lo) *lo = lo_y < lo_x ? lo_y : lo_x;
    if (hi) *hi = hi_y > hi_x ? hi_y : hi_x;
    return lo_y >= 1 && lo_x >= 1 && hi_y <= N - 2 && hi_x <= N - 2;
}

// everything aoenv_set_science_direction checks, and the table it uploads: out [n_layer][n_env]
inline OaRefusal oa_make(int n_layer, int n_env, int R, double D, double fov_arcsec, const double* altitude, const int* N_l,
                         const double* zenith, const double* azimuth, OaShift* out, int* where_env, int* where_layer) {
    if (n_layer < 1) return kOaNoLayers;
    if (!zenith || !azimuth || !altitude || !N_l) return kOaNull;
    if (!(isfinite(D) && D > 0) || !(isfinite(fov_arcsec) && fov_arcsec >= 0)) return kOaGeometry;
    for (int l = 0; l < n_layer; ++l)
        if (!(isfinite(altitude[l]) && altitude[l] >= 0)) return kOaGeometry;
    for (int e = 0; e < n_env; ++e) {
        if (where_env) *where_env = e;
        if (!isfinite(zenith[e]) || zenith[e] < 0 || zenith[e] > fov_arcsec / 2) return kOaZenith;
        if (!isfinite(azimuth[e])) return kOaAzimuth;
    }
    for (int l = 0; l < n_layer; ++l)
        for (int e = 0; e < n_env; ++e) {
            const OaShift s = oa_shift(oa_ref_shift(altitude[l], zenith[e], azimuth[e], R, D, N_l[l]));
            if (!oa_plan_layer(s, R, N_l[l], nullptr, nullptr)) {
                if (where_env) *where_env = e;
                if (where_layer) *where_layer = l;
                return kOaPlan;
            }
            out[(size_t)l * n_env + e] = s;
        }
    return kOaOk;
}

// the bilinear stage in T: rows first along x, then along y
template <typename T>
AO_OA_HD inline T oa_blend(T p00, T p01, T p10, T p11, T ty, T tx) {
#pragma clang fp contract(off)
    const T a = ((T)1 - tx) * p00 + tx * p01;
    const T b = ((T)1 - tx) * p10 + tx * p11;
    return ((T)1 - ty) * a + ty * b;
}

}  // namespace ao
