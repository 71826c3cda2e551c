// Wavefront modes on the device (aoenv_set_wavefront_basis, aoenv_project_wavefront, aoenv_set_wavefront_record): the modal
// coefficients of the residual and of the atmosphere OPD, the reference's `opd2m @ tel.OPD[xpupil, ypupil]` with
// opd2m = pinv(M2OPD) (MAIN_CODE/OOPAOEnv/SinEnv.py:150-204, predictiveControl/EOF/EOF_POL.py:105-123, make_dataset.py:84-103,
// Plots/AO_plots.py zernike_dist).
// ONE host/device source: wavefront_kernels.hip compiles it for the device, env.hip and tests/native/wavefront_driver.cpp for the host.
//   env e, K modes, R^2 pixels, T the env dtype:
//     c[e][m] = s * sum over q < R^2 of P[m][q] * X[e][q]
//     P   the projector [K][n_pix] scattered to the full grid in T: pupil pixel p (the p-th set pixel of the pupil in row-major
//         order, np.where(tel.pupil == 1)) goes to its column q, every other column is 0; the row stride is R^2 rounded up to a
//         multiple of 4 elements (16-byte loads of float32 rows), the pad is 0
//     residual    X = AOENV_B_PHASE [rad at the source wavelength], s = (T)(lambda_src / 2 pi): metres, the coefficients of tel.OPD
//     atmosphere  X = AOENV_B_OPD_ATM [m], no scale: the coefficients of the pupil-masked atm.OPD (P is 0 outside the pupil)
// Order of the sum.  [0, R^2) is cut into n_slices slices of slice_len elements (the last one shorter), both from (R^2, K) alone
// (wf_plan): never from n_env or from an env's place in the shard.  Every slice is summed on its own from 0 -- by the general kernel
// as ONE fma chain in index order (wf_chain), by the matrix-core kernel in the order of wavefront_kernels.hip -- the slice sums
// are then added in slice order starting from slice 0's, and s is applied once to the total, one multiply in T (wf_scale).  No
// atomics: the same env with the same buffers has the same bits in any shard.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define AO_WF_HD __host__ __device__
#else
#define AO_WF_HD
#endif

namespace ao {

constexpr int kWfMaxModes = 1024;      // AOENV_MAX_WF_MODES
constexpr int kWfMaxSlices = 64;
constexpr int kWfRound = 16;           // elements of a row one matrix-core round of a wave takes: slice_len is a multiple of it

struct WfPlan {
    int n_slices, slice_len;
};

// The slices of (R^2, K).  A slice costs one [n_env][K] slab written and read again against n_env * slice_len elements of X read:
// slices stay at least 4 K elements long, so the slabs move at most a quarter of what X does; up to kWfMaxSlices of them.
AO_WF_HD inline WfPlan wf_plan(int r2, int n_modes) {
    int want = r2 / (4 * n_modes);
    want = want < 1 ? 1 : want > kWfMaxSlices ? kWfMaxSlices : want;
    int len = (r2 + want - 1) / want;
    len = (len + kWfRound - 1) / kWfRound * kWfRound;
    WfPlan p;
    p.slice_len = len;
    p.n_slices = (r2 + len - 1) / len;
    return p;
}
AO_WF_HD inline int wf_slice_lo(const WfPlan& p, int z) { return z * p.slice_len; }
AO_WF_HD inline int wf_slice_hi(const WfPlan& p, int z, int r2) {
    const int hi = (z + 1) * p.slice_len;
    return hi < r2 ? hi : r2;
}

// row stride of P: R^2 rounded up to 4 elements
AO_WF_HD inline int wf_row_stride(int r2) { return (r2 + 3) & ~3; }

AO_WF_HD inline float wf_fma(float a, float b, float c) { return __builtin_fmaf(a, b, c); }
AO_WF_HD inline double wf_fma(double a, double b, double c) { return __builtin_fma(a, b, c); }

// one slice of one (env, mode) as the general kernel sums it
template <typename T>
AO_WF_HD inline T wf_chain(const T* p_row, const T* x_row, int lo, int hi) {
    T v = (T)0;
    for (int q = lo; q < hi; ++q) v = wf_fma(p_row[q], x_row[q], v);
    return v;
}

// the scale of the residual: one multiply in T
template <typename T>
AO_WF_HD inline T wf_scale(T sum, T s) {
#pragma clang fp contract(off)
    return sum * s;
}

// ---- the host side: what aoenv_set_wavefront_basis checks and builds ----------------------------------------------------------------
enum WfRefusal {
    kWfOk = 0,
    kWfModes,          // K outside [1, min(n_pix, kWfMaxModes)]
    kWfPix,            // n_pix < 1
    kWfNoPupil,        // no pupil uploaded
    kWfPupilCount,     // n_pix is not the number of pupil pixels
    kWfNullTable,
    kWfNotFinite       // an entry that is not finite (in T: a float64 beyond float32's range counts)
};

template <typename T>
inline WfRefusal wf_validate(int n_modes, int n_pix, const uint8_t* pupil, int r2, const double* opd2m, size_t* where) {
    if (n_pix < 1) return kWfPix;
    if (n_modes < 1 || n_modes > n_pix || n_modes > kWfMaxModes) return kWfModes;
    if (!pupil || r2 < 1) return kWfNoPupil;
    int count = 0;
    for (int q = 0; q < r2; ++q) count += pupil[q] != 0;
    if (count != n_pix) return kWfPupilCount;
    if (!opd2m) return kWfNullTable;
    const size_t n = (size_t)n_modes * n_pix;
    const double t_max = sizeof(T) == 4 ? 3.4028234663852886e38 : 1.7976931348623157e308;
    for (size_t i = 0; i < n; ++i)
        if (!isfinite(opd2m[i]) || fabs(opd2m[i]) > t_max) {
            if (where) *where = i;
            return kWfNotFinite;
        }
    return kWfOk;
}

// P [K][wf_row_stride(r2)] from opd2m [K][n_pix]; `out` is overwritten whole
template <typename T>
inline void wf_scatter(const double* opd2m, int n_modes, int n_pix, const uint8_t* pupil, int r2, T* out) {
    const size_t ld = (size_t)wf_row_stride(r2);
    for (size_t i = 0; i < (size_t)n_modes * ld; ++i) out[i] = (T)0;
    int p = 0;
    for (int q = 0; q < r2; ++q) {
        if (!pupil[q]) continue;
        for (int m = 0; m < n_modes; ++m) out[(size_t)m * ld + q] = (T)opd2m[(size_t)m * n_pix + p];
        ++p;
    }
}

// c[e][m] as the general kernel and the finish kernel form it (scale == null: the atmosphere)
template <typename T>
inline T wf_project_one(const T* p_row, const T* x_row, int r2, int n_modes, const T* scale) {
    const WfPlan pl = wf_plan(r2, n_modes);
    T acc = wf_chain<T>(p_row, x_row, 0, wf_slice_hi(pl, 0, r2));
    for (int z = 1; z < pl.n_slices; ++z) acc += wf_chain<T>(p_row, x_row, wf_slice_lo(pl, z), wf_slice_hi(pl, z, r2));
    return scale ? wf_scale<T>(acc, *scale) : acc;
}

}  // namespace ao
