// Science camera on the device (aoenv_set_science, aoenv_science_psf, aoenv_set_science_accumulator): a W x W window around the
// core of the short-exposure PSF of every env, and its sum over the frames of a loop -- the long exposure the reference's
// evaluation scripts form on the host from full renders (MAIN_CODE/predictiveControl/POL_error_CL.py: tel.computePSF(4),
// PSF[175:-175, 175:-175], mean; MAIN_CODE/integrator_network.py:134-138; MAIN_CODE/OOPAOEnv/OOPAOEnv.py:473-482 render4plot).
// ONE host/device source: science_kernels.hip compiles it for the device, env.hip and tests/native/science_driver.cpp for the host.
//   M = zp R (even), the reference's PropagateField at oversampling 2 (OOPAO/Telescope.py:296-351): the field is padded by
//   pad = ceil((2 M - R) / 2) on every side to n_fft = R + 2 pad (2 M for even R, 2 M + 1 for odd R: np.pad adds the same on
//   both sides), multiplied by the phasor exp(-i pi (x + y) / n_fft), transformed between ifftshift and fftshift, divided by
//   n_fft, cropped to its first 2 M rows and columns, squared and sum-binned 2 x 2.  The shifts, the padding offset and the
//   phasor are separable, so oversampled row j of the image is the product with ONE row of a table:
//     F[j][x] = exp(-2 pi i (j - M)(x + pad - M) / n_fft) * exp(-i pi (x + pad) / n_fft) = exp(-i pi m / n_fft),
//     m = (2 (j - M)(x + pad - M) + (x + pad)) mod 2 n_fft          (the integer is reduced BEFORE the angle is formed)
//   evaluated in float64 (the integer folded into the first octant first: sci_dft_entry) and rounded once to the env dtype.
//   The window's output pixel (a, b) is pixel (M/2 - W/2 + a, M/2 - W/2 + b) of the full image: oversampled rows j in
//   [M - W, M + W), U = 2 W of them, row u of the table is j = M - W + u.
//     P = F E F^T  (U x U complex),  E[y][x] = amp[y][x] exp(i phase[y][x])  (0 where amp == 0: outside the pupil)
//     out[a][b] = ((|P[2a][2b]|^2 + |P[2a+1][2b]|^2) + (|P[2a][2b+1]|^2 + |P[2a+1][2b+1]|^2)) * (T)(1 / n_fft^2)
//   |.|^2 = fma(re, re, im * im); ONE multiplication by the scale, in T.
// The table is stored as two planes [2][up][rp] (re, then im), rows and columns zero padded to the tile: rp = R rounded up to 16,
// up = U rounded up to 32.  Both kernels read this one table.  Nothing but (R, W) goes into the plan; zp only moves n_fft.
// Order of the sums.  The general kernel: T1[y][c] = sum_x E[y][x] F[c][x] and P[j][c] = sum_y F[j][y] T1[y][c] as fma chains in
// ascending index (sci_cmac).  The matrix-core kernel: the same two products on v_mfma_f32_16x16x4_f32 in the fixed order of
// science_kernels.hip.  Neither depends on n_env or on the env's place in the shard, and there are no atomics.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define AO_SCI_HD __host__ __device__
#else
#define AO_SCI_HD
#endif

namespace ao {

constexpr int kSciMaxZp = 8;
constexpr int kSciTileK = 16;          // R rounds up to this: the rows of a chunk and a k round of the matrix-core kernel
constexpr int kSciColBlock = 32;       // oversampled columns of a workgroup of the matrix-core kernel; U rounds up to this
constexpr int kSciMaxTilesPerWave = 8; // 16-row tiles of P a wave keeps in registers (16 accumulator registers each)
constexpr int kSciGeneralCols = 8;     // oversampled columns of a workgroup of the general kernel
constexpr int kSciLdsLimit = 64 * 1024;
enum { kSciLog10 = 1 };                // AOENV_SCI_LOG10

struct SciGeom {
    int R, zp, W;
    int M;             // zp R: the full image is M x M
    int U;             // 2 W oversampled rows and columns
    int pad, n_fft;    // the reference's padding and transform length
};

AO_SCI_HD inline SciGeom sci_geom(int R, int zp, int W) {
    SciGeom g;
    g.R = R; g.zp = zp; g.W = W;
    g.M = zp * R;
    g.U = 2 * W;
    g.pad = (2 * g.M - R + 1) / 2;
    g.n_fft = R + 2 * g.pad;
    return g;
}

// the tile plan of both kernels, from (R, W) alone
struct SciPlan {
    int rp, up;               // padded strides of the table
    int n_row_tiles;          // 16-row tiles of P: ceil(U / 16)
    int tiles_per_wave;       // 1 .. 8: ceil(n_row_tiles / 4) up to the 8 a wave's registers hold
    int n_row_groups;         // workgroups along the rows of P: 4 waves x tiles_per_wave tiles each
    int n_col_blocks;         // workgroups along its columns: up / 32
    int lds_bytes;            // of the matrix-core kernel
    int mfma_ok;              // 0: the matrix-core kernel refuses (LDS), the general kernel serves
    int general_blocks;       // column blocks of the general kernel
};

AO_SCI_HD inline int sci_round_up(int v, int to) { return (v + to - 1) / to * to; }
// LDS of the matrix-core kernel: the chunk's field (re, im: 16 rows, stride rp + 4) and the chunk's first product transposed
// (re, im: 32 columns, stride 20), float32
AO_SCI_HD inline int sci_mfma_lds_bytes(int rp) { return (2 * kSciTileK * (rp + 4) + 2 * kSciColBlock * 20) * 4; }

AO_SCI_HD inline SciPlan sci_plan(int R, int W) {
    SciPlan p;
    const int U = 2 * W;
    p.rp = sci_round_up(R, kSciTileK);
    p.up = sci_round_up(U, kSciColBlock);
    p.n_row_tiles = (U + 15) / 16;
    const int per_wave = (p.n_row_tiles + 3) / 4;
    p.tiles_per_wave = per_wave < kSciMaxTilesPerWave ? per_wave : kSciMaxTilesPerWave;
    p.n_row_groups = (p.n_row_tiles + 4 * p.tiles_per_wave - 1) / (4 * p.tiles_per_wave);
    p.n_col_blocks = p.up / kSciColBlock;
    p.lds_bytes = sci_mfma_lds_bytes(p.rp);
    p.mfma_ok = p.lds_bytes <= kSciLdsLimit ? 1 : 0;
    p.general_blocks = (U + kSciGeneralCols - 1) / kSciGeneralCols;
    return p;
}
AO_SCI_HD inline size_t sci_table_elems(const SciPlan& p) { return (size_t)2 * p.up * p.rp; }

AO_SCI_HD inline float sci_fma(float a, float b, float c) { return __builtin_fmaf(a, b, c); }
AO_SCI_HD inline double sci_fma(double a, double b, double c) { return __builtin_fma(a, b, c); }

// (acc_r, acc_i) += (ar + i ai)(br + i bi): the step of the general kernel's chains
template <typename T>
AO_SCI_HD inline void sci_cmac(T ar, T ai, T br, T bi, T& acc_r, T& acc_i) {
    acc_r = sci_fma(ar, br, acc_r);
    acc_r = sci_fma(-ai, bi, acc_r);
    acc_i = sci_fma(ar, bi, acc_i);
    acc_i = sci_fma(ai, br, acc_i);
}
template <typename T>
AO_SCI_HD inline T sci_power(T re, T im) { return sci_fma(re, re, im * im); }
// one output pixel from the four oversampled powers p[row][column] of its 2 x 2 cell: one multiply by the scale, in T
template <typename T>
AO_SCI_HD inline T sci_bin(T p00, T p10, T p01, T p11, T scale) {
#pragma clang fp contract(off)
    const T s0 = p00 + p10, s1 = p01 + p11;
    const T s = s0 + s1;
    return s * scale;
}
template <typename T>
AO_SCI_HD inline T sci_scale(const SciGeom& g) { return (T)(1.0 / ((double)g.n_fft * (double)g.n_fft)); }

// ---- the host side: what aoenv_set_science checks and builds --------------------------------------------------------------------
enum SciRefusal {
    kSciOk = 0,
    kSciZp,            // zp outside [1, 8]
    kSciOddImage,      // zp * R odd
    kSciWindowOdd,     // W odd
    kSciWindowRange,   // W outside [2, zp * R]
    kSciFirstFrame,    // first_frame < 0
    kSciFlags,         // a bit other than AOENV_SCI_LOG10
    kSciNotFinite      // an entry of h_dft that is not finite in T
};

template <typename T>
inline SciRefusal sci_validate(int R, int zp, int W, int first_frame, int flags, const double* h_dft, size_t* where) {
    if (zp < 1 || zp > kSciMaxZp) return kSciZp;
    if ((zp * R) % 2) return kSciOddImage;
    if (W % 2) return kSciWindowOdd;
    if (W < 2 || W > zp * R) return kSciWindowRange;
    if (first_frame < 0) return kSciFirstFrame;
    if (flags & ~kSciLog10) return kSciFlags;
    if (h_dft) {
        const size_t n = (size_t)2 * W * R * 2;
        const double t_max = sizeof(T) == 4 ? 3.4028234663852886e38 : 1.7976931348623157e308;
        for (size_t i = 0; i < n; ++i)
            if (!isfinite(h_dft[i]) || fabs(h_dft[i]) > t_max) {
                if (where) *where = i;
                return kSciNotFinite;
            }
    }
    return kSciOk;
}

// entry (u, x) of the table in float64: row u is oversampled row j = M - W + u
inline void sci_dft_entry(const SciGeom& g, int u, int x, double* re, double* im) {
    const int64_t two_n = 2 * (int64_t)g.n_fft;
    const int64_t a = (int64_t)u - g.W, b = (int64_t)x + g.pad - g.M, c = (int64_t)x + g.pad;
    int64_t m = (2 * a * b + c) % two_n;
    if (m < 0) m += two_n;
    // exp(-i pi m / n) through the symmetries of the circle ON THE INTEGER: the angle handed to cos / sin lies in [0, pi / 4], and
    // the entries on the axes and the diagonals' zeros are exact
    const int64_t n = g.n_fft;
    const bool neg_sin = m > n;                    // the lower half: (cos, sin)(2 pi - t) = (cos, -sin)(t)
    if (neg_sin) m = two_n - m;
    const bool neg_cos = 2 * m > n;                // the second quadrant: (cos, sin)(pi - t) = (-cos, sin)(t)
    if (neg_cos) m = n - m;
    const bool swap = 4 * m > n;                   // above pi / 4: (cos, sin)(pi / 2 - t) = (sin, cos)(t)
    const int64_t num = swap ? n - 2 * m : 2 * m;  // t = pi num / (2 n), num in [0, n / 2]
    const double ang = 3.14159265358979323846 * (double)num / (double)(2 * n);
    const double c0 = swap ? sin(ang) : cos(ang), s0 = swap ? cos(ang) : sin(ang);
    *re = neg_cos ? -c0 : c0;
    *im = neg_sin ? s0 : -s0;
}

// the padded table [2][up][rp] in T: from h_dft [U][R][2] when given, the library's otherwise; `out` is overwritten whole
template <typename T>
inline void sci_fill_table(const SciGeom& g, const SciPlan& p, const double* h_dft, T* out) {
    const size_t plane = (size_t)p.up * p.rp;
    for (size_t i = 0; i < 2 * plane; ++i) out[i] = (T)0;
    for (int u = 0; u < g.U; ++u)
        for (int x = 0; x < g.R; ++x) {
            double re, im;
            if (h_dft) {
                re = h_dft[((size_t)u * g.R + x) * 2];
                im = h_dft[((size_t)u * g.R + x) * 2 + 1];
            } else {
                sci_dft_entry(g, u, x, &re, &im);
            }
            out[(size_t)u * p.rp + x] = (T)re;
            out[plane + (size_t)u * p.rp + x] = (T)im;
        }
}

}  // namespace ao
