// Geometric Shack-Hartmann (OOPAO/ShackHartmann.py:382-394, 676-695, is_geometric=True): the signal is the pupil-masked gradient
// of the UNMASKED phase, summed per lenslet and divided by slopes_units -- no spots, no camera, no threshold, no reference slopes.
//     gx = np.gradient(phi, axis=0) * pupil,  gy = np.gradient(phi, axis=1) * pupil          (central differences inside, the
//                                                                                              one-sided first-order ones on the
//                                                                                              first / last row and column)
//     signal = [bin(gy) | bin(gx)][valid] / (slopes_units pixelSize),   bin = the sum over a lenslet's p x p pixels
// The library has no telescope diameter: the host folds 1 / pixelSize into the uploaded AOENV_C_WFS_UNITS.
// This header is plain C++ (the launch plan of the fused tail is host code and has a native driver, tests/native/geometric_driver.cpp).
#pragma once
#include <cstddef>

namespace ao {

// Order of the sums (the determinism argument): a lenslet's p^2 terms are added per column over its p rows in ascending row order,
// then the p column sums in ascending column order -- by one lane each, without atomics.  The order depends on p alone: an env has the
// same bits in any shard, at any place in it, from the stand-alone kernel and from the fused tail, whatever band height either takes.

// LDS elements (of esz bytes) of a band of g lenslet rows: the staged rows (the band's g p rows and one neighbour row on each side),
// the two column sums per band row, the two totals per lenslet, and the band's pupil flags, one byte a pixel, rounded up to elements
inline size_t geo_band_elems(int R, int n_subap, int g, size_t esz) {
    const int p = R / n_subap;
    return (size_t)(g * p + 2) * R + (size_t)2 * g * R + (size_t)2 * g * n_subap + ((size_t)g * p * R + esz - 1) / esz;
}

// elements the tail itself needs in front of the band (k_sh_tail's layout): slopes, observation image, modal coefficients
inline size_t geo_tail_base_elems(int n_valid, int n_act, int n_modes) {
    return (size_t)2 * n_valid + (size_t)n_act * n_act + (size_t)n_modes;
}

// static LDS of k_geo_tail beside its dynamic image (the reduction scratch of tail_from_slopes: 16 doubles)
constexpr size_t kGeoTailStaticLds = 128;

// Band height of the fused geometric tail (k_geo_tail): the largest g <= n_subap whose LDS image fits, with the tail's own arrays
// and the kernel's static LDS, the 64 KB a launch gets without asking for more.  0: it does not fit, the step takes the separate
// kernels.
inline int geo_tail_band(int R, int n_subap, int n_valid, int n_act, int n_modes, size_t esz) {
    if (n_subap < 1 || R < 2 || R % n_subap) return 0;
    const size_t cap = 64 * 1024 - kGeoTailStaticLds;
    const size_t base = geo_tail_base_elems(n_valid, n_act, n_modes);
    int g = 0;
    while (g < n_subap && esz * (base + geo_band_elems(R, n_subap, g + 1, esz)) <= cap) ++g;
    return g;
}

// LDS bytes of the stand-alone kernel (one lenslet row per workgroup); above 160 KB the geometry is refused
inline size_t geo_row_lds_bytes(int R, int n_subap, size_t esz) { return esz * geo_band_elems(R, n_subap, 1, esz); }

}  // namespace ao
