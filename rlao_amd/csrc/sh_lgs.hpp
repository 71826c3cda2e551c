// Laser-guide-star Shack-Hartmann (OOPAO/ShackHartmann.py:396-503, 554-556): every valid lenslet's UNBINNED n x n spot intensity
// (n = 2 p) is convolved with a kernel of that lenslet's own -- the projected sodium column -- before the 2 x 2 binning, the camera
// and the centroid:
//     I = fftshift(abs(ifft2(fft2(I) * C)), axes = [1, 2]);   camera = bin2x2(I)                      C[k] = fft2(K[k])
// In real space, with the shift and the binning folded into the taps (the host forms them, rlao_amd/calib.py::lgs_binned_taps):
//     Kb[x][y]     = K[x][y] + K[x+1][y] + K[x][y+1] + K[x+1][y+1]                                      (indices mod n)
//     camera[P][Q] = sum_{s,t} I[s][t] Kb[(2 P + n/2 - s) mod n][(2 Q + n/2 - t) mod n]
// so the device needs n^2 taps per lenslet and forms p^2 outputs.  The table is [n_tab][n_valid][n*n] in the env dtype, n_tab = the
// shard's env count or 1 (read with a per-env stride of 0).  The taps outside a cyclic box [x0, x0 + nx) x [y0, y0 + ny) (mod n)
// are zero for every lenslet of the table and the kernel's tap loop runs over the box alone.
// This header is plain C++: the validation of a table and the launch plan are host code and have a native driver
// (tests/native/lgs_driver.cpp).
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>

namespace ao {

// Order of the sum (the determinism argument): a camera pixel adds its taps in ascending (x, y) of the tap index, x outermost,
// whatever the box is -- a box that wraps is walked as its two pieces in ascending order (lgs_ranges).  A zero tap adds exactly
// nothing (the intensities are finite), so an env's bits depend on its own taps and on p alone: not on the box, which is the union over
// the table, nor on the other envs' taps, nor on the env's place in the shard.

constexpr size_t kLgsLdsCap = 64 * 1024;             // what a launch gets without asking for more

// LDS bytes of k_sh_spots_lgs with L lenslets (waves) per workgroup: the twiddles [n], per lenslet the field [p][p] and the
// half transform [p][n] (complex, as in k_sh_spots) and the unbinned intensity, four parity blocks of [n][n] (real; a block holds its
// p x p samples twice along each axis, so that a cyclic shift is a plain offset)
inline size_t lgs_lds_bytes(int p, int L, size_t esz) {
    const size_t n = 2 * (size_t)p, pp = (size_t)p * p;
    return 2 * esz * (n + (size_t)L * (pp + p * n)) + esz * (size_t)L * 4 * n * n;
}

// lenslets per workgroup: 4 like k_sh_spots where the LDS image fits, else 2, else 1; 0: not even one fits (refused)
inline int lgs_lenslets_per_group(int p, size_t esz) {
    if (p < 1) return 0;
    for (int L = 4; L >= 1; L >>= 1)
        if (lgs_lds_bytes(p, L, esz) <= kLgsLdsCap) return L;
    return 0;
}

// a cyclic interval [start, start + len) mod n as at most two plain ones in ascending order: [lo[0], hi[0]) and [lo[1], hi[1])
struct LgsRanges {
    int lo[2], hi[2];
};
inline LgsRanges lgs_ranges(int start, int len, int n) {
    LgsRanges r{};
    if (start + len <= n) {
        r.lo[0] = start; r.hi[0] = start + len;
        r.lo[1] = r.hi[1] = 0;                       // (empty)
    } else {
        r.lo[0] = 0; r.hi[0] = start + len - n;
        r.lo[1] = start; r.hi[1] = n;
    }
    return r;
}
inline bool lgs_in_range(const LgsRanges& r, int x) { return (x >= r.lo[0] && x < r.hi[0]) || (x >= r.lo[1] && x < r.hi[1]); }

enum LgsVerdict {
    kLgsOk = 0,
    kLgsBytes,                                       // the byte count is not n_tab n_valid n^2 doubles
    kLgsBox,                                         // the box is not inside [0, n): x0, y0 in [0, n), nx, ny in [1, n]
    kLgsNotFinite,                                   // a tap is NaN or infinite, also after rounding to float32 (narrow)
    kLgsNegative,                                    // a tap is negative
    kLgsOutside,                                     // a non-zero tap lies outside the box
    kLgsZeroSum                                      // a lenslet's taps sum to zero (after rounding to float32 if narrow)
};
struct LgsCheck {
    LgsVerdict verdict = kLgsOk;
    size_t table = 0, lenslet = 0, tap = 0;          // where (verdicts from kLgsNotFinite on)
};

// box = {x0, y0, nx, ny}; narrow: the shard holds the taps as float32
inline LgsCheck lgs_validate(const double* taps, size_t bytes, int n_tab, int n_valid, int n, const int32_t box[4], bool narrow) {
    LgsCheck c;
    const size_t nn = (size_t)n * n;
    if (n_tab < 1 || n_valid < 1 || n < 2 || bytes != (size_t)n_tab * n_valid * nn * sizeof(double)) {
        c.verdict = kLgsBytes;
        return c;
    }
    if (box[0] < 0 || box[0] >= n || box[1] < 0 || box[1] >= n || box[2] < 1 || box[2] > n || box[3] < 1 || box[3] > n) {
        c.verdict = kLgsBox;
        return c;
    }
    const LgsRanges rx = lgs_ranges(box[0], box[2], n), ry = lgs_ranges(box[1], box[3], n);
    for (int t = 0; t < n_tab; ++t)
        for (int s = 0; s < n_valid; ++s) {
            const double* k = taps + ((size_t)t * n_valid + s) * nn;
            double sum = 0;
            c.table = t;
            c.lenslet = s;
            for (size_t q = 0; q < nn; ++q) {
                const double v = narrow ? (double)(float)k[q] : k[q];
                c.tap = q;
                if (!std::isfinite(v)) { c.verdict = kLgsNotFinite; return c; }
                if (v < 0) { c.verdict = kLgsNegative; return c; }
                if (v != 0 && !(lgs_in_range(rx, (int)(q / n)) && lgs_in_range(ry, (int)(q % n)))) { c.verdict = kLgsOutside; return c; }
                sum += v;
            }
            c.tap = 0;
            if (!(sum > 0)) { c.verdict = kLgsZeroSum; return c; }
        }
    c.table = c.lenslet = 0;
    return c;
}

}  // namespace ao
