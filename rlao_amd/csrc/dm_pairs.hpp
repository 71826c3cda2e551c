// Per-env actuator factor pairs (aoenv_set_dm_pairs): a mirror whose actuator grid is rotated is no longer Gy C Gx^T, but every
// actuator's Gaussian is still a product of a y factor and an x factor, so the surface of env e is
//     S_e[y][x] = sum_k c_e[k] py_e[y][k] px_e[x][k],   k over the A valid actuators,
// one product (Py diag(c)) Px^T with K = A per env.  Host only: aoenv_set_dm_pairs and the stand-alone driver
// tests/native/dm_pairs_driver.cpp share this one re-layout; the kernels are in dm_pairs_kernels.hip.
//
// One pair of float64 tables py, px [R][A] is kept on the device in these layouts:
//   t   [A][R]              env dtype, the TRANSPOSE (k_dm_pairs<T>: lanes along x read consecutive elements for every k;
//                           aoenv_get_dm_pairs transposes back)
//   ga  [R pad 128 / 16][ga_stride / 4][64 lanes][4]   float32 MFMA operand table, the layout of the separable mirror's gxa / gya
//                           (ga_index(), common.hpp; dm_fill_ga, dm_tables.hpp) with n_act := A: zero padded to R pad 128 rows and
//                           to 4 ga_stride >= A actuators, so the padding rows and the K tail of k_dm_pairs_mfma multiply zeros
// A set is n_env such blocks one after the other, env e at element e * block of every layout.
// Device bytes per env: 2 R A esz + 2 (R pad 128) 4 ga_stride 4.
#pragma once
#include <cstddef>
#include <vector>

#include "dm_tables.hpp"

namespace ao {

struct PairsLayout {
    int R = 0, A = 0;
    DmLayout ga() const { DmLayout l; l.R = R; l.n_act = A; l.ga_stride = dm_ga_stride(A); return l; }
    int ga_stride() const { return dm_ga_stride(A); }
    int r_pad() const { return ga().r_pad(); }
    int k_pad() const { return 4 * ga_stride(); }                              // actuators the operand table has room for
    size_t t_elems() const { return (size_t)A * R; }                           // elements of one t block (and of the float64 input)
    size_t ga_elems() const { return ga().ga_elems(); }                        // floats of one operand table
    // device bytes of ONE env's tables at element size esz: pyt, pxt, pya, pxa
    size_t bytes(size_t esz) const { return 2 * t_elems() * esz + 2 * ga_elems() * sizeof(float); }
};

// d [R][A] float64 -> t [A][R] in the env dtype (one rounding per element)
template <typename T>
void pairs_fill_t(const PairsLayout& L, const double* d, T* t) {
    for (int x = 0; x < L.R; ++x)
        for (int k = 0; k < L.A; ++k) t[(size_t)k * L.R + x] = (T)d[(size_t)x * L.A + k];
}
// ... and back, widened: what aoenv_get_dm_pairs returns
template <typename T>
void pairs_read_t(const PairsLayout& L, const T* t, double* d) {
    for (int x = 0; x < L.R; ++x)
        for (int k = 0; k < L.A; ++k) d[(size_t)x * L.A + k] = (double)t[(size_t)k * L.R + x];
}

// Every layout of n_env pairs of tables (h_py, h_px: [n_env][R][A] float64), env e's block at e * (elements of one block).
template <typename T>
struct PairsHostTables {
    std::vector<T> pyt, pxt;
    std::vector<float> pya, pxa;
};
template <typename T>
void pairs_relayout(const PairsLayout& L, int n_env, const double* h_py, const double* h_px, PairsHostTables<T>& out) {
    const DmLayout g = L.ga();
    out.pyt.resize(n_env * L.t_elems());
    out.pxt.resize(n_env * L.t_elems());
    out.pya.resize(n_env * L.ga_elems());
    out.pxa.resize(n_env * L.ga_elems());
    for (int e = 0; e < n_env; ++e) {
        const double* dy = h_py + (size_t)e * L.t_elems();
        const double* dx = h_px + (size_t)e * L.t_elems();
        pairs_fill_t<T>(L, dy, out.pyt.data() + (size_t)e * L.t_elems());
        pairs_fill_t<T>(L, dx, out.pxt.data() + (size_t)e * L.t_elems());
        dm_fill_ga(g, dy, out.pya.data() + (size_t)e * L.ga_elems());
        dm_fill_ga(g, dx, out.pxa.data() + (size_t)e * L.ga_elems());
    }
}

// what the kernels of dm_pairs_kernels.hip are handed
template <typename T>
struct PairsArgs {
    const T* coefs;          // [E][A] the command on the mirror
    const T* pyt;            // [E] x t
    const T* pxt;
    const float* pya;        // [E] x ga
    const float* pxa;
    T* out;                  // [E][R*R] dm_opd
    int R, A, ga_stride;
    size_t t_env, ga_env;    // elements between the envs' blocks
};
// general: k_dm_pairs<T> on float32 too (float64 always runs it)
template <typename T>
int launch_dm_pairs(const PairsArgs<T>& a, int n_env, bool general, hipStream_t st);

}  // namespace ao
