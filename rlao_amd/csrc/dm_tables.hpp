// Host re-layout of the separable DM's influence factors (host only: aoenv_upload(AOENV_C_DM_GX / _GY), aoenv_set_dm_env and the
// stand-alone driver tests/native/dm_env_driver.cpp share this one routine).
//
// One pair of float64 tables gx, gy [R][n_act] (AOENV_C_DM_GX / _GY) is kept on the device in these layouts:
//   g    [R][n_act]                 env dtype, row-major              (k_phase<T>: pb.gx / pb.gy)
//   gxt  [n_act pad 4][R pad 128]   env dtype, transpose of gx, zero padded   (kept up to date, but NO kernel reads it at present:
//                                   the phase kernels take gx through the operand table; per env it is held for parity with the
//                                   shared tables and costs (n_act pad 4)(R pad 128) elements of device memory that nothing loads)
//   ga   [R pad 128 / 16][ga_stride / 4][64 lanes][4]   float32 MFMA operand table (ga_index(), common.hpp), zero padded
//                                                       (k_env_step_sh6, k_phase_mfma*, k_dm_rows: gxa / gya)
// A per-env set (aoenv_set_dm_env) is n_env such blocks one after the other, env e at element e * block of every layout.
#pragma once
#include <cstddef>
#include <vector>

#include "common.hpp"

namespace ao {

struct DmLayout {
    int R = 0, n_act = 0, ga_stride = 8;
    int r_pad() const { return cdiv(R, 128) * 128; }
    int act_pad() const { return (n_act + 3) & ~3; }
    size_t g_elems() const { return (size_t)R * n_act; }                       // elements of one g block (and of the float64 input)
    size_t gxt_elems() const { return (size_t)act_pad() * r_pad(); }
    size_t ga_elems() const { return (size_t)r_pad() * 4 * ga_stride; }        // floats of one operand table
    // device bytes of ONE env's tables at element size esz: gx, gy, gxt, gxa, gya
    size_t bytes(size_t esz) const { return (2 * g_elems() + gxt_elems()) * esz + 2 * ga_elems() * sizeof(float); }
};
inline int dm_ga_stride(int n_act) { int s = ((cdiv(n_act, 4) + 3) / 4) * 4; return s < 8 ? 8 : s; }

// d [R][n_act] float64 -> g in the env dtype (one rounding per element)
template <typename T>
void dm_fill_g(const DmLayout& L, const double* d, T* g) {
    for (size_t i = 0; i < L.g_elems(); ++i) g[i] = (T)d[i];
}
// ... -> the zero padded transpose [act_pad][r_pad]
template <typename T>
void dm_fill_gxt(const DmLayout& L, const double* d, T* gxt) {
    const int rp = L.r_pad();
    for (size_t i = 0; i < L.gxt_elems(); ++i) gxt[i] = (T)0;
    for (int x = 0; x < L.R; ++x)
        for (int ix = 0; ix < L.n_act; ++ix) gxt[(size_t)ix * rp + x] = (T)d[(size_t)x * L.n_act + ix];
}
// ... -> the float32 MFMA operand table, zero padded to r_pad rows and ga_stride k steps per (row, q)
inline void dm_fill_ga(const DmLayout& L, const double* d, float* ga) {
    for (size_t i = 0; i < L.ga_elems(); ++i) ga[i] = 0.f;
    for (int x = 0; x < L.R; ++x)
        for (int k = 0; k < L.n_act; ++k) ga[ga_index(x, k, L.ga_stride)] = (float)d[(size_t)x * L.n_act + k];
}

// Every layout of n_env pairs of tables (h_gx, h_gy: [n_env][R][n_act] float64), env e's block at e * (elements of one block).
template <typename T>
struct DmHostTables {
    std::vector<T> gx, gy, gxt;
    std::vector<float> gxa, gya;
};
template <typename T>
void dm_relayout(const DmLayout& L, int n_env, const double* h_gx, const double* h_gy, DmHostTables<T>& out) {
    out.gx.resize(n_env * L.g_elems());
    out.gy.resize(n_env * L.g_elems());
    out.gxt.resize(n_env * L.gxt_elems());
    out.gxa.resize(n_env * L.ga_elems());
    out.gya.resize(n_env * L.ga_elems());
    for (int e = 0; e < n_env; ++e) {
        const double* dx = h_gx + (size_t)e * L.g_elems();
        const double* dy = h_gy + (size_t)e * L.g_elems();
        dm_fill_g<T>(L, dx, out.gx.data() + (size_t)e * L.g_elems());
        dm_fill_g<T>(L, dy, out.gy.data() + (size_t)e * L.g_elems());
        dm_fill_gxt<T>(L, dx, out.gxt.data() + (size_t)e * L.gxt_elems());
        dm_fill_ga(L, dx, out.gxa.data() + (size_t)e * L.ga_elems());
        dm_fill_ga(L, dy, out.gya.data() + (size_t)e * L.ga_elems());
    }
}

}  // namespace ao
