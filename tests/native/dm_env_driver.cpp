// Host driver of the DM table re-layout (rlao_amd/csrc/dm_tables.hpp: the routine aoenv_upload(AOENV_C_DM_GX / _GY) and
// aoenv_set_dm_env share).  No arguments: for 3 envs at (R, n_act) = (24, 5), (30, 6), (144, 37), in float and in double, it fills
// gx / gy with values that name their own (env, table, row, actuator), runs dm_relayout and checks EVERY element of every layout:
//   g    [e][x][k]                                        the value rounded to the dtype
//   gxt  [e][k][x] at stride R pad 128, k < n_act pad 4   the value, zero in the padding
//   ga   [e] ga_index(x, k, ga_stride)                    the value as float; every other slot of the block zero
// ga_index() is checked against the operand layout restated here from its definition (tile, k quad, lane, k step), and is a bijection
// onto distinct slots of ONE env's block, so that env blocks cannot overlap.  Prints "ok <checks>"; any mismatch is a message and exit 1.
// Built with `hipcc -x hip --cuda-host-only`; tests/test_dm_env_host.py runs it under ASan + UBSan.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "dm_tables.hpp"

namespace {
long g_checks = 0;
int bad(const char* what, int R, int nA, long i) {
    std::fprintf(stderr, "dm_env_driver: %s at R=%d n_act=%d index %ld\n", what, R, nA, i);
    return 1;
}
double value(int e, int table, int x, int k) { return 1.0 / 3.0 + e * 1000.0 + table * 100.0 + x + k / 64.0; }

// the operand layout from its description (common.hpp): [x / 16][(k / 4) / 4][q = k % 4 -> lane quarter][x % 16][(k / 4) % 4]
size_t operand_slot(int x, int k, int ga_stride) {
    const int tile = x / 16, lc = x % 16, q = k % 4, s = k / 4;
    const int quads = ga_stride / 4;
    return ((((size_t)tile * quads + s / 4) * 4 + q) * 16 + lc) * 4 + s % 4;
}

template <typename T>
int run(int R, int nA, int E) {
    ao::DmLayout L;
    L.R = R;
    L.n_act = nA;
    L.ga_stride = ao::dm_ga_stride(nA);
    if (L.ga_stride % 4 || L.ga_stride < 8 || 4 * L.ga_stride < nA) return bad("ga_stride", R, nA, L.ga_stride);
    const size_t ng = L.g_elems();
    std::vector<double> gx((size_t)E * ng), gy((size_t)E * ng);
    for (int e = 0; e < E; ++e)
        for (int x = 0; x < R; ++x)
            for (int k = 0; k < nA; ++k) {
                gx[(size_t)e * ng + (size_t)x * nA + k] = value(e, 0, x, k);
                gy[(size_t)e * ng + (size_t)x * nA + k] = value(e, 1, x, k);
            }
    ao::DmHostTables<T> h;
    ao::dm_relayout<T>(L, E, gx.data(), gy.data(), h);
    const int rp = L.r_pad(), nap = L.act_pad();
    if (rp % 128 || rp < R || rp >= R + 128 || nap % 4 || nap < nA || nap >= nA + 4) return bad("padding sizes", R, nA, rp);
    if (h.gx.size() != E * ng || h.gy.size() != E * ng || h.gxt.size() != (size_t)E * nap * rp ||
        h.gxa.size() != (size_t)E * rp * 4 * L.ga_stride || h.gya.size() != h.gxa.size())
        return bad("table sizes", R, nA, 0);
    for (int e = 0; e < E; ++e) {
        const T* g0 = h.gx.data() + (size_t)e * ng;
        const T* g1 = h.gy.data() + (size_t)e * ng;
        const T* gt = h.gxt.data() + (size_t)e * L.gxt_elems();
        for (int x = 0; x < R; ++x)
            for (int k = 0; k < nA; ++k, g_checks += 3) {
                if (g0[(size_t)x * nA + k] != (T)value(e, 0, x, k)) return bad("gx", R, nA, (long)x * nA + k);
                if (g1[(size_t)x * nA + k] != (T)value(e, 1, x, k)) return bad("gy", R, nA, (long)x * nA + k);
                if (gt[(size_t)k * rp + x] != (T)value(e, 0, x, k)) return bad("gxt", R, nA, (long)k * rp + x);
            }
        for (int k = 0; k < nap; ++k)
            for (int x = 0; x < rp; ++x, ++g_checks)
                if ((k >= nA || x >= R) && gt[(size_t)k * rp + x] != (T)0) return bad("gxt padding", R, nA, (long)k * rp + x);
        for (int table = 0; table < 2; ++table) {
            const float* ga = (table ? h.gya : h.gxa).data() + (size_t)e * L.ga_elems();
            std::vector<char> used(L.ga_elems(), 0);
            for (int x = 0; x < R; ++x)
                for (int k = 0; k < nA; ++k, ++g_checks) {
                    const size_t i = ao::ga_index(x, k, L.ga_stride);
                    if (i != operand_slot(x, k, L.ga_stride)) return bad("ga_index against the layout", R, nA, (long)i);
                    if (i >= L.ga_elems()) return bad("ga_index outside the env's block", R, nA, (long)i);
                    if (used[i]) return bad("ga_index hits a slot twice", R, nA, (long)i);
                    used[i] = 1;
                    if (ga[i] != (float)value(e, table, x, k)) return bad(table ? "gya" : "gxa", R, nA, (long)i);
                }
            for (size_t i = 0; i < L.ga_elems(); ++i, ++g_checks)
                if (!used[i] && ga[i] != 0.f) return bad("operand padding", R, nA, (long)i);
        }
    }
    return 0;
}
}  // namespace

int main() {
    const int cases[3][2] = {{24, 5}, {30, 6}, {144, 37}};
    for (const auto& c : cases) {
        if (run<float>(c[0], c[1], 3)) return 1;
        if (run<double>(c[0], c[1], 3)) return 1;
    }
    std::printf("ok %ld\n", g_checks);
    return 0;
}
