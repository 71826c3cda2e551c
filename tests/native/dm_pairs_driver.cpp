// Host driver of the actuator-pair re-layout (rlao_amd/csrc/dm_pairs.hpp: the routine aoenv_set_dm_pairs uses).  No arguments: for 3
// envs at (R, A) = (24, 21), (30, 32), (48, 69), (144, 357), in float and in double, it fills py / px with values that name their own
// (env, table, row, actuator), runs pairs_relayout and checks EVERY element of every layout against its definition:
//   t   [e][k][x]                                          the value rounded to the dtype (the transpose of the input)
//   ga  [e][x / 16][(k / 4) / 4][k % 4][x % 16][(k / 4) % 4]   the value as float, restated here from the description of the operand
//                                                          layout; every other slot of the env's block zero: the rows R .. R pad 128
//                                                          and the actuators A .. 4 ga_stride that k_dm_pairs_mfma multiplies
// and that what the kernel relies on holds: 32 ceil(R / 32) <= R pad 128, 4 ga_stride >= A, ga_stride % 4 == 0, the slots of one env
// distinct and inside its block (env blocks one after the other cannot overlap), pairs_read_t inverts pairs_fill_t.
// Prints "ok <checks>"; any mismatch is a message and exit 1.  Built with `hipcc -x hip --cuda-host-only`;
// tests/test_dm_pairs_host.py runs it under ASan + UBSan.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "dm_pairs.hpp"

namespace {
long g_checks = 0;
int bad(const char* what, int R, int A, long i) {
    std::fprintf(stderr, "dm_pairs_driver: %s at R=%d A=%d index %ld\n", what, R, A, i);
    return 1;
}
double value(int e, int table, int x, int k) { return 1.0 / 3.0 + e * 4096.0 + table * 2048.0 + x + k / 512.0; }

// the operand layout from its description: tile of 16 rows, quad of 4 k steps, lane = (k % 4) * 16 + row % 16, step within the quad
size_t operand_slot(int x, int k, int ga_stride) {
    const int tile = x / 16, lc = x % 16, q = k % 4, s = k / 4;
    const int quads = ga_stride / 4;
    return ((((size_t)tile * quads + s / 4) * 4 + q) * 16 + lc) * 4 + s % 4;
}

template <typename T>
int run(int R, int A, int E) {
    ao::PairsLayout L;
    L.R = R;
    L.A = A;
    const int gs = L.ga_stride(), rp = L.r_pad();
    if (gs % 4 || gs < 8 || 4 * gs < A || L.k_pad() != 4 * gs) return bad("ga_stride", R, A, gs);
    if (rp % 128 || rp < R || rp >= R + 128 || 32 * ((R + 31) / 32) > rp) return bad("row padding", R, A, rp);
    if (L.ga_elems() != (size_t)rp * 4 * gs || L.t_elems() != (size_t)R * A) return bad("element counts", R, A, 0);
    if (L.bytes(sizeof(T)) != 2 * (size_t)R * A * sizeof(T) + 2 * (size_t)rp * 4 * gs * sizeof(float)) return bad("byte count", R, A, 0);
    const size_t nt = L.t_elems();
    std::vector<double> py((size_t)E * nt), px((size_t)E * nt);
    for (int e = 0; e < E; ++e)
        for (int x = 0; x < R; ++x)
            for (int k = 0; k < A; ++k) {
                py[(size_t)e * nt + (size_t)x * A + k] = value(e, 0, x, k);
                px[(size_t)e * nt + (size_t)x * A + k] = value(e, 1, x, k);
            }
    ao::PairsHostTables<T> h;
    ao::pairs_relayout<T>(L, E, py.data(), px.data(), h);
    if (h.pyt.size() != E * nt || h.pxt.size() != E * nt || h.pya.size() != (size_t)E * L.ga_elems() || h.pxa.size() != h.pya.size())
        return bad("table sizes", R, A, 0);
    std::vector<double> back(nt);
    for (int e = 0; e < E; ++e) {
        for (int table = 0; table < 2; ++table) {
            const T* t = (table ? h.pxt : h.pyt).data() + (size_t)e * nt;
            for (int x = 0; x < R; ++x)
                for (int k = 0; k < A; ++k, ++g_checks)
                    if (t[(size_t)k * R + x] != (T)value(e, table, x, k)) return bad(table ? "pxt" : "pyt", R, A, (long)k * R + x);
            ao::pairs_read_t<T>(L, t, back.data());
            for (int x = 0; x < R; ++x)
                for (int k = 0; k < A; ++k, ++g_checks)
                    if (back[(size_t)x * A + k] != (double)(T)value(e, table, x, k)) return bad("read back", R, A, (long)x * A + k);
            const float* ga = (table ? h.pxa : h.pya).data() + (size_t)e * L.ga_elems();
            std::vector<char> used(L.ga_elems(), 0);
            for (int x = 0; x < R; ++x)
                for (int k = 0; k < A; ++k, ++g_checks) {
                    const size_t i = operand_slot(x, k, gs);
                    if (i != ao::ga_index(x, k, gs)) return bad("ga_index against the layout", R, A, (long)i);
                    if (i >= L.ga_elems()) return bad("slot outside the env's block", R, A, (long)i);
                    if (used[i]) return bad("slot hit twice", R, A, (long)i);
                    used[i] = 1;
                    if (ga[i] != (float)value(e, table, x, k)) return bad(table ? "pxa" : "pya", R, A, (long)i);
                }
            // the padding: every slot of a row >= R or an actuator >= A, and nothing else, is unused -- and zero
            for (int x = 0; x < rp; ++x)
                for (int k = 0; k < 4 * gs; ++k, ++g_checks) {
                    const size_t i = operand_slot(x, k, gs);
                    if (i >= L.ga_elems()) return bad("padding slot outside the env's block", R, A, (long)i);
                    const bool pad = x >= R || k >= A;
                    if (pad == (bool)used[i]) return bad("padding map", R, A, (long)i);
                    if (pad && ga[i] != 0.f) return bad(x >= R ? "padding row not zero" : "K tail not zero", R, A, (long)i);
                }
        }
    }
    return 0;
}
}  // namespace

int main() {
    const int cases[4][2] = {{24, 21}, {30, 32}, {48, 69}, {144, 357}};
    for (const auto& c : cases) {
        if (run<float>(c[0], c[1], 3)) return 1;
        if (run<double>(c[0], c[1], 3)) return 1;
    }
    std::printf("ok %ld\n", g_checks);
    return 0;
}
