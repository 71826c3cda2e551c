// Host-side check of the laser-guide-star table's validation and launch plan (rlao_amd/csrc/sh_lgs.hpp), the header the library
// validates with and plans its launch from.  Plain C++ with its own main (tests/test_lgs_host.py builds it with the host compiler, once
// more under ASan + UBSan, and runs it as a program).  Prints "ok <checks>", or the first failed check and exits 1.
//   lgs_driver plan      additionally prints "p esz L bytes" for p = 1 .. 20 and both element sizes
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "sh_lgs.hpp"

static int checks = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        ++checks;                                                          \
        if (!(cond)) {                                                     \
            std::printf("FAILED line %d: %s\n", __LINE__, #cond);          \
            return 1;                                                      \
        }                                                                  \
    } while (0)

int main(int argc, char** argv) {
    using namespace ao;
    // ---- the launch plan: the LDS image fits, more lenslets per workgroup would not, and it is what the formula says
    for (int esz = 4; esz <= 8; esz += 4)
        for (int p = 1; p <= 40; ++p) {
            const int L = lgs_lenslets_per_group(p, esz);
            CHECK(L == 0 || L == 1 || L == 2 || L == 4);
            const size_t n = 2 * (size_t)p;
            if (L) {
                CHECK(lgs_lds_bytes(p, L, esz) <= kLgsLdsCap);
                CHECK(lgs_lds_bytes(p, L, esz) == (size_t)esz * (2 * n + (size_t)L * (2 * ((size_t)p * p + p * n) + 4 * n * n)));
            }
            if (L < 4) CHECK(lgs_lds_bytes(p, L ? 2 * L : 1, esz) > kLgsLdsCap);
            // every p the generic spots kernel takes (its image: complex (n + 4 (p^2 + p n)) <= 64 KB) has a plan
            if (2 * (size_t)esz * (n + 4 * ((size_t)p * p + p * n)) <= 64 * 1024) CHECK(L >= 1);
            if (argc > 1 && !std::strcmp(argv[1], "plan") && p <= 20) std::printf("%d %d %d %zu\n", p, esz, L, L ? lgs_lds_bytes(p, L, esz) : 0);
        }
    CHECK(lgs_lenslets_per_group(6, 4) == 4 && lgs_lenslets_per_group(6, 8) == 4 && lgs_lenslets_per_group(0, 4) == 0);

    // ---- a cyclic interval as ascending plain ones
    for (int n = 2; n <= 16; n += 2)
        for (int start = 0; start < n; ++start)
            for (int len = 1; len <= n; ++len) {
                const LgsRanges r = lgs_ranges(start, len, n);
                int count = 0, last = -1;
                for (int h = 0; h < 2; ++h)
                    for (int x = r.lo[h]; x < r.hi[h]; ++x) {
                        CHECK(x >= 0 && x < n && x > last);        // inside, ascending, no index twice
                        CHECK(((x - start + n) % n) < len);        // a member of the cyclic interval
                        last = x;
                        ++count;
                    }
                CHECK(count == len);
                for (int x = 0; x < n; ++x) CHECK(lgs_in_range(r, x) == (((x - start + n) % n) < len));
            }

    // ---- validation
    const int n = 8, nv = 3, ntab = 2;
    const size_t nn = (size_t)n * n, count = (size_t)ntab * nv * nn, bytes = count * sizeof(double);
    const int32_t box[4] = {6, 1, 4, 3};                           // rows 6, 7, 0, 1 (a box that wraps), columns 1, 2, 3
    std::vector<double> good(count, 0.0);
    for (int t = 0; t < ntab; ++t)
        for (int s = 0; s < nv; ++s)
            for (int dx = 0; dx < 4; ++dx)
                for (int dy = 0; dy < 3; ++dy) good[((size_t)t * nv + s) * nn + (size_t)((6 + dx) % n) * n + 1 + dy] = 0.01 * (1 + dx + dy + s + t);
    for (int narrow = 0; narrow < 2; ++narrow) {
        LgsCheck c = lgs_validate(good.data(), bytes, ntab, nv, n, box, narrow);
        CHECK(c.verdict == kLgsOk);
        CHECK(lgs_validate(good.data(), bytes - 8, ntab, nv, n, box, narrow).verdict == kLgsBytes);
        CHECK(lgs_validate(good.data(), bytes, 1, nv, n, box, narrow).verdict == kLgsBytes);
        CHECK(lgs_validate(good.data(), bytes / 2, 1, nv, n, box, narrow).verdict == kLgsOk);      // one table of the two
        const int32_t bad_boxes[6][4] = {{-1, 1, 4, 3}, {8, 1, 4, 3}, {6, 8, 4, 3}, {6, 1, 0, 3}, {6, 1, 9, 3}, {6, 1, 4, 9}};
        for (const auto& b : bad_boxes) CHECK(lgs_validate(good.data(), bytes, ntab, nv, n, b, narrow).verdict == kLgsBox);
        const int32_t whole[4] = {0, 0, n, n}, whole_from_5[4] = {5, 3, n, n};
        CHECK(lgs_validate(good.data(), bytes, ntab, nv, n, whole, narrow).verdict == kLgsOk);
        CHECK(lgs_validate(good.data(), bytes, ntab, nv, n, whole_from_5, narrow).verdict == kLgsOk);
        const size_t where = ((size_t)1 * nv + 2) * nn + 7 * n + 2;                                // table 1, lenslet 2, tap (7, 2): in the box
        std::vector<double> bad = good;
        bad[where] = -1e-9;
        c = lgs_validate(bad.data(), bytes, ntab, nv, n, box, narrow);
        CHECK(c.verdict == kLgsNegative && c.table == 1 && c.lenslet == 2 && c.tap == 7 * n + 2);
        bad[where] = std::numeric_limits<double>::quiet_NaN();
        c = lgs_validate(bad.data(), bytes, ntab, nv, n, box, narrow);
        CHECK(c.verdict == kLgsNotFinite && c.table == 1 && c.lenslet == 2 && c.tap == 7 * n + 2);
        bad[where] = std::numeric_limits<double>::infinity();
        CHECK(lgs_validate(bad.data(), bytes, ntab, nv, n, box, narrow).verdict == kLgsNotFinite);
        bad[where] = 1e300;                                        // finite in float64, not in float32
        CHECK(lgs_validate(bad.data(), bytes, ntab, nv, n, box, narrow).verdict == (narrow ? kLgsNotFinite : kLgsOk));
        bad = good;
        bad[(size_t)2 * nn + 3 * n + 2] = 0.25;                    // row 3 is outside the box
        c = lgs_validate(bad.data(), bytes, ntab, nv, n, box, narrow);
        CHECK(c.verdict == kLgsOutside && c.table == 0 && c.lenslet == 2 && c.tap == 3 * n + 2);
        bad = good;
        for (size_t q = 0; q < nn; ++q) bad[(size_t)4 * nn + q] = 0.0;                            // table 1, lenslet 1
        c = lgs_validate(bad.data(), bytes, ntab, nv, n, box, narrow);
        CHECK(c.verdict == kLgsZeroSum && c.table == 1 && c.lenslet == 1);
        for (size_t q = 0; q < nn; ++q) bad[(size_t)4 * nn + q] = good[(size_t)4 * nn + q] * 1e-60;  // a sum that float32 rounds to zero
        CHECK(lgs_validate(bad.data(), bytes, ntab, nv, n, box, narrow).verdict == (narrow ? kLgsZeroSum : kLgsOk));
    }
    std::printf("ok %d\n", checks);
    return 0;
}
