// Host-side check of the whole-pixel rounds of the atmosphere clock (rlao_amd/csrc/common.hpp: clock_rounds, clock_rounds_origin),
// the schedule the shared host clock and the per-env device clocks (k_ring_round_env) both follow.  For every "rx ry n S" line on
// stdin it prints "R mx" and one "r j sx sy oy ox" line per round j = 0 .. mx (the last one sits out: 0 0; (oy, ox) is the torus
// origin after j rounds from origin 0), then n steps of the whole clock from buff = 0, origin 0: "s dx dy oy ox" with the
// pixels moved in that step (rounds + sub-pixel crossing) and the origin after it, which is how k_ring_prepare_env chains the two.
// Built with hipcc for the HOST only (tests/test_wind_rounds_host.py); the same source is compiled into the kernels.
#include <cstdio>

#include "common.hpp"

int main() {
    double rx, ry;
    int n, S;
    while (std::scanf("%lf %lf %d %d", &rx, &ry, &n, &S) == 4) {
        const double ratio[2] = {rx, ry};
        int sx, sy;
        const int mx = ao::clock_rounds(ratio, 0, &sx, &sy);
        std::printf("R %d\n", mx);
        for (int j = 0; j <= mx; ++j) {
            int org[2] = {0, 0};
            ao::clock_rounds(ratio, j, &sx, &sy);
            ao::clock_rounds_origin(ratio, j, S, org);
            std::printf("r %d %d %d %d %d\n", j, sx, sy, org[0], org[1]);
        }
        double buff[2] = {0, 0};
        int org[2] = {0, 0};
        for (int i = 0; i < n; ++i) {
            int dx = 0, dy = 0;
            for (int j = 0; j < mx; ++j) {
                ao::clock_rounds(ratio, j, &sx, &sy);
                dx += sx;
                dy += sy;
            }
            ao::clock_rounds_origin(ratio, mx, S, org);
            int bx, by;
            ao::clock_subpixel(ratio, buff, &bx, &by);
            org[0] = ((org[0] - by) % S + S) % S;
            org[1] = ((org[1] - bx) % S + S) % S;
            std::printf("s %d %d %d %d\n", dx + bx, dy + by, org[0], org[1]);
        }
    }
    return 0;
}
