// Host-side check of plan_step_pair (rlao_amd/csrc/common.hpp): which launches of aoenv_run_integrator take the step behind them
// along.  For every line "n_layer call_len n_calls rx0 ry0 rx1 ry1 ..." on stdin it runs the loop of aoenv_run_integrator on clocks
// that start at rest -- plan, then the real clock of step k (whole-pixel rounds, sub-pixel crossing), then, for a pair, the real
// clock of the covered step -- and prints "C" for the case, then per launch "L call k pair" followed, for a pair, by one
// "b l bx by" line per layer: the accumulators plan_step_pair handed out for the second step.  An "X" line reports a covered step
// whose real clock crossed a pixel or made a round (the library's internal error).  Built with hipcc for the HOST only
// (tests/test_step_pairs_host.py).
#include <cstdio>

#include "common.hpp"

int main() {
    int n_layer, call_len, n_calls;
    while (std::scanf("%d %d %d", &n_layer, &call_len, &n_calls) == 3) {
        double ratio[ao::kMaxLayer][2] = {}, buff[ao::kMaxLayer][2] = {}, buff2[ao::kMaxLayer][2] = {};
        for (int l = 0; l < n_layer; ++l)
            if (std::scanf("%lf %lf", &ratio[l][0], &ratio[l][1]) != 2) return 1;
        std::printf("C\n");
        for (int c = 0; c < n_calls; ++c) {
            for (int k = 0; k < call_len;) {
                const bool pair = ao::plan_step_pair(true, k, call_len, n_layer, ratio, buff, buff2);
                std::printf("L %d %d %d\n", c, k, pair ? 1 : 0);
                int bx, by;
                for (int l = 0; l < n_layer; ++l) {
                    if (ratio[l][0] == 0 && ratio[l][1] == 0) continue;
                    ao::clock_subpixel(ratio[l], buff[l], &bx, &by);
                }
                if (pair) {
                    for (int l = 0; l < n_layer; ++l) {
                        std::printf("b %d %.17g %.17g\n", l, buff2[l][0], buff2[l][1]);
                        if (ratio[l][0] == 0 && ratio[l][1] == 0) continue;
                        if (ao::clock_rounds(ratio[l], 0, &bx, &by) > 0 || ao::clock_subpixel(ratio[l], buff[l], &bx, &by)) std::printf("X %d %d\n", c, k);
                    }
                }
                k += pair ? 2 : 1;
            }
        }
        // not eligible, and the ends of a call, whatever the clocks say
        std::printf("E %d %d %d %d\n", ao::plan_step_pair(false, 0, 4, n_layer, ratio, buff, buff2) ? 1 : 0,
                    ao::plan_step_pair(true, 0, 1, n_layer, ratio, buff, buff2) ? 1 : 0,
                    ao::plan_step_pair(true, 3, 4, n_layer, ratio, buff, buff2) ? 1 : 0,
                    ao::plan_step_pair(true, -1, 4, n_layer, ratio, buff, buff2) ? 1 : 0);
    }
    return 0;
}
