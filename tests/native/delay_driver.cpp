// Host driver of the delay line's index arithmetic (rlao_amd/csrc/delay.hpp: the source env.hip uses for every loop).
//   delay_driver D  < operations          (text on stdin, one per line)
//     P id                 a step that issues action `id` (aoenv_step, a step of aoenv_run_integrator)
//     L n id_0 .. id_n-1   a recorded loop of n steps whose step k issues id_k (aoenv_run_rollout, aoenv_run_policy_rollout)
//     C                    clear (aoenv_set_delay with the delay in force)
// The ring holds action ids instead of images (0 = the zero action) and every operation is carried out the way env.hip does it:
// a step writes delay_write_slot, applies delay_apply_slot and moves on; a loop reads delay_loop_source for every step, then makes
// the copies of delay_refill and moves on by n.  Per operation one line on stdout: the ids applied, in step order, a '|', the line
// in logical order (oldest first).  Every slot index is checked against its array before use (exit 3); tests/test_delay_host.py
// compares the output with a Python list FIFO and also runs the driver under ASan + UBSan.
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "delay.hpp"

static void die(const char* what, long long v) {
    std::fprintf(stderr, "delay_driver: %s (%lld)\n", what, v);
    std::exit(3);
}

int main(int argc, char** argv) {
    if (argc != 2) {
        std::fprintf(stderr, "usage: %s D < operations\n", argv[0]);
        return 2;
    }
    const int d = std::atoi(argv[1]);
    if (d < 0 || d > ao::kMaxDelay) {
        std::fprintf(stderr, "bad delay\n");
        return 2;
    }
    ao::DelayLine r{d, 0};
    std::vector<long long> ring((size_t)ao::delay_slots(r), 0);
    auto slot = [&](int s) -> long long& {
        if (s < 0 || s >= (int)ring.size()) die("ring slot out of range", s);
        return ring[(size_t)s];
    };
    std::string text;
    while (std::getline(std::cin, text)) {
        std::istringstream in(text);
        std::string op;
        if (!(in >> op)) continue;
        std::ostringstream out;
        if (op == "P") {
            long long id = 0;
            if (!(in >> id)) return 2;
            slot(ao::delay_write_slot(r)) = id;
            out << slot(ao::delay_apply_slot(r)) << ' ';
            r = ao::delay_after(r, 1);
        } else if (op == "L") {
            int n = 0;
            if (!(in >> n) || n < 0) return 2;
            std::vector<long long> traj((size_t)n);
            for (auto& v : traj)
                if (!(in >> v)) return 2;
            for (int k = 0; k < n; ++k) {
                const ao::DelaySource s = ao::delay_loop_source(r, k);
                if (s.trajectory) {
                    if (s.slot < 0 || s.slot >= k + (d == 0)) die("trajectory slot not yet written", s.slot);   // (no delay: its own)
                    out << traj[(size_t)s.slot] << ' ';
                } else {
                    out << slot(s.slot) << ' ';
                }
            }
            const ao::DelayRefill f = ao::delay_refill(r, n);
            if (f.m < 0 || f.m > d || f.m > n || f.first_traj != n - f.m) die("refill count", f.m);
            for (int c = 0; c < f.m; ++c) slot((f.first_slot + c) % ao::delay_slots(r)) = traj[(size_t)(f.first_traj + c)];
            r = ao::delay_after(r, n);
        } else if (op == "C") {
            r = ao::DelayLine{d, 0};
            for (auto& v : ring) v = 0;
        } else {
            return 2;
        }
        if (r.w < 0 || r.w > d) die("write index out of range", r.w);
        out << '|';
        for (int j = 0; j < d; ++j) out << ' ' << slot(ao::delay_pending_slot(r, j));
        std::puts(out.str().c_str());
    }
    return 0;
}
