// Control delay of the stepped loops (aoenv_set_delay): the action FIFO of the reference's TimeDelayEnv
// (MAIN/PO4AO/util_simple.py:25-52: append the new action, apply action_buffer[0], drop it; every gymnasium env carries the same
// action_buffer, OOPAOEnv_VPG.py:562-566) as state of the library.  ONE host-side source of the index arithmetic: env.hip uses it for
// every loop, tests/native/delay_driver.cpp replays it against a list FIFO.
//
// With a delay of d frames the line holds the d actions issued but not yet applied, oldest first ("pending row" j = 0 .. d - 1).
// It lives in a ring of d + 1 image slots with a host write index w: pending row j is slot (w - d + j) mod (d + 1), slot w is spare.
//   a step      writes its action into slot w, applies slot (w + 1) mod (d + 1) -- pending row 0 of before the write -- and moves
//               w on by one: the slot it applied is the next spare one.
//   a recorded  loop of n steps (aoenv_run_rollout, aoenv_run_policy_rollout) writes nothing while it runs: the trajectory is the
//               line.  Step k applies trajectory slot k - d when k >= d and pending row k otherwise.  Afterwards w moves on by n:
//               the pending rows that survive (old row n + j, n + j < d) are then new row j WHERE THEY LIE, and only the newest
//               min(n, d) actions of the trajectory are copied in, trajectory slot n - m + c into new pending row d - m + c.
// After either, the line is what that many appends would have left.
#pragma once

namespace ao {

constexpr int kMaxDelay = 8;           // AOENV_MAX_DELAY

struct DelayLine {
    int d = 0;                         // frames of delay, 0 = none (no ring)
    int w = 0;                         // the slot the next step writes, in [0, d]
};

inline int delay_slots(const DelayLine& r) { return r.d + 1; }

// the ring slot of pending row j (0 = oldest, d - 1 = newest)
inline int delay_pending_slot(const DelayLine& r, int j) { return ((r.w - r.d + j) % (r.d + 1) + (r.d + 1)) % (r.d + 1); }

// one step: the slot it writes, and the slot it applies once that is written
inline int delay_write_slot(const DelayLine& r) { return r.w; }
inline int delay_apply_slot(const DelayLine& r) { return (r.w + 1) % (r.d + 1); }

// step k of a recorded loop that started at `r`: where its applied action lies
struct DelaySource {
    bool trajectory;                   // true: trajectory slot `slot` (= k - d); false: ring slot `slot`
    int slot;
};
inline DelaySource delay_loop_source(const DelayLine& r, int k) {
    if (k >= r.d) return DelaySource{true, k - r.d};
    return DelaySource{false, delay_pending_slot(r, k)};
}

// the index after n steps of either kind
inline DelayLine delay_after(const DelayLine& r, long long n) { return DelayLine{r.d, (int)((r.w + n) % (r.d + 1))}; }

// the refill behind a recorded loop of n steps: m = min(n, d) images, copy c < m goes from trajectory slot first_traj + c into
// ring slot (first_slot + c) mod (d + 1), with `r` the index of BEFORE the loop
struct DelayRefill {
    int m, first_traj, first_slot;
};
inline DelayRefill delay_refill(const DelayLine& r, int n) {
    const int m = n < r.d ? n : r.d;
    return DelayRefill{m, n - m, delay_pending_slot(delay_after(r, n), r.d - m)};
}

}  // namespace ao
