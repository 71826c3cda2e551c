// Exploration noise of the on-device rollout (aoenv_run_rollout): the N(0,1)^A draw of env.sample_noise
// (MAIN/OOPAOEnv/OOPAOEnv.py:566-570), from a counter-based stream instead of NumPy's global generator.
//   generator  Philox4x32-7, the rounds of the camera streams (detector.hpp), restated here for host AND device: one source
//              serves k_rollout_action and the host driver of tests/native/explore_driver.cpp
//   key        (seed_lo, seed_hi) of the exploration seed
//   counter    (q, env_index_offset + e, c, kExplorePurpose):  q = quad of valid actuators in AOENV_C_ACT_IDX order,
//              c = exploration step counter (word 1 of AOENV_B_COUNTERS), the purpose a word no camera stream uses
//              (those are 0 .. 5 and 16 + j for the few rounds j of a PTRS rejection)
//   normals    Box-Muller on the 23-bit uniforms u = u01(word), strictly inside (0, 1):
//              z[4q] = r0 cos(2 pi u(o1)), z[4q + 1] = r0 sin(2 pi u(o1)), r0 = sqrt(-2 ln u(o0));  z[4q + 2], z[4q + 3] from (o2, o3).
//              float32 arithmetic for both env dtypes (the uniforms carry 23 bits); |z| <= sqrt(48 ln 2) = 5.77
// Reproducible, the same for an env wherever it sits in a shard or on which GPU, and checkpointed with the counter.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define AO_EXPLORE_HD __host__ __device__
#else
#define AO_EXPLORE_HD
#endif

namespace ao {

constexpr uint32_t kExplorePurpose = 0x45585031u;   // "EXP1"

AO_EXPLORE_HD inline void explore_philox(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1, uint32_t o[4]) {
    for (int i = 0; i < 7; ++i) {                                  // Philox4x32-7 (Salmon et al. 2011), as Philox::round of detector.hpp
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c0 = n0; c1 = (uint32_t)p1; c2 = n2; c3 = (uint32_t)p0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    o[0] = c0; o[1] = c1; o[2] = c2; o[3] = c3;
}

// strictly inside (0, 1): 23 bits + 1/2 (u01 of detector.hpp)
AO_EXPLORE_HD inline float explore_u01(uint32_t x) { return ((float)(x >> 9) + 0.5f) * (1.0f / 8388608.0f); }

// the four normals of quad q of env (global index) `env` at exploration step c
AO_EXPLORE_HD inline void explore_normals(uint32_t seed_lo, uint32_t seed_hi, uint32_t q, uint32_t env, uint32_t c, float z[4]) {
    uint32_t o[4];
    explore_philox(q, env, c, kExplorePurpose, seed_lo, seed_hi, o);
    for (int h = 0; h < 2; ++h) {
        const float r = sqrtf(-2.0f * logf(explore_u01(o[2 * h])));
        const float t = 6.28318530717958648f * explore_u01(o[2 * h + 1]);
        z[2 * h] = r * cosf(t);
        z[2 * h + 1] = r * sinf(t);
    }
}

}  // namespace ao
