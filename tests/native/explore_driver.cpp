// Host driver of the exploration noise stream (rlao_amd/csrc/explore.hpp: the source k_rollout_action compiles for the device).
//   explore_driver SEED ENV0 N_ENV C0 N_C A
// writes float32 z[N_ENV][N_C][A] to stdout, raw: the normals of the envs ENV0 .. (global indices), the exploration steps C0 ..,
// the A valid actuators.  Built with `hipcc -x hip --cuda-host-only`; tests/test_explore_host.py also runs it under ASan + UBSan.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "explore.hpp"

int main(int argc, char** argv) {
    if (argc != 7) {
        std::fprintf(stderr, "usage: %s SEED ENV0 N_ENV C0 N_C A\n", argv[0]);
        return 2;
    }
    const uint64_t seed = std::strtoull(argv[1], nullptr, 0);
    const uint32_t env0 = (uint32_t)std::strtoul(argv[2], nullptr, 0), c0 = (uint32_t)std::strtoul(argv[4], nullptr, 0);
    const int n_env = std::atoi(argv[3]), n_c = std::atoi(argv[5]), A = std::atoi(argv[6]);
    if (n_env < 1 || n_c < 1 || A < 1 || (double)n_env * n_c * A > 1e8) {
        std::fprintf(stderr, "bad sizes\n");
        return 2;
    }
    std::vector<float> row((size_t)A);
    for (int e = 0; e < n_env; ++e)
        for (int c = 0; c < n_c; ++c) {
            for (int q = 0; 4 * q < A; ++q) {
                float z[4];
                ao::explore_normals((uint32_t)(seed & 0xffffffffu), (uint32_t)(seed >> 32), (uint32_t)q, env0 + (uint32_t)e, c0 + (uint32_t)c, z);
                for (int j = 0; j < 4 && 4 * q + j < A; ++j) row[(size_t)4 * q + j] = z[j];
            }
            if (std::fwrite(row.data(), sizeof(float), row.size(), stdout) != row.size()) return 1;
        }
    return 0;
}
