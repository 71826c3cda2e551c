// Host driver of the modal control surface's model (rlao_amd/csrc/modal.hpp: the source modal_kernels.hip compiles for the device).
//   modal_driver expand  f32|f64 K A E  < m2c_t[K][A] a[E][K]              -> v[E][A]: the command of every actuator, the fma chain
//   modal_driver expandg f32|f64 K A E  < m2c_t[K][A] o[E][K] g[E][K]      -> the same on a = g * o (the modal integrator)
//   modal_driver project f32|f64 K S E  < cm[K][S] signal[E][S]            -> o[E][K], then reward[E] as float64
// Everything raw on stdin / stdout in the named dtype.  Built with `hipcc -x hip --cuda-host-only`; tests/test_modal_host.py also
// runs it under ASan + UBSan.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "modal.hpp"

template <typename T>
static bool read_all(std::vector<T>& v) { return std::fread(v.data(), sizeof(T), v.size(), stdin) == v.size(); }
template <typename T>
static bool write_all(const std::vector<T>& v) { return std::fwrite(v.data(), sizeof(T), v.size(), stdout) == v.size(); }

template <typename T>
static int run(const char* what, int K, int N, int E) {
    const bool gains = !std::strcmp(what, "expandg");
    if (gains || !std::strcmp(what, "expand")) {
        std::vector<T> m2c_t((size_t)K * N), a((size_t)E * K), g(gains ? (size_t)E * K : 0), v((size_t)E * N);
        if (!read_all(m2c_t) || !read_all(a) || !read_all(g)) return 2;
        for (size_t i = 0; i < g.size(); ++i) a[i] = ao::modal_gain<T>(g[i], a[i]);
        for (int e = 0; e < E; ++e)
            for (int k = 0; k < N; ++k) v[(size_t)e * N + k] = ao::modal_expand<T>(m2c_t.data() + k, (size_t)N, a.data() + (size_t)e * K, K);
        return write_all(v) ? 0 : 1;
    }
    if (!std::strcmp(what, "project")) {
        std::vector<T> cm((size_t)K * N), sig((size_t)E * N), o((size_t)E * K);
        std::vector<double> r((size_t)E);
        if (!read_all(cm) || !read_all(sig)) return 2;
        for (int e = 0; e < E; ++e) r[(size_t)e] = ao::modal_project_env<T>(cm.data(), sig.data() + (size_t)e * N, K, N, o.data() + (size_t)e * K);
        return write_all(o) && write_all(r) ? 0 : 1;
    }
    return 2;
}

int main(int argc, char** argv) {
    if (argc != 6) {
        std::fprintf(stderr, "usage: %s expand|expandg|project f32|f64 K N E < tables\n", argv[0]);
        return 2;
    }
    const int K = std::atoi(argv[3]), N = std::atoi(argv[4]), E = std::atoi(argv[5]);
    if (K < 1 || N < 1 || E < 1) {
        std::fprintf(stderr, "bad sizes\n");
        return 2;
    }
    const int rc = !std::strcmp(argv[2], "f32") ? run<float>(argv[1], K, N, E) : run<double>(argv[1], K, N, E);
    if (rc == 2) std::fprintf(stderr, "bad mode or short input\n");
    return rc;
}
