// Host driver of the wavefront read-out's model (rlao_amd/csrc/wavefront.hpp: the source wavefront_kernels.hip compiles for the
// device and env.hip for aoenv_set_wavefront_basis).
//   wavefront_driver plan R2 K                                        -> text: "n_slices slice_len stride", then "lo hi" per slice
//   wavefront_driver scatter f32|f64 R2 K P  < pupil[R2] u8, opd2m[K][P] f64   -> the padded full-grid table [K][stride], raw, env dtype
//   wavefront_driver validate f32|f64 R2 K P CASE < pupil[R2] u8, opd2m[K][P] f64 -> text: the refusal's number (0 = accepted)
//       CASE: table (as given) | nopupil (no pupil uploaded) | nulltable (a null opd2m)
//   wavefront_driver project f32|f64 R2 K E < p[K][stride], x[E][R2], scale[1] (env dtype)  -> c[E][K] scaled, then c[E][K] unscaled:
//       the general kernel's chain per slice, the slices added in order, one multiply
// Built with `hipcc -x hip --cuda-host-only`; tests/test_wavefront_host.py also runs it under ASan + UBSan.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "wavefront.hpp"

template <typename T>
static bool read_all(std::vector<T>& v) { return v.empty() || std::fread(v.data(), sizeof(T), v.size(), stdin) == v.size(); }
template <typename T>
static bool write_all(const std::vector<T>& v) { return std::fwrite(v.data(), sizeof(T), v.size(), stdout) == v.size(); }

template <typename T>
static int run(const char* what, int R2, int K, int N, const char* kase) {
    if (!std::strcmp(what, "scatter") || !std::strcmp(what, "validate")) {
        // (a refused K or P is still read as sent: the sizes of the input are the test's, not the validation's)
        std::vector<uint8_t> pupil((size_t)R2);
        std::vector<double> opd2m((size_t)(K > 0 ? K : 0) * (size_t)(N > 0 ? N : 0));
        if (!read_all(pupil) || !read_all(opd2m)) return 2;
        const bool nopupil = kase && !std::strcmp(kase, "nopupil"), nulltable = kase && !std::strcmp(kase, "nulltable");
        size_t where = 0;
        const ao::WfRefusal r = ao::wf_validate<T>(K, N, nopupil ? nullptr : pupil.data(), R2, nulltable ? nullptr : opd2m.data(), &where);
        if (!std::strcmp(what, "validate")) {
            std::printf("%d\n", (int)r);
            return 0;
        }
        if (r != ao::kWfOk) return 3;
        std::vector<T> table((size_t)K * ao::wf_row_stride(R2), (T)7);        // (the scatter overwrites all of it)
        ao::wf_scatter<T>(opd2m.data(), K, N, pupil.data(), R2, table.data());
        return write_all(table) ? 0 : 1;
    }
    if (!std::strcmp(what, "project") && K >= 1 && N >= 1) {
        const size_t ld = (size_t)ao::wf_row_stride(R2);
        std::vector<T> p((size_t)K * ld), x((size_t)N * R2), s(1), c((size_t)N * K), c0((size_t)N * K);
        if (!read_all(p) || !read_all(x) || !read_all(s)) return 2;
        for (int e = 0; e < N; ++e)
            for (int m = 0; m < K; ++m) {
                c[(size_t)e * K + m] = ao::wf_project_one<T>(p.data() + (size_t)m * ld, x.data() + (size_t)e * R2, R2, K, s.data());
                c0[(size_t)e * K + m] = ao::wf_project_one<T>(p.data() + (size_t)m * ld, x.data() + (size_t)e * R2, R2, K, nullptr);
            }
        return write_all(c) && write_all(c0) ? 0 : 1;
    }
    return 2;
}

int main(int argc, char** argv) {
    if (argc == 4 && !std::strcmp(argv[1], "plan")) {
        const int R2 = std::atoi(argv[2]), K = std::atoi(argv[3]);
        if (R2 < 1 || K < 1) return 2;
        const ao::WfPlan pl = ao::wf_plan(R2, K);
        std::printf("%d %d %d\n", pl.n_slices, pl.slice_len, ao::wf_row_stride(R2));
        for (int z = 0; z < pl.n_slices; ++z) std::printf("%d %d\n", ao::wf_slice_lo(pl, z), ao::wf_slice_hi(pl, z, R2));
        return 0;
    }
    if (argc < 6 || argc > 7) {
        std::fprintf(stderr, "usage: %s plan R2 K | scatter|validate|project f32|f64 R2 K N [CASE] < tables\n", argv[0]);
        return 2;
    }
    const int R2 = std::atoi(argv[3]), K = std::atoi(argv[4]), N = std::atoi(argv[5]);
    if (R2 < 1 || R2 > (1 << 24)) {
        std::fprintf(stderr, "bad sizes\n");
        return 2;
    }
    const char* kase = argc == 7 ? argv[6] : nullptr;
    const int rc = !std::strcmp(argv[2], "f32") ? run<float>(argv[1], R2, K, N, kase) : run<double>(argv[1], R2, K, N, kase);
    if (rc == 2) std::fprintf(stderr, "bad mode or short input\n");
    return rc;
}
