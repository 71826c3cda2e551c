// Host driver of the science window's model (rlao_amd/csrc/science.hpp: the source science_kernels.hip compiles for the device and
// env.hip for aoenv_set_science).
//   science_driver geom R ZP W                                   -> text: "M U pad n_fft"
//   science_driver plan R W                                      -> text: "rp up n_row_tiles tiles_per_wave n_row_groups n_col_blocks lds_bytes mfma_ok general_blocks"
//   science_driver table f32|f64 R ZP W own|given  [< dft[2W][R][2] f64]   -> the padded table [2][up][rp], raw, env dtype
//   science_driver validate f32|f64 R ZP W FIRST FLAGS own|given [< dft[2W][R][2] f64] -> text: the refusal's number (0 = accepted)
// Built with `hipcc -x hip --cuda-host-only`; tests/test_science_host.py also runs it under ASan + UBSan.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "science.hpp"

template <typename T>
static bool read_all(std::vector<T>& v) { return v.empty() || std::fread(v.data(), sizeof(T), v.size(), stdin) == v.size(); }
template <typename T>
static bool write_all(const std::vector<T>& v) { return std::fwrite(v.data(), sizeof(T), v.size(), stdout) == v.size(); }

template <typename T>
static int run(const char* what, int R, int zp, int W, int first, int flags, bool given) {
    // (a refused W is still read as sent: the size of the input is the test's, not the validation's)
    std::vector<double> dft(given && W > 0 ? (size_t)2 * W * R * 2 : 0);
    if (!read_all(dft)) return 2;
    size_t where = 0;
    const ao::SciRefusal r = ao::sci_validate<T>(R, zp, W, first, flags, given ? dft.data() : nullptr, &where);
    if (!std::strcmp(what, "validate")) {
        std::printf("%d\n", (int)r);
        return 0;
    }
    if (r != ao::kSciOk) return 3;
    const ao::SciGeom g = ao::sci_geom(R, zp, W);
    const ao::SciPlan pl = ao::sci_plan(R, W);
    std::vector<T> table(ao::sci_table_elems(pl), (T)7);          // (the fill overwrites all of it)
    ao::sci_fill_table<T>(g, pl, given ? dft.data() : nullptr, table.data());
    return write_all(table) ? 0 : 1;
}

int main(int argc, char** argv) {
    if (argc == 5 && !std::strcmp(argv[1], "geom")) {
        const ao::SciGeom g = ao::sci_geom(std::atoi(argv[2]), std::atoi(argv[3]), std::atoi(argv[4]));
        std::printf("%d %d %d %d\n", g.M, g.U, g.pad, g.n_fft);
        return 0;
    }
    if (argc == 4 && !std::strcmp(argv[1], "plan")) {
        const int R = std::atoi(argv[2]), W = std::atoi(argv[3]);
        if (R < 1 || W < 2) return 2;
        const ao::SciPlan p = ao::sci_plan(R, W);
        std::printf("%d %d %d %d %d %d %d %d %d\n", p.rp, p.up, p.n_row_tiles, p.tiles_per_wave, p.n_row_groups, p.n_col_blocks, p.lds_bytes,
                    p.mfma_ok, p.general_blocks);
        return 0;
    }
    const bool table = argc == 7 && !std::strcmp(argv[1], "table"), validate = argc == 9 && !std::strcmp(argv[1], "validate");
    if (!table && !validate) {
        std::fprintf(stderr, "usage: %s geom R ZP W | plan R W | table f32|f64 R ZP W own|given | validate f32|f64 R ZP W FIRST FLAGS own|given\n", argv[0]);
        return 2;
    }
    const int R = std::atoi(argv[3]), zp = std::atoi(argv[4]), W = std::atoi(argv[5]);
    if (R < 1 || R > 4096 || W > 65536) {
        std::fprintf(stderr, "bad sizes\n");
        return 2;
    }
    const int first = validate ? std::atoi(argv[6]) : 0, flags = validate ? std::atoi(argv[7]) : 0;
    const bool given = !std::strcmp(argv[argc - 1], "given");
    const int rc = !std::strcmp(argv[2], "f32") ? run<float>(argv[1], R, zp, W, first, flags, given) : run<double>(argv[1], R, zp, W, first, flags, given);
    if (rc == 2) std::fprintf(stderr, "bad mode or short input\n");
    return rc;
}
