// Host driver of rlao_amd/csrc/offaxis.hpp (tests/test_offaxis_host.py): the plan aoenv_set_science_direction makes, printed.
//   offaxis_driver R D fov n_layer (altitude N){n_layer} n_env (zenith azimuth){n_env}
// first line: the refusal code, the env and the layer it names; then, when accepted, one line per (layer, env):
//   l e fy fx ty tx ix iy extra_sx extra_sy row0 col0 lo hi        (floating-point values as hex floats)
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "offaxis.hpp"

int main(int argc, char** argv) {
    if (argc < 6) return 2;
    int k = 1;
    const int R = atoi(argv[k++]);
    const double D = atof(argv[k++]), fov = atof(argv[k++]);
    const int L = atoi(argv[k++]);
    if (L < 0 || argc < k + 2 * L + 1) return 2;
    std::vector<double> alt(L > 0 ? L : 1);
    std::vector<int> N(L > 0 ? L : 1);
    for (int l = 0; l < L; ++l) {
        alt[l] = atof(argv[k++]);
        N[l] = atoi(argv[k++]);
    }
    const int E = atoi(argv[k++]);
    if (E < 1 || argc < k + 2 * E) return 2;
    std::vector<double> zen(E), az(E);
    for (int e = 0; e < E; ++e) {
        zen[e] = atof(argv[k++]);
        az[e] = atof(argv[k++]);
    }
    std::vector<ao::OaShift> out((size_t)(L > 0 ? L : 1) * E);
    int we = -1, wl = -1;
    const ao::OaRefusal rc = ao::oa_make(L, E, R, D, fov, alt.data(), N.data(), zen.data(), az.data(), out.data(), &we, &wl);
    printf("%d %d %d\n", (int)rc, we, wl);
    if (rc != ao::kOaOk) return 0;
    for (int l = 0; l < L; ++l)
        for (int e = 0; e < E; ++e) {
            const ao::OaRefShift r = ao::oa_ref_shift(alt[l], zen[e], az[e], R, D, N[l]);
            const ao::OaShift& s = out[(size_t)l * E + e];
            int lo = 0, hi = 0;
            ao::oa_plan_layer(s, R, N[l], &lo, &hi);
            printf("%d %d %d %d %a %a %d %d %a %a %d %d %d %d\n", l, e, s.fy, s.fx, s.ty, s.tx, r.ix, r.iy, r.extra_sx, r.extra_sy, r.row0, r.col0, lo, hi);
        }
    return 0;
}
