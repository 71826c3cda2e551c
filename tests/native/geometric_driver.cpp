// Host-side check of the geometric sensor's launch plan (rlao_amd/csrc/sh_geometric.hpp): for every line
// "R n_subap n_valid n_act n_modes esz" on stdin it prints "g base band row": the band height geo_tail_band chooses for the fused
// tail (0 = the separate kernels), the tail's own LDS elements, the elements of a band of that height (of one row when g is 0) and
// the LDS bytes of the stand-alone kernel.  Plain C++ (tests/test_geometric_host.py builds it with the host compiler).
#include <cstdio>

#include "sh_geometric.hpp"

int main() {
    int R, ns, nv, na, nm, esz;
    while (std::scanf("%d %d %d %d %d %d", &R, &ns, &nv, &na, &nm, &esz) == 6) {
        const int g = ao::geo_tail_band(R, ns, nv, na, nm, (size_t)esz);
        std::printf("%d %zu %zu %zu\n", g, ao::geo_tail_base_elems(nv, na, nm), ao::geo_band_elems(R, ns, g > 0 ? g : 1, (size_t)esz),
                    ao::geo_row_lds_bytes(R, ns, (size_t)esz));
    }
    return 0;
}
