// Host driver of the per-env guide-star arithmetic (rlao_amd/csrc/star_env.hpp: the validation and the factors aoenv_set_flux_env
// and aoenv_set_threshold_env use).  No arguments.  It checks, in float and in double:
//   scale 1 -> a factor of exactly 1; scale 4 -> exactly 2; every factor == (T)sqrt(scale) and a * a within 2 ulp of the scale
//   thresholds stored as (T)thr; 0 accepted
//   every refusal (NaN, +-inf, 0 and negative scales; NaN, inf and negative thresholds) names the first bad index and leaves the
//   output untouched (the library validates before it converts)
//   the shards without a per-env threshold: a Pyramid, max_group > 1
// Prints "ok <checks>"; any mismatch is a message and exit 1.  Plain C++; tests/test_star_env_host.py runs it under ASan + UBSan.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "star_env.hpp"

namespace {
long g_checks = 0;
int bad(const char* what, long i) {
    std::fprintf(stderr, "star_env_driver: %s at %ld\n", what, i);
    return 1;
}

template <typename T>
int run() {
    const int n = 37;
    std::vector<double> scale(n);
    for (int e = 0; e < n; ++e) scale[e] = std::pow(10.0, -0.4 * (e - 10) * 0.5);       // magnitudes -5 .. +13 around the calibrated one
    scale[10] = 1.0;
    scale[3] = 4.0;
    char msg[96] = "";
    if (ao::star_flux_check(scale.data(), n, msg, sizeof msg)) return bad("valid scales refused", 0);
    std::vector<T> a(n, (T)-7);
    ao::star_amp_factors<T>(scale.data(), n, a.data());
    if (a[10] != (T)1) return bad("scale 1 is not exactly 1", 10);
    if (a[3] != (T)2) return bad("scale 4 is not exactly 2", 3);
    for (int e = 0; e < n; ++e, g_checks += 2) {
        if (a[e] != (T)std::sqrt(scale[e])) return bad("factor is not (T)sqrt(scale)", e);
        const double back = (double)a[e] * (double)a[e];
        if (std::fabs(back - scale[e]) > 2.0 * std::numeric_limits<T>::epsilon() * scale[e]) return bad("a * a away from the scale", e);
    }
    // thresholds
    std::vector<double> thr = {0.0, 0.01, 0.05, 0.2, 1.0, 3.5};
    if (ao::star_threshold_check(thr.data(), (int)thr.size(), msg, sizeof msg)) return bad("valid thresholds refused", 0);
    std::vector<T> t(thr.size(), (T)-7);
    ao::star_thresholds<T>(thr.data(), (int)thr.size(), t.data());
    for (size_t i = 0; i < thr.size(); ++i, ++g_checks)
        if (t[i] != (T)thr[i]) return bad("threshold is not (T)thr", (long)i);
    // refusals: the first bad index is named
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    const double bad_scale[] = {nan, inf, -inf, 0.0, -0.0, -1.0, -1e-300};
    for (double v : bad_scale) {
        for (int at : {0, 5, n - 1}) {
            std::vector<double> s = scale;
            s[at] = v;
            if (at < n - 1) s[n - 1] = nan;                                                // a later one too: the first is reported
            std::memset(msg, 0, sizeof msg);
            if (!ao::star_flux_check(s.data(), n, msg, sizeof msg)) return bad("bad scale accepted", at);
            char want[32];
            std::snprintf(want, sizeof want, "scale[%d]", at);
            if (!std::strstr(msg, want)) return bad("refusal does not name the index", at);
            ++g_checks;
        }
    }
    const double bad_thr[] = {nan, inf, -inf, -1e-12, -0.5};
    for (double v : bad_thr) {
        std::vector<double> s = thr;
        s[2] = v;
        std::memset(msg, 0, sizeof msg);
        if (!ao::star_threshold_check(s.data(), (int)s.size(), msg, sizeof msg)) return bad("bad threshold accepted", 2);
        if (!std::strstr(msg, "threshold[2]")) return bad("threshold refusal does not name the index", 2);
        ++g_checks;
    }
    // a message that does not fit is truncated, never written past the buffer
    char tiny[8];
    std::vector<double> s = scale;
    s[n - 1] = nan;
    if (!ao::star_flux_check(s.data(), n, tiny, sizeof tiny) || tiny[sizeof tiny - 1] != 0) return bad("short message buffer", 0);
    ++g_checks;
    return 0;
}
}  // namespace

int main() {
    if (run<float>()) return 1;
    if (run<double>()) return 1;
    if (ao::star_threshold_refusal(false, 1) != nullptr) return bad("a Shack-Hartmann shard with max_group 1 refused", 0);
    if (!ao::star_threshold_refusal(true, 1) || !std::strstr(ao::star_threshold_refusal(true, 1), "Pyramid")) return bad("Pyramid accepted", 0);
    if (!ao::star_threshold_refusal(false, 2) || !std::strstr(ao::star_threshold_refusal(false, 2), "max_group")) return bad("max_group 2 accepted", 0);
    g_checks += 3;
    std::printf("ok %ld\n", g_checks);
    return 0;
}
