// Host driver of the policy's host-side model (rlao_amd/csrc/policy.hpp: the source env.hip and policy_kernels.hip use).
//   policy_driver < requests          (text on stdin, one request per line, one answer line per request on stdout)
//     plan a C               rows bands lds_bytes lds_of_one_row fits ksteps   (policy_bands, policy_conv_lds, policy_conv_lds_rows(.., 1),
//                            policy_mfma_fits, policy_ksteps)
//     select esz path F a C1 1 when aoenv_set_policy takes the MFMA kernel, 0 for the general one (policy_uses_mfma)
//     relayout F C           the next line holds the F C 9 weights in torch order [F][C][3][3]; the answer is the operand order
//                            [ksteps][F / 16][64] (policy_relayout), every float32 printed with 9 digits
//     channel H k E e        for c = 0 .. 2H - 2 the source conv_channel picks for env e at step k: "O s" / "A s" slot s of the
//                            observation / action trajectory, "PO r" / "PA r" row r of the caller's windows
// The channel request runs conv_channel on real arrays ([k + 1][E][img] and [E][H - 1][img], img = 3) and names the pointer it
// returns by the array it lies in; a pointer outside every array, inside an image or in another env's rows ends the program
// (exit 3).  tests/test_policy_host.py compares the answers with NumPy restatements and also runs the driver under ASan + UBSan.
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "policy.hpp"

static void die(const char* what, long long v) {
    std::fprintf(stderr, "policy_driver: %s (%lld)\n", what, v);
    std::exit(3);
}

int main() {
    std::string text;
    while (std::getline(std::cin, text)) {
        std::istringstream in(text);
        std::string op;
        if (!(in >> op)) continue;
        std::ostringstream out;
        if (op == "plan") {
            int a = 0, c = 0;
            if (!(in >> a >> c) || a < 1 || c < 1) return 2;
            int rows = 0, bands = 0;
            ao::policy_bands(a, c, &rows, &bands);
            out << rows << ' ' << bands << ' ' << ao::policy_conv_lds(a, c) << ' ' << ao::policy_conv_lds_rows(a, c, 1) << ' '
                << (ao::policy_mfma_fits(a, c) ? 1 : 0) << ' ' << ao::policy_ksteps(c);
        } else if (op == "select") {
            long long esz = 0;
            int path = 0, f = 0, a = 0, c1 = 0;
            if (!(in >> esz >> path >> f >> a >> c1) || a < 1 || c1 < 1 || f < 1) return 2;
            out << (ao::policy_uses_mfma((size_t)esz, path, f, a, c1) ? 1 : 0);
        } else if (op == "relayout") {
            int f = 0, c = 0;
            if (!(in >> f >> c) || f < 16 || f % 16 != 0 || c < 1) return 2;
            std::vector<double> w((size_t)f * c * 9);
            if (!std::getline(std::cin, text)) return 2;
            std::istringstream vals(text);
            for (auto& v : w)
                if (!(vals >> v)) return 2;
            std::vector<float> t;
            ao::policy_relayout(w.data(), f, c, t);
            if (t.size() != (size_t)ao::policy_ksteps(c) * (f / 16) * 64) die("relayout size", (long long)t.size());
            char buf[32];
            for (float v : t) {
                std::snprintf(buf, sizeof buf, "%.9g ", (double)v);
                out << buf;
            }
        } else if (op == "channel") {
            int H = 0, k = 0, E = 0, e = 0;
            if (!(in >> H >> k >> E >> e) || H < 1 || H > ao::kPolicyMaxHistory || k < 0 || E < 1 || e < 0 || e >= E) return 2;
            const int img = 3;
            std::vector<float> obs((size_t)(k + 1) * E * img), act((size_t)(k + 1) * E * img), po((size_t)E * (H - 1) * img),
                pa((size_t)E * (H - 1) * img);
            ao::ConvIn<float> s{nullptr, obs.data(), act.data(), po.data(), pa.data(), k, H, 2 * H - 1, E, img};
            for (int c = 0; c < s.C; ++c) {
                const float* p = ao::conv_channel(s, c, e);
                auto inside = [&](const std::vector<float>& v) { return !v.empty() && p >= v.data() && p < v.data() + v.size(); };
                const bool traj = inside(obs) || inside(act), is_act = inside(act) || inside(pa);
                if (!traj && !inside(po) && !inside(pa)) die("channel outside every array", c);
                const std::vector<float>& v = inside(obs) ? obs : inside(act) ? act : inside(po) ? po : pa;
                const long long off = p - v.data();
                if (off % img != 0) die("channel inside an image", c);
                const long long row = off / img;               // trajectory: slot * E + e;  windows: e * (H - 1) + r
                if (traj) {
                    if (row % E != e) die("another env's slot", c);
                    if (is_act && row / E >= k) die("action slot not yet written", c);
                    out << (is_act ? "A " : "O ") << row / E << ' ';
                } else {
                    if (row / (H - 1) != e) die("another env's window", c);
                    out << (is_act ? "PA " : "PO ") << row % (H - 1) << ' ';
                }
            }
        } else {
            return 2;
        }
        std::puts(out.str().c_str());
    }
    return 0;
}
