// The fused step kernel's host side: its LDS layout, the envelope it serves and the choice of the instantiation for a launch.
// The kernels are step_kernel_body.hpp (their body: step_body_text.hpp); its instantiations are compiled in step_kernel_general.hip, step_kernel_nocam.hip,
// step_kernel_photon.hip, step_kernel_camera.hip and step_kernel_star.hip.
#include "step_kernel.hpp"

#include "sh_device.hpp"

namespace ao {

StepLds step_lds_layout(int n_act, int n_subap, int n_valid, int n_modes) {
    using namespace fstep;
    StepLds L;
    const int nAp = (n_act + 3) & ~3, SS = nAp + 1;
    int o = 0;
    auto take = [&](int words) { const int at = o; o += (words + 3) & ~3; return at; };
    // What stage A leaves behind is dead at the barrier in front of stage B: the command image, Gy C (s1) and the waves' layer
    // tiles make room for the alias tables of the camera's photon draw (poisson_alias.hpp; copied there by direct loads while the
    // spots are computed).  The slopes and the observation image / modal coefficients of stages B-C live where the lenslet
    // fields (E0) were: written only behind the barrier that follows the spots of every wave.
    const int sl_words = (2 * n_valid + 3) & ~3, img_words = n_act * n_act + n_modes;
    L.cimg = take(n_act * n_act);
    L.s1 = take(2 * PR * SS);
    L.mapt = take(16 * WR * WC);
    L.tab = L.cimg;
    L.tab_cap = o - L.tab;
    L.slot = take((n_subap * n_subap + 1) / 2);
    L.e0 = take(std::max(2 * n_valid * fast6::EST, sl_words + img_words));
    L.sl = L.e0;
    L.img = L.e0 + sl_words;
    L.total = o;
    L.pair = L.pair_tm = 0;
    return L;
}

// A launch of two steps: the first copy's slopes (2 n_valid words) and modal coefficients (n_modes words) behind everything else.
// `sl` and `img` lie in E0, which stage A of the second step overwrites while the first step's slopes are still to be
// reconstructed.  At C2 (316 valid lenslets, 50 modes): 632 + 52 = 684 words, 2 736 bytes.
StepLds step_pair_lds_layout(int n_act, int n_subap, int n_valid, int n_modes) {
    StepLds L = step_lds_layout(n_act, n_subap, n_valid, n_modes);
    L.pair = L.total;
    L.pair_tm = L.pair + ((2 * n_valid + 3) & ~3);
    L.total = L.pair_tm + ((n_modes + 3) & ~3);
    return L;
}

int step_fused_supported(int R, int n_subap, int n_valid, int n_act, int n_modes) {
    if (R % n_subap || R / n_subap != fast6::P) return 0;
    if (R > fstep::TX || R % 4) return 0;
    if (n_valid > 16 * 21 || n_subap * n_subap > 32767 || n_act > 32) return 0;
    if (n_modes < 1 || n_modes > 52 || (2 * n_valid) % 4 != 0 || 2 * n_valid > 640) return 0;   // stage C register blocking
    const StepLds L = step_lds_layout(n_act, n_subap, n_valid, n_modes);
    return (size_t)L.total * 4 <= (size_t)kStepLdsBytes ? 1 : 0;     // static __shared__ of the kernel: < 1 KB
}

// words of LDS the fused kernel has for the camera's alias tables (where stage A's buffers were): the env keeps the part of the
// tables that fits there for ALL its camera kernels, so that a pixel is drawn the same way whichever kernel meets it
int step_alias_capacity(int n_act) { return step_lds_layout(n_act, 1, 1, 1).tab_cap; }

// the instantiation of a launch: per-env stars have their own; the general one without fast trig or under AOENV_PATH_SH_PLAIN,
// else by the camera's kind
static StepSpec step_spec(const StepArgs& a, const StarEnv<float>& star) {
    if (star.amp || star.thr) return STEP_STAR;
    if (!a.sc.fast_trig || a.sc.plain) return STEP_GENERAL;
    if (!a.det.active) return STEP_NOCAM;
    const DetectorCfg& d = a.det;
    // (the condition under which camera_sh6_lane has nothing to do behind the photon draw)
    const bool after_photons = d.dark_e > 0.f || d.readout_noise != 0.f || d.qe != 1.f || d.gain != 1.f || d.fwc > 0.f || d.bits > 0;
    return d.photon_noise && !after_photons ? STEP_PHOTON : STEP_CAMERA;
}

static int step_tables_fit(const StepArgs& a, const StepLds& L) {
    if (a.det.active && a.det.photon_noise && (!a.pa.tab || a.pa.words > L.tab_cap || a.pa.lmax < palias::kCoarseStep))
        return fail("fused step: the photon-noise tables are missing or do not fit (%d words, room for %d)", a.pa.words, L.tab_cap);
    return 0;
}

int launch_env_step(const StepArgs& a, const StarEnv<float>& star, hipStream_t st) {
    const StepLds L = step_lds_layout(a.k.n_act, a.n_subap, a.n_valid, a.n_modes);
    AO_TRY(step_tables_fit(a, L));
    switch (step_spec(a, star)) {
        case STEP_STAR: return launch_env_step_spec<STEP_STAR>(a, L, star, st);
        case STEP_GENERAL: return launch_env_step_spec<STEP_GENERAL>(a, L, star, st);
        case STEP_NOCAM: return launch_env_step_spec<STEP_NOCAM>(a, L, star, st);
        case STEP_PHOTON: return launch_env_step_spec<STEP_PHOTON>(a, L, star, st);
        default: return launch_env_step_spec<STEP_CAMERA>(a, L, star, st);
    }
}

bool env_step_pairable(const StepArgs& a, const StarEnv<float>& star) {
    const StepSpec s = step_spec(a, star);
    // Only where the camera's pixels are whole numbers -- photon counts, or ADC steps.  The centre of gravity's
    // `xa * q3 + xb * (q3 + 3)` is a sum of two products; a launch of one step fuses five of its six terms and leaves one as two
    // rounded products (the vectoriser packs that term's add with the sum of the intensities), the copies of a pair fuse other
    // ones, and no way of writing the line makes a copy repeat that.  With whole-number pixels below 2^24 / 5 every product is
    // exact and every form gives the same slopes; with float pixels (the ideal detector, read-out noise or a quantum efficiency
    // without an ADC) the slopes of a pair differed from one launch per step in the last bit, so those launches do not pair.
    if (a.k.pa.env_taps != nullptr) return false;
    // ... and only where the pair's own LDS words fit beside the single step's layout; otherwise one launch per step, as before
    if ((size_t)step_pair_lds_layout(a.k.n_act, a.n_subap, a.n_valid, a.n_modes).total * 4 > (size_t)kStepLdsBytes) return false;
    return s == STEP_PHOTON || (s == STEP_CAMERA && a.det.bits > 0 && a.det.bits <= 21);   // (5 (2^bits - 1) < 2^24)
}

int launch_env_step_pair(const StepArgs& a, hipStream_t st) {
    const StepLds L = step_pair_lds_layout(a.k.n_act, a.n_subap, a.n_valid, a.n_modes);
    const StarEnv<float> star{nullptr, nullptr};
    if (!env_step_pairable(a, star)) return fail("internal: a step pair on a launch that has no pair kernel");
    // (the second step takes the integrator's inputs from the first one's registers)
    if (!a.fa.do_integrate || a.fa.gain_from_obs == 0.f) return fail("internal: a step pair without the on-device integrator");
    AO_TRY(step_tables_fit(a, L));
    switch (step_spec(a, star)) {
        case STEP_PHOTON: return launch_env_step_pair_spec<STEP_PHOTON>(a, L, star, st);
        default: return launch_env_step_pair_spec<STEP_CAMERA>(a, L, star, st);
    }
}

}  // namespace ao

extern "C" int aoenv_test_step_lds(int n_act, int n_subap, int n_valid, int n_modes, int32_t* h_out) {
    using namespace ao;
    if (!h_out || n_act < 1 || n_subap < 1 || n_valid < 1 || n_modes < 1) return fail("aoenv_test_step_lds: bad arguments");
    const StepLds one = step_lds_layout(n_act, n_subap, n_valid, n_modes), two = step_pair_lds_layout(n_act, n_subap, n_valid, n_modes);
    StepArgs a{};                                                  // a photon-noise launch of this geometry: pairable but for the layout
    a.sc.fast_trig = 1;
    a.det.active = a.det.photon_noise = 1;
    a.det.qe = a.det.gain = 1.f;
    a.k.n_act = n_act;
    a.n_subap = n_subap;
    a.n_valid = n_valid;
    a.n_modes = n_modes;
    h_out[0] = one.total;
    h_out[1] = two.total;
    h_out[2] = two.pair;
    h_out[3] = two.pair_tm;
    h_out[4] = kStepLdsBytes;
    h_out[5] = env_step_pairable(a, StarEnv<float>{nullptr, nullptr}) ? 1 : 0;
    return 0;
}
