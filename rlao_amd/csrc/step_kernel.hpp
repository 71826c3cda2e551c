// What the translation units of the fused step kernel share: its LDS layout and the instantiations' launchers.
// (step_kernel.hip: layout, envelope and dispatch; step_kernel_body.hpp: the kernels, step_body_text.hpp: their body; step_kernel_<spec>.hip: one SPEC each, so
// that a parallel build compiles them side by side)
#pragma once
#include "common.hpp"

namespace ao {

// What the kernel knows at compile time about its launch (template parameter SPEC of k_env_step_sh6)
enum StepSpec {
    STEP_GENERAL = 0,      // nothing: run-time fast_trig and camera tests, the plain lenslet transform
    STEP_NOCAM = 1,        // fast trig, the ideal detector
    STEP_PHOTON = 2,       // fast trig, photon noise and nothing else: QE 1, no dark current, read-out noise, full well, gain or ADC
    STEP_CAMERA = 3,       // fast trig, any other camera
    STEP_STAR = 4          // what STEP_GENERAL knows, and every env its own amplitude factor and centroid threshold (StarEnv)
};

namespace fstep {
constexpr int TX = 128, PR = 64;                       // widest pupil, rows per pass
constexpr int WR = 16 + 3, WC = 32 + 4;                // a wave's private layer tile: 19 rows x 35 columns (stride 36)
constexpr int WC4 = WC / 4;                            // float4 per staged row of the wave tile
constexpr int NV4 = (WR * WC4 + 63) / 64;              // 16-byte staging loads per lane and layer
}  // namespace fstep

struct StepLds {
    int cimg, s1, mapt, slot, e0, sl, img, total;      // offsets in 4-byte words
    int tab, tab_cap;                                  // the camera's alias tables (stage B) and the words there are for them
    // a launch of two steps only (step_pair_lds_layout; 0 otherwise): the first step's slopes and modal coefficients, in words
    // that no stage of the second step aliases -- its stage C reconstructs both steps
    int pair, pair_tm;
};

// the layouts (step_kernel.hip); what a workgroup has for them beside the kernels' static __shared__ (< 1 KB)
constexpr int kStepLdsBytes = 160 * 1024 - 1024;
StepLds step_lds_layout(int n_act, int n_subap, int n_valid, int n_modes);
StepLds step_pair_lds_layout(int n_act, int n_subap, int n_valid, int n_modes);   // the same, plus the pair's words at the end

template <int SPEC>
int launch_env_step_spec(const StepArgs& a, const StepLds& L, const StarEnv<float>& star, hipStream_t st);
extern template int launch_env_step_spec<STEP_GENERAL>(const StepArgs&, const StepLds&, const StarEnv<float>&, hipStream_t);
extern template int launch_env_step_spec<STEP_NOCAM>(const StepArgs&, const StepLds&, const StarEnv<float>&, hipStream_t);
extern template int launch_env_step_spec<STEP_PHOTON>(const StepArgs&, const StepLds&, const StarEnv<float>&, hipStream_t);
extern template int launch_env_step_spec<STEP_CAMERA>(const StepArgs&, const StepLds&, const StarEnv<float>&, hipStream_t);
extern template int launch_env_step_spec<STEP_STAR>(const StepArgs&, const StepLds&, const StarEnv<float>&, hipStream_t);

// the step and the quiet step behind it in one launch (k_env_step_pair_sh6): the specialised instantiations with a camera, shared clock
template <int SPEC>
int launch_env_step_pair_spec(const StepArgs& a, const StepLds& L, const StarEnv<float>& star, hipStream_t st);
extern template int launch_env_step_pair_spec<STEP_PHOTON>(const StepArgs&, const StepLds&, const StarEnv<float>&, hipStream_t);
extern template int launch_env_step_pair_spec<STEP_CAMERA>(const StepArgs&, const StepLds&, const StarEnv<float>&, hipStream_t);

}  // namespace ao
