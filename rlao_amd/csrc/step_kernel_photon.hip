// The fused step kernel, fast trig, photon noise and nothing else (the headline's camera): KS = 6 / 8, shared and per-env clocks.
#include "step_kernel_body.hpp"

namespace ao {
template int launch_env_step_spec<STEP_PHOTON>(const StepArgs&, const StepLds&, const StarEnv<float>&, hipStream_t);
template int launch_env_step_pair_spec<STEP_PHOTON>(const StepArgs&, const StepLds&, const StarEnv<float>&, hipStream_t);
}  // namespace ao
