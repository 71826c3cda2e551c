// The fused step kernel, the general instantiation (run-time fast_trig and camera tests, the plain lenslet transform): KS = 6 / 8, shared and per-env clocks.
#include "step_kernel_body.hpp"

namespace ao {
template int launch_env_step_spec<STEP_GENERAL>(const StepArgs&, const StepLds&, const StarEnv<float>&, hipStream_t);
}  // namespace ao
