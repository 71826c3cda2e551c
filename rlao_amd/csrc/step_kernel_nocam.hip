// The fused step kernel, fast trig, the ideal detector: KS = 6 / 8, shared and per-env clocks.
#include "step_kernel_body.hpp"

namespace ao {
template int launch_env_step_spec<STEP_NOCAM>(const StepArgs&, const StepLds&, const StarEnv<float>&, hipStream_t);
}  // namespace ao
