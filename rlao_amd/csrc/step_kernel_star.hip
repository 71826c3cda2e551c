// The fused step kernel, the per-env guide-star instantiation (aoenv_set_flux_env / aoenv_set_threshold_env): the general body plus each env's amplitude factor and centroid threshold.
#include "step_kernel_body.hpp"

namespace ao {
template int launch_env_step_spec<STEP_STAR>(const StepArgs&, const StepLds&, const StarEnv<float>&, hipStream_t);
}  // namespace ao
