// The command the measurement of one step sees when a disturbance is set (aoenv_set_disturbance; the model is disturb.hpp):
//   seen[e][a] = coefs[e][a] + sum_m B[a][m] v[e][m](tau)
// as ONE launch in front of the step.  The step is then launched with its mirror-command pointer aimed at `seen`
// (AOENV_B_COEFS_SEEN) and goes on writing the pure command to AOENV_B_COEFS / AOENV_B_DM_PREV: the integrator state holds the
// correction alone, as in MAIN/OOPAOEnv/vibrationEnv.py:197-202 (dm.coefs = vibration_state + correction_state).
//
// One workgroup per env, 256 lanes; workgroup e touches nothing of another env.  LDS: v [M] in the env dtype.
//   1. lane m < M forms v[m] by looping over its J lines in order (float64: 3 J doubles read, J sines), converts it once
//   2. barrier
//   3. lane a (a, a + 256, ...) runs the fma chain over m; B is stored TRANSPOSED ([M][A]) so that a wave reads 64 consecutive
//      elements per m (the layout k_rollout_action uses for Fl), then adds the command: one read and one write of [A] per env.
// Bytes per env: 24 M J of parameters, 2 A of command in and out; B (M A elements) is shared by all envs and comes from L2.
#include "common.hpp"
#include "disturb.hpp"

namespace ao {

namespace {

template <typename T>
__global__ __launch_bounds__(256) void k_disturb_apply(DisturbArgs<T> a) {
    __shared__ T vs[kDisturbMaxModes];
    const int e = blockIdx.x, tid = threadIdx.x;
    const int A = a.n_valid_act, M = a.n_modes, J = a.n_lines;
    if (tid < M) {
        const size_t o = ((size_t)e * M + tid) * J;
        vs[tid] = (T)disturb_mode(a.amp + o, a.freq + o, a.phase + o, J, a.tau);
    }
    __syncthreads();
    const T* cf = a.coefs + (size_t)e * A;
    T* out = a.seen + (size_t)e * A;
    for (int k = tid; k < A; k += 256) out[k] = cf[k] + disturb_command<T>(a.modes_t + k, (size_t)A, vs, M);
}

}  // namespace

template <typename T>
int launch_disturb_apply(const DisturbArgs<T>& a, int n_env, hipStream_t st) {
    if (a.n_modes < 1 || a.n_modes > kDisturbMaxModes || a.n_lines < 1 || a.n_lines > kDisturbMaxLines)
        return fail("disturbance: %d modes / %d lines outside [1, %d] / [1, %d]", a.n_modes, a.n_lines, kDisturbMaxModes, kDisturbMaxLines);
    hipLaunchKernelGGL(k_disturb_apply<T>, dim3(n_env), dim3(256), 0, st, a);
    AO_HIP(hipGetLastError());
    return 0;
}
template int launch_disturb_apply<float>(const DisturbArgs<float>&, int, hipStream_t);
template int launch_disturb_apply<double>(const DisturbArgs<double>&, int, hipStream_t);

}  // namespace ao
