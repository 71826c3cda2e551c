// The whole env.step() of one AO loop in ONE workgroup: one launch per step, one workgroup (16 waves) per env.
//
//   MAIN/OOPAOEnv/OOPAOEnv.py:485-536 (step)  =  atmosphere sub-pixel translation + footprint + layer sum
//   (OOPAO/Atmosphere.py:406-407, 439-450, 474-477)  ->  DM surface and residual phase (DeformableMirror.py:556, 469;
//   Telescope.py:404-412, 540-542)  ->  Shack-Hartmann spots, camera frame, thresholded centre of gravity, slopes
//   (ShackHartmann.py:340-347, 539-601)  ->  reconstruction, reward, leaky integrator, Strehl / rms telemetry
//   (OOPAOEnv.py:491-536).
//
// Why one workgroup per env: at the BASELINE sizes (R = 120: 57.6 KB of phase, 316 valid lenslets) every intermediate
// of an env fits in the 160 KB of LDS of one CU, so the residual phase never has to be re-read from HBM by the WFS,
// the camera frame never by the centroid, and the five dependent launches of the separate-kernel path (each mostly
// launch + memory latency at a few hundred envs) collapse into one.  256 envs = one workgroup on each of the 256 CUs.
//
//   stage A (2 passes of 64 rows): layer tile -> LDS, separable Catmull-Rom, DM surface s1 . Gx^T on the matrix
//            cores (v_mfma_f32_16x16x4_f32, whose output layout is the lane -> pixel map), pupil, phase store,
//            E0 = amp e^{i phi} parked in LDS per lenslet, float64 telemetry sums
//   stage B  3 lanes per valid lenslet (948 of 1024 lanes at 316 lenslets): register-resident 12 x 12 DFT + 2 x 2
//            binning (sh_device.hpp), frame store, workgroup max -> threshold -> centre of gravity in registers
//   stage C  t = M s, o = -M2C t, integrator, observation image, reward, telemetry (tail_from_slopes)
//
// Stage A's tile load, warp, pixel and pupil sums are the functions of phase_device.hpp that the batched kernels call; against
// the separate kernels (phase_kernel.hip, sh_kernels.hip) the results differ at rounding level: here the residual OPD is one
// contracted fma of the layer sum, there a rounded product and an add, and the summation orders of the centroid
// and of the telemetry differ.  No atomics: bitwise reproducible.
// (the body of the kernel and its launcher: step_kernel_general.hip, _nocam.hip, _photon.hip and _camera.hip instantiate one
// value of SPEC each, step_kernel_star.hip the one with per-env guide stars, step_kernel.hip holds the layout and the dispatch)
#pragma once
#include "step_kernel.hpp"

#include "phase_device.hpp"
#include "sh_device.hpp"
#include "detector.hpp"
#include "ring_device.hpp"

#include "camera_sh6.hpp"


namespace ao {

typedef float f32x4s __attribute__((ext_vector_type(4)));

// p[idx] if ok else 0, as an UNCONDITIONAL load from a clamped (always valid) index: a predicated load compiles to a
// branch around the load, and a run of them to a chain of dependent memory latencies.
template <typename P>
__device__ inline float ld_or0(const P* __restrict__ p, long idx, bool ok) {
    const float v = (float)p[ok ? idx : 0];
    return ok ? v : 0.f;
}

template <bool PE>
__device__ inline const LayerTaps& step_taps(const PhaseArgs& pa, int l, int e) {
    if constexpr (PE) return pa.env_taps[(size_t)l * pa.n_env + e];
    else return pa.taps[l];
}

// KS: k steps (of 4) of the DM product whose B operands are held in registers, n_act <= 4 KS
// PE: per-env clocks (aoenv_set_wind_env): the layer taps come from the env's own record in global memory instead of the kernel
// arguments (a variant of its own: read through a pointer chosen at run time, the shared-clock path lost 3 %)
// SPEC: what is constant for a launch (step_kernel.hpp).  STEP_GENERAL tests fast_trig and the camera's switches at run time and
// runs the plain lenslet transform: it serves AOENV_OPT_FAST_TRIG = 0 and AOENV_PATH_SH_PLAIN, and is what the specialised forms
// are compared with bit for bit.  The others have fast trig and the camera's kind fixed, so that neither sincosf's slow path
// (inlined at every pixel) nor the camera blocks a launch cannot reach are in their code, and run the register-pair transform.
// What changes between the steps of one call (store_phase / store_frame / store_atm, do_integrate, the ring) stays run-time.
// STEP_STAR is the general body with every env's own guide star: `star` is a third argument, read by that instantiation alone, so
// that the argument blocks and the code of the others are what they were without it.
template <int KS, bool PE, int SPEC>
__global__ void __launch_bounds__(1024) k_env_step_sh6(const StepArgs a, const StepLds L, const StarEnv<float> star) {
#define STEP_BODY_SUB 0
#include "step_body_text.hpp"
}

// Two steps in one launch: step k of aoenv_run_integrator and, behind a workgroup barrier, the quiet step k + 1 (plan_step_pair,
// common.hpp).  Straight-line: no loop over the steps and no call, so nothing of the body is hoisted in front of both copies.
// The second copy reads the kernel arguments, the lane and the env through values the compiler cannot tie to the first copy's
// (an opaque zero added to the arguments' addresses, opaque copies of the indices): what it would otherwise keep in registers
// from one copy into the other -- every argument, every lane address -- is more than the 128 registers a 1024-lane workgroup has.
// The integrator's command for step k + 1 does not depend on the observation of step k (the one-frame delay), so the first copy
// stops behind its centre of gravity: it leaves its slopes in the pair's LDS words (step_pair_lds_layout) and the lane's next
// command in carry_cn, and forms Gy C of the second step on its last barriers.  The second copy starts at stage A and
// reconstructs both steps in one pass of stage C (step_body_text.hpp).
template <int KS, int SPEC>
__global__ void __launch_bounds__(1024) k_env_step_pair_sh6(const StepArgs a, const StepLds L, const StarEnv<float> star) {
    constexpr bool PE = false;
    float carry_cn = 0.f;
#define STEP_BODY_SUB 1
#include "step_body_text.hpp"
    lds_barrier();                                               // the second step re-uses the LDS of the first; its s1 is complete
    int kz;
    asm volatile("s_mov_b32 %0, 0" : "=s"(kz));
    const StepArgs* a_p2 = reinterpret_cast<const StepArgs*>(reinterpret_cast<const char*>(&a) + kz);
    const StepLds* L_p2 = reinterpret_cast<const StepLds*>(reinterpret_cast<const char*>(&L) + kz);
    const StarEnv<float>* star_p2 = reinterpret_cast<const StarEnv<float>*>(reinterpret_cast<const char*>(&star) + kz);
    int tid2 = threadIdx.x, e2 = blockIdx.x;
    asm volatile("" : "+v"(tid2));
    asm volatile("" : "+s"(e2));
    // The second inclusion shadows `a`, `L`, `star` with the opaque references below and declares its own locals; from the first one
    // it takes, by name, the static LDS arrays red, red_tail, red_mx and lohi (lohi with its contents), and from this kernel's
    // scope the register carry_cn and the opaque indices tid2, e2.
    {
        const StepArgs& a = *a_p2;
        const StepLds& L = *L_p2;
        const StarEnv<float>& star = *star_p2;
#define STEP_BODY_SUB 2
#include "step_body_text.hpp"
    }
}

template <int SPEC>
int launch_env_step_spec(const StepArgs& a, const StepLds& L, const StarEnv<float>& star, hipStream_t st) {
    const size_t lds = (size_t)L.total * 4;
    const int v = a.k.n_act <= 24 ? 0 : 1;
    const bool pe = a.k.pa.env_taps != nullptr;
    const void* fn = v == 0 ? (pe ? reinterpret_cast<const void*>(k_env_step_sh6<6, true, SPEC>) : reinterpret_cast<const void*>(k_env_step_sh6<6, false, SPEC>))
                            : (pe ? reinterpret_cast<const void*>(k_env_step_sh6<8, true, SPEC>) : reinterpret_cast<const void*>(k_env_step_sh6<8, false, SPEC>));
    static size_t attr_set[4] = {0, 0, 0, 0};
    const int vi = 2 * v + (pe ? 1 : 0);
    if (lds > 64 * 1024 && lds > attr_set[vi]) {
        AO_HIP(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        attr_set[vi] = lds;
    }
    if (v == 0 && !pe) hipLaunchKernelGGL((k_env_step_sh6<6, false, SPEC>), dim3(a.n_env), dim3(1024), lds, st, a, L, star);
    else if (v == 0) hipLaunchKernelGGL((k_env_step_sh6<6, true, SPEC>), dim3(a.n_env), dim3(1024), lds, st, a, L, star);
    else if (!pe) hipLaunchKernelGGL((k_env_step_sh6<8, false, SPEC>), dim3(a.n_env), dim3(1024), lds, st, a, L, star);
    else hipLaunchKernelGGL((k_env_step_sh6<8, true, SPEC>), dim3(a.n_env), dim3(1024), lds, st, a, L, star);
    AO_HIP(hipGetLastError());
    return 0;
}

template <int SPEC>
int launch_env_step_pair_spec(const StepArgs& a, const StepLds& L, const StarEnv<float>& star, hipStream_t st) {
    const size_t lds = (size_t)L.total * 4;
    const int v = a.k.n_act <= 24 ? 0 : 1;
    const void* fn = v == 0 ? reinterpret_cast<const void*>(k_env_step_pair_sh6<6, SPEC>) : reinterpret_cast<const void*>(k_env_step_pair_sh6<8, SPEC>);
    static size_t attr_set[2] = {0, 0};
    if (lds > 64 * 1024 && lds > attr_set[v]) {
        AO_HIP(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        attr_set[v] = lds;
    }
    if (v == 0) hipLaunchKernelGGL((k_env_step_pair_sh6<6, SPEC>), dim3(a.n_env), dim3(1024), lds, st, a, L, star);
    else hipLaunchKernelGGL((k_env_step_pair_sh6<8, SPEC>), dim3(a.n_env), dim3(1024), lds, st, a, L, star);
    AO_HIP(hipGetLastError());
    return 0;
}

}  // namespace ao
