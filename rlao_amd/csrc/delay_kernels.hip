// The delay line of aoenv_set_delay on the device (the action FIFO of the reference's TimeDelayEnv, MAIN/PO4AO/util_simple.py:25-52;
// the index arithmetic is delay.hpp): a ring of image slots, each [E][nAct^2] in the env dtype.  Three streaming kernels:
//   k_delay_push<T>       one launch in front of a delayed step: the caller's action image (aoenv_step) or gain * obs
//                         (aoenv_run_integrator: one multiply in the env dtype, not contracted, the bits a caller forms and
//                         k_rollout_action forms at sigma 0) into the slot the step writes
//   k_delay_refill<T>     one launch behind a recorded loop: the newest min(n_steps, d) actions of the trajectory into their slots
//   k_delay_zero_rows<T>  aoenv_reset_envs: the rows of the listed envs zeroed in every slot
// Alignment.  A slot of E nAct^2 elements is in general no multiple of 16 bytes (5 envs of a 9 x 9 image: 1620 bytes in float32), so
// the ring's slot stride is padded to one and every slot starts 16-byte aligned; a source -- a caller's tensor, slot k of a
// trajectory -- is aligned or not.  Per source image: 16-byte aligned, every lane moves one 16-byte vector and the last elements
// (E nAct^2 mod 4 or 2) go one by one; otherwise the whole image goes element by element, consecutive lanes on consecutive
// elements.  The choice is uniform over a workgroup.  A row of one env inside a slot (k_delay_zero_rows) starts anywhere: scalar
// stores.  Bytes: one read and one write of the image per push, of min(n_steps, d) images per refill.
#include "common.hpp"

namespace ao {

namespace {

template <typename T> struct Vec16;
template <> struct Vec16<float> { using type = float4; static constexpr int N = 4; };
template <> struct Vec16<double> { using type = double2; static constexpr int N = 2; };

template <typename T, bool SCALE>
__device__ __forceinline__ T delay_value(T v, T g) {
#pragma clang fp contract(off)
    return SCALE ? g * v : v;
}

// dst (16-byte aligned) = src or g * src, n elements; the workgroup blockIdx.x covers elements [256 V blockIdx.x, 256 V (blockIdx.x + 1))
template <typename T, bool SCALE>
__device__ __forceinline__ void delay_copy_image(T* __restrict__ dst, const T* __restrict__ src, size_t n, T g) {
    constexpr int V = Vec16<T>::N;
    using vec = typename Vec16<T>::type;
    const size_t b0 = (size_t)blockIdx.x * (256 * V);
    if ((reinterpret_cast<uintptr_t>(src) & 15) == 0) {
        size_t i = b0 + (size_t)threadIdx.x * V;
        if (i + V <= n) {
            vec v = *reinterpret_cast<const vec*>(src + i);
            v.x = delay_value<T, SCALE>(v.x, g);
            v.y = delay_value<T, SCALE>(v.y, g);
            if constexpr (V == 4) {
                v.z = delay_value<T, SCALE>(v.z, g);
                v.w = delay_value<T, SCALE>(v.w, g);
            }
            *reinterpret_cast<vec*>(dst + i) = v;
        } else {
            for (; i < n; ++i) dst[i] = delay_value<T, SCALE>(src[i], g);
        }
    } else {
        for (int j = 0; j < V; ++j) {
            const size_t i = b0 + (size_t)j * 256 + threadIdx.x;
            if (i < n) dst[i] = delay_value<T, SCALE>(src[i], g);
        }
    }
}

template <typename T, bool SCALE>
__global__ __launch_bounds__(256) void k_delay_push(T* __restrict__ dst, const T* __restrict__ src, size_t n, T g) {
    delay_copy_image<T, SCALE>(dst, src, n, g);
}

template <typename T>
__global__ __launch_bounds__(256) void k_delay_refill(T* __restrict__ ring, size_t slot_stride, int n_slots, int first_slot,
                                                      const T* __restrict__ traj, int first_traj, size_t n) {
    const int c = blockIdx.y;
    delay_copy_image<T, false>(ring + (size_t)((first_slot + c) % n_slots) * slot_stride, traj + (size_t)(first_traj + c) * n, n, (T)0);
}

template <typename T>
__global__ __launch_bounds__(256) void k_delay_zero_rows(T* __restrict__ ring, size_t slot_stride, const int* __restrict__ env_idx, int img) {
    T* row = ring + (size_t)blockIdx.y * slot_stride + (size_t)env_idx[blockIdx.x] * img;
    for (int p = threadIdx.x; p < img; p += 256) row[p] = (T)0;
}

template <typename T>
unsigned image_blocks(size_t n) { return (unsigned)((n + 256 * Vec16<T>::N - 1) / (256 * Vec16<T>::N)); }

}  // namespace

template <typename T>
int launch_delay_push(T* ring, size_t slot_stride, int slot, const T* src, size_t n, double scale, hipStream_t st) {
    if (n == 0 || n > slot_stride || slot < 0) return fail("delay push: %zu elements into slot %d of stride %zu", n, slot, slot_stride);
    T* dst = ring + (size_t)slot * slot_stride;
    if (scale != 0) hipLaunchKernelGGL((k_delay_push<T, true>), dim3(image_blocks<T>(n)), dim3(256), 0, st, dst, src, n, (T)scale);
    else hipLaunchKernelGGL((k_delay_push<T, false>), dim3(image_blocks<T>(n)), dim3(256), 0, st, dst, src, n, (T)0);
    AO_HIP(hipGetLastError());
    return 0;
}

template <typename T>
int launch_delay_refill(T* ring, size_t slot_stride, int n_slots, int first_slot, const T* traj, int first_traj, int m, size_t n, hipStream_t st) {
    if (m <= 0) return 0;
    if (n == 0 || n > slot_stride || m >= n_slots || first_slot < 0 || first_slot >= n_slots || first_traj < 0)
        return fail("delay refill: %d images of %zu elements from trajectory slot %d into slot %d of %d (stride %zu)", m, n, first_traj, first_slot, n_slots, slot_stride);
    hipLaunchKernelGGL(k_delay_refill<T>, dim3(image_blocks<T>(n), m), dim3(256), 0, st, ring, slot_stride, n_slots, first_slot, traj, first_traj, n);
    AO_HIP(hipGetLastError());
    return 0;
}

template <typename T>
int launch_delay_zero_rows(T* ring, size_t slot_stride, int n_slots, const int* env_idx, int n_idx, int img, hipStream_t st) {
    if (n_idx <= 0) return 0;
    hipLaunchKernelGGL(k_delay_zero_rows<T>, dim3(n_idx, n_slots), dim3(256), 0, st, ring, slot_stride, env_idx, img);
    AO_HIP(hipGetLastError());
    return 0;
}

#define AO_INST_DELAY(T)                                                                                            \
    template int launch_delay_push<T>(T*, size_t, int, const T*, size_t, double, hipStream_t);                      \
    template int launch_delay_refill<T>(T*, size_t, int, int, const T*, int, int, size_t, hipStream_t);             \
    template int launch_delay_zero_rows<T>(T*, size_t, int, const int*, int, int, hipStream_t);
AO_INST_DELAY(float)
AO_INST_DELAY(double)
#undef AO_INST_DELAY

}  // namespace ao
