// Geometric Shack-Hartmann kernels (OOPAO/ShackHartmann.py:382-394, 676-695; the model and the order of the sums: sh_geometric.hpp).
//   k_sh_geometric  the stand-alone sensor: unmasked phase + pupil -> AOENV_B_SIGNAL; grid = (lenslet rows, n_env)
//   k_geo_tail      the same slopes into LDS, then tail_from_slopes (sh_device.hpp): where k_sh_tail sits in a diffractive step
// Both call geo_band_slopes, so the signal of the two is the same bits.
#include "common.hpp"
#include "sh_device.hpp"
#include "sh_geometric.hpp"

namespace ao {

// Slope sums of the g lenslet rows i0 .. i0 + g - 1 of one env, by the whole workgroup (nt lanes, lane tid).
//   phi [R][R] the env's unmasked phase, pupil [R][R]
//   work    LDS, geo_band_elems(R, n_subap, g, sizeof(T)) elements: strip [(g p + 2)][R] | col [g][2][R] | tot [g][2][n_subap] |
//           pup [g p][R] bytes
// On return (behind a barrier) tot[(gi * 2 + 0) * n_subap + j] is the sum of the axis-1 (along a row) gradient over lenslet
// (i0 + gi, j) and tot[(gi * 2 + 1) * n_subap + j] that of the axis-0 gradient.
// The strip and the band's pupil flags are read from memory once, row-contiguous, four loads of a lane in flight together; every
// neighbour and every flag then comes from LDS (a flag loaded where it is used made the column sums a chain of p memory latencies).
// Rows outside the grid are staged from a clamped row and never used: the first / last row and column take the one-sided difference.
template <typename T>
__device__ __forceinline__ T* geo_band_slopes(const T* __restrict__ phi, const uint8_t* __restrict__ pupil, T* work, int i0, int g,
                                              int R, int n_subap, int p, int tid, int nt) {
    const int rows = g * p + 2, rbase = i0 * p - 1;
    T* strip = work;
    T* col = strip + (size_t)rows * R;
    T* tot = col + (size_t)2 * g * R;
    uint8_t* pup = reinterpret_cast<uint8_t*>(tot + (size_t)2 * g * n_subap);
    for (int q0 = tid; q0 < rows * R; q0 += 4 * nt) {
        T v[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int idx = q0 + q * nt < rows * R ? q0 + q * nt : q0;
            const int k = idx / R, x = idx - k * R;
            int r = rbase + k;
            r = r < 0 ? 0 : (r > R - 1 ? R - 1 : r);
            v[q] = phi[(size_t)r * R + x];
        }
#pragma unroll
        for (int q = 0; q < 4; ++q)
            if (q0 + q * nt < rows * R) strip[q0 + q * nt] = v[q];
    }
    {
        const uint8_t* src = pupil + (size_t)i0 * p * R;         // the band's g p rows are contiguous in the pupil
        const int n = g * p * R;
        for (int j0 = tid; j0 < n; j0 += 4 * nt) {
            uint8_t v[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) v[q] = src[j0 + q * nt < n ? j0 + q * nt : j0];
#pragma unroll
            for (int q = 0; q < 4; ++q)
                if (j0 + q * nt < n) pup[j0 + q * nt] = v[q];
        }
    }
    __syncthreads();
    // one lane per (band row, column): the column's p terms of both gradients in ascending row order
    for (int idx = tid; idx < g * R; idx += nt) {
        const int gi = idx / R, x = idx - gi * R;
        T a0 = (T)0, a1 = (T)0;
        for (int u = 0; u < p; ++u) {
            const int k = gi * p + u + 1, r = rbase + k;
            const T* s = strip + (size_t)k * R + x;
            const T c = s[0];
            const T g0 = r == 0 ? s[R] - c : (r == R - 1 ? c - s[-R] : (s[R] - s[-R]) * (T)0.5);
            const T g1 = x == 0 ? s[1] - c : (x == R - 1 ? c - s[-1] : (s[1] - s[-1]) * (T)0.5);
            if (pup[(gi * p + u) * R + x]) {
                a0 += g0;
                a1 += g1;
            }
        }
        col[(size_t)(gi * 2 + 0) * R + x] = a1;
        col[(size_t)(gi * 2 + 1) * R + x] = a0;
    }
    __syncthreads();
    // one lane per (band row, block, lenslet): its p column sums in ascending column order
    for (int idx = tid; idx < 2 * g * n_subap; idx += nt) {
        const int gb = idx / n_subap, j = idx - gb * n_subap;
        const T* c = col + (size_t)gb * R + j * p;
        T acc = (T)0;
        for (int v = 0; v < p; ++v) acc += c[v];
        tot[idx] = acc;
    }
    __syncthreads();
    return tot;
}

template <typename T>
__global__ void __launch_bounds__(256) k_sh_geometric(const T* __restrict__ phase_np, const uint8_t* __restrict__ pupil,
                                                      const short* __restrict__ slot_of, T units, T* __restrict__ signal, int R,
                                                      int n_subap, int n_valid) {
    extern __shared__ __align__(16) unsigned char lds_raw[];
    T* work = reinterpret_cast<T*>(lds_raw);
    const int e = blockIdx.y, i = blockIdx.x, tid = threadIdx.x;
    const int p = R / n_subap;
    const T* tot = geo_band_slopes<T>(phase_np + (size_t)e * R * R, pupil, work, i, 1, R, n_subap, p, tid, blockDim.x);
    T* sg = signal + (size_t)e * 2 * n_valid;
    for (int j = tid; j < n_subap; j += blockDim.x) {
        const int s = slot_of[i * n_subap + j];
        if (s >= 0) {
            sg[s] = tot[j] / units;                                   // first block: the axis-1 gradient
            sg[n_valid + s] = tot[n_subap + j] / units;
        }
    }
}

template <typename T>
int launch_sh_geometric(const T* phase_np, const uint8_t* pupil, const short* slot_of, double units, T* signal, int n_env, int R,
                        int n_subap, int n_valid, hipStream_t st) {
    const size_t lds = geo_row_lds_bytes(R, n_subap, sizeof(T));
    if (lds > 160 * 1024) return fail("geometric sensor: a lenslet row of %d x %d pixels needs %zu B of LDS", R / n_subap, R, lds);
    if (lds > 64 * 1024)
        AO_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(k_sh_geometric<T>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                   (int)lds));
    hipLaunchKernelGGL(k_sh_geometric<T>, dim3(n_subap, n_env), dim3(256), lds, st, phase_np, pupil, slot_of, (T)units, signal, R,
                       n_subap, n_valid);
    AO_HIP(hipGetLastError());
    return 0;
}

// Fused tail of a geometric step: one workgroup (1024 lanes) per env.  LDS: sl [2 nValid] | img_s [nAct^2 + n_modes] (k_sh_tail's
// layout, what tail_from_slopes expects) | the band's work area.  The env's lenslet rows are taken g at a time.
template <typename T>
__global__ void __launch_bounds__(1024) k_geo_tail(const T* __restrict__ phase_np, const uint8_t* __restrict__ pupil,
                                                    const short* __restrict__ slot_of, T units, T* __restrict__ signal,
                                                    const T* __restrict__ fac_m, const T* __restrict__ fac_m2c_t, int n_modes,
                                                    const FinishArgs<T> f, int R, int n_subap, int n_valid, int g, int n_env) {
    extern __shared__ __align__(16) unsigned char lds_raw[];
    T* sl = reinterpret_cast<T*>(lds_raw);                     // [2 nValid] slopes
    T* img_s = sl + 2 * n_valid;                               // [nAct^2] observation image, [n_modes] modal coefficients
    const int img = f.n_act * f.n_act;
    T* work = img_s + img + n_modes;
    __shared__ double red[16];
    static_assert(sizeof(red) == kGeoTailStaticLds, "geo_tail_band leaves room for the kernel's static LDS");
    const int e = blockIdx.x, tid = threadIdx.x;
    const int p = R / n_subap;
    for (int q = tid; q < img; q += blockDim.x) img_s[q] = (T)0;
    const T* phi = phase_np + (size_t)e * R * R;
    T* sg = signal + (size_t)e * 2 * n_valid;
    for (int i0 = 0; i0 < n_subap; i0 += g) {
        const int gg = min(g, n_subap - i0);
        const T* tot = geo_band_slopes<T>(phi, pupil, work, i0, gg, R, n_subap, p, tid, blockDim.x);
        for (int idx = tid; idx < gg * n_subap; idx += blockDim.x) {
            const int gi = idx / n_subap, j = idx - gi * n_subap;
            const int s = slot_of[(i0 + gi) * n_subap + j];
            if (s >= 0) {
                const T s0 = tot[(gi * 2 + 0) * n_subap + j] / units, s1 = tot[(gi * 2 + 1) * n_subap + j] / units;
                sl[s] = s0;
                sl[n_valid + s] = s1;
                sg[s] = s0;
                sg[n_valid + s] = s1;
            }
        }
        // a partial last band (gg < g) lays its work area out anew: its staging would write where lanes of this band still read tot.
        // The barrier also completes sl for tail_from_slopes behind the last band.
        __syncthreads();
    }
    tail_from_slopes<T>(sl, img_s, red, fac_m, fac_m2c_t, n_modes, f, e, n_valid, n_env);
}

template <typename T>
int launch_geo_tail(const T* phase_np, const uint8_t* pupil, const short* slot_of, double units, T* signal, const T* fac_m,
                    const T* fac_m2c_t, int n_modes, const FinishArgs<T>& fa, int n_env, int R, int n_subap, int n_valid,
                    hipStream_t st) {
    const int g = geo_tail_band(R, n_subap, n_valid, fa.n_act, n_modes, sizeof(T));
    if (g < 1) return -1;
    const size_t lds = sizeof(T) * (geo_tail_base_elems(n_valid, fa.n_act, n_modes) + geo_band_elems(R, n_subap, g, sizeof(T)));
    hipLaunchKernelGGL(k_geo_tail<T>, dim3(n_env), dim3(1024), lds, st, phase_np, pupil, slot_of, (T)units, signal, fac_m, fac_m2c_t,
                       n_modes, fa, R, n_subap, n_valid, g, n_env);
    AO_HIP(hipGetLastError());
    return 0;
}

#define INST(T)                                                                                                                  \
    template int launch_sh_geometric<T>(const T*, const uint8_t*, const short*, double, T*, int, int, int, int, hipStream_t);     \
    template int launch_geo_tail<T>(const T*, const uint8_t*, const short*, double, T*, const T*, const T*, int,                  \
                                    const FinishArgs<T>&, int, int, int, int, hipStream_t);
INST(float)
INST(double)
#undef INST

}  // namespace ao
