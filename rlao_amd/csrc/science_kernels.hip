// Science window on the device (aoenv_science_psf and the long-exposure accumulators; the model, the table, the plan and the
// order of the general kernel's sums are science.hpp): out[e] = bin2x2(|F E_e F^T|^2) / n_fft^2, two small complex products per env
// that never leave the chip.  F [2][up][rp] is shared by every env and stays in L2.
//   k_science_window_mfma   float32 shards.  One workgroup (4 waves) per (block of 32 oversampled columns, group of row tiles, env)
//                           walks the field in chunks of 16 rows y:
//                             field    E of the chunk (sincosf of AOENV_B_PHASE times the amplitude, 0 where the amplitude is 0 and
//                                      in the padding) into LDS, re and im, row stride rp + 4
//                             stage 1  T1[y][c] = sum_x E[y][x] F[c0 + c][x], 16 x 32 complex: wave w takes column tile w & 1 and the
//                                      real (w < 2) or imaginary part; K = rp in rounds of 16.  Lane (r = l & 15, g = l >> 4) loads
//                                      E[r][x0 + 4 g .. + 3] from LDS and F[c][x0 + 4 g .. + 3] from the table as 16 bytes each and
//                                      issues four v_mfma_f32_16x16x4_f32, step s contracting over x0 + 4 g' + s, g' = 0 .. 3, on
//                                      BOTH operands.  Two accumulators, one per product of the complex multiply (re: Er Fr and
//                                      -Ei Fi; im: Er Fi and Ei Fr), added once at the end.  D (lane: column l & 15, rows
//                                      4 (l >> 4) + v) goes to LDS transposed, [part][column][y] at stride 20: 16 bytes per lane,
//                                      and the very layout stage 2 reads its B operand in.
//                             stage 2  P[j][c] += sum_y F[j][y0 + y] T1[y][c]: wave w owns row tiles w, w + 4, ... of its group
//                                      (tiles_per_wave of them, 1 .. 8, 16 rows each) times both column tiles, re and im: 16
//                                      accumulator registers per tile.  A = F[j][y0 + 4 g .. + 3] from the table (16 bytes), B =
//                                      T1^T[c][4 g .. + 3] from LDS, four steps as above; re += Fr T1r, re += -Fi T1i, im += Fr T1i,
//                                      im += Fi T1r, in that order, every chunk.
//                           Epilogue in registers: |P|^2 per element, the two rows of an output pixel are registers (v, v + 1) of
//                           one lane, its two columns lanes (l, l ^ 1): one DPP exchange, the even lane owns the pixel (sci_bin's
//                           order), ONE multiply by the scale, then a store or the accumulators' += .  No atomics.
//                           Guards: table rows and columns are padded to the tile with zeros, so no operand load is guarded; a
//                           row tile >= n_row_tiles is skipped by its wave (uniform); the phase is read for y < R, x < R alone;
//                           only pixels a < W, b < W are written.
//   k_science_window<T>     the general kernel: float64 shards, AOENV_PATH_SCI_GENERAL, a plan the matrix-core kernel refuses.  One
//                           workgroup per (8 oversampled columns, env): lane y forms row y of E and its 8 first products as fma
//                           chains over x (sci_cmac) into LDS, then a lane per output pixel runs the four chains over y.
//   Both add 1 to count[e] by one lane of the env's first workgroup when they accumulate.
#include "common.hpp"
#include "science.hpp"

namespace ao {

namespace {

using sci_f32x4 = __attribute__((ext_vector_type(4))) float;

__device__ __forceinline__ void sci_sincos(float p, float* s, float* c) { sincosf(p, s, c); }
__device__ __forceinline__ void sci_sincos(double p, double* s, double* c) { sincos(p, s, c); }
__device__ __forceinline__ float sci_log10(float v) { return log10f(v); }
__device__ __forceinline__ double sci_log10(double v) { return log10(v); }

// E[y][x] of env e (0 where the amplitude is 0: outside the pupil the phase buffer is not the field's)
template <typename T>
__device__ __forceinline__ void sci_field(const SciArgs<T>& a, const T* phase, int y, int x, T* re, T* im) {
    *re = (T)0;
    *im = (T)0;
    if (y >= a.R || x >= a.R) return;
    const T am = a.amp[y * a.R + x];
    if (am == (T)0) return;
    if (a.flat) {
        *re = am;
        return;
    }
    T s, c;
    sci_sincos(phase[y * a.R + x], &s, &c);
    *re = am * c;
    *im = am * s;
}

// the pixel (a_, b) of env e: stored, or added to the accumulators
template <typename T>
__device__ __forceinline__ void sci_emit(const SciArgs<T>& a, int e, int a_, int b, T v) {
    const size_t i = ((size_t)e * a.W + a_) * a.W + b;
    if (a.out) {
        a.out[i] = v;
        return;
    }
    a.sum[i] = a.sum[i] + v;
    if (a.sum_log10) a.sum_log10[i] = a.sum_log10[i] + sci_log10(v);
}

template <int NT>
__global__ void __launch_bounds__(256) k_science_window_mfma(const SciArgs<float> a, const SciPlan pl) {
    extern __shared__ __align__(16) float sci_lds[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r = lane & 15, g = lane >> 4;
    const int blk = blockIdx.x, grp = blockIdx.y, e = blockIdx.z;
    const int rp = pl.rp, es = rp + 4;
    float* Er = sci_lds;
    float* Ei = Er + kSciTileK * es;
    float* Tt = Ei + kSciTileK * es;                               // [2][32][20]
    const float* Fr = a.table;
    const float* Fi = a.table + (size_t)pl.up * rp;
    const float* phase = a.phase + (size_t)e * a.R * a.R;
    if (a.sum && a.count && blk == 0 && grp == 0 && threadIdx.x == 0) a.count[e] = a.count[e] + 1;
    // stage 1: this wave's tile of T1
    const int ct = wave & 1, part = wave >> 1;
    const size_t row1 = (size_t)(blk * kSciColBlock + ct * 16 + r) * rp;
    const float* b0p = (part ? Fi : Fr) + row1;                    // the table plane Er meets
    const float* b1p = (part ? Fr : Fi) + row1;                    // ... and the one Ei meets
    const float sgn = part ? 1.f : -1.f;                           // re: -Ei Fi
    sci_f32x4 pr[NT][2], pi[NT][2];
#pragma unroll
    for (int i = 0; i < NT; ++i)
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            pr[i][c] = sci_f32x4{0.f, 0.f, 0.f, 0.f};
            pi[i][c] = sci_f32x4{0.f, 0.f, 0.f, 0.f};
        }
    for (int y0 = 0; y0 < rp; y0 += kSciTileK) {
        __syncthreads();                                           // the previous chunk's readers of E and T1 are done
        for (int idx = threadIdx.x; idx < kSciTileK * rp; idx += 256) {
            const int y = idx / rp, x = idx - y * rp;
            float re, im;
            sci_field<float>(a, phase, y0 + y, x, &re, &im);
            Er[y * es + x] = re;
            Ei[y * es + x] = im;
        }
        __syncthreads();
        sci_f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
        for (int x0 = 0; x0 < rp; x0 += 16) {
            const int k = x0 + 4 * g;
            const sci_f32x4 er = *reinterpret_cast<const sci_f32x4*>(Er + r * es + k);
            const sci_f32x4 ei = *reinterpret_cast<const sci_f32x4*>(Ei + r * es + k);
            const sci_f32x4 f0 = *reinterpret_cast<const sci_f32x4*>(b0p + k);
            const sci_f32x4 f1 = *reinterpret_cast<const sci_f32x4*>(b1p + k);
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(er[s], f0[s], acc0, 0, 0, 0);
                acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(sgn * ei[s], f1[s], acc1, 0, 0, 0);
            }
        }
        // D: column r of the tile, rows 4 g + v -> T1^T[part][ct * 16 + r][4 g .. 4 g + 3]
        *reinterpret_cast<sci_f32x4*>(Tt + (part * kSciColBlock + ct * 16 + r) * 20 + 4 * g) = acc0 + acc1;
        __syncthreads();
        sci_f32x4 tr[2], ti[2];
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            tr[c] = *reinterpret_cast<const sci_f32x4*>(Tt + (c * 16 + r) * 20 + 4 * g);
            ti[c] = *reinterpret_cast<const sci_f32x4*>(Tt + (kSciColBlock + c * 16 + r) * 20 + 4 * g);
        }
#pragma unroll
        for (int i = 0; i < NT; ++i) {
            const int tile = grp * 4 * NT + 4 * i + wave;
            if (tile >= pl.n_row_tiles) continue;                  // (wave-uniform)
            const size_t row2 = (size_t)(tile * 16 + r) * rp + y0 + 4 * g;
            const sci_f32x4 fr = *reinterpret_cast<const sci_f32x4*>(Fr + row2);
            const sci_f32x4 fi = *reinterpret_cast<const sci_f32x4*>(Fi + row2);
#pragma unroll
            for (int c = 0; c < 2; ++c)
#pragma unroll
                for (int s = 0; s < 4; ++s) {
                    pr[i][c] = __builtin_amdgcn_mfma_f32_16x16x4f32(fr[s], tr[c][s], pr[i][c], 0, 0, 0);
                    pr[i][c] = __builtin_amdgcn_mfma_f32_16x16x4f32(-fi[s], ti[c][s], pr[i][c], 0, 0, 0);
                    pi[i][c] = __builtin_amdgcn_mfma_f32_16x16x4f32(fr[s], ti[c][s], pi[i][c], 0, 0, 0);
                    pi[i][c] = __builtin_amdgcn_mfma_f32_16x16x4f32(fi[s], tr[c][s], pi[i][c], 0, 0, 0);
                }
        }
    }
    // epilogue: lane (r, g) holds P[tile * 16 + 4 g + v][blk * 32 + c * 16 + r]
#pragma unroll
    for (int i = 0; i < NT; ++i) {
        const int tile = grp * 4 * NT + 4 * i + wave;
        if (tile >= pl.n_row_tiles) continue;
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            float p[4];
#pragma unroll
            for (int v = 0; v < 4; ++v) p[v] = sci_power<float>(pr[i][c][v], pi[i][c][v]);
            const int b = (blk * kSciColBlock + c * 16 + r) >> 1;
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const float q0 = p[2 * h], q1 = p[2 * h + 1];
                const float o0 = __shfl_xor(q0, 1), o1 = __shfl_xor(q1, 1);     // the odd column's rows
                const int a_ = tile * 8 + 2 * g + h;
                if ((r & 1) == 0 && a_ < a.W && b < a.W) sci_emit<float>(a, e, a_, b, sci_bin<float>(q0, q1, o0, o1, a.scale));
            }
        }
    }
}

template <typename T>
__global__ void __launch_bounds__(256) k_science_window(const SciArgs<T> a, const SciPlan pl) {
    extern __shared__ __align__(16) unsigned char sci_raw[];
    constexpr int CB = kSciGeneralCols;
    T* Tr = reinterpret_cast<T*>(sci_raw);                         // [R][CB]
    T* Ti = Tr + (size_t)a.R * CB;
    const int e = blockIdx.z, c0 = blockIdx.x * CB, rp = pl.rp;
    const T* Fr = a.table;
    const T* Fi = a.table + (size_t)pl.up * rp;
    const T* phase = a.phase + (size_t)e * a.R * a.R;
    if (a.sum && a.count && blockIdx.x == 0 && threadIdx.x == 0) a.count[e] = a.count[e] + 1;
    for (int y = threadIdx.x; y < a.R; y += 256) {
        T tr[CB], ti[CB];
#pragma unroll
        for (int c = 0; c < CB; ++c) tr[c] = ti[c] = (T)0;
        for (int x = 0; x < a.R; ++x) {
            T er, ei;
            sci_field<T>(a, phase, y, x, &er, &ei);
#pragma unroll
            for (int c = 0; c < CB; ++c) sci_cmac<T>(er, ei, Fr[(size_t)(c0 + c) * rp + x], Fi[(size_t)(c0 + c) * rp + x], tr[c], ti[c]);
        }
#pragma unroll
        for (int c = 0; c < CB; ++c) {
            Tr[y * CB + c] = tr[c];
            Ti[y * CB + c] = ti[c];
        }
    }
    __syncthreads();
    for (int idx = threadIdx.x; idx < a.W * (CB / 2); idx += 256) {
        const int a_ = idx / (CB / 2), b4 = idx - a_ * (CB / 2), b = blockIdx.x * (CB / 2) + b4;
        if (b >= a.W) continue;
        T p[2][2];                                                 // [row][column] of the pixel's cell
#pragma unroll
        for (int dj = 0; dj < 2; ++dj)
#pragma unroll
            for (int dc = 0; dc < 2; ++dc) {
                const size_t row = (size_t)(2 * a_ + dj) * rp;
                const int c = 2 * b4 + dc;
                T re = (T)0, im = (T)0;
                for (int y = 0; y < a.R; ++y) sci_cmac<T>(Fr[row + y], Fi[row + y], Tr[y * CB + c], Ti[y * CB + c], re, im);
                p[dj][dc] = sci_power<T>(re, im);
            }
        sci_emit<T>(a, e, a_, b, sci_bin<T>(p[0][0], p[1][0], p[0][1], p[1][1], a.scale));
    }
}

template <typename T>
int sci_launch_general(const SciArgs<T>& a, const SciPlan& pl, hipStream_t st) {
    const size_t lds = (size_t)2 * a.R * kSciGeneralCols * sizeof(T);
    if (lds > 160 * 1024) return fail("science window: R = %d does not fit the general kernel's LDS", a.R);
    if (lds > 64 * 1024)
        AO_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(k_science_window<T>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(k_science_window<T>, dim3(pl.general_blocks, 1, a.n_env), dim3(256), lds, st, a, pl);
    return 0;
}

template <typename T>
int sci_dispatch(const SciArgs<T>& a, const SciPlan& pl, bool, hipStream_t st) { return sci_launch_general<T>(a, pl, st); }
template <>
int sci_dispatch<float>(const SciArgs<float>& a, const SciPlan& pl, bool general, hipStream_t st) {
    if (general || !pl.mfma_ok) return sci_launch_general<float>(a, pl, st);
    const dim3 grid(pl.n_col_blocks, pl.n_row_groups, a.n_env);
    switch (pl.tiles_per_wave) {
#define AO_SCI_CASE(NT) \
    case NT: hipLaunchKernelGGL(k_science_window_mfma<NT>, grid, dim3(256), pl.lds_bytes, st, a, pl); break;
        AO_SCI_CASE(1) AO_SCI_CASE(2) AO_SCI_CASE(3) AO_SCI_CASE(4) AO_SCI_CASE(5) AO_SCI_CASE(6) AO_SCI_CASE(7) AO_SCI_CASE(8)
#undef AO_SCI_CASE
        default: return fail("science window: %d tiles per wave", pl.tiles_per_wave);
    }
    return 0;
}

}  // namespace

template <typename T>
int launch_science_window(const SciArgs<T>& a, bool general, hipStream_t st) {
    if (a.n_env < 1 || a.n_env > 65535 || a.R < 1 || a.W < 2 || a.W % 2 || !a.amp || !a.table || (!a.flat && !a.phase) ||
        (a.out != nullptr) == (a.sum != nullptr))
        return fail("science window: %d envs, R = %d, W = %d, or not exactly one of output and accumulator", a.n_env, a.R, a.W);
    const SciPlan pl = sci_plan(a.R, a.W);
    if (pl.n_row_groups > 65535) return fail("science window: W = %d too large", a.W);
    AO_TRY(sci_dispatch<T>(a, pl, general, st));
    AO_HIP(hipGetLastError());
    return 0;
}
template int launch_science_window<float>(const SciArgs<float>&, bool, hipStream_t);
template int launch_science_window<double>(const SciArgs<double>&, bool, hipStream_t);

}  // namespace ao
