// The policy of the PO4AO trainer inside the library: ConvPolicy (MAIN/PO4AO/conv_models_simple.py:56-111),
//   out = net(cat([obs, past_obs, past_act]));  out = clamp(out, -1, 1);  action = vec_to_img(F @ out[valid])
// with net = Conv2d(2H-1, F, 3, padding=1), LeakyReLU, Conv2d(F, F, 3, padding=1), LeakyReLU, Conv2d(F, 1, 3, padding=1).
// Three launches per evaluation: the two wide convolutions, hidden images in device buffers ([E][F][a^2]), and a last stage per env.
//
// k_policy_conv_mfma<NT>  float32, implicit GEMM on v_mfma_f32_16x16x4_f32 (an exact k-ordered fma chain):
//     M = the pixels of one band of image rows (at most 256, 16 tiles of 16), N = filters, K = 9 C_in walked as (ci, ky, kx).
//     Workgroup (band, env), 256 lanes.  LDS: the band's input with its one-pixel frame of zeros, [C_in][rows + 2][a + 2] (a hidden
//     image does not fit whole: 64 x 43 x 43 floats = 473 KB; policy_bands picks the tallest band of which two fit a CU: 5 rows at
//     a = 41 and 64 channels, 77 KB, so that one workgroup stages while the other multiplies), staged from the contiguous span of source rows of every channel (the first layer
//     resolves a channel's source once, into a pointer table in LDS), and koff[k], the offset of tap k = (ci, ky, kx) inside that tile
//     (0 in the K padding, where the weight is zero).
//     Wave w owns the M tiles w, w + 4, w + 8, w + 12 and, per pass, NT N tiles: 4 NT accumulators of 4 registers.  Per k step of 4 taps a
//     lane reads koff once, one A element per M tile from LDS (A[m = lane & 15][k = lane >> 4]: the pixel's window base + koff) and
//     one B element per N tile from the re-laid weights ([kstep][F / 16][64]: B[k = lane >> 4][n = lane & 15], 256 contiguous
//     bytes per wave, L2 resident), then issues 4 NT MFMAs; the operands of step s + 1 are loaded before the MFMAs of step s (two
//     register sets used in turn).  A wave runs the loop written for its number of live tiles (1 .. 4); a lane past the last pixel inside a tile computes pixel 0's window again and
//     does not store.  Epilogue: + bias, LeakyReLU, store (D[m = 4 (lane >> 4) + r][n = lane & 15]: 4 consecutive pixels per lane).
//     An output element is fma(x_K, w_K, .. fma(x_1, w_1, fma(x_0, w_0, 0))) over k = (ci, ky, kx) in order, padding taps entering
//     as x = 0: the order depends on the network's shape alone, not on n_env, the env's row, the band or the tile.
// k_policy_conv_general<T>  one output element per lane, the same chain written with fma (conv_point; padding taps enter as x = 0).
//     path = 1, float64 shards, n_filt % 16 != 0, and geometries whose band does not fit in LDS.
// k_policy_action<T>  one workgroup of 1024 lanes per env: conv3 (one filter: 15/16 of an MFMA tile would be padding, so the VALU
//     chain of the general kernel, for both paths) + bias + clamp at the valid actuators only, v = Fl (Fr v) with the policy's
//     factors, the exploration noise of k_rollout_action (noise_device.hpp: same draw, same filter, same bits), scatter.
// k_policy_roll<T>  after the last step of a rollout: the caller's windows shifted by n_steps and refilled from the trajectory.
#include "policy.hpp"
#include "noise_device.hpp"

namespace ao {

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

__device__ inline int cdiv16(int n) { return (n + 15) >> 4; }

// The GEMM of one wave: MTN M tiles (w, w + 4, ..) x all N tiles, NT at a time.  Two operand sets in registers, used in turn: the
// loads of step s + 1 are issued before the MFMAs of step s and awaited after them.
template <int NT, int MTN>
__device__ inline void conv_tiles(const float* tile, const int* koff, const float* __restrict__ wt, const float* __restrict__ bias,
                                  float* __restrict__ o, int img, int n_act, int W, int npx, int nt_all, int ksteps, float slope, int w,
                                  int lane) {
    const int kq = lane >> 4;
    int base[MTN];
#pragma unroll
    for (int j = 0; j < MTN; ++j) {
        const int p = 16 * (4 * j + w) + (lane & 15);
        const int pc = p < npx ? p : 0;
        const int r = pc / n_act;
        base[j] = r * W + (pc - r * n_act);
    }
    const size_t wstep = (size_t)nt_all * 64;
    for (int ng = 0; ng < nt_all / NT; ++ng) {
        f32x4 acc[MTN][NT];
#pragma unroll
        for (int j = 0; j < MTN; ++j)
#pragma unroll
            for (int n = 0; n < NT; ++n) acc[j][n] = f32x4{0.f, 0.f, 0.f, 0.f};
        const float* wp = wt + (size_t)ng * NT * 64 + lane;
        float a0[MTN], b0[NT], a1[MTN], b1[NT];
        auto load = [&](int ks, float (&a)[MTN], float (&b)[NT]) {
            const int off = koff[4 * ks + kq];
#pragma unroll
            for (int n = 0; n < NT; ++n) b[n] = wp[(size_t)ks * wstep + n * 64];
#pragma unroll
            for (int j = 0; j < MTN; ++j) a[j] = tile[base[j] + off];
        };
        auto mma = [&](const float (&a)[MTN], const float (&b)[NT]) {
#pragma unroll
            for (int j = 0; j < MTN; ++j)
#pragma unroll
                for (int n = 0; n < NT; ++n) acc[j][n] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[j], b[n], acc[j][n], 0, 0, 0);
        };
        load(0, a0, b0);
        int ks = 0;
        // (the scheduling fences keep each set's loads in front of the other set's MFMAs: left alone, the scheduler sinks a load
        // behind the last use of the register it reuses and the MFMAs of the next step wait for L2)
        for (; ks + 1 < ksteps; ks += 2) {
            load(ks + 1, a1, b1);
            __builtin_amdgcn_sched_barrier(0);
            mma(a0, b0);
            __builtin_amdgcn_sched_barrier(0);
            load(min(ks + 2, ksteps - 1), a0, b0);                 // (unconditional: a branch here makes the waits of the next MFMAs cover these loads)
            __builtin_amdgcn_sched_barrier(0);
            mma(a1, b1);
            __builtin_amdgcn_sched_barrier(0);
        }
        if (ks < ksteps) mma(a0, b0);                              // an odd number of steps: the last one sits in set 0
#pragma unroll
        for (int n = 0; n < NT; ++n) {
            const int f = (ng * NT + n) * 16 + (lane & 15);
            const float bf = bias[f];
            float* of = o + (size_t)f * img;
#pragma unroll
            for (int j = 0; j < MTN; ++j)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int p = 16 * (4 * j + w) + 4 * kq + r;
                    if (p < npx) {
                        const float v = acc[j][n][r] + bf;
                        of[p] = v > 0.0f ? v : v * slope;
                    }
                }
        }
    }
}

template <int NT>
__global__ __launch_bounds__(256) void k_policy_conv_mfma(ConvIn<float> in, const float* __restrict__ wt, const float* __restrict__ bias,
                                                          float* __restrict__ out, int n_act, int n_filt, int band_rows, int ksteps,
                                                          float slope) {
    extern __shared__ __attribute__((aligned(16))) char policy_smem[];
    const int tid = threadIdx.x, lane = tid & (kWave - 1), w = tid / kWave;
    const int e = blockIdx.y, y0 = blockIdx.x * band_rows;
    const int rows = min(band_rows, n_act - y0);                   // rows of this band (the last one may be shorter)
    const int W = n_act + 2, TH = band_rows + 2, plane = TH * W, C = in.C;
    float* tile = reinterpret_cast<float*>(policy_smem);           // [C][TH][W]
    int* koff = reinterpret_cast<int*>(tile + (size_t)C * plane);  // [4 ksteps]

    for (int k = tid; k < 4 * ksteps; k += 256) {
        const int ci = k / 9, t = k - 9 * ci;
        koff[k] = ci < C ? ci * plane + (t / 3) * W + (t % 3) : 0;
    }
    // The band's source rows y0 - 1 .. y0 + rows (clipped to the image) are one contiguous span of every channel: zero the tile (its
    // frame stays zero), then copy the spans, eight independent loads in flight per lane (the copy is latency bound: one load per
    // lane and trip leaves the matrix cores waiting for HBM)
    const float** chan = reinterpret_cast<const float**>(koff + 4 * ksteps + ((C * plane) & 1));   // [C], 8-byte aligned
    for (int c = tid; c < C; c += 256) chan[c] = conv_channel(in, c, e);
    for (int i = tid; i < C * plane; i += 256) tile[i] = 0.0f;
    __syncthreads();
    const int gy0 = max(y0 - 1, 0), gy1 = min(y0 + rows + 1, n_act);             // source rows [gy0, gy1)
    const int span = (gy1 - gy0) * n_act, total = C * span;
    const uint32_t m_span = (uint32_t)(((1ull << 32) + span - 1) / span), m_act = (uint32_t)(((1ull << 32) + n_act - 1) / n_act);
    const int src0 = gy0 * n_act, dst0 = (gy0 - (y0 - 1)) * W + 1;
    constexpr int kInFlight = 8;
    for (int i0 = tid; i0 < total; i0 += 256 * kInFlight) {
        float v[kInFlight];
        int d[kInFlight];
#pragma unroll
        for (int u = 0; u < kInFlight; ++u) {
            const int i = i0 + 256 * u;
            d[u] = -1;
            if (i < total) {
                // exact for i < 2^32 / divisor: i < 128 x 768, divisors <= 768
                const int c = (int)__umulhi((uint32_t)i, m_span), q = i - c * span;
                const int r = (int)__umulhi((uint32_t)q, m_act);
                v[u] = chan[c][src0 + q];
                d[u] = c * plane + dst0 + r * W + (q - r * n_act);
            }
        }
#pragma unroll
        for (int u = 0; u < kInFlight; ++u)
            if (d[u] >= 0) tile[d[u]] = v[u];
    }
    __syncthreads();

    const int npx = rows * n_act;
    const int ntile = __builtin_amdgcn_readfirstlane((cdiv16(npx) - w + 3) >> 2);   // live M tiles of this wave: w, w + 4, .. < ceil(npx / 16)
    float* o = out + (size_t)e * n_filt * in.img + (size_t)y0 * n_act;
    switch (ntile) {                                               // (no barrier follows: a wave without a tile leaves)
        case 4: conv_tiles<NT, 4>(tile, koff, wt, bias, o, in.img, n_act, W, npx, n_filt / 16, ksteps, slope, w, lane); break;
        case 3: conv_tiles<NT, 3>(tile, koff, wt, bias, o, in.img, n_act, W, npx, n_filt / 16, ksteps, slope, w, lane); break;
        case 2: conv_tiles<NT, 2>(tile, koff, wt, bias, o, in.img, n_act, W, npx, n_filt / 16, ksteps, slope, w, lane); break;
        case 1: conv_tiles<NT, 1>(tile, koff, wt, bias, o, in.img, n_act, W, npx, n_filt / 16, ksteps, slope, w, lane); break;
        default: break;
    }
}

// One output element of a 3x3 convolution with padding 1, summed as the chain fma(x, w, acc) over (ci, ky, kx) in order.  A tap
// outside the image is loaded from the clamped address and enters as x = 0 (fma(0, w, acc) = acc): no branch, so the nine loads of
// a channel go out together -- with a branch per tap every load waits for the one before it.  chan(c): the channel's image.
template <typename T, typename Chan>
__device__ inline T conv_point(Chan chan, const T* __restrict__ w, int C, int y, int x, int n_act) {
    int off[9];
    bool in[9];
#pragma unroll
    for (int t = 0; t < 9; ++t) {
        const int yy = y + t / 3 - 1, xx = x + t % 3 - 1;
        in[t] = yy >= 0 && yy < n_act && xx >= 0 && xx < n_act;
        off[t] = min(max(yy, 0), n_act - 1) * n_act + min(max(xx, 0), n_act - 1);
    }
    T acc = 0;
    for (int c = 0; c < C; ++c) {
        const T* src = chan(c);
        T v[9];
#pragma unroll
        for (int t = 0; t < 9; ++t) v[t] = src[off[t]];
#pragma unroll
        for (int t = 0; t < 9; ++t) acc = fma(in[t] ? v[t] : (T)0, w[c * 9 + t], acc);
    }
    return acc;
}

template <typename T>
__global__ __launch_bounds__(256) void k_policy_conv_general(ConvIn<T> in, const T* __restrict__ wgt, const T* __restrict__ bias,
                                                             T* __restrict__ out, int n_act, int n_filt, T slope) {
    const int p = blockIdx.x * 256 + threadIdx.x, f = blockIdx.y, e = blockIdx.z;
    if (p >= in.img) return;
    const int y = p / n_act, x = p - y * n_act;
    const T acc = conv_point<T>([&](int c) { return conv_channel(in, c, e); }, wgt + (size_t)f * in.C * 9, in.C, y, x, n_act);
    const T v = acc + bias[f];
    out[((size_t)e * n_filt + f) * in.img + p] = v > (T)0 ? v : v * slope;
}

constexpr int kActionLanes = 1024;

template <typename T>
__global__ __launch_bounds__(kActionLanes) void k_policy_action(PolicyActionArgs<T> a) {
    extern __shared__ __attribute__((aligned(16))) char policy_smem[];
    const int A = a.n_valid_act, A4 = (A + 3) & ~3, Kp = a.proj_rank, Kn = a.n_filter;
    T* vs = reinterpret_cast<T*>(policy_smem);                     // [A4]: the clamped network output, then its projection
    T* zs = vs + A4;                                               // [A4]: z, then the filtered noise
    T* ts = zs + A4;                                               // [max(Kp, Kn)]
    const int e = blockIdx.x, tid = threadIdx.x;
    const int n_act = a.n_act, img = n_act * n_act, F = a.n_filt;
    const T* hid = a.hidden + (size_t)e * F * img;
    for (int p = tid; p < img; p += kActionLanes) {
        const int s = a.act_slot[p];
        if (s < 0) continue;
        const int y = p / n_act, x = p - y * n_act;
        const T acc = conv_point<T>([&](int c) { return hid + (size_t)c * img; }, a.w3, F, y, x, n_act);
        const T v = acc + a.b3;
        vs[s] = v < -a.clamp_abs ? -a.clamp_abs : (v > a.clamp_abs ? a.clamp_abs : v);
    }
    __syncthreads();
    if (Kp > 0) apply_factored_lds<T, kActionLanes>(a.proj_fr, a.proj_fl_t, vs, ts, A, Kp);
    const T sigma = a.sigma_env ? a.sigma_env[e] : a.sigma;        // (uniform over the workgroup)
    if (sigma != (T)0) {
        explore_draw_lds<T, kActionLanes>(zs, A, a.seed_lo, a.seed_hi, a.env_offset + (uint32_t)e, a.counter);
        if (Kn > 0) apply_factored_lds<T, kActionLanes>(a.fr, a.fl_t, zs, ts, A, Kn);
    }
    T* ac = a.action + (size_t)e * img;
    for (int p = tid; p < img; p += kActionLanes) {
#pragma clang fp contract(off)
        const int s = a.act_slot[p];
        T v = s >= 0 ? vs[s] : (T)0;
        if (s >= 0 && sigma != (T)0) v = v + sigma * zs[s];        // sigma == 0: the bits of the policy's output
        ac[p] = v;
    }
}

template <typename T>
__global__ __launch_bounds__(256) void k_policy_roll(T* past, const T* __restrict__ traj, int n_steps, int H, int n_env, int img) {
    const int p = blockIdx.x * 256 + threadIdx.x, e = blockIdx.y;
    if (p >= img) return;
    T* win = past + (size_t)e * (H - 1) * img + p;
    for (int c = 0; c < H - 1; ++c) {                              // row c + n_steps is read before iteration c + n_steps writes it
        const int slot = n_steps - (H - 1) + c;
        win[(size_t)c * img] = slot >= 0 ? traj[((size_t)slot * n_env + e) * img + p] : win[(size_t)(c + n_steps) * img];
    }
}

template <typename K>
int allow_lds(K kern, size_t lds, size_t* granted) {
    if (lds > 64 * 1024 && lds > *granted) {
        AO_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        *granted = lds;
    }
    return 0;
}

template <int NT>
int launch_conv_mfma_nt(const ConvIn<float>& in, const float* wt, const float* bias, float* out, int n_act, int n_filt, float slope,
                        int n_env, hipStream_t st) {
    int rows, bands;
    policy_bands(n_act, in.C, &rows, &bands);
    const size_t lds = policy_conv_lds(n_act, in.C);
    static size_t granted = 0;                                     // (per instantiation)
    AO_TRY(allow_lds(k_policy_conv_mfma<NT>, lds, &granted));
    hipLaunchKernelGGL(k_policy_conv_mfma<NT>, dim3(bands, n_env), dim3(256), lds, st, in, wt, bias, out, n_act, n_filt, rows,
                       policy_ksteps(in.C), slope);
    AO_HIP(hipGetLastError());
    return 0;
}

}  // namespace

int launch_policy_conv_mfma(const ConvIn<float>& in, const float* wt, const float* bias, float* out, int n_act, int n_filt,
                            float slope, int n_env, hipStream_t st) {
    if (n_filt % 16 != 0 || !policy_mfma_fits(n_act, in.C))
        return fail("policy convolution: %d filters, %d channels at %d x %d do not fit the MFMA kernel", n_filt, in.C, n_act, n_act);
    const int nt = n_filt / 16;
    if (nt % 4 == 0) return launch_conv_mfma_nt<4>(in, wt, bias, out, n_act, n_filt, slope, n_env, st);
    if (nt % 2 == 0) return launch_conv_mfma_nt<2>(in, wt, bias, out, n_act, n_filt, slope, n_env, st);
    return launch_conv_mfma_nt<1>(in, wt, bias, out, n_act, n_filt, slope, n_env, st);
}

template <typename T>
int launch_policy_conv_general(const ConvIn<T>& in, const T* w, const T* bias, T* out, int n_act, int n_filt, T slope, int n_env,
                               hipStream_t st) {
    if (n_env > 65535) return fail("policy convolution: %d envs in one shard, the general kernel takes 65535", n_env);
    hipLaunchKernelGGL(k_policy_conv_general<T>, dim3(cdiv(in.img, 256), n_filt, n_env), dim3(256), 0, st, in, w, bias, out, n_act,
                       n_filt, slope);
    AO_HIP(hipGetLastError());
    return 0;
}
template int launch_policy_conv_general<float>(const ConvIn<float>&, const float*, const float*, float*, int, int, float, int, hipStream_t);
template int launch_policy_conv_general<double>(const ConvIn<double>&, const double*, const double*, double*, int, int, double, int,
                                                hipStream_t);

template <typename T>
int launch_policy_action(const PolicyActionArgs<T>& a, int n_env, hipStream_t st) {
    const size_t lds = policy_action_lds(a.n_valid_act, a.proj_rank, a.n_filter, sizeof(T));
    if (lds > kPolicyLdsMax)
        return fail("policy action: %zu bytes of LDS for %d actuators and ranks %d / %d, %zu at the most", lds, a.n_valid_act, a.proj_rank,
                    a.n_filter, kPolicyLdsMax);
    static size_t granted = 0;                                     // (per instantiation)
    AO_TRY(allow_lds(k_policy_action<T>, lds, &granted));
    hipLaunchKernelGGL(k_policy_action<T>, dim3(n_env), dim3(kActionLanes), lds, st, a);
    AO_HIP(hipGetLastError());
    return 0;
}
template int launch_policy_action<float>(const PolicyActionArgs<float>&, int, hipStream_t);
template int launch_policy_action<double>(const PolicyActionArgs<double>&, int, hipStream_t);

template <typename T>
int launch_policy_roll(T* past, const T* traj, int n_steps, int H, int n_env, int img, hipStream_t st) {
    if (H <= 1 || n_steps <= 0) return 0;
    if (n_env > 65535) return fail("policy rollout: %d envs in one shard, the window roll takes 65535", n_env);
    hipLaunchKernelGGL(k_policy_roll<T>, dim3(cdiv(img, 256), n_env), dim3(256), 0, st, past, traj, n_steps, H, n_env, img);
    AO_HIP(hipGetLastError());
    return 0;
}
template int launch_policy_roll<float>(float*, const float*, int, int, int, int, hipStream_t);
template int launch_policy_roll<double>(double*, const double*, int, int, int, int, hipStream_t);

}  // namespace ao
