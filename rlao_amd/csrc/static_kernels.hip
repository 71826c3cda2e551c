// Static aberrations per env (static_opd.hpp): the kernels.
//
// k_dm_static_mfma (float32): the surface of a separable mirror with the sensor arm's map,
//     out_e[y][x] = S_w[e][y][x] + sum_k (Gy_e C_e)[y][k] gx_e[x][k],   k over the n_act actuator columns,
//   one wave per workgroup and per 32 x 32 patch, grid (ceil(R / 32), ceil(R / 32), E), the shape of k_dm_pairs_mfma: 2 x 2 tiles of
//   v_mfma_f32_16x16x4_f32, four independent accumulators, the product formed TRANSPOSED (A operand: gx rows, B operand: Gy C rows)
//   so that a lane owns out[y][x0 .. x0 + 3].  Gy C comes from k_dm_rows in the operand layout (ga_index()) the phase kernels read
//   it in, gx is the table gxa as it is: each of the 4 operand loads per 16 MFMAs is one coalesced 16-byte-per-lane access, and
//   because rows R .. R pad 128 and actuators n_act .. 4 ga_stride of both tables are zero no load is guarded.  The accumulators are
//   INITIALISED from the map's tile: the map costs one load and no add, and the sum is the fma chain
//   fma(a_k, b_k, ... fma(a_0, b_0, S_w)) in ascending k.  The k order depends on ga_stride = f(n_act) alone: an env has the same
//   bits in any shard and at any place in it.  Stores: float4 per lane where R % 4 == 0, dwords otherwise (so are the map's loads).
// k_dm_static<T> (float64 shards; float32 under AOENV_PATH_DM_STATIC_GENERAL or above 128 actuators across): one lane per pixel,
//   64 x 4 pixels per workgroup; the 4 rows of Gy C the workgroup needs are formed in LDS from the command image first, then a
//   lane adds its n_act products to the map's pixel by fma in ascending k.
// k_static_add<T>: out = base + S_w for a shard whose mirror surface is formed ahead anyway (actuator pairs, a dense mirror); the
//   mirror's own buffer stays the mirror alone.
// k_science_static<T>: phase_sci = phase + D 2 pi / lambda_src inside the pupil, 0 outside, and the pupil sums of the result in
//   float64: one workgroup of 1024 lanes per env, a lane adds its pixels in ascending index, the wave is reduced by shuffles, the 16
//   waves are added in order by lane 0 (as k_science_residual does).  No layer is touched.
#include "common.hpp"
#include "static_opd.hpp"

namespace ao {

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

__global__ __launch_bounds__(64) void k_dm_static_mfma(StaticDmArgs<float> a) {
    const int lane = threadIdx.x, lc = lane & 15, lq = lane >> 4;
    const int e = blockIdx.z, tx0 = 2 * blockIdx.x, ty0 = 2 * blockIdx.y;
    const int R = a.R, nq = a.ga_stride >> 2;
    const size_t rows_env = (size_t)(((R + 127) >> 7) * 128) * 4 * a.ga_stride;   // floats of one env's Gy C (k_dm_rows)
    const float4* gxa = reinterpret_cast<const float4*>(a.gxa + (size_t)e * a.ga_env) + lane;
    const float4* s1a = reinterpret_cast<const float4*>(a.s1a + (size_t)e * rows_env) + lane;
    const float4* x0p = gxa + (size_t)tx0 * nq * 64;
    const float4* x1p = x0p + (size_t)nq * 64;
    const float4* y0p = s1a + (size_t)ty0 * nq * 64;
    const float4* y1p = y0p + (size_t)nq * 64;
    const float* map = a.map + (size_t)e * a.map_env;
    const bool vec = (R & 3) == 0;
    // D[i][j]: i = the A operand's row = x within the tile, j = the B operand's column = y; lane (lc, lq) holds j = lc, i = 4 lq + reg
    auto tile = [&](int ty, int tx) {
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        const int y = 16 * ty + lc, x = 16 * tx + 4 * lq;
        if (y >= R || x >= R) return v;
        const float* p = map + (size_t)y * R + x;
        if (vec) {
            const float4 t = *reinterpret_cast<const float4*>(p);
            v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
        } else {
            v[0] = p[0];
            if (x + 1 < R) v[1] = p[1];
            if (x + 2 < R) v[2] = p[2];
            if (x + 3 < R) v[3] = p[3];
        }
        return v;
    };
    f32x4 acc00 = tile(ty0, tx0), acc01 = tile(ty0, tx0 + 1), acc10 = tile(ty0 + 1, tx0), acc11 = tile(ty0 + 1, tx0 + 1);   // acc<y tile><x tile>
    for (int s = 0; s < nq; ++s) {
        const size_t o = (size_t)s * 64;
        const float4 x0 = x0p[o], x1 = x1p[o], y0 = y0p[o], y1 = y1p[o];
#define AO_STATIC_STEP(m)                                                               \
    acc00 = __builtin_amdgcn_mfma_f32_16x16x4f32(x0.m, y0.m, acc00, 0, 0, 0);           \
    acc01 = __builtin_amdgcn_mfma_f32_16x16x4f32(x1.m, y0.m, acc01, 0, 0, 0);           \
    acc10 = __builtin_amdgcn_mfma_f32_16x16x4f32(x0.m, y1.m, acc10, 0, 0, 0);           \
    acc11 = __builtin_amdgcn_mfma_f32_16x16x4f32(x1.m, y1.m, acc11, 0, 0, 0)
        AO_STATIC_STEP(x);
        AO_STATIC_STEP(y);
        AO_STATIC_STEP(z);
        AO_STATIC_STEP(w);
#undef AO_STATIC_STEP
    }
    float* out = a.out + (size_t)e * R * R;
    auto store = [&](const f32x4& v, int ty, int tx) {
        const int y = 16 * ty + lc, x = 16 * tx + 4 * lq;
        if (y >= R || x >= R) return;
        float* p = out + (size_t)y * R + x;
        if (vec) {
            *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
        } else {
            p[0] = v[0];
            if (x + 1 < R) p[1] = v[1];
            if (x + 2 < R) p[2] = v[2];
            if (x + 3 < R) p[3] = v[3];
        }
    };
    store(acc00, ty0, tx0);
    store(acc01, ty0, tx0 + 1);
    store(acc10, ty0 + 1, tx0);
    store(acc11, ty0 + 1, tx0 + 1);
}

template <typename T>
__global__ __launch_bounds__(256) void k_dm_static(StaticDmArgs<T> a) {
    extern __shared__ __align__(16) unsigned char lds_raw[];
    T* s1 = reinterpret_cast<T*>(lds_raw);                         // [4][n_act]: (Gy C)[y0 + r][ix]
    const int e = blockIdx.z, R = a.R, nA = a.n_act;
    const int lx = threadIdx.x, ly = threadIdx.y, tid = ly * 64 + lx;
    const int x = blockIdx.x * 64 + lx, y0 = blockIdx.y * 4, y = y0 + ly;
    const T* ci = a.coefs_img + (size_t)e * nA * nA;
    const T* gy = a.gy + (size_t)e * a.g_env;
    for (int i = tid; i < 4 * nA; i += 256) {
        const int r = i / nA, ix = i - r * nA;
        T acc = (T)0;
        if (y0 + r < R) {
            const T* g = gy + (size_t)(y0 + r) * nA;
            for (int iy = 0; iy < nA; ++iy) acc = fma(g[iy], ci[(size_t)iy * nA + ix], acc);
        }
        s1[i] = acc;
    }
    __syncthreads();
    if (x >= R || y >= R) return;
    const size_t q = (size_t)y * R + x;
    const T* gx = a.gx + (size_t)e * a.g_env + (size_t)x * nA;
    const T* sr = s1 + ly * nA;
    T acc = a.map[(size_t)e * a.map_env + q];
    for (int ix = 0; ix < nA; ++ix) acc = fma(sr[ix], gx[ix], acc);
    a.out[(size_t)e * R * R + q] = acc;
}

template <typename T>
__global__ __launch_bounds__(256) void k_static_add(StaticDmArgs<T> a) {
    const size_t r2 = (size_t)a.R * a.R, q = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (q >= r2) return;
    const size_t e = blockIdx.y;
    a.out[e * r2 + q] = a.base[e * r2 + q] + a.map[e * a.map_env + q];
}

template <typename T>
__global__ __launch_bounds__(1024) void k_science_static(SciStaticArgs<T> a) {
    __shared__ double red[2][16];
    const int e = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r2 = a.R * a.R;
    const size_t pix0 = (size_t)e * r2;
    const T* delta = a.delta + (size_t)e * a.delta_env;
    double s_phi = 0.0, q_phi = 0.0;
    for (int q = tid; q < r2; q += 1024) {
        const bool in = a.pupil[q] != 0;
        const T phi = in ? a.phase[pix0 + q] + delta[q] * a.src_scale : (T)0;
        if (a.phase_sci) a.phase_sci[pix0 + q] = phi;
        if (in) {
            const double d = (double)phi;
            s_phi += d;
            q_phi += d * d;
        }
    }
    s_phi = wave_sum_f64(s_phi);
    q_phi = wave_sum_f64(q_phi);
    if (lane == 0) {
        red[0][wave] = s_phi;
        red[1][wave] = q_phi;
    }
    __syncthreads();
    if (tid == 0) {
        double s = red[0][0], q = red[1][0];
        for (int w = 1; w < 16; ++w) {
            s += red[0][w];
            q += red[1][w];
        }
        const double n = (double)a.n_pupil;
        double var = q / n - (s / n) * (s / n);
        var = var > 0 ? var : 0;
        if (a.rms_nm) a.rms_nm[e] = (T)(sqrt(var) / a.src_scale_d * 1e9);
        if (a.strehl) a.strehl[e] = (T)exp(-var);
    }
}

}  // namespace

int launch_dm_static_mfma(const StaticDmArgs<float>& a, int n_env, hipStream_t st) {
    if (a.R < 1 || a.n_act < 1 || n_env < 1) return fail("static surface: R = %d, %d actuators across, %d envs", a.R, a.n_act, n_env);
    // what the kernel's unguarded loads rely on: both operand tables cover every tile of the grid and every k step
    if (a.ga_stride < 8 || (a.ga_stride & 3) || 4 * a.ga_stride < a.n_act || !a.s1a || !a.gxa || !a.map || !a.out)
        return fail("static surface: operand tables of stride %d do not fit %d actuators across", a.ga_stride, a.n_act);
    const int t = cdiv(a.R, 32);
    hipLaunchKernelGGL(k_dm_static_mfma, dim3(t, t, n_env), dim3(64), 0, st, a);
    AO_HIP(hipGetLastError());
    return 0;
}

template <typename T>
int launch_dm_static(const StaticDmArgs<T>& a, int n_env, hipStream_t st) {
    if (a.R < 1 || a.n_act < 1 || n_env < 1) return fail("static surface: R = %d, %d actuators across, %d envs", a.R, a.n_act, n_env);
    const size_t lds = (size_t)4 * a.n_act * sizeof(T);
    if (lds > 64 * 1024) return fail("static surface: %d actuators across need %zu B of LDS", a.n_act, lds);
    hipLaunchKernelGGL(k_dm_static<T>, dim3(cdiv(a.R, 64), cdiv(a.R, 4), n_env), dim3(64, 4), lds, st, a);
    AO_HIP(hipGetLastError());
    return 0;
}
template int launch_dm_static<float>(const StaticDmArgs<float>&, int, hipStream_t);
template int launch_dm_static<double>(const StaticDmArgs<double>&, int, hipStream_t);

template <typename T>
int launch_static_add(const StaticDmArgs<T>& a, int n_env, hipStream_t st) {
    if (a.R < 1 || n_env < 1) return 0;
    hipLaunchKernelGGL(k_static_add<T>, dim3(cdiv(a.R * a.R, 256), n_env), dim3(256), 0, st, a);
    AO_HIP(hipGetLastError());
    return 0;
}
template int launch_static_add<float>(const StaticDmArgs<float>&, int, hipStream_t);
template int launch_static_add<double>(const StaticDmArgs<double>&, int, hipStream_t);

template <typename T>
int launch_science_static(const SciStaticArgs<T>& a, int n_env, hipStream_t st) {
    if (n_env < 1 || a.R < 1) return 0;
    hipLaunchKernelGGL(k_science_static<T>, dim3(n_env), dim3(1024), 0, st, a);
    AO_HIP(hipGetLastError());
    return 0;
}
template int launch_science_static<float>(const SciStaticArgs<float>&, int, hipStream_t);
template int launch_science_static<double>(const SciStaticArgs<double>&, int, hipStream_t);

}  // namespace ao
