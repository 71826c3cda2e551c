// The residual toward an off-axis science target (offaxis.hpp): per env, the layers' screens warped by the wind as the phase
// kernels warp them, read at the target's footprint, blended bilinearly by the env's two fractions and summed; the mirror's
// surface is the one the sensor saw, taken over from the step's own outputs:
//     opd_atm_sci = sum_l blend_l(clip(warp(screen_l))[footprint_l(env)]) sqrt(fractionalR0_l) * lambda_atm / 2 pi
//     phase_sci   = phase + (opd_atm_sci - opd_atm) * 2 pi / lambda_src   inside the pupil, 0 outside
//                   (with a static difference map D = S_s - S_w, aoenv_set_static_opd: ((opd_atm_sci - opd_atm) + D) * 2 pi / lambda_src)
//     rms_nm      = std(phase_sci[pupil]) * lambda_src / 2 pi * 1e9,   strehl = exp(-var(phase_sci[pupil]))
// with `phase` = AOENV_B_PHASE and `opd_atm` the on-axis atmosphere OPD of the same step: the mirror product is not repeated and
// every kind of mirror is served.
//
// Launch shape: one workgroup of 64 x 16 lanes per env, which walks the pupil in tiles of 16 rows x up to 128 columns.  Per tile and
// layer the (rows + 3 + b) x (columns + 3 + b) apron of the torus screen is staged in LDS (b = 1 where the env blends), the
// Catmull-Rom warp runs as in the phase kernels -- horizontal pass, vertical pass, clip_to_range, the same 4-tap sums (oa_tap4) -- into the
// (rows + b) x (columns + b) patch, and a lane blends the four neighbours of its pixels and applies the layer weight last.  Where
// both fractions are zero the blend is skipped, as in the reference, and opd_atm_sci is then bit for bit the phase kernels' OPD.
// The pupil sums are float64: a lane adds its pixels in tile order, the wave is reduced by shuffles, the 16 waves are added in
// order by lane 0.  No atomics, nothing depends on n_env or on the env's place in the shard.
// The host has asserted (oa_plan_layer) that every tap of every patch lies inside the screen; the staging loads are bounds-checked
// all the same, as the phase kernels' are.
//
// k_guide_opd (aoenv_set_guide_direction) writes the same sum toward every env's GUIDE star into the atmosphere OPD buffer the phase
// kernels then read (update_atm = 0): opd_atm = sum_l blend_l(...) sqrt(fractionalR0_l) * lambda_atm / 2 pi for all R x R pixels.
// It needs no pupil sums, so nothing ties an env's tiles together: a workgroup of 64 x 16 lanes per (16-row x 64-column tile, env),
// one pixel per lane, (R / 16) (R / 64) E workgroups where k_science_residual has E.  Per (tile, layer) both kernels run ONE
// function, oa_layer_patch, and one accumulate, oa_add_pixel: for the same direction they give the same bits.
#include "phase_device.hpp"
#include "offaxis.hpp"

namespace ao {

constexpr int kOaTY = 16, kOaTX = 128;
constexpr int kOaMW = kOaTX + 8;                             // row stride of the staged apron (kOaTX + 4 used)
constexpr int kOaPW = kOaTX + 1;                             // ... of the horizontal pass and of the patch

// One 4-tap sum of the warp, ((w0 t0 + w1 t1) + w2 t2) + w3 t3 as the phase kernels state it.  float32: the compiler contracts that
// expression in k_phase_mfma, k_phase_mfma4 and stage A of the fused step kernel to fma(w3, t3, fma(w2, t2, fma(w0, t0, w1 t1)));
// here, between two LDS passes, it would pack the products and add them unfused, one rounding more per tap.  So the float32 form is
// written out: at zenith 0 the result is then bit for bit those kernels' (tests/test_gpu_offaxis.py holds it there).  float64 takes
// the plain expression, as k_phase<double> does.
template <typename T>
__device__ __forceinline__ T oa_tap4(T w0, T w1, T w2, T w3, T t0, T t1, T t2, T t3) {
    if constexpr (sizeof(T) == 4) {
#pragma clang fp contract(off)
        const float p = w1 * t1;
        return __builtin_fmaf(w3, t3, __builtin_fmaf(w2, t2, __builtin_fmaf(w0, t0, p)));
    } else {
        return ((w0 * t0 + w1 * t1) + w2 * t2) + w3 * t3;
    }
}

// One layer of one tile of TY = 16 rows x txe <= PW - 1 columns at (y0, x0) of env e, by a workgroup of 64 x 16 lanes (lx, ly): the
// (tye + 3 + b) x (txe + 3 + b) apron of the torus screen into mapt (row stride MW), the horizontal pass into ht and the vertical
// pass with the clip into the (tye + b) x (txe + b) patch pt (row stride PW); b = 1 where the env blends.  Opens with the barrier
// behind which the previous layer's patch is no longer read and closes with the one that completes the patch.  Returns the layer
// weight.  k_science_residual and k_guide_opd agree because they run this function.
template <typename T, int MW, int PW>
__device__ __forceinline__ T oa_layer_patch(const PhaseArgs& pa, const OaShift& sh, int b, int l, int e, int y0, int x0, int tye, int txe,
                                            int lx, int ly, T* mapt, T* ht, T* pt) {
    const LayerTaps& tp = layer_taps(pa, l, e);
    const int S = pa.S_l[l], foot = pa.foot_l[l];
    const T* map = static_cast<const T*>(pa.screen[l]) + (size_t)e * S * S;
    const int r0 = y0 + foot + sh.fy + tp.dy - 1, c0 = x0 + foot + sh.fx + tp.dx - 1;
    __syncthreads();                                          // the previous layer's patch is no longer read
    for (int r = ly; r < tye + 3 + b; r += 16) {
        const int rr = r0 + r;
        for (int c = lx; c < txe + 3 + b; c += 64) {
            const int cc = c0 + c;
            const bool ok = rr >= 0 && rr < S && cc >= 0 && cc < S;
            int pr = (ok ? rr : 0) + tp.oy, pc = (ok ? cc : 0) + tp.ox;   // torus: physical = (logical + origin) mod S
            pr = pr >= S ? pr - S : pr;
            pc = pc >= S ? pc - S : pc;
            const T v = map[(size_t)pr * S + pc];
            mapt[r * MW + c] = ok ? v : (T)0;
        }
    }
    __syncthreads();
    const T wx0 = (T)tp.wx[0], wx1 = (T)tp.wx[1], wx2 = (T)tp.wx[2], wx3 = (T)tp.wx[3];
    for (int r = ly; r < tye + 3 + b; r += 16) {
        const T* m = mapt + r * MW;
        for (int x = lx; x < txe + b; x += 64)
            ht[r * PW + x] = oa_tap4<T>(wx0, wx1, wx2, wx3, m[x], m[x + 1], m[x + 2], m[x + 3]);
    }
    __syncthreads();
    const T wy0 = (T)tp.wy[0], wy1 = (T)tp.wy[1], wy2 = (T)tp.wy[2], wy3 = (T)tp.wy[3];
    const T* mm = static_cast<const T*>(pa.minmax[l]) + 2 * e;
    const T lo = mm[0], hi = mm[1];
    const bool zero_outside = (lo > (T)0 || hi < (T)0);
    for (int y = ly; y < tye + b; y += 16) {
        for (int x = lx; x < txe + b; x += 64) {
            const T* h = ht + y * PW + x;
            const T v = oa_tap4<T>(wy0, wy1, wy2, wy3, h[0], h[PW], h[2 * PW], h[3 * PW]);
            pt[y * PW + x] = clip_to_range(v, lo, hi, zero_outside);
        }
    }
    __syncthreads();
    return (T)tp.weight;
}

// ... and a lane's pixel of that patch: the four neighbours blended (oa_blend), or the first alone where the env does not blend, the
// layer weight last
template <typename T, int PW>
__device__ __forceinline__ void oa_add_pixel(T& sup, const T* p, bool blend, T ty, T tx, T wl) {
    const T v = blend ? oa_blend<T>(p[0], p[1], p[PW], p[PW + 1], ty, tx) : p[0];
    sup += v * wl;
}

template <typename T>
__global__ void __launch_bounds__(1024) k_science_residual(const OaArgs<T> a) {
    __shared__ T mapt[(kOaTY + 4) * kOaMW];
    __shared__ T ht[(kOaTY + 4) * kOaPW];
    __shared__ T pt[(kOaTY + 1) * kOaPW];
    __shared__ double red[2][16];

    const int R = a.R, e = blockIdx.x;
    const int lx = threadIdx.x, ly = threadIdx.y;
    const size_t pix0 = (size_t)e * R * R;
    double s_phi = 0.0, q_phi = 0.0;

    for (int y0 = 0; y0 < R; y0 += kOaTY) {
        const int tye = min(kOaTY, R - y0);
        for (int x0 = 0; x0 < R; x0 += kOaTX) {
            const int txe = min(kOaTX, R - x0);
            T sup[2] = {(T)0, (T)0};
            for (int l = 0; l < a.pa.n_layer; ++l) {
                const OaShift sh = a.dir[(size_t)l * a.pa.n_env + e];
                const bool blend = oa_blends(sh.ty, sh.tx);  // (the same for the whole workgroup)
                const T wl = oa_layer_patch<T, kOaMW, kOaPW>(a.pa, sh, blend ? 1 : 0, l, e, y0, x0, tye, txe, lx, ly, mapt, ht, pt);
                if (ly < tye) {
                    const T ty = (T)sh.ty, tx = (T)sh.tx;
#pragma unroll
                    for (int i = 0; i < 2; ++i) {
                        const int x = lx + 64 * i;
                        if (x < txe) oa_add_pixel<T, kOaPW>(sup[i], pt + ly * kOaPW + x, blend, ty, tx, wl);
                    }
                }
            }
            if (ly < tye) {
#pragma unroll
                for (int i = 0; i < 2; ++i) {
                    const int x = lx + 64 * i;
                    if (x < txe) {
                        const size_t q = (size_t)(y0 + ly) * R + (x0 + x);
                        const T atm_sci = sup[i] * a.atm_scale;
                        if (a.opd_atm_sci) a.opd_atm_sci[pix0 + q] = atm_sci;
                        const bool in = a.pupil[q] != 0;
                        T phi = (T)0;
                        if (in) {                             // (a static difference map is one more term of the bracket)
                            T d = atm_sci - a.opd_atm[pix0 + q];
                            if (a.delta) d += a.delta[(size_t)e * a.delta_env + q];
                            phi = a.phase[pix0 + q] + d * a.src_scale;
                        }
                        if (a.phase_sci) a.phase_sci[pix0 + q] = phi;
                        if (in) {
                            const double d = (double)phi;
                            s_phi += d;
                            q_phi += d * d;
                        }
                    }
                }
            }
        }
    }
    s_phi = wave_sum_f64(s_phi);
    q_phi = wave_sum_f64(q_phi);
    if (lx == 0) {
        red[0][ly] = s_phi;
        red[1][ly] = q_phi;
    }
    __syncthreads();
    if (lx == 0 && ly == 0) {
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

template <typename T>
int launch_science_residual(const OaArgs<T>& a, hipStream_t st) {
    if (a.pa.n_env < 1 || a.R < 1) return 0;
    hipLaunchKernelGGL(k_science_residual<T>, dim3(a.pa.n_env), dim3(64, 16), 0, st, a);
    AO_HIP(hipGetLastError());
    return 0;
}
template int launch_science_residual<float>(const OaArgs<float>&, hipStream_t);
template int launch_science_residual<double>(const OaArgs<double>&, hipStream_t);

// ---- the guide star's line of sight ----------------------------------------------------------------------------------------------
constexpr int kGdTY = 16, kGdTX = 64;                        // one pixel per lane
constexpr int kGdMW = kGdTX + 8, kGdPW = kGdTX + 1;

template <typename T>
__global__ void __launch_bounds__(1024) k_guide_opd(const GuideArgs<T> a, int tiles_x, int tiles) {
    __shared__ T mapt[(kGdTY + 4) * kGdMW];
    __shared__ T ht[(kGdTY + 4) * kGdPW];
    __shared__ T pt[(kGdTY + 1) * kGdPW];

    const int R = a.R, e = blockIdx.x / tiles, tile = blockIdx.x - e * tiles;
    const int y0 = (tile / tiles_x) * kGdTY, x0 = (tile % tiles_x) * kGdTX;
    const int lx = threadIdx.x, ly = threadIdx.y;
    const int tye = min(kGdTY, R - y0), txe = min(kGdTX, R - x0);
    const bool mine = ly < tye && lx < txe;
    T sup = (T)0;
    for (int l = 0; l < a.pa.n_layer; ++l) {
        const OaShift sh = a.dir[(size_t)l * a.pa.n_env + e];
        const bool blend = oa_blends(sh.ty, sh.tx);          // (the same for the whole workgroup)
        const T wl = oa_layer_patch<T, kGdMW, kGdPW>(a.pa, sh, blend ? 1 : 0, l, e, y0, x0, tye, txe, lx, ly, mapt, ht, pt);
        if (mine) oa_add_pixel<T, kGdPW>(sup, pt + ly * kGdPW + lx, blend, (T)sh.ty, (T)sh.tx, wl);
    }
    if (mine) a.opd_atm[(size_t)e * R * R + (size_t)(y0 + ly) * R + (x0 + lx)] = sup * a.atm_scale;
}

template <typename T>
int launch_guide_opd(const GuideArgs<T>& a, hipStream_t st) {
    if (a.pa.n_env < 1 || a.R < 1) return 0;
    const int tiles_x = (a.R + kGdTX - 1) / kGdTX, tiles = tiles_x * ((a.R + kGdTY - 1) / kGdTY);
    hipLaunchKernelGGL(k_guide_opd<T>, dim3((unsigned)a.pa.n_env * tiles), dim3(64, 16), 0, st, a, tiles_x, tiles);
    AO_HIP(hipGetLastError());
    return 0;
}
template int launch_guide_opd<float>(const GuideArgs<float>&, hipStream_t);
template int launch_guide_opd<double>(const GuideArgs<double>&, hipStream_t);

}  // namespace ao
