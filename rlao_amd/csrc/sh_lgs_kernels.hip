// Laser-guide-star Shack-Hartmann spots (sh_lgs.hpp): the diffractive spots of k_sh_spots, kept UNBINNED, then every lenslet's own
// tap sum into its p x p camera pixels.
//   OOPAO/ShackHartmann.py:539      I = |FFT2(E) / n|^2                                    (n = 2p)
//   OOPAO/ShackHartmann.py:554-556  I = fftshift(abs(ifft2(fft2(I) * C)))                  (C: get_convolution_spot, :396-503)
//   OOPAO/ShackHartmann.py:565      2 x 2 sum-binning to p x p
#include "common.hpp"
#include "sh_device.hpp"
#include "sh_lgs.hpp"

namespace ao {

// lane j's value of v for every lane, j wave-uniform (v_readlane: no LDS round trip)
__device__ inline float lane_value(float v, int j) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), j)); }
__device__ inline double lane_value(double v, int j) {
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), j), __builtin_amdgcn_readlane(__double2loint(v), j));
}

// acc + w a in ONE rounding, spelled out: left to contraction the compiler may pair the products of neighbouring taps into packed
// multiplies and add afterwards, and a tap's rounding would then depend on where in its lot of 64 it stands -- on the box
__device__ inline float tap_fma(float w, float a, float acc) { return __builtin_fmaf(w, a, acc); }
__device__ inline double tap_fma(double w, double a, double acc) { return __builtin_fma(w, a, acc); }

// One wavefront per valid lenslet, L = blockDim.x / 64 lenslets per workgroup (4, or fewer where the LDS image asks for it:
// lgs_lenslets_per_group); grid = (ceil(nValid / L), n_env).  Stages 0-2 are k_sh_spots' (the same sums in the same order: the
// unbinned |F / n|^2 is what that kernel bins), with every one of the n x n spectral samples kept in LDS.  They are stored split by
// the parity of their two indices, four blocks, and each p x p block is laid out twice along both axes (n x n elements a block)
//     Iu[(u & 1) * 2 + (v & 1)][(u >> 1) + {0, p}][(v >> 1) + {0, p}]
// because one tap (x, y) pairs camera pixel (P, Q) with sample ((2P + n/2 - x) mod n, (2Q + n/2 - y) mod n): with cx = (n/2 - x) mod n
// that is the block of parity (cx & 1, cy & 1) at ((P + (cx >> 1)) mod p, (Q + (cy >> 1)) mod p), and in the doubled block the wrap
// needs no arithmetic: the lane reads element  off(x, y) + P n + Q,  off = block n^2 + (cx >> 1) n + (cy >> 1)  wave-uniform.  The
// lanes of one read are p runs of p consecutive elements, n apart (the plain [n][n] layout would put the lanes two elements apart,
// all on even banks).  Tap and offset are wave-uniform (the wave's lenslet, the env of the workgroup): the wave fetches 64 taps at
// once, one per lane in the order they are summed, each lane forms its tap's offset, and both go round by readlane -- per tap the
// inner loop is two readlanes, one add, one LDS read and one fma.  The table is read-mostly and stays in L2.
// Barriers are workgroup-wide and unconditional: a wave without a lenslet (nValid not a multiple of L) runs no loop body.
template <typename T>
__global__ void __launch_bounds__(256) k_sh_spots_lgs(const T* __restrict__ phase, const ShConst<T> sc, const T* __restrict__ amp_env,
                                                      const T* __restrict__ taps, size_t tap_env, const LgsRanges rx, const LgsRanges ry,
                                                      T* __restrict__ frame, T* __restrict__ wfs_max, int R, int n_subap, int n_valid) {
    extern __shared__ __align__(16) unsigned char lds_raw[];
    const int p = R / n_subap, n = 2 * p, lo = n / 2 - p / 2, pp = p * p;
    const int L = blockDim.x / kWave;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave), lane = threadIdx.x & (kWave - 1);
    cplx<T>* tw = reinterpret_cast<cplx<T>*>(lds_raw);                       // [n]
    cplx<T>* Et = tw + n + wave * (pp + p * n);                               // [p][p]
    cplx<T>* G = Et + pp;                                                     // [p][n]
    T* Iu = reinterpret_cast<T*>(tw + n + L * (pp + p * n)) + wave * (4 * n * n); // [2][2][n][n]: every p x p block twice along each axis
    for (int k = threadIdx.x; k < n; k += blockDim.x) tw[k] = {sc.tw[2 * k], sc.tw[2 * k + 1]};
    __syncthreads();

    const int s = blockIdx.x * L + wave;
    const int e = blockIdx.y;
    const bool active = s < n_valid;          // no early return: the barriers below are workgroup-wide
    const int k = active ? sc.subap_idx[s] : 0, i = k / n_subap, j = k % n_subap;
    const T* ph = phase + (size_t)e * R * R;
    const T star = amp_env ? amp_env[e] : (T)1;               // the env's own guide star: workgroup-uniform, null = the shard's

    for (int idx = lane; active && idx < pp; idx += kWave) {
        const int a = idx / p, b = idx % p;
        const int pix = (i * p + b) * R + (j * p + a);
        T sn, cs;
        sincos_t<T>(ph[pix], &sn, &cs);
        T am = sc.amp[pix];
        if (amp_env) am = am * star;
        const T pr = sc.ph[2 * a] * sc.ph[2 * b] - sc.ph[2 * a + 1] * sc.ph[2 * b + 1];
        const T pi = sc.ph[2 * a] * sc.ph[2 * b + 1] + sc.ph[2 * a + 1] * sc.ph[2 * b];
        const T er = am * cs, ei = am * sn;
        Et[idx] = {er * pr - ei * pi, er * pi + ei * pr};
    }
    __syncthreads();

    for (int idx = lane; active && idx < p * n; idx += kWave) {
        const int a = idx / n, v = idx % n;
        T gr = 0, gi = 0;
        int t = (lo * v) % n;
        for (int b = 0; b < p; ++b) {
            const cplx<T> x = Et[a * p + b], w = tw[t];
            gr += x.re * w.re - x.im * w.im;
            gi += x.re * w.im + x.im * w.re;
            t += v;
            t = t >= n ? t - n : t;
        }
        G[idx] = {gr, gi};
    }
    __syncthreads();

    // every spectral sample |F[u][v] / n|^2, as the reference normalises the field before squaring
    for (int idx = lane; active && idx < n * n; idx += kWave) {
        const int u = idx / n, v = idx % n;
        T fr_ = 0, fi_ = 0;
        int t = (lo * u) % n;
        for (int a = 0; a < p; ++a) {
            const cplx<T> g = G[a * n + v], w = tw[t];
            fr_ += g.re * w.re - g.im * w.im;
            fi_ += g.re * w.im + g.im * w.re;
            t += u;
            t = t >= n ? t - n : t;
        }
        const T ar = fr_ / (T)n, ai = fi_ / (T)n;
        const T val = ar * ar + ai * ai;
        T* blk = Iu + ((u & 1) * 2 + (v & 1)) * (n * n) + (u >> 1) * n + (v >> 1);
        blk[0] = val;
        blk[p] = val;
        blk[p * n] = val;
        blk[p * n + p] = val;
    }
    __syncthreads();

    // the lenslet's taps over the box, in ascending (x, y) (sh_lgs.hpp): tap b of nxb nyb is (xs(b / nyb), ys(b % nyb)), the two
    // pieces of a wrapped interval in ascending order
    const T* tp = taps + (size_t)e * tap_env + (size_t)(active ? s : 0) * n * n;
    const int nx0 = rx.hi[0] - rx.lo[0], nxb = nx0 + rx.hi[1] - rx.lo[1];
    const int ny0 = ry.hi[0] - ry.lo[0], nyb = ny0 + ry.hi[1] - ry.lo[1];
    const int nb = active ? nxb * nyb : 0;                      // (wave-uniform: a wave without a lenslet walks no tap)
    T mx = 0;
    T* fr = frame + (size_t)e * R * R;
    for (int i0 = 0; i0 < pp; i0 += kWave) {                    // camera pixels, 64 at a time (one pass up to p = 8)
        const int idx = i0 + lane;
        const bool px = idx < pp;
        const int P = px ? idx / p : 0, Q = px ? idx - (idx / p) * p : 0;
        const T* mine_px = Iu + P * n + Q;
        T acc = 0;
        for (int b0 = 0; b0 < nb; b0 += kWave) {
            T mine = 0;
            int off = 0;
            if (b0 + lane < nb) {
                const int bx = (b0 + lane) / nyb, by = (b0 + lane) - bx * nyb;
                const int x = bx < nx0 ? rx.lo[0] + bx : rx.lo[1] + bx - nx0, y = by < ny0 ? ry.lo[0] + by : ry.lo[1] + by - ny0;
                const int cx = x <= p ? p - x : p - x + n, cy = y <= p ? p - y : p - y + n;
                mine = tp[x * n + y];
                off = ((cx & 1) * 2 + (cy & 1)) * (n * n) + (cx >> 1) * n + (cy >> 1);
            }
            const int lot = min(kWave, nb - b0);
            int t = 0;
            for (; t + 4 <= lot; t += 4) {                          // four LDS reads in flight; the fmas stay in tap order
                const T a0 = mine_px[__builtin_amdgcn_readlane(off, t)], a1 = mine_px[__builtin_amdgcn_readlane(off, t + 1)];
                const T a2 = mine_px[__builtin_amdgcn_readlane(off, t + 2)], a3 = mine_px[__builtin_amdgcn_readlane(off, t + 3)];
                acc = tap_fma(lane_value(mine, t), a0, acc);
                acc = tap_fma(lane_value(mine, t + 1), a1, acc);
                acc = tap_fma(lane_value(mine, t + 2), a2, acc);
                acc = tap_fma(lane_value(mine, t + 3), a3, acc);
            }
            for (; t < lot; ++t) acc = tap_fma(lane_value(mine, t), mine_px[__builtin_amdgcn_readlane(off, t)], acc);
        }
        if (px && active) {
            fr[(i * p + P) * R + (j * p + Q)] = acc;
            mx = acc > mx ? acc : mx;
        }
    }
    for (int off = 32; off > 0; off >>= 1) {
        const T o = __shfl_down(mx, off);
        mx = o > mx ? o : mx;
    }
    if (active && lane == 0) atomic_max_nonneg(&wfs_max[e], mx);
}

template <typename T>
int launch_sh_spots_lgs(const T* phase, const ShConst<T>& sc, const T* amp_env, const T* taps, size_t tap_env, const int32_t* box,
                        T* frame, T* wfs_max, int n_env, int R, int n_subap, int n_valid, hipStream_t st) {
    const int p = R / n_subap, n = 2 * p;
    const int L = lgs_lenslets_per_group(p, sizeof(T));
    if (L == 0) return fail("sh_spots_lgs: %d px per lenslet needs %zu B of LDS for one lenslet", p, lgs_lds_bytes(p, 1, sizeof(T)));
    const LgsRanges rx = lgs_ranges(box[0], box[2], n), ry = lgs_ranges(box[1], box[3], n);
    hipLaunchKernelGGL(k_sh_spots_lgs<T>, dim3(cdiv(n_valid, L), n_env), dim3(kWave * L), lgs_lds_bytes(p, L, sizeof(T)), st, phase, sc,
                       amp_env, taps, tap_env, rx, ry, frame, wfs_max, R, n_subap, n_valid);
    AO_HIP(hipGetLastError());
    return 0;
}

#define INST(T)                                                                                                               \
    template int launch_sh_spots_lgs<T>(const T*, const ShConst<T>&, const T*, const T*, size_t, const int32_t*, T*, T*, int, int, int, \
                                        int, hipStream_t);
INST(float)
INST(double)
#undef INST

}  // namespace ao
