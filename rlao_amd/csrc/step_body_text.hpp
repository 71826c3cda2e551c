// The body of the fused step kernel as TEXT (step_kernel_body.hpp includes it: once in k_env_step_sh6, twice in k_env_step_pair_sh6).
// No include guard.  The including kernel has the by-value arguments `a`, `L`, `star` in scope and defines STEP_BODY_SUB:
//   0  a launch of one step: the text below is then, token for token, the kernel it always was
//   1  the first step of a pair: it is never a call's last, so it stores neither phase nor frame nor atmosphere.  It ends behind
//      its centre of gravity: the slopes go to the pair's own LDS (StepLds::pair), the lane's next command to carry_cn -- it
//      depends on the observation of the step BEFORE this one, not on this step's -- and its reconstruction is left to the second
//      copy.  On its last barriers it builds the second step's Gy C in s1, which is that step's prologue.
//   2  the second step of a pair, in a scope of its own behind a workgroup barrier (which also means "s1 complete"): a step in
//      which no layer crosses a pixel -- no ring, no gather, no range scan (lohi[] of the first stands in LDS), no prologue barrier,
//      taps from StepArgs::taps2, telemetry index and frame counter plus one, the command from carry_cn.  Its stage C reconstructs
//      both steps with one fetch of the rows of M and M2C^T, and stores coefs, dm_prev, obs, reward and the return once:
//      nothing the launch wrote to global memory is read back.  `a`, `L`, `star`, tid2, e2 are the scope's opaque copies.
// A function would have to be handed the kernel's by-value arguments by reference; the instantiations at the 128-register ceiling
// then spill, and the compiler's contraction choices move.
    constexpr bool STAR = SPEC == STEP_STAR;
    constexpr bool GEN = SPEC == STEP_GENERAL || STAR;
    constexpr bool CAM_PHOTON_ONLY = SPEC == STEP_PHOTON;
    using namespace fstep;
    using fast6::EST;
    extern __shared__ __align__(16) unsigned char lds_raw[];
    float* lds = reinterpret_cast<float*>(lds_raw);
    const KArgs<float>& k = a.k;
    const int R = k.R, nA = k.n_act, S = k.pa.S;
    const int nAp = (nA + 3) & ~3, SS = nAp + 1;
#if STEP_BODY_SUB != 2
    float* cimg = lds + L.cimg;                                  // [nA][nA] command image
#endif
    float* s1 = lds + L.s1;                                      // [2 PR][SS]  Gy C, every row
#if STEP_BODY_SUB != 2
    const int w_ = threadIdx.x >> 6;
#else
    const int w_ = tid2 >> 6;
#endif
    float* mapt = lds + L.mapt + w_ * (WR * WC);                   // [WR][WC] this wave's private layer tile
    short* slot_s = reinterpret_cast<short*>(lds + L.slot);      // [nSub^2] lenslet -> compact valid index or -1
    cplx<float>* E0 = reinterpret_cast<cplx<float>*>(lds + L.e0);    // [nValid][EST]
#if STEP_BODY_SUB != 1
    float* sl = lds + L.sl;                                      // [2 nValid] slopes            (aliases E0: behind the threshold barrier)
    float* img_s = lds + L.img;                                  // [nA^2 + n_modes]             (aliases E0: stage C)
#else
    float* sl = lds + L.pair;                                    // [2 nValid] (the pair's own words: E0 is the second step's before they are read)
#endif
    const uint32_t* tab_s = reinterpret_cast<const uint32_t*>(lds + L.tab);   // camera: alias tables (alias cimg, s1, the layer tiles: stage B)
#if STEP_BODY_SUB != 2
    __shared__ double red[4][16];
    __shared__ double red_tail[16];
    __shared__ float red_mx[16];

    const int e = blockIdx.x;
    const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
#else
    const int e = e2;
    const int tid = tid2, w = tid >> 6, lane = tid & 63;
#endif
    const int lc = lane & 15, lq = lane >> 4;                    // MFMA lane decomposition
    const int band = w >> 2, cg = w & 3;                         // 16-row band of the pass, 32-column group
    const size_t pix0 = (size_t)e * R * R;
    const int n_sub = a.n_subap, n_valid = a.n_valid;

    // ---- prologue: every global load of the prologue is issued before the first barrier ------------------------------------
    // (the barriers are compiler fences for memory operations: a load written after one is issued after it)
    // A operands of the DM product, Gx[x][k = lane >> 4 + 4 step]: the lane's two column tiles are the same in every
    // pass, so they are loaded once, long before the matrix cores need them.  The host re-lays the influence factors
    // out as operand tables (ga_index(), common.hpp): a lane's 6..8 values are two coalesced 16-byte loads, not 6..8 dwords.
#if STEP_BODY_SUB != 2
    const float ctab = fast6::cos_table_lane<float>();           // stage B twiddles, fetched by wave shuffles there
#else
    const float ctab = (float)fast6::kCos[lane % 24];            // (cos_table_lane() of the scope's own lane index)
#endif
#if STEP_BODY_SUB != 2
    f32x4s gx_raw[2][2], gy_raw[2];
#else
    f32x4s gx_raw[2][2];                                         // (Gy C of this step stands in s1: the tail of the first copy)
#endif
#pragma unroll
    for (int tt = 0; tt < 2; ++tt) {
        const f32x4s* src = reinterpret_cast<const f32x4s*>(a.gxa + e * a.ga_env) + (2 * cg + tt) * 2 * 64 + (tid & 63);   // ga_index(), stride 8
        gx_raw[tt][0] = src[0];
        gx_raw[tt][1] = src[64];
    }
#if STEP_BODY_SUB != 2
    const int rt = w >> 1, ct = w & 1;                           // s1 tile of this wave: rows 16 rt.., command columns 16 ct..
    {
        const f32x4s* src = reinterpret_cast<const f32x4s*>(a.gya + e * a.ga_env) + rt * 2 * 64 + (tid & 63);   // gy[16 rt + lc][lq + 4 step]
        gy_raw[0] = src[0];
        gy_raw[1] = src[64];
    }
    float mm_pre[kMaxLayer];                                     // stored range of every layer's screen (lane & 1: min / max)
#pragma unroll
    for (int l = 0; l < kMaxLayer; ++l)
        mm_pre[l] = l < k.pa.n_layer ? static_cast<const float*>(k.pa.minmax[l])[2 * e + (tid & 1)] : 0.f;
#endif
    const bool has_act = tid < k.n_valid_act;                    // n_valid_act <= 1024 (n_act <= 32)
#if STEP_BODY_SUB != 2
    const int act_px = k.pb.act_idx[has_act ? tid : 0];
    const float act_c = k.pb.coefs[(size_t)e * k.n_valid_act + (has_act ? tid : 0)];
    const short slot_v = a.slot_of[tid < n_sub * n_sub ? tid : 0];
    for (int i = tid; i < nA * nA; i += 1024) cimg[i] = 0.f;
    for (int i = tid; i < 2 * PR * SS; i += 1024) s1[i] = 0.f;
    if (tid < n_sub * n_sub) slot_s[tid] = slot_v;
    for (int i = tid + 1024; i < n_sub * n_sub; i += 1024) slot_s[i] = a.slot_of[i];
    lds_barrier();
    if (has_act) cimg[act_px] = act_c;
#endif   // (second step of a pair: cimg and s1 were made in the first copy's tail, slot_s stands)
    float breg[2][KS];
#pragma unroll
    for (int tt = 0; tt < 2; ++tt) {
        const float t[8] = {gx_raw[tt][0][0], gx_raw[tt][0][1], gx_raw[tt][0][2], gx_raw[tt][0][3],
                            gx_raw[tt][1][0], gx_raw[tt][1][1], gx_raw[tt][1][2], gx_raw[tt][1][3]};
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) breg[tt][ks] = t[ks];
    }

#if STEP_BODY_SUB != 2
    // ---- s1[y][ix] = sum_iy gy[y][iy] C[iy][ix] for every row, on the matrix cores: 8 x 2 tiles of 16 x 16, one per wave ---
    lds_barrier();                                             // cimg complete
    {
        const int ix = 16 * ct + lc;
        float av[KS], bv[KS];
        {
            const float t[8] = {gy_raw[0][0], gy_raw[0][1], gy_raw[0][2], gy_raw[0][3], gy_raw[1][0], gy_raw[1][1], gy_raw[1][2], gy_raw[1][3]};
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) av[ks] = t[ks];                                   // A[i = lane & 15][k = lane >> 4]
        }
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            const int iy = lq + 4 * ks;
            bv[ks] = ld_or0(cimg, iy * nA + ix, iy < nA && ix < nA);                      // B[k = lane >> 4][j = lane & 15]
        }
        f32x4s d = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) d = __builtin_amdgcn_mfma_f32_16x16x4f32(av[ks], bv[ks], d, 0, 0, 0);
        if (ix < nA) {
#pragma unroll
            for (int r = 0; r < 4; ++r) s1[(16 * rt + 4 * lq + r) * SS + ix] = d[r];
        }
    }

    // ---- deferred ring scatter: map_full[outerMask] = X of a layer that crossed a pixel this step ----------------------------
    // The ring values are the fixed-order sum of the GEMM's split-K slabs, written through the torus origin.  This
    // workgroup is the only reader of this env's map in this launch, and its vector L1 holds no line of it yet (no load of
    // the map has been issued in this kernel): after the stores are acknowledged (vmcnt 0) and the barrier, the loads below
    // read them back from L2.
    {
        bool any = false;
        for (int l = 0; l < k.pa.n_layer; ++l) {
            const float* x = a.ring_x[l];
            if (x == nullptr) continue;
            any = true;                                           // (uniform over the workgroup: the barrier below)
            const LayerTaps& tl = step_taps<PE>(k.pa, l, e);
            if (PE && !tl.ring) continue;              // per-env clocks: this env's layer did not cross a pixel
            float* map = const_cast<float*>(static_cast<const float*>(k.pa.screen[l])) + (size_t)e * S * S;
            const size_t slab = (size_t)a.n_env * a.n_outer;
            const int oy = tl.oy, ox = tl.ox;
            for (int q = tid; q < a.n_outer; q += 1024) {
                float xv[kMaxSplits];                             // all slabs in flight at once, summed in slab order
#pragma unroll
                for (int z = 0; z < kMaxSplits; ++z)
                    xv[z] = x[(size_t)(z < a.ring_splits[l] ? z : 0) * slab + (size_t)e * a.n_outer + q];
                float v = xv[0];
#pragma unroll
                for (int z = 1; z < kMaxSplits; ++z) v += z < a.ring_splits[l] ? xv[z] : 0.f;
                const int idx = a.outer_idx[q];
                int pr = idx / S + oy, pc = idx % S + ox;
                pr = pr >= S ? pr - S : pr;
                pc = pc >= S ? pc - S : pc;
                map[pr * S + pc] = v;
            }
        }
        if (any) __syncthreads();                                // s_waitcnt vmcnt(0) lgkmcnt(0) + barrier: stores acknowledged
        // Z of the layer's next crossing (env.hip: ring pipeline): the two rings inside the new border, through the new origin
        if (!PE) {
            for (int l = 0; l < k.pa.n_layer; ++l)
                if (a.next_zx[l] != nullptr)
                    gather_ring<float>(static_cast<const float*>(k.pa.screen[l]), a.next_zx[l], a.inner_idx, S, a.n_inner, a.zx_ld,
                                       a.next_sx[l], a.next_sy[l], k.pa.taps[l].oy, k.pa.taps[l].ox, e, tid, 1024);
        }
    }

    // ---- range of every layer's screen (the warp clips to it): read back, or recomputed here after a ring extrusion -------
    __shared__ float lohi[kMaxLayer][2];
    __shared__ float red_lo[16], red_hi[16];
    for (int l = 0; l < k.pa.n_layer; ++l) {
        float* mm = const_cast<float*>(static_cast<const float*>(k.pa.minmax[l])) + 2 * e;
        const bool dirty = k.pa.minmax_dirty[l] || (PE && a.ring_x[l] != nullptr && step_taps<PE>(k.pa, l, e).ring);
        if (!dirty) {
            float pre = 0.f;
#pragma unroll
            for (int q = 0; q < kMaxLayer; ++q) pre = q == l ? mm_pre[q] : pre;
            if (tid < 2) lohi[l][tid] = pre;
            continue;
        }
        // the torus is a permutation of the (N+2)^2 pixels: scan it physically with 16-byte loads
        const float* map = static_cast<const float*>(k.pa.screen[l]) + (size_t)e * S * S;
        const int n4 = (S * S) / 4;                              // env maps are 16-byte aligned when S*S % 4 == 0
        float lo = 3.0e38f, hi = -3.0e38f;
        if ((S * S) % 4 == 0) {
            for (int i0 = tid; i0 < n4; i0 += 4 * 1024) {           // 4 independent 16-byte loads per lane in flight
                f32x4s v[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) v[u] = *reinterpret_cast<const f32x4s*>(map + 4 * (i0 + 1024 * u < n4 ? i0 + 1024 * u : i0));
#pragma unroll
                for (int u = 0; u < 4; ++u)
#pragma unroll
                    for (int d = 0; d < 4; ++d) { lo = v[u][d] < lo ? v[u][d] : lo; hi = v[u][d] > hi ? v[u][d] : hi; }
            }
        } else {
            for (int i = tid; i < S * S; i += 1024) { const float v = map[i]; lo = v < lo ? v : lo; hi = v > hi ? v : hi; }
        }
        for (int off = 32; off > 0; off >>= 1) {
            const float ol = __shfl_down(lo, off), oh = __shfl_down(hi, off);
            lo = ol < lo ? ol : lo;
            hi = oh > hi ? oh : hi;
        }
        lds_barrier();                                           // red_lo / red_hi of the previous layer consumed
        if (lane == 0) { red_lo[w] = lo; red_hi[w] = hi; }
        lds_barrier();
        if (tid == 0) {
            for (int i = 1; i < 16; ++i) { lo = red_lo[i] < lo ? red_lo[i] : lo; hi = red_hi[i] > hi ? red_hi[i] : hi; }
            lohi[l][0] = lo; lohi[l][1] = hi;
            mm[0] = lo; mm[1] = hi;
        }
    }
#endif   // (second step of a pair: s1 = Gy C from the first copy's tail, no ring, no gather, lohi[] of the first stands)

    // Lane -> pixel map of a pass (64 rows): wave = (band = w >> 2: 16 rows, cg = w & 3: 32 columns = 2 tiles of 16);
    // in a tile the lane owns ONE row y = 16 band + (lane & 15) and FOUR CONSECUTIVE columns x = 16 tile + 4 (lane >> 4) + r.
    // That is the output layout of the matrix cores for D[x][y] = sum_k Gx^T[k][x] s1[y][k] (rows 4 (lane >> 4) + r = x,
    // column lane & 15 = y), and it makes every global access of the pass a 16-byte one (the vector-memory path takes
    // ~16 cycles per wave-instruction whatever the width: dword accesses were 3/4 of this kernel's time).
    PupilSums sums;
    for (int pass = 0; pass < (R + PR - 1) / PR; ++pass) {
        const int y0 = pass * PR;
        const int tye = min(PR, R - y0);
        const int yl = 16 * band + lc, y = y0 + yl;              // the lane's row
        const bool row_ok = yl < tye;
#if STEP_BODY_SUB != 2
        if (pass == 0) lds_barrier();                            // s1 and the screen ranges complete
#endif   // (second step of a pair: that is the barrier between the copies)
        // pupil + WFS amplitude of the lane's 2 x 4 pixels (one table: amplitude, or -1 outside the pupil), long before use
        f32x4s apv[2];
#pragma unroll
        for (int tt = 0; tt < 2; ++tt) {
            const int x = 16 * (2 * cg + tt) + 4 * lq;
            const bool okp = row_ok && x < R;
            apv[tt] = *reinterpret_cast<const f32x4s*>(a.amp_pupil + (okp ? (size_t)y * R + x : 0));
            if (!okp) apv[tt] = f32x4s{-1.f, -1.f, -1.f, -1.f};
        }
        float star_amp = 1.f;                                    // (scalar: the env is the workgroup)
        if constexpr (STAR) star_amp = star.amp ? star.amp[e] : 1.f;

        // ---- atmosphere: every layer's tile through LDS (16-byte loads), separable Catmull-Rom ----------------------------
        f32x4s sup[2];
#pragma unroll
        for (int tt = 0; tt < 2; ++tt) sup[tt] = f32x4s{0.f, 0.f, 0.f, 0.f};
        for (int l = 0; l < k.pa.n_layer; ++l) {
#if STEP_BODY_SUB != 2
            const LayerTaps& tp = step_taps<PE>(k.pa, l, e);
#else
            const LayerTaps& tp = a.taps2[l];
#endif
            const float* map = static_cast<const float*>(k.pa.screen[l]) + (size_t)e * S * S;
            const int r0 = y0 + k.pa.foot + tp.dy - 1, c0 = k.pa.foot + tp.dx - 1;
            // Every wave stages ITS tile (16 rows x 32 columns + the 4 x 4 stencil apron) in a private LDS slice: no
            // workgroup barrier in the atmosphere / DM part, so the 16 waves drift apart and one wave's loads overlap
            // another's arithmetic.  LDS operations of one wave execute in order: a compiler fence is all that is needed
            // between the tile writes and the reads of other lanes' data.
            asm volatile("" ::: "memory");
            {
                // tile element (r, c) = map[r0 + 16 band + r][c0 + 32 cg + c], staged as rows of WC4 float4
                const int rw0 = r0 + 16 * band, cw0 = c0 + 32 * cg;
                f32x4s v[NV4];
#pragma unroll
                for (int q = 0; q < NV4; ++q) {
                    const int idx = lane + 64 * q;
                    const int r = idx / WC4, c = 4 * (idx - r * WC4);
                    const int rr = rw0 + r, cc = cw0 + c;
                    const bool need = idx < WR * WC4 && 16 * band + r < tye + 3 && 32 * cg + c < R + 3 && rr >= 0 && rr < S && cc >= 0 && cc < S;
                    v[q] = torus_tile4(map, S, tp.oy, tp.ox, rr, cc, need);
                }
#pragma unroll
                for (int q = 0; q < NV4; ++q) {
                    const int idx = lane + 64 * q;
                    if (idx < WR * WC4) *reinterpret_cast<f32x4s*>(mapt + 4 * idx) = v[q];
                }
            }
            asm volatile("" ::: "memory");
            const float wx[4] = {(float)tp.wx[0], (float)tp.wx[1], (float)tp.wx[2], (float)tp.wx[3]};
            const float wy[4] = {(float)tp.wy[0], (float)tp.wy[1], (float)tp.wy[2], (float)tp.wy[3]};
            const float lo = lohi[l][0], hi = lohi[l][1], wl = (float)tp.weight;
            const bool zero_outside = (lo > 0.f || hi < 0.f);
#pragma unroll
            for (int tt = 0; tt < 2; ++tt) {
                const int xt = 16 * tt + 4 * lq;                  // wave-tile column of the first tap of the lane's first pixel
                warp_row4(mapt, WC, lc, xt, wx, wy, lo, hi, zero_outside, wl, sup[tt]);
            }
        }

        // ---- DM surface on the matrix cores, pupil, phase store, E0 -> LDS, telemetry sums -----------------------------
        const int iy = y / 6, by = y - 6 * iy;
#pragma unroll
        for (int tt = 0; tt < 2; ++tt) {
            const int x = 16 * (2 * cg + tt) + 4 * lq;
            f32x4s dmv = {0.f, 0.f, 0.f, 0.f};
            const float* bp = s1 + (size_t)(row_ok ? y : 0) * SS + lq;   // B[k = lane >> 4][j = lane & 15 -> row y]   (LDS)
#pragma unroll
            for (int ks = 0; ks < KS; ++ks)                              // A[i = lane & 15 -> column][k = lane >> 4] = breg
                if (4 * ks < nAp) dmv = __builtin_amdgcn_mfma_f32_16x16x4f32(breg[tt][ks], bp[4 * ks], dmv, 0, 0, 0);
            if (row_ok && x < R) {
                const size_t q = (size_t)y * R + x;
                f32x4s atm, phi;
                const bool in[4] = {apv[tt][0] >= 0.f, apv[tt][1] >= 0.f, apv[tt][2] >= 0.f, apv[tt][3] >= 0.f};   // -1 = outside the pupil
                residual_pixel4(true, sup[tt], dmv, in, k.atm_scale, k.src_scale, atm, phi, sums);
#if STEP_BODY_SUB != 1
                if (k.pa.store_atm) *reinterpret_cast<f32x4s*>(k.pb.opd_atm + pix0 + q) = atm;
                if (a.store_phase) *reinterpret_cast<f32x4s*>(k.pb.phase + pix0 + q) = phi;   // only where it can be read (StepArgs)
#else
                (void)q;
#endif
                // lenslet (i, j) element E[a][b] = phase[i p + b][j p + a]: the reference tiles phase.T
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int jx = (x + r) / 6, ax = (x + r) - 6 * jx;
                    const int slot = slot_s[iy * n_sub + jx];
                    if (slot >= 0) {                                      // every pixel of a valid lenslet, lit or not
                        float am;
                        if constexpr (STAR) {
                            // the env's factor, a product of its own (one rounding); the test is on the table's value: -1 = outside the pupil
                            const float amp = apv[tt][r] * star_amp;
                            am = apv[tt][r] >= 0.f ? amp * (1.f / 12.f) : 0.f;
                        } else {
                            am = apv[tt][r] >= 0.f ? apv[tt][r] * (1.f / 12.f) : 0.f;   // 1/n of |FFT2(E)/n|^2 (ShackHartmann.py:539)
                        }
                        float sn = 0.f, cs = 0.f;
                        if (am != 0.f) {
                            if (!GEN || a.sc.fast_trig) sincos_fast(phi[r], &sn, &cs); else sincosf(phi[r], &sn, &cs);
                        }
                        E0[slot * EST + ax * 6 + by] = {am * cs, am * sn};
                    }
                }
            }
        }
    }
    // telemetry: waves in a fixed order
    sums.wave_reduce();                                        // (red stored here, not through reduce_pupil_sums: DESIGN.md 4.3a)
    if (lane == 0) {
        red[0][w] = sums.s_atm;
        red[1][w] = sums.q_atm;
        red[2][w] = sums.s_res;
        red[3][w] = sums.q_res;
    }
    lds_barrier();                                             // E0 complete, red complete, cimg / s1 / layer tiles dead
    // the camera's tables on their way into LDS (no registers, nobody waits): they land while the spots are computed
    const bool cam_active = GEN ? a.det.active != 0 : SPEC != STEP_NOCAM;
    const bool cam_photons = GEN ? (a.det.active && a.det.photon_noise) : (SPEC == STEP_PHOTON || (SPEC == STEP_CAMERA && a.det.photon_noise));
    if (cam_photons) alias_table_to_lds(a.pa.tab, a.pa.words, reinterpret_cast<uint32_t*>(lds + L.tab), w, 16, lane);
    if (tid == 1023) {                                           // an idle lane: runs beside the spots of the other waves
        double v[4];
        for (int c = 0; c < 4; ++c) {
            double t = 0;
            for (int q = 0; q < 16; ++q) t += red[c][q];
            v[c] = t;
        }
        double* pp = k.pb.part + (size_t)e * 4;                  // kept for state inspection (FinishArgs.n_tiles == 1)
        for (int c = 0; c < 4; ++c) pp[c] = v[c];
#if STEP_BODY_SUB != 2
        telemetry_scalars<float>(a.fa, e, a.n_env, v);
#else
        FinishArgs<float> fs = a.fa;
        if (fs.telemetry_index >= 0) fs.telemetry_index += 1;
        telemetry_scalars<float>(fs, e, a.n_env, v);
#endif
    }

    // ---- stage B: spots, frame, threshold, centre of gravity ---------------------------------------------------------------
    const int sl_i = lane / 3, q3 = lane - 3 * sl_i;
    const int s = 21 * w + sl_i;
    const bool ok = lane < 63 && s < n_valid;
    float Ia[6], Ib[6];
#pragma unroll
    for (int u = 0; u < 6; ++u) Ia[u] = Ib[u] = 0.f;
    float mx = 0.f;
    int li = 0, lj = 0;
    if (21 * w < n_valid) {                                      // wave-uniform: the twiddle shuffles need every lane
        fast6::lenslet_spots_sel<float, 2, true, !GEN>(E0 + (ok ? s : 0) * EST, q3, ctab, Ia, Ib);
        if (!ok) {
#pragma unroll
            for (int u = 0; u < 6; ++u) Ia[u] = Ib[u] = 0.f;
        }
    }
    if (ok) {
        const int kk = a.sc.subap_idx[s];
        li = kk / n_sub;
        lj = kk - li * n_sub;
    }
#if STEP_BODY_SUB == 2
    DetectorCfg det2 = a.det;
    det2.frame_counter += 1u;                                    // every measurement is a new frame of the noise streams
#define STEP_BODY_DET det2
#else
#define STEP_BODY_DET a.det
#endif
#if STEP_BODY_SUB == 1
#define STEP_BODY_STORE_FRAME false
#else
#define STEP_BODY_STORE_FRAME a.store_frame
#endif
    if (cam_active) {
        // ---- self*self.cam: the camera on the lane's 12 pixels (detector.hpp, "Stream layout") --------------------------------
        // (camera_sh6.hpp: shared with the stand-alone camera kernel)
        f32x16s pxv = camera_pack(Ia, Ib);
        if (cam_photons) {                                        // this wave's share of the tables has landed; then everybody's
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            lds_barrier();
        }
        camera_sh6_lane<CAM_PHOTON_ONLY>(pxv, ok, (uint32_t)((li * 6) * R + lj * 6 + q3), R, (uint32_t)e, STEP_BODY_DET, tab_s, a.pa.lmax);
        camera_unpack(pxv, Ia, Ib);
    }
    // the frame goes to memory only on a step after which it can be read (StepArgs): the centroid below has it in registers
    if (ok) {
        if (STEP_BODY_STORE_FRAME) {
            float* fr = a.frame + pix0 + (size_t)(li * 6) * R + lj * 6 + q3;
#pragma unroll
            for (int u = 0; u < 6; ++u) {
                fr[(size_t)u * R] = Ia[u];
                fr[(size_t)u * R + 3] = Ib[u];
            }
        }
#pragma unroll
        for (int u = 0; u < 6; ++u) {
            mx = Ia[u] > mx ? Ia[u] : mx;
            mx = Ib[u] > mx ? Ib[u] : mx;
        }
    }
    // (counter-based streams: nothing but the frame depends on these pixels, so an unread frame skips them altogether)
    if ((GEN || SPEC == STEP_CAMERA) && STEP_BODY_STORE_FRAME && cam_active && (a.det.dark_e > 0.f || a.det.readout_noise != 0.f)) {
        // the camera also reads out the pixels of the lenslets that are not valid (no light): dark + read-out noise, ADC
#if STEP_BODY_SUB != 2
        const float rtab = recip_table_lane();
#else
        const float rtab = 1.0f / (float)(lane + 1);
#endif
        for (int idx = tid; idx < n_sub * n_sub * 9; idx += 1024) {
            const int kk = idx / 9, j = idx - 9 * kk;
            if (slot_s[kk] < 0) {
                const int i2 = kk / n_sub, j2 = kk - i2 * n_sub;
                uint32_t pix[4];
                sh6_quad_pixels(j, i2 * 6, j2 * 6, R, pix);
                f32x4d v = {0.f, 0.f, 0.f, 0.f};
                detector_quad<false>(v, pix, pix[0], (uint32_t)e, STEP_BODY_DET, rtab, a.pa);
#pragma unroll
                for (int s4 = 0; s4 < 4; ++s4) a.frame[pix0 + pix[s4]] = v[s4];
            }
        }
    }
    // Stage C operands that do not depend on the slopes are requested now: the rows of M (16 lanes per mode, 16-byte
    // loads) and the reference slopes; their latency overlaps the threshold barrier and the centre of gravity.
    // (an opaque zero in the address pins these loads here: loads from read-only kernel arguments may otherwise be
    //  hoisted to the top of the kernel, where 40 more live registers spill)
    int late0;
    asm volatile("v_mov_b32 %0, 0" : "=v"(late0) : "v"(mx));
#if STEP_BODY_SUB == 1
    // (the first step of a pair requests no row of M or M2C^T: the second copy's stage C reconstructs both steps with one fetch.
    //  In their place: the Gy operand of the second step's command product, which this copy forms on its last barriers)
    f32x4s gy_nx[2];
    {
        const f32x4s* src = reinterpret_cast<const f32x4s*>(a.gya + e * a.ga_env) + rt * 2 * 64 + (tid & 63) + late0;
        gy_nx[0] = src[0];
        gy_nx[1] = src[64];
    }
#else
    const int n_sig = 2 * n_valid, n4 = n_sig / 4, A = k.n_valid_act;
    const int km = tid >> 4, l16 = tid & 15;                     // (host: n_modes <= 52, nSig % 4 == 0, nSig <= 640)
    f32x4s mv[10];
    // (a wave without a valid mode requests nothing: a load of a dummy address still takes its turn in the wave-instruction queue of the
    //  vector-memory path, in front of the loads somebody waits for -- the 160 such loads of M and M2C^T cost the step 1.3 us)
    if (4 * w < a.n_modes) {                                     // (wave-uniform: a wave holds the modes 4 w .. 4 w + 3)
        const f32x4s* row = reinterpret_cast<const f32x4s*>(a.fac_m + (size_t)(km < a.n_modes ? km : 0) * n_sig);
#pragma unroll
        for (int j = 0; j < 10; ++j) mv[j] = row[(l16 + 16 * j < n4 ? l16 + 16 * j : 0) + late0];
    } else {
#pragma unroll
        for (int j = 0; j < 10; ++j) mv[j] = f32x4s{0.f, 0.f, 0.f, 0.f};
    }
#endif
    const float ref0 = a.sc.ref[ok ? s : 0], ref1 = a.sc.ref[ok ? n_valid + s : 0];
    // the integrator's inputs of this lane's actuator -- the previous observation (or the caller's action) and env.dm_prev
    // (OOPAOEnv.py:508) -- are requested here too: held from the prologue on they were two more live registers across stages A and B
#if STEP_BODY_SUB == 2
    // (a pair: do_integrate and gain_from_obs != 0, launch_env_step_pair.  The state is the command the first copy formed; the
    //  input is that copy's observation, which the joint pass of stage C below reconstructs.  The lane's image index, which the
    //  other copies hold from the prologue on, is requested here)
    const float dm_prev_c = carry_cn;
    const int act_px = k.pb.act_idx[(has_act ? tid : 0) + late0];
#else
    float act_prev = 0.f, dm_prev_c = 0.f;
    if (a.fa.do_integrate) {
        const size_t io = (size_t)e * (nA * nA) + (has_act ? act_px : 0) + late0;
        act_prev = (a.fa.gain_from_obs != 0.f) ? a.fa.obs[io] : a.fa.action[io];
        dm_prev_c = a.fa.dm_prev[(size_t)e * k.n_valid_act + (has_act ? tid : 0) + late0];
    }
#endif
    for (int off = 32; off > 0; off >>= 1) {
        const float o = __shfl_down(mx, off);
        mx = o > mx ? o : mx;
    }
    if (lane == 0) red_mx[w] = mx;
    lds_barrier();
    mx = red_mx[0];
#pragma unroll
    for (int q = 1; q < 16; ++q) mx = red_mx[q] > mx ? red_mx[q] : mx;
    if (tid == 0) a.wfs_max[e] = mx;
    // (aliases E0: every wave has its spots by now) zero at non-actuators: vec_to_img.  Stage C writes the actuators' values two
    // barriers from here.
#if STEP_BODY_SUB != 1
    for (int i = tid; i < nA * nA; i += 1024) img_s[i] = 0.f;
#else
    // (the first step of a pair has no image.  Every wave has left the camera: the tables' region is dead, and the second step's
    //  command image and Gy C are zeroed there instead -- that step's prologue, on this copy's barriers.  The slopes go to the
    //  pair's own words: `sl` lies in E0, which stage A of the second step overwrites.)
    for (int i = tid; i < nA * nA; i += 1024) cimg[i] = 0.f;
    for (int i = tid; i < 2 * PR * SS; i += 1024) s1[i] = 0.f;
#endif
    float cut;
    if constexpr (STAR) cut = (star.thr ? star.thr[e] : a.sc.threshold) * mx;
    else cut = a.sc.threshold * mx;
    {
        float norm = 0.f, m0 = 0.f, m1 = 0.f;
#pragma unroll
        for (int u = 0; u < 6; ++u) {
            const float xa = Ia[u] < cut ? 0.f : Ia[u], xb = Ib[u] < cut ? 0.f : Ib[u];
            const float rs = xa + xb;
            norm += rs;
            m0 += rs * (float)u;
            m1 += xa * (float)q3 + xb * (float)(q3 + 3);
        }
        norm += __shfl_down(norm, 1) + __shfl_down(norm, 2);
        m0 += __shfl_down(m0, 1) + __shfl_down(m0, 2);
        m1 += __shfl_down(m1, 1) + __shfl_down(m1, 2);
        if (ok && q3 == 0) {
            float c0 = 0.f, c1 = 0.f;
            if (norm != 0.f) {
                c0 = m0 / norm;
                c1 = m1 / norm;
            }
            const float v0 = (c0 - ref0) / a.sc.units, v1 = (c1 - ref1) / a.sc.units;
            sl[s] = v0;
            sl[n_valid + s] = v1;
            a.signal[(size_t)e * 2 * n_valid + s] = v0;
            a.signal[(size_t)e * 2 * n_valid + n_valid + s] = v1;
        }
    }
    lds_barrier();

#if STEP_BODY_SUB == 0
    // ---- stage C ------------------------------------------------------------------------------------------------------------
    // Same arithmetic as tail_from_slopes (sh_device.hpp), with every operand that does not depend on the slopes already
    // in registers: t = M s ; o = -M2C t 1e6 ; integrator ; obs image ; reward          (MAIN/OOPAOEnv/OOPAOEnv.py:491-536)
    const int img = nA * nA;
    float* tm = img_s + img;                                     // [K] modal coefficients
    {
        const f32x4s* s4 = reinterpret_cast<const f32x4s*>(sl);
        float acc = 0.f;
#pragma unroll
        for (int j = 0; j < 10; ++j) {
            const bool okj = l16 + 16 * j < n4;
            const f32x4s sv = s4[okj ? l16 + 16 * j : 0];
            const float d = ((mv[j][0] * sv[0] + mv[j][1] * sv[1]) + mv[j][2] * sv[2]) + mv[j][3] * sv[3];
            acc += okj ? d : 0.f;
        }
#pragma unroll
        for (int off = 8; off > 0; off >>= 1) acc += __shfl_xor(acc, off, 16);
        if (km < a.n_modes && l16 == 0) tm[km] = acc;
    }
    // M2C^T rows for the lane's group of 4 actuators (4 lanes per group, lane part p takes the modes p, p + 4, ...):
    // requested before the barrier, they do not depend on t
    const int n_grp = (A + 3) / 4, g = tid >> 2, part = tid & 3;
    const bool g_ok = g < n_grp;
    f32x4s cv[13];
    int late1;
    asm volatile("v_mov_b32 %0, 0" : "=v"(late1) : "v"(late0));
    if (16 * w < n_grp) {                                        // (wave-uniform: a wave holds the groups 16 w .. 16 w + 15)
#pragma unroll
        for (int j = 0; j < 13; ++j)
            __builtin_memcpy(&cv[j], a.fac_m2c_t + (part + 4 * j < a.n_modes ? (size_t)(part + 4 * j) * A + 4 * (g_ok ? g : 0) : 0) + late1, 16);
    } else {
#pragma unroll
        for (int j = 0; j < 13; ++j) cv[j] = f32x4s{0.f, 0.f, 0.f, 0.f};
    }
    lds_barrier();
    double ss = 0.0;
    {
        float acc[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int j = 0; j < 13; ++j) {
            const bool okj = part + 4 * j < a.n_modes;
            const float t = tm[okj ? part + 4 * j : 0];
#pragma unroll
            for (int d = 0; d < 4; ++d) acc[d] += okj ? cv[j][d] * t : 0.f;
        }
#pragma unroll
        for (int d = 0; d < 4; ++d) {
            acc[d] += __shfl_xor(acc[d], 1, 4);
            acc[d] += __shfl_xor(acc[d], 2, 4);
        }
        // lane tid finishes actuator k = tid (= 4 g + part): its command, image index and integrator input are in registers
        if (has_act) {
            const float mine = part == 0 ? acc[0] : (part == 1 ? acc[1] : (part == 2 ? acc[2] : acc[3]));
            if (a.fa.do_integrate) {
                const float act = (a.fa.gain_from_obs != 0.f) ? a.fa.gain_from_obs * act_prev : act_prev;
                const float cn = dm_prev_c * a.fa.leak + act * 1e-6f;                    // float32 increment (k_recon_finish)
                a.fa.coefs[(size_t)e * A + tid] = cn;
                a.fa.dm_prev[(size_t)e * A + tid] = cn;
            }
            const float o = -mine * 1e6f;
            img_s[act_px] = o;
            ss += (double)o * (double)o;
        }
    }
    lds_barrier();
    {
        float* ob = a.fa.obs + (size_t)e * img;
        for (int q = tid; q < img; q += 1024) ob[q] = img_s[q];
    }
    ss = wave_sum_f64(ss);
    if (lane == 0) red_tail[w] = ss;
    lds_barrier();
    if (tid == 0) {
        double tot = 0;
        for (int q = 0; q < 16; ++q) tot += red_tail[q];
        if (a.fa.reward) a.fa.reward[e] = (float)(-sqrt(tot));
        if (a.fa.ret && a.fa.do_integrate) a.fa.ret[e] += (float)(-sqrt(tot));
    }
#elif STEP_BODY_SUB == 1
    // ---- the first step of a pair ends behind its centre of gravity --------------------------------------------------------
    // The command of the next step, c_{k+1} = leak c_k + gain 1e-6 obs_{k-1} (the reference's one-frame delay, OOPAOEnv.py:508),
    // depends on the observation the step BEFORE this one stored, not on this step's: it is complete here.  This step's own
    // reconstruction (t = M s_k from the slopes above, o_k, the reward) is needed only by the integrator at the end of the second
    // copy, whose stage C forms it beside its own from one fetch of the rows of M and M2C^T; coefs, dm_prev, obs and reward,
    // which that copy overwrites unread, are not stored.  The contraction is written out -- the rounded increment, then one fma,
    // which is what the compiler makes of `dm_prev * leak + act * 1e-6f` in every launch of one step: left to it, this copy rounds
    // both products (a packed multiply).
    if (has_act && a.fa.do_integrate) {
        const float act = (a.fa.gain_from_obs != 0.f) ? a.fa.gain_from_obs * act_prev : act_prev;
        carry_cn = __builtin_fmaf(dm_prev_c, a.fa.leak, act * 1e-6f);
    }
    // ---- the second step's prologue: its command image (zeroed behind the threshold barrier) and s1 = Gy C, as at the top ----
    if (has_act) cimg[act_px] = carry_cn;
    lds_barrier();                                             // cimg complete
    {
        const int ix = 16 * ct + lc;
        float av[KS], bv[KS];
        {
            const float t[8] = {gy_nx[0][0], gy_nx[0][1], gy_nx[0][2], gy_nx[0][3], gy_nx[1][0], gy_nx[1][1], gy_nx[1][2], gy_nx[1][3]};
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) av[ks] = t[ks];
        }
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            const int iy = lq + 4 * ks;
            bv[ks] = ld_or0(cimg, iy * nA + ix, iy < nA && ix < nA);
        }
        f32x4s d = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) d = __builtin_amdgcn_mfma_f32_16x16x4f32(av[ks], bv[ks], d, 0, 0, 0);
        if (ix < nA) {
#pragma unroll
            for (int r = 0; r < 4; ++r) s1[(16 * rt + 4 * lq + r) * SS + ix] = d[r];
        }
    }
    // (the barrier between the copies, step_kernel_body.hpp, then also means "s1 complete")
#else
    // ---- stage C of both steps of a pair: one pass over the rows of M and of M2C^T ------------------------------------------
    // Every sum has the operands and the order it has in a launch of one step; each operand register serves two steps.
    //   t_k = M s_k (the first copy's slopes, StepLds::pair), t_k1 = M s_k1 ; o = -M2C t 1e6 for both ;
    //   c_{k+2} = leak c_{k+1} + gain 1e-6 o_k ; the image, obs and reward of the second step ; return += r_k, then r_k1
    const int img = nA * nA;
    float* tm = img_s + img;                                     // [K] modal coefficients of this step
    float* tm_k = lds + L.pair_tm;                               // [K] ... and of the first step
    {
        const f32x4s* s4 = reinterpret_cast<const f32x4s*>(sl);
        const f32x4s* s4k = reinterpret_cast<const f32x4s*>(lds + L.pair);
        float acc = 0.f, acck = 0.f;
#pragma unroll
        for (int j = 0; j < 10; ++j) {
            const bool okj = l16 + 16 * j < n4;
            const f32x4s sv = s4[okj ? l16 + 16 * j : 0], svk = s4k[okj ? l16 + 16 * j : 0];
            // (a launch of one step rounds mv1 sv1 and chains three fmas onto it)
            const float d = __builtin_fmaf(mv[j][3], sv[3], __builtin_fmaf(mv[j][2], sv[2], __builtin_fmaf(mv[j][0], sv[0], mv[j][1] * sv[1])));
            const float dk = __builtin_fmaf(mv[j][3], svk[3], __builtin_fmaf(mv[j][2], svk[2], __builtin_fmaf(mv[j][0], svk[0], mv[j][1] * svk[1])));
            acc += okj ? d : 0.f;
            acck += okj ? dk : 0.f;
        }
#pragma unroll
        for (int off = 8; off > 0; off >>= 1) {
            acc += __shfl_xor(acc, off, 16);
            acck += __shfl_xor(acck, off, 16);
        }
        if (km < a.n_modes && l16 == 0) {
            tm[km] = acc;
            tm_k[km] = acck;
        }
    }
    // M2C^T rows for the lane's group of 4 actuators (4 lanes per group, lane part p takes the modes p, p + 4, ...):
    // requested before the barrier, they do not depend on t
    const int n_grp = (A + 3) / 4, g = tid >> 2, part = tid & 3;
    const bool g_ok = g < n_grp;
    f32x4s cv[13];
    int late1;
    asm volatile("v_mov_b32 %0, 0" : "=v"(late1) : "v"(late0));
    if (16 * w < n_grp) {                                        // (wave-uniform: a wave holds the groups 16 w .. 16 w + 15)
#pragma unroll
        for (int j = 0; j < 13; ++j)
            __builtin_memcpy(&cv[j], a.fac_m2c_t + (part + 4 * j < a.n_modes ? (size_t)(part + 4 * j) * A + 4 * (g_ok ? g : 0) : 0) + late1, 16);
    } else {
#pragma unroll
        for (int j = 0; j < 13; ++j) cv[j] = f32x4s{0.f, 0.f, 0.f, 0.f};
    }
    lds_barrier();
    double ss = 0.0, ssk = 0.0;
    {
        float acc[4] = {0.f, 0.f, 0.f, 0.f}, acck[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int j = 0; j < 13; ++j) {
            const bool okj = part + 4 * j < a.n_modes;
            const float t = tm[okj ? part + 4 * j : 0], tk = tm_k[okj ? part + 4 * j : 0];
#pragma unroll
            for (int d = 0; d < 4; ++d) acc[d] += okj ? cv[j][d] * t : 0.f;
#pragma unroll
            for (int d = 0; d < 4; ++d) acck[d] += okj ? cv[j][d] * tk : 0.f;
        }
#pragma unroll
        for (int d = 0; d < 4; ++d) {
            acc[d] += __shfl_xor(acc[d], 1, 4);
            acc[d] += __shfl_xor(acc[d], 2, 4);
            acck[d] += __shfl_xor(acck[d], 1, 4);
            acck[d] += __shfl_xor(acck[d], 2, 4);
        }
        // lane tid finishes actuator k = tid (= 4 g + part) of both steps
        if (has_act) {
            const float mine = part == 0 ? acc[0] : (part == 1 ? acc[1] : (part == 2 ? acc[2] : acc[3]));
            const float minek = part == 0 ? acck[0] : (part == 1 ? acck[1] : (part == 2 ? acck[2] : acck[3]));
            const float o_k = -minek * 1e6f;                       // the first step's observation: this step's integrator input
            {
                const float act = (a.fa.gain_from_obs != 0.f) ? a.fa.gain_from_obs * o_k : o_k;
                // (the contraction written out, as in the first copy)
                const float cn = __builtin_fmaf(dm_prev_c, a.fa.leak, act * 1e-6f);
                a.fa.coefs[(size_t)e * A + tid] = cn;
                a.fa.dm_prev[(size_t)e * A + tid] = cn;
            }
            const float o = -mine * 1e6f;
            img_s[act_px] = o;
            ssk += (double)o_k * (double)o_k;
            ss += (double)o * (double)o;
        }
    }
    lds_barrier();
    {
        float* ob = a.fa.obs + (size_t)e * img;
        for (int q = tid; q < img; q += 1024) ob[q] = img_s[q];
    }
    ssk = wave_sum_f64(ssk);
    ss = wave_sum_f64(ss);
    if (lane == 0) {
        red[0][w] = ssk;                                         // (the pupil sums there were consumed in front of the spots)
        red_tail[w] = ss;
    }
    lds_barrier();
    if (tid == 0) {
        double totk = 0, tot = 0;
        for (int q = 0; q < 16; ++q) totk += red[0][q];
        for (int q = 0; q < 16; ++q) tot += red_tail[q];
        if (a.fa.reward) a.fa.reward[e] = (float)(-sqrt(tot));
        // the return takes the first step's reward, then the second's: what two launches add to it one after the other
        if (a.fa.ret && a.fa.do_integrate) a.fa.ret[e] = (a.fa.ret[e] + (float)(-sqrt(totk))) + (float)(-sqrt(tot));
    }
#endif
#undef STEP_BODY_DET
#undef STEP_BODY_STORE_FRAME
#undef STEP_BODY_SUB
