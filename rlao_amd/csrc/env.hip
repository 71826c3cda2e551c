// Host side of libaoenv: the AoEnv object, the atmosphere clock and the C ABI of include/aoenv.h.
#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <initializer_list>
#include <new>
#include <utility>

#include "common.hpp"
#include "delay.hpp"
#include "dev_block.hpp"
#include "dm_pairs.hpp"
#include "dm_tables.hpp"
#include "detector.hpp"
#include "disturb.hpp"
#include "modal.hpp"
#include "policy.hpp"
#include "sh_device.hpp"
#include "sh_geometric.hpp"
#include "sh_lgs.hpp"
#include "science.hpp"
#include "star_env.hpp"
#include "static_opd.hpp"
#include "wavefront.hpp"
#include "offaxis.hpp"

namespace ao {

static thread_local std::string g_err;

int fail(const char* fmt, ...) {
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_err = buf;
    return 1;
}

struct LayerClock {
    double ratio[2] = {0, 0};   // pixels per frame (x, y)          OOPAO/Atmosphere.py:362-363
    double buff[2] = {0, 0};    // sub-pixel accumulator            OOPAO/Atmosphere.py:392-404
};

// Ring pipeline (float32 fused path, shared clock): the operand [Z | xi] of a layer's NEXT pixel crossing is put together while
// the current crossing is being served -- xi by extra workgroups of the ring GEMM's launch (the stream position only moves at
// crossings), Z by the fused step kernel right after it has written the ring (the screen does not change until the next
// crossing) -- so a crossing step launches the GEMM and nothing else in front of the step kernel: k_ring_prepare (9 us, the
// Gaussian draw) leaves the critical path.  [An earlier form ran prepare + GEMM one crossing ahead on a second stream: with one
// 1024-lane workgroup resident on every CU the side-stream kernels found no free CU and time-sliced with the step kernel: slower.]
struct RingAhead { bool valid = false; int sx = 0, sy = 0, buf = 0; };   // zx_pipe[buf][l] holds [Z | xi] for a crossing in direction (sx, sy); mt_alt the stream after it

// One atmosphere layer of a shard (AoEnv::layer).
struct Layer {
    int N = 0, S = 0, nin = 0, nout = 0, K = 0;   // grid: fov != 0 puts a layer at altitude h on one of its own (OOPAO/Atmosphere.py:216-218)
    size_t scr_off = 0;                     // element offset of the layer's [E][S^2] block in AoEnv::screen
    void* ab = nullptr;                     // [nout][K] ring operators [A | B] (layers of a uniform shard share the ring tables)
    int* inner_idx = nullptr;
    int* outer_idx = nullptr;
    bool have_ab = false, have_in = false, have_out = false;
    double weight = 0;
    LayerClock clk;                         // shared clock
    int org[2] = {0, 0};                    // torus origin (oy, ox): logical (r, c) at ((r + oy) % S, (c + ox) % S)
    uint32_t* mt_cur = nullptr;             // ring stream ([E][624] MT19937 states, [E] positions): committed copy ...
    int* pos_cur = nullptr;
    uint32_t* mt_alt = nullptr;             // ... and the one a look-ahead writes (swapped in when the look-ahead is consumed)
    int* pos_alt = nullptr;
    int ring_pending = 0;                   // > 0: split count of a ring extrusion whose scatter the next fused step kernel will do
    const void* ring_src = nullptr;         // its slabs
    RingAhead ahead;
    bool gather_next = false;               // the next fused step kernel is to gather Z into zx_pipe[ahead.buf][l]
    bool minmax_dirty = false;              // the min / max table is stale (ring extruded without the min / max pass)
    int env_rounds = 0;                     // per-env clocks: whole-pixel rounds of a step, the maximum over the envs (clock_rounds)
};

}  // namespace ao

using namespace ao;

// The primitives of the owner of every device allocation (DevBlock, dev_block.hpp) on HIP.  A failure leaves no error pending.
struct HipMem {
    static bool ok(hipError_t e) { if (e != hipSuccess) (void)hipGetLastError(); return e == hipSuccess; }
    static bool alloc(void** p, size_t bytes) { return ok(hipMalloc(p, bytes)); }
    static void free(void* p) { (void)hipFree(p); }              // (waits for the device)
    static bool zero(void* p, size_t bytes) { return ok(hipMemset(p, 0, bytes)); }
    static bool copy_in(void* dst, const void* src, size_t bytes) { return ok(hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice)); }
};
using Block = DevBlock<HipMem>;

#define AO_DISPATCH(env, fn, ...) ((env)->c.dtype == AOENV_F32 ? fn<float>(__VA_ARGS__) : fn<double>(__VA_ARGS__))

struct AoEnv {
    AoCfg c{};
    int device = 0;
    size_t esz = 4;
    int R = 0, A = 0, nAct = 0, E = 0, L = 0, nSig = 0, nSub = 0, nVal = 0;
    int p = 0, n = 0, n_pupil = 0;
    Layer layer[kMaxLayer];                  // layer[0].N / S are set with no atmosphere too (the phase kernels' footprint)
    size_t scr_elems = 0;                    // elements of `screen`
    int Kmax = 0, noutmax = 0, Smax = 0;
    bool uniform = true;                     // every layer on one grid
    int last_zx_layer = 0;
    // per-env clocks (aoenv_set_wind_env): every env its own wind vector per layer; clocks, origins and taps live on the device
    bool per_env_wind = false;
    EnvClock* env_clk[2] = {nullptr, nullptr};   // [L][E] each: current / next (k_ring_prepare_env reads one, writes the other)
    int clk_cur = 0;
    int wind_pixels = 1;                     // aoenv_set_option(AOENV_OPT_ENV_WIND_PIXELS): per-env clocks take |ratio| < wind_pixels
    LayerTaps* env_taps = nullptr;           // [L][E] taps of the current step
    // per-env Fried parameter (aoenv_set_r0_env): the ring tables stay those of r0_tables; env e's innovations are multiplied by
    // sigma_e = (r0_tables / r0_e)^(5/6) where they are written into [Z | xi] (mt_normal_body), its new screens by (r0 / r0_e)^(5/6)
    bool per_env_r0 = false;
    std::vector<double> h_r0;                // [E] metres at 500 nm (the resets and checkpoints read it)
    double* xi_scale = nullptr;              // [E] float64 sigma_e on the device
    const double* sigma() const { return per_env_r0 ? xi_scale : nullptr; }   // what every launch that draws innovations is handed
    bool use_coefs_img = false;              // aoenv_set_option(AOENV_OPT_COEFS_IMAGE); always on above 1024 actuators
    bool defer_ring = true;                  // aoenv_set_option(AOENV_OPT_DEFER_RING)
    bool have[AOENV_C_COUNT] = {false};
    double units = 1.0;
    // device memory (element type = dtype unless noted)
    void* screen = nullptr;                 // [L][E][S*S], every screen a torus (see atm_kernels.hip)
    void* minmax = nullptr;                 // [L][E][2]
    void* zx_pipe = nullptr;                // [2][L][E][K]
    const void* last_zx = nullptr;          // operand of the last ring GEMM (AOENV_B_XI)
    bool use_lookahead = true;              // aoenv_set_option(AOENV_OPT_RING_LOOKAHEAD): the ring pipeline
    void* zx = nullptr;                     // [E][K]  [Z | xi]
    void* xbuf = nullptr;                   // [splits][E][nout] split-K slabs of the ring GEMM
    void* gx = nullptr;
    void* gy = nullptr;
    void* gxt = nullptr;                    // [nActPad4][Rpad128] transpose of gx, zero padded
    void* modes = nullptr;                  // [R*R][A]
    void* dm_opd = nullptr;                 // [E][R*R] dense path
    int* act_idx = nullptr;
    uint8_t* pupil = nullptr;
    void* opd_atm = nullptr;
    void* coefs = nullptr;
    void* dm_prev = nullptr;                // [E][A] env.dm_prev, the integrator state (not touched by aoenv_set_coefs)
    // command-space disturbance (aoenv_set_disturbance, disturb.hpp): in front of every stepped measurement k_disturb_apply writes
    // coefs + B v(tau) into coefs_seen and the step reads its mirror command there; everything else reads and writes coefs
    void* coefs_seen = nullptr;             // [E][A] AOENV_B_COEFS_SEEN
    void* step_cmd = nullptr;               // coefs_seen for the duration of a disturbed step, null otherwise
    void* cmd() const { return step_cmd ? step_cmd : coefs; }   // the command the phase kernels show on the mirror
    struct Disturb {
        bool set = false;
        int M = 0, J = 0;
        int64_t t0 = 0;
        Block mem;                          // both tables; replaced by a larger block when either must grow
        void* modes_t = nullptr;            // [M][A] B transposed, env dtype
        double* par = nullptr;              // amp, freq, phase: [E][M][J] float64 each, one after the other
        size_t modes_cap = 0, par_cap = 0;  // elements the two are sized for
    } disturb;
    // control delay (aoenv_set_delay, delay.hpp): the d actions issued but not yet applied, in a ring of d + 1 image slots
    // ([E][nAct^2] each at a stride padded to 16 bytes); allocated for kMaxDelay + 1 slots by the first delay > 0
    DelayLine delay;
    void* delay_ring = nullptr;
    size_t delay_stride = 0;                // elements between slots
    void* delay_slot(int slot) const { return static_cast<char*>(delay_ring) + (size_t)slot * delay_stride * esz; }
    // modal control surface (aoenv_set_modal, modal.hpp): configuration like the disturbance, in ONE block of its own (a NULL basis
    // frees it)
    struct Modal {
        bool set = false, have_gain = false;
        int K = 0;
        size_t gain_env = 0;                // 0: one gain row for every env, K: a row per env
        Block mem;
        void* m2c_t = nullptr;              // [K][A] M2C transposed
        void* cm = nullptr;                 // [K][nSig] modal command matrix
        void* gain = nullptr;               // [E][K] (the first row alone when gain_env == 0)
        void* image = nullptr;              // [E][nAct^2] the expanded action of a step without delay
        void* zobs = nullptr;               // [E][nAct^2] the zonal observation the step kernel writes
        void* zscal = nullptr;              // [2][E] its reward, and a Strehl row nobody asked for
        void* slabs = nullptr;              // [splits][E][K] products of the GEMM path
    } modal;
    // wavefront modes (aoenv_set_wavefront_basis, wavefront.hpp): configuration like the modal basis, in ONE block of its own (a NULL
    // basis frees it); the record is the caller's memory
    struct Wavefront {
        bool set = false;
        int K = 0;
        WfPlan plan{};
        Block mem;
        void* p = nullptr;                  // [K][wf_row_stride(R^2)] the projector on the full grid
        void* slabs = nullptr;              // [n_slices][2][E][K]
        void* rec = nullptr;                // caller-owned [n_slots][W][E][K], or null: nothing is recorded
        int rec_what = 0, i_base = 0, n_slots = 0;
        int recorded() const { return rec ? rec_what : 0; }
    } wf;
    // science camera (aoenv_set_science, science.hpp): configuration like the wavefront basis, in ONE block of its own (a NULL config
    // frees it); the long-exposure accumulators are the caller's memory
    struct Science {
        bool set = false;
        SciGeom g{};
        int first_frame = 0, flags = 0;
        Block mem;
        void* table = nullptr;              // [2][up][rp] the DFT rows of the window
        void* amp = nullptr;                // [R*R] the field's amplitude (aoenv_compute_psf's)
        void *sum = nullptr, *sum_log10 = nullptr;   // caller-owned [E][W][W] each, or null: nothing is accumulated
        int32_t* count = nullptr;           // caller-owned [E]
        bool accumulates(int i) const { return sum && i >= first_frame; }
    } sci;
    // off-axis science target (aoenv_set_science_direction, offaxis.hpp): configuration like the science camera, in ONE block of its
    // own (NULL arrays free it); the record is the caller's memory.  The field (aoenv_set_field) is what the library is otherwise
    // never told: the telescope's diameter and field of view and the layers' altitudes
    struct OffAxis {
        bool set = false, have_field = false;
        double D = 0, fov = 0, altitude[kMaxLayer] = {};
        std::vector<double> zenith, azimuth;   // [E] arcsec, deg
        Block mem;
        OaShift* dir = nullptr;             // [L][E] the footprints toward the target
        void* phase_sci = nullptr;          // [E][R*R] what the science camera and the projection look at
        void* rec = nullptr;                // caller-owned [n_slots][2][E] (rms nm, Strehl), or null: nothing is recorded
        int i_base = 0, n_slots = 0;
    } oa;
    // off-axis guide star (aoenv_set_guide_direction, offaxis.hpp): the footprints toward the star of every env, in ONE block of its
    // own (NULL arrays free it).  While set, run_phase forms the atmosphere OPD toward the star (k_guide_opd) ahead of the phase kernel
    struct Guide {
        bool set = false;
        std::vector<double> zenith, azimuth;   // [E] arcsec, deg
        Block mem;
        OaShift* dir = nullptr;             // [L][E]
    } guide;
    float* dm_rows = nullptr;               // [E][Rpad128][4][ga_stride] Gy C per env (float32; k_dm_rows), the same switch
    void* coefs_img = nullptr;              // [E][nAct^2] command images for the phase kernels of large DMs (A > 1024)
    void* phase = nullptr;
    void* phase_np = nullptr;               // [E][R*R] geometric shards only: the unmasked phase the slopes are differentiated from
    bool geometric() const { return c.wfs_type == AOENV_WFS_SH_GEOMETRIC; }
    void* scal = nullptr;                   // [E][4]
    double* part = nullptr;                 // [E][tiles][4] telemetry partial sums of the phase kernel
    int n_tiles = 0;
    void* total = nullptr;
    void* residual = nullptr;
    void* wfs_max = nullptr;
    void* amp = nullptr;
    int* subap_idx = nullptr;
    uint8_t* valid2d = nullptr;             // [nSub*nSub]
    short* slot_of = nullptr;               // [nSub*nSub] lenslet -> compact valid index, -1 = not valid
    float* amp_pupil = nullptr;             // [R*R] fused step kernel: amplitude inside the pupil, -1 outside
    float* gxa = nullptr;                   // gx / gy re-laid out as MFMA operand tables (ga_index(), common.hpp), zero padded to Rpad128
    float* gya = nullptr;
    int ga_stride = 8;                      // k steps per (row, q), a multiple of 4 (16-byte loads), >= ceil(nAct / 4)
    // per-env mirrors (aoenv_set_dm_env): E blocks of every layout of the shared tables (dm_tables.hpp) in ONE block of its own
    // (returning to the shared tables frees it); the kernels are handed these pointers and the block sizes as per-env strides while
    // `on`, the shared tables and stride 0 otherwise
    struct DmEnv {
        bool on = false;
        Block mem;
        void *gx = nullptr, *gy = nullptr, *gxt = nullptr;
        float *gxa = nullptr, *gya = nullptr;
    } dm_env;
    // per-env actuator factor pairs (aoenv_set_dm_pairs, dm_pairs.hpp): E blocks of both layouts of py / px and the surface buffer
    // [E][R*R] they are multiplied into, in ONE block of its own (clearing frees it).  While `on` the surface is formed ahead of the
    // phase kernel, like a dense mirror's.
    struct DmPairs {
        bool on = false;
        Block mem;
        void *pyt = nullptr, *pxt = nullptr, *opd = nullptr;
        float *pya = nullptr, *pxa = nullptr;
    } dm_pairs;
    PairsLayout pairs_layout() const { PairsLayout l; l.R = R; l.A = A; return l; }
    // static aberrations (aoenv_set_static_opd, static_opd.hpp): configuration like the guide direction, in ONE block of its own
    // (two NULL arms free it).  w: the sensor arm's map S_w; delta: S_s - S_w, what the science arm adds to the sensor's phase;
    // either may be absent: w is held whenever the caller passed the sensor arm (zeros included: the shard then takes the path of a
    // shard with a map), delta only where it is not zero everywhere in the env dtype
    struct Static {
        Block mem;
        void* w = nullptr;                  // [n][R*R] env dtype, n = E or 1 (map_env = 0)
        void* delta = nullptr;              // [n][R*R]
        size_t map_env = 0;                 // elements between the envs' maps: R*R, or 0 for one map for the shard
        void* surf = nullptr;               // [E][R*R] mirror surface + S_w, what k_phase<T> reads while w is set
        float* rows = nullptr;              // [E][Rpad128][4][ga_stride] Gy C (k_dm_rows): float32 separable mirrors up to 128 across
        void* cimg = nullptr;               // [E][nAct^2] command images: the other separable mirrors
        void* phase_sci = nullptr;          // [E][R*R] the science arm's phase while delta is set and no science direction owns one
        std::vector<double> h_w, h_s;       // the arms as given ([n][R*R]; empty: a NULL arm), for aoenv_get_static_opd
        bool on = false;
    } stat;
    // laser-guide-star spots (aoenv_set_lgs_spots, sh_lgs.hpp): every valid lenslet's binned taps in ONE block of its own (NULL frees
    // it); configuration like the mirror tables.  While `on` the spots come from k_sh_spots_lgs and the shard runs the batched kernels
    struct Lgs {
        bool on = false;
        Block mem;
        void* taps = nullptr;               // [n][nVal][n_pix^2] env dtype, n = E or 1 (tap_env = 0)
        size_t tap_env = 0;                 // elements between the envs' tables: nVal n_pix^2, or 0 for one table for the shard
        int32_t box[4] = {0, 0, 0, 0};      // x0, y0, nx, ny: the cyclic box that holds every non-zero tap
        std::vector<double> h_taps;         // the table as given, for aoenv_get_lgs_spots
    } lgs;
    // the mirror's own surface is formed ahead of the phase kernel (actuator pairs, a dense mirror) in mirror_surface()
    bool mirror_ahead() const { return !c.dm_separable || dm_pairs.on; }
    void* mirror_surface() const { return dm_pairs.on ? dm_pairs.opd : dm_opd; }
    // this shard forms its DM surface ahead of the phase kernel (refresh_dense_dm), which reads it from surface(): the mirror's own
    // where there is one, and the sum of mirror and map for every kind of mirror while a sensor-arm static map is set
    bool dm_surface_ahead() const { return mirror_ahead() || stat.w; }
    // which launch forms mirror + map (aoenv_static_surface_path): 0 no sensor-arm map, 1 k_dm_rows + k_dm_static_mfma, 2
    // k_coefs_image + k_dm_static<T>, 3 the trailing k_static_add behind a mirror that is formed ahead anyway.  refresh_dense_dm
    // branches on this and counts what it launched
    int static_path() const {
        if (!stat.w) return 0;
        if (mirror_ahead()) return 3;
        return esz == 4 && stat.rows && use_mfma && !(force_path & AOENV_PATH_DM_STATIC_GENERAL) ? 1 : 2;
    }
    int64_t static_launches[4] = {0, 0, 0, 0};                     // refreshes of the surface by path, for the shard's life
    void* surface() const { return stat.w ? stat.surf : mirror_surface(); }
    // the science arm differs from the sensor's: a science direction, or a static difference map; its phase lives in sci_phase()
    bool sci_differs() const { return oa.set || stat.delta; }
    void* sci_phase() const { return oa.set ? oa.phase_sci : stat.phase_sci; }
    // stepped frame i needs the step's phase (and, for a direction, the on-axis atmosphere OPD) in HBM
    bool sci_reads_step(bool accumulates) const { return oa.rec || (sci_differs() && accumulates); }
    // per-env guide stars (aoenv_set_flux_env / aoenv_set_threshold_env, star_env.hpp): [E] each in the env dtype, a block of its
    // own each (NULL frees it); absent = null, and the kernels are then handed null pointers
    struct StarDev {
        Block amp_mem, thr_mem;
        void* amp = nullptr;                // sqrt of the env's flux relative to the uploaded AOENV_C_WFS_AMP
        void* thr = nullptr;                // the env's centroid threshold
    } star;
    template <typename T> StarEnv<T> star_env() const { return StarEnv<T>{static_cast<const T*>(star.amp), static_cast<const T*>(star.thr)}; }
    DmLayout dm_layout() const { DmLayout l; l.R = R; l.n_act = nAct; l.ga_stride = ga_stride; return l; }
    std::vector<uint8_t> h_pupil;           // host copies, to rebuild amp_pupil
    std::vector<double> h_amp;
    bool amp_pupil_dirty = true;
    void* sh_ref = nullptr;
    void* tw = nullptr;
    void* phs = nullptr;
    void* frame = nullptr;
    void* signal = nullptr;
    void* recon = nullptr;                  // [A][nSig]
    void* fac_m = nullptr;                  // [K][nSig] modal command matrix calib.M          (AOENV_C_RECON_FACTORS)
    void* fac_m2c_t = nullptr;              // [K][A]    transposed M2C
    void* fac_m2c = nullptr;                // [A][Kp]   M2C, rows zero padded to Kp = n_modes rounded up to 4 (16-byte rows)
    void* tbuf = nullptr;                   // [splits][E][Kp] modal coefficients t = M s of the factored reconstruction
    Block fac_mem;                          // the two buffers above; replaced by a larger block when the rank outgrows it
    size_t fac_cap = 0;                     // modes it is sized for
    bool use_factored_recon = true;         // aoenv_set_option(AOENV_OPT_FACTORED_RECON)
    int n_modes = 0;
    // Pyramid
    void* pyr_mask = nullptr;               // [N*N][2]
    void* pyr_tt = nullptr;                 // [nTheta][R*R]
    void* pyr_tw = nullptr;                 // [N][2]
    void* pyr_t1 = nullptr;                 // [E][chunk][R][N] complex
    void* pyr_t2 = nullptr;                 // [E][chunk][N][N] complex
    FftPlan pyr_plan{};
    int pyr_chunk = 1;
    void* vbuf = nullptr;                   // [E][A]
    DetectorCfg det{};                      // aoenv_set_detector(); det.active = 0: ideal camera
    uint32_t* alias_tab = nullptr;          // alias tables of the photon-noise sampler (poisson_alias.hpp), whole
    int alias_words = 0;                    // the part of them this env's kernels use, and the photon count it reaches: geometries
    float alias_lmax = 0.f;                 // the fused step kernel can take keep what fits in ITS LDS, for every camera kernel
    PoissonAlias alias() const { return PoissonAlias{alias_tab, alias_words, alias_lmax}; }
    bool det_seeded = false;                // a seed has been set: the frame counter survives later aoenv_set_detector calls
    void* ret_acc = nullptr;                // caller-owned [E] episode-return accumulator (aoenv_set_return_accumulator)
    // exploration rollout (aoenv_run_rollout): the noise filter F = Fl Fr in factored form, the inverse of act_idx, the stream position
    void* noise_fr = nullptr;               // [K][A]
    void* noise_fl_t = nullptr;             // [K][A] Fl transposed
    Block noise_mem;                        // the two factors; replaced by a larger block when they must grow
    size_t noise_cap = 0;                   // elements each of the two is sized for
    int noise_K = 0;                        // 0: no filter (n = z)
    std::vector<int32_t> h_act_idx;         // host copy of AOENV_C_ACT_IDX
    int* act_slot = nullptr;                // [nAct^2] pixel -> index among the valid actuators, -1 elsewhere
    bool act_slot_dirty = true;
    void* rollout_scratch = nullptr;        // [2][E] reward / strehl rows nobody asked for
    uint32_t explore_counter = 0;           // word 1 of AOENV_B_COUNTERS
    uint64_t explore_seed = 0;
    bool explore_seeded = false;            // false: the counter (0, or an uploaded checkpoint's) belongs to the next call's seed
    // the policy (aoenv_set_policy), in ONE block: weights in the env dtype (torch layout), the two wide layers re-laid for the MFMA
    // kernel, the projection factors, the two hidden images [E][n_filt][nAct^2]
    struct Policy {
        bool set = false, mfma = false;
        Block mem;
        int H = 0, F = 0, Kp = 0;
        double slope = 0, clamp_abs = 0, b3 = 0;
        void *w1 = nullptr, *b1 = nullptr, *w2 = nullptr, *b2 = nullptr, *w3 = nullptr, *wt1 = nullptr, *wt2 = nullptr;
        void *proj_fr = nullptr, *proj_fl_t = nullptr, *hid1 = nullptr, *hid2 = nullptr;
    } policy;
    std::vector<Block> allocs;              // what dmalloc handed out: for the shard's life
    // optional per-kernel timing with HIP events on the launch stream (bench.py roofline leg)
    bool use_fast_wfs = true;               // aoenv_set_option(AOENV_OPT_FAST_WFS)
    bool use_mfma = true;                   // aoenv_set_option(AOENV_OPT_MFMA_GEMM)
    bool use_fast_trig = true;              // aoenv_set_option(AOENV_OPT_FAST_TRIG)
    bool use_fused_tail = true;             // aoenv_set_option(AOENV_OPT_FUSED_TAIL); needs AOENV_C_RECON_FACTORS
    bool use_fused_step = true;             // aoenv_set_option(AOENV_OPT_FUSED_STEP): the whole step in one kernel
    bool store_opd_atm = false;             // aoenv_set_option(AOENV_OPT_STORE_ATM_OPD): write atm.OPD every step
    bool atm_user_defined = false;          // aoenv_set_atm_opd() until the next step / new screens
    int force_path = 0;                     // aoenv_set_option(AOENV_OPT_FORCE_PATH): AoPath bits
    bool use_step_pairs = true;             // aoenv_set_option(AOENV_OPT_STEP_PAIRS): aoenv_run_integrator takes a quiet step along in the launch before it
    // set by aoenv_run_integrator around a step (plan_step_pair): this launch covers the step behind it too, whose clocks stand at buff2
    struct StepPair { bool on = false; double buff2[kMaxLayer][2] = {}; } pair;
    int64_t step_launches = 0, step_covered = 0;   // fused-step launches and the steps they covered, since aoenv_profile(env, 1)
    bool prof_on = false;
    struct ProfEv { int stage; hipEvent_t a, b; int n; };   // n: what the stage counts for the event (env_step: steps covered)
    std::vector<ProfEv> prof_ev;

    template <typename T> T* as(void* p_) const { return static_cast<T*>(p_); }
    void* screen_ptr(int l) const { return static_cast<char*>(screen) + layer[l].scr_off * esz; }
    void* minmax_ptr(int l) const { return static_cast<char*>(minmax) + (size_t)l * E * 2 * esz; }
    void* xbuf_ptr(int l) const { return static_cast<char*>(xbuf) + (size_t)l * kMaxSplits * E * noutmax * esz; }
    void* zx_pipe_ptr(int buf, int l) const { return static_cast<char*>(zx_pipe) + ((size_t)buf * L + l) * E * Kmax * esz; }
};

namespace {

int dmalloc(AoEnv* env, void** p, size_t bytes, bool zero = true);
// per-env DM command products shared by the tiles of the phase kernels (AOENV_OPT_COEFS_IMAGE): float32 shards keep Gy C in
// MFMA operand layout (k_dm_rows; its padding stays zero from here on), float64 shards the scattered command image
static int alloc_dm_rows(AoEnv* env) {
    if (env->esz == 4 && env->nAct <= 128) {
        if (!env->dm_rows)
            AO_TRY(dmalloc(env, (void**)&env->dm_rows, (size_t)env->E * (cdiv(env->R, 128) * 128) * 4 * env->ga_stride * sizeof(float)));
    } else if (!env->coefs_img) {
        AO_TRY(dmalloc(env, &env->coefs_img, (size_t)env->E * env->nAct * env->nAct * env->esz));
    }
    return 0;
}
// what every block of `parts` that cannot be had reports, unless its caller has words of its own
int block_alloc(Block& b, std::initializer_list<size_t> parts, bool zero) {
    return b.alloc(parts, zero) ? fail("no device memory for %zu bytes", dev_layout(parts).total) : 0;
}
int dmalloc(AoEnv* env, void** p, size_t bytes, bool zero) {
    Block b;
    AO_TRY(block_alloc(b, {bytes ? bytes : 16}, zero));
    *p = b.part(0);
    env->allocs.push_back(std::move(b));
    return 0;
}
// Scratch of one reset, released on every exit path.  The resets return with the kernels that read it still queued on the stream:
// the free of a block waits for the device (dev_block.hpp), which is what keeps this safe.
struct TmpFree {
    std::vector<Block> p;
    int get(std::initializer_list<size_t> parts) { p.emplace_back(); return block_alloc(p.back(), parts, false); }   // one more block ...
    template <typename T> T* part(int k) const { return static_cast<T*>(p.back().part(k)); }                         // ... and its part k
};

// Wraps one kernel launch in a hipEvent pair when profiling is enabled (events are recorded on the same
// stream as the kernel, so the elapsed time is that kernel's device time plus its launch gap).
struct ProfScope {
    AoEnv* env; hipStream_t st; hipEvent_t a = nullptr, b = nullptr; int stage; int n = 1;
    ProfScope(AoEnv* e, int stage_, hipStream_t s) : env(e), st(s), stage(stage_) {
        if (!env->prof_on) return;
        if (hipEventCreate(&a) != hipSuccess || hipEventCreate(&b) != hipSuccess) { a = b = nullptr; return; }
        (void)hipEventRecord(a, st);
    }
    ~ProfScope() {
        if (!a) return;
        (void)hipEventRecord(b, st);
        env->prof_ev.push_back({stage, a, b, n});
    }
};
#define AO_PROF(env, stage, st) ProfScope prof_scope_##stage(env, AOENV_K_##stage, st)
// ... of a launch that counts `count` times in its stage (env_step: the steps it covers)
#define AO_PROF_N(env, stage, st, count)                      \
    ProfScope prof_scope_##stage(env, AOENV_K_##stage, st); \
    prof_scope_##stage.n = (count)

template <typename T>
int upload_f64(void* dst, const double* src, size_t n) {
    std::vector<T> tmp(n);
    for (size_t i = 0; i < n; ++i) tmp[i] = (T)src[i];
    AO_HIP(hipMemcpy(dst, tmp.data(), n * sizeof(T), hipMemcpyHostToDevice));
    return 0;
}

int upload_real(AoEnv* env, void* dst, const double* src, size_t n) { return AO_DISPATCH(env, upload_f64, dst, src, n); }

// ... and back: n values of the env dtype on the device as float64 on the host
template <typename T>
int download_f64(double* dst, const void* src, size_t n) {
    std::vector<T> tmp(n);
    AO_HIP(hipMemcpy(tmp.data(), src, n * sizeof(T), hipMemcpyDeviceToHost));
    for (size_t i = 0; i < n; ++i) dst[i] = (double)tmp[i];
    return 0;
}
int download_real(AoEnv* env, double* dst, const void* src, size_t n) { return AO_DISPATCH(env, download_f64, dst, src, n); }

// src [rows][cols] on the host into dst [cols][rows] in the env dtype
int upload_transposed(AoEnv* env, void* dst, const double* src, size_t rows, size_t cols) {
    std::vector<double> t(rows * cols);
    for (size_t r = 0; r < rows; ++r)
        for (size_t c = 0; c < cols; ++c) t[c * rows + r] = src[r * cols + c];
    return upload_real(env, dst, t.data(), t.size());
}

// index of the first entry of h[0, n) that is not finite; n when every entry is
size_t first_not_finite(const double* h, size_t n) {
    size_t i = 0;
    while (i < n && std::isfinite(h[i])) ++i;
    return i;
}

double sgn(double v) { return (v > 0) - (v < 0); }

template <typename T>
ShConst<T> sh_const(const AoEnv* env) {
    ShConst<T> sc;
    sc.amp = env->as<T>(env->amp);
    sc.subap_idx = env->subap_idx;
    sc.valid2d = env->use_fast_wfs ? env->valid2d : nullptr;
    sc.ref = env->as<T>(env->sh_ref);
    sc.tw = env->as<T>(env->tw);
    sc.ph = env->as<T>(env->phs);
    sc.units = (T)env->units;
    sc.threshold = (T)env->c.threshold_cog;
    sc.fast_trig = (env->use_fast_trig && sizeof(T) == 4) ? 1 : 0;
    sc.plain = (env->force_path & AOENV_PATH_SH_PLAIN) ? 1 : 0;
    return sc;
}

// C[M][N] (+ split-K slabs) = X . W^T: float32 shards use the MFMA kernel, float64 the generic one.
template <typename T>
int gemm_dispatch(AoEnv* env, const T* X, const T* W, T* C, int M, int N, int K, int* splits, hipStream_t st);
template <>
int gemm_dispatch<float>(AoEnv* env, const float* X, const float* W, float* C, int M, int N, int K, int* splits,
                         hipStream_t st) {
    if (!env->use_mfma) { *splits = 1; return launch_gemm_nt<float>(X, W, C, M, N, K, K, K, N, st); }
    *splits = gemm_splits(M, N, K);
    return launch_gemm_nt_mfma(X, W, C, M, N, K, K, K, *splits, st);
}
template <>
int gemm_dispatch<double>(AoEnv*, const double* X, const double* W, double* C, int M, int N, int K, int* splits,
                          hipStream_t st) {
    *splits = 1;
    return launch_gemm_nt<double>(X, W, C, M, N, K, K, K, N, st);
}

// ---- the state changes of a layer's ring pipeline (Layer), each made in one place ---------------------------------------
// The operand prepared for a layer's next crossing will not be used (the screens, the stream or the wind changed): nothing of it
// was committed -- the stream copy it advanced is the alternate one -- so it is simply forgotten; the crossing draws in place.
void forget_lookahead(Layer& y) { y.ahead.valid = false; y.gather_next = false; }

// A deferred ring that is moot (the screens or the clocks it was computed for are gone): it is never scattered.
void drop_ring(Layer& y) { y.ring_pending = 0; }

// the shift of a crossing (sx, sy) on the shared clock: move the origin of the torus
void move_origin(Layer& y, int sx, int sy) {
    y.org[0] = ((y.org[0] - sy) % y.S + y.S) % y.S;
    y.org[1] = ((y.org[1] - sx) % y.S + y.S) % y.S;
}

// The ring GEMM of a crossing of layer l ran on the operand zx and left `splits` split-K slabs in xbuf_ptr(l): the scatter is left
// to the next fused step kernel, or to flush_ring.
void defer_ring(AoEnv* env, int l, const void* zx, int splits) {
    env->last_zx = zx;
    env->last_zx_layer = l;
    env->layer[l].ring_pending = splits;
    env->layer[l].ring_src = env->xbuf_ptr(l);
}

// The fused step kernel of this step takes the deferred rings, and gathers the Z of a look-ahead it was asked for (a look-ahead
// whose ring is not pending has nothing to gather from: it is forgotten).
void take_rings(AoEnv* env, StepArgs& a) {
    for (int l = 0; l < env->L; ++l) {
        Layer& y = env->layer[l];
        a.ring_x[l] = y.ring_pending ? static_cast<const float*>(y.ring_src) : nullptr;
        a.ring_splits[l] = y.ring_pending;
        const bool g = y.gather_next && y.ring_pending && y.ahead.valid;
        a.next_zx[l] = g ? static_cast<float*>(env->zx_pipe_ptr(y.ahead.buf, l)) : nullptr;
        a.next_sx[l] = y.ahead.sx;
        a.next_sy[l] = y.ahead.sy;
        if (y.gather_next && !g) y.ahead.valid = false;
        y.gather_next = false;
    }
}

// ... and has written them, and recomputed and stored every layer's min / max
void rings_written(AoEnv* env) {
    for (int l = 0; l < env->L; ++l) { env->layer[l].ring_pending = 0; env->layer[l].minmax_dirty = false; }
}

// ---- add_row on the device (OOPAO/Atmosphere.py:301-311) for every env of the shard ---------------
// The pending ring of layer l, scattered now: through the shared origin (et = null; with_minmax: with the min / max pass), or per-env
// clocks (et = their taps): only the envs that crossed, each through its own origin.
template <typename T>
int scatter_ring(AoEnv* env, int l, const LayerTaps* et, bool with_minmax, hipStream_t st) {
    Layer& y = env->layer[l];
    AO_PROF(env, SCATTER, st);
    AO_TRY(launch_scatter_minmax<T>(env->as<T>(env->screen_ptr(l)), static_cast<const T*>(y.ring_src), y.outer_idx,
                                    env->as<T>(env->minmax_ptr(l)), nullptr, env->E, env->E, y.S, y.nout, y.ring_pending, y.org[0],
                                    y.org[1], with_minmax ? 1 : 0, st, et));
    y.ring_pending = 0;
    return 0;
}

// A deferred ring of layer l, if any, scattered without the min / max pass (the fused step kernel recomputes the range from the
// map); per-env clocks compute the range of the envs that crossed right away -- there is no per-env "dirty" flag on the host.
template <typename T>
int flush_ring(AoEnv* env, int l, hipStream_t st) {
    Layer& y = env->layer[l];
    if (!y.ring_pending) return 0;
    if (y.gather_next) forget_lookahead(y);                        // (the step kernel that would have gathered the next Z is not coming)
    const LayerTaps* et = env->per_env_wind ? env->env_taps + (size_t)l * env->E : nullptr;
    return scatter_ring<T>(env, l, et, et != nullptr, st);
}
template <typename T>
int flush_rings(AoEnv* env, hipStream_t st) {
    for (int l = 0; l < env->L; ++l) AO_TRY(flush_ring<T>(env, l, st));
    return 0;
}

// The ring GEMM X = [A | B] [Z | xi] of a crossing of layer l into xbuf_ptr(l).
template <typename T>
int ring_gemm(AoEnv* env, int l, const T* zx, int* splits, hipStream_t st) {
    const Layer& y = env->layer[l];
    AO_PROF(env, GEMM_RING, st);
    return gemm_dispatch<T>(env, zx, env->as<T>(y.ab), env->as<T>(env->xbuf_ptr(l)), env->E, y.nout, y.K, splits, st);
}

// lean: no min / max pass (the fused step kernel recomputes the range from the map);  defer: not even the scatter -- the
// fused step kernel of this step writes the ring itself (one launch less per crossing)
template <typename T>
int extrude(AoEnv* env, int l, int sx, int sy, bool lean, hipStream_t st, bool defer = false) {
    Layer& y = env->layer[l];
    forget_lookahead(y);                                           // computed from the screen and the stream as they were
    AO_TRY(flush_ring<T>(env, l, st));                             // an earlier extrusion of this layer in the same step
    T* zx = env->as<T>(env->zx);
    {
        AO_PROF(env, SHIFT_GATHER, st);                           // Z gather + xi draw, one launch
        AO_TRY(launch_ring_prepare<T>(env->as<T>(env->screen_ptr(l)), zx, y.inner_idx, y.mt_cur, y.pos_cur, y.mt_cur, y.pos_cur, nullptr,
                                      env->E, y.S, y.nin, y.nout, y.K, sx, sy, y.org[0], y.org[1], env->sigma(), st));
    }
    int splits = 1;
    AO_TRY(ring_gemm<T>(env, l, zx, &splits, st));
    move_origin(y, sx, sy);
    defer_ring(env, l, zx, splits);
    if (!(defer && lean)) AO_TRY(scatter_ring<T>(env, l, nullptr, !lean, st));
    y.minmax_dirty = lean;
    return 0;
}

// The first ring of an episode (generateNewPhaseScreen, OOPAO/Atmosphere.py:579-585) of layer l for the n envs of the device list
// d_idx (null: env c is row c, the whole shard): the extrusion (sx, sy) = (0, 0) at origin 0 from the stream just seeded, in place,
// scattered with the min / max pass.  The callers have put those envs at origin 0 with no ring pending and no look-ahead.  The GEMM
// runs over the whole shard whatever the list -- its split count and the order of its sums do not depend on it; the rows of the
// other envs are computed and never used.
template <typename T>
int first_ring(AoEnv* env, int l, const int* d_idx, int n, hipStream_t st) {
    Layer& y = env->layer[l];
    T* zx = env->as<T>(env->zx);
    T* map = env->as<T>(env->screen_ptr(l));
    {
        AO_PROF(env, SHIFT_GATHER, st);
        AO_TRY(launch_ring_prepare<T>(map, zx, y.inner_idx, y.mt_cur, y.pos_cur, y.mt_cur, y.pos_cur, d_idx, n, y.S, y.nin, y.nout, y.K, 0, 0,
                                      0, 0, env->sigma(), st));
    }
    int splits = 1;
    AO_TRY(ring_gemm<T>(env, l, zx, &splits, st));
    env->last_zx = zx;
    env->last_zx_layer = l;
    {
        AO_PROF(env, SCATTER, st);
        AO_TRY(launch_scatter_minmax<T>(map, env->as<T>(env->xbuf_ptr(l)), y.outer_idx, env->as<T>(env->minmax_ptr(l)), d_idx, n, env->E,
                                        y.S, y.nout, splits, 0, 0, 1, st));
    }
    if (!d_idx) y.minmax_dirty = false;                            // (a list leaves the other envs' range as stale as it was)
    return 0;
}

// make every layer's min / max table current (consumers other than the fused step kernel)
template <typename T>
int refresh_minmax(AoEnv* env, hipStream_t st) {
    AO_TRY(flush_rings<T>(env, st));
    for (int l = 0; l < env->L; ++l)
        if (env->layer[l].minmax_dirty) {
            AO_TRY(launch_minmax<T>(env->as<T>(env->screen_ptr(l)), env->as<T>(env->minmax_ptr(l)), env->E, env->layer[l].S, st));
            env->layer[l].minmax_dirty = false;
        }
    return 0;
}

// ---- atm.update(): host clock of updateLayer (OOPAO/Atmosphere.py:350-407) -----------------------
// The direction of a layer's next sub-pixel crossing, by running its clock forward (same arithmetic as advance_atmosphere).
bool next_crossing(const LayerClock& k0, int* sx, int* sy) {
    if ((int)std::fabs(k0.ratio[0]) > 0 || (int)std::fabs(k0.ratio[1]) > 0) return false;   // whole-pixel shifts every step: no look-ahead
    if (k0.ratio[0] == 0 && k0.ratio[1] == 0) return false;
    double b[2] = {k0.buff[0], k0.buff[1]};
    for (int it = 0; it < 1000000; ++it) {
        for (int d = 0; d < 2; ++d) b[d] += std::fmod(std::fabs(k0.ratio[d]), 1.0) * sgn(k0.ratio[d]);
        if (std::fabs(b[0]) >= 1 || std::fabs(b[1]) >= 1) {
            *sx = std::fabs(b[0]) < 1 ? 0 : (int)sgn(b[0]);
            *sy = std::fabs(b[1]) < 1 ? 0 : (int)sgn(b[1]);
            return true;
        }
        for (int d = 0; d < 2; ++d) b[d] = std::fmod(std::fabs(b[d]), 1.0) * sgn(b[d]);
    }
    return false;
}

// A crossing of the float32 fused path through the ring pipeline (RingAhead): if the operand [Z | xi] of this crossing was
// put together ahead, commit its stream copy and launch the GEMM alone; else prepare it in place as extrude() does.  Either way
// the GEMM's launch also draws the innovations of the NEXT crossing, and the step kernel of this step is asked to gather its Z.
// The ring itself is left to that kernel (deferred scatter).  Bit-identical to extrude(): the same Z, the same xi, the same product.
int extrude_pipelined(AoEnv* env, int l, int sx, int sy, hipStream_t st) {
    Layer& y = env->layer[l];
    const int cur = y.ahead.buf;
    float* op = static_cast<float*>(env->zx_pipe_ptr(cur, l));
    if (y.ahead.valid && y.ahead.sx == sx && y.ahead.sy == sy) {
        std::swap(y.mt_cur, y.mt_alt);                             // the draw made ahead becomes the layer's stream
        std::swap(y.pos_cur, y.pos_alt);
    } else {
        AO_PROF(env, SHIFT_GATHER, st);
        AO_TRY(launch_ring_prepare<float>(env->as<float>(env->screen_ptr(l)), op, y.inner_idx, y.mt_cur, y.pos_cur, y.mt_cur, y.pos_cur,
                                          nullptr, env->E, y.S, y.nin, y.nout, y.K, sx, sy, y.org[0], y.org[1], env->sigma(), st));
    }
    forget_lookahead(y);
    const int splits = gemm_splits(env->E, y.nout, y.K);
    MtAhead m{y.mt_cur, y.pos_cur, y.mt_alt, y.pos_alt, static_cast<float*>(env->zx_pipe_ptr(1 - cur, l)), y.K, y.nin, y.nout, env->E,
              env->sigma()};
    {
        AO_PROF(env, GEMM_RING, st);
        AO_TRY(launch_ring_gemm_draw_ahead(op, env->as<float>(y.ab), static_cast<float*>(env->xbuf_ptr(l)), env->E, y.nout, y.K, splits, m,
                                           st));
    }
    move_origin(y, sx, sy);
    defer_ring(env, l, op, splits);
    y.minmax_dirty = true;
    int nsx = 0, nsy = 0;
    if (next_crossing(y.clk, &nsx, &nsy)) {                        // (the clock has been advanced for this step already)
        y.ahead = RingAhead{true, nsx, nsy, 1 - cur};
        y.gather_next = true;
    }
    return 0;
}

// Per-env clocks: one launch per layer advances every env's clock on the device and prepares [Z | xi] of the envs that cross a
// pixel; the ring GEMM runs over the whole shard (rows of the other envs are computed and never used: which envs cross is
// not known on the host, and with independent winds some env crosses on nearly every step anyway).
// A layer in which some env's wind is a pixel per frame or more (Layer::env_rounds > 0) first makes that many whole-pixel rounds,
// as the shared clock does in advance_atmosphere: per round the previous round's ring is scattered (the gather reads the screen),
// k_ring_round_env prepares [Z | xi] of the envs that take part, and the GEMM again runs over the whole shard -- its split count and
// the order of its sums must not depend on who takes part.  The rounds leave the clocks alone; k_ring_prepare_env then starts from the
// origin after them.  Per env this is the shared clock's order, all whole rounds and then the sub-pixel crossing, from one stream.
template <typename T>
int advance_atmosphere_env(AoEnv* env, bool lean, hipStream_t st) {
    for (int l = 0; l < env->L; ++l) {
        AO_TRY(flush_ring<T>(env, l, st));
        const Layer& y = env->layer[l];
        T* zx = env->as<T>(env->zx);
        const size_t row = (size_t)l * env->E;
        for (int j = 0; j < y.env_rounds; ++j) {
            {
                AO_PROF(env, SHIFT_GATHER, st);
                AO_TRY(launch_ring_round_env<T>(env->as<T>(env->screen_ptr(l)), zx, y.inner_idx, y.mt_cur, y.pos_cur,
                                                env->env_clk[env->clk_cur] + row, env->env_taps + row, j, env->E, y.S, y.nin, y.nout,
                                                y.K, env->sigma(), st));
            }
            int splits = 1;
            AO_TRY(ring_gemm<T>(env, l, zx, &splits, st));
            defer_ring(env, l, zx, splits);
            AO_TRY(flush_ring<T>(env, l, st));                     // the next gather reads the screen
        }
        {
            AO_PROF(env, SHIFT_GATHER, st);
            AO_TRY(launch_ring_prepare_env<T>(env->as<T>(env->screen_ptr(l)), zx, y.inner_idx, y.mt_cur, y.pos_cur,
                                              env->env_clk[env->clk_cur] + row, env->env_clk[1 - env->clk_cur] + row, env->env_taps + row,
                                              y.weight, env->E, y.S, y.nin, y.nout, y.K, env->sigma(), st));
        }
        int splits = 1;
        AO_TRY(ring_gemm<T>(env, l, zx, &splits, st));
        defer_ring(env, l, zx, splits);
        if (!(lean && env->defer_ring)) AO_TRY(flush_ring<T>(env, l, st));
    }
    env->clk_cur = 1 - env->clk_cur;
    return 0;
}

template <typename T>
int advance_atmosphere(AoEnv* env, bool lean, hipStream_t st) {
    if (env->per_env_wind) return advance_atmosphere_env<T>(env, lean, st);
    for (int l = 0; l < env->L; ++l) {
        LayerClock& k = env->layer[l].clk;
        if (k.ratio[0] == 0 && k.ratio[1] == 0) continue;
        int b0, b1;
        for (int j = 0, mx = clock_rounds(k.ratio, 0, &b0, &b1); j < mx; ++j) {   // whole pixels first (common.hpp)
            clock_rounds(k.ratio, j, &b0, &b1);
            AO_TRY(extrude<T>(env, l, b0, b1, lean, st));
        }
        if (clock_subpixel(k.ratio, k.buff, &b0, &b1)) {          // (the arithmetic the per-env device clocks share, common.hpp)
            if (lean && env->defer_ring && env->use_lookahead && env->zx_pipe && !env->layer[l].ring_pending) {
                AO_TRY(extrude_pipelined(env, l, b0, b1, st));
            } else {
                AO_TRY(extrude<T>(env, l, b0, b1, lean, st, lean && env->defer_ring));
            }
        }
    }
    return 0;
}

template <typename T>
void fill_phase_args(AoEnv* env, PhaseArgs& pa, PhaseBuffers<T>& pb, int update_atm, int store_atm, int store_phase);

template <typename T>
int run_phase(AoEnv* env, int update_atm, int store_atm, hipStream_t st, int store_phase = 1) {
    AO_TRY(refresh_minmax<T>(env, st));
    if (env->use_coefs_img && !env->dm_surface_ahead()) {          // ELT-size DMs: once per env instead of once per tile
        if constexpr (std::is_same<T, float>::value) {
            if (env->dm_rows)                                       // Gy C on the matrix cores, in operand layout
                AO_TRY(launch_dm_rows(env->as<float>(env->cmd()), env->act_idx, env->dm_env.on ? env->dm_env.gya : env->gya,
                                      env->dm_env.on ? env->dm_layout().ga_elems() : 0, env->dm_rows, env->E, env->R, env->nAct, env->A,
                                      env->ga_stride, st));
        }
        if (env->coefs_img)
            AO_TRY(launch_coefs_image<T>(env->as<T>(env->cmd()), env->act_idx, env->as<T>(env->coefs_img), env->E, env->nAct, env->A, st));
    }
    PhaseArgs pa;
    PhaseBuffers<T> pb;
    fill_phase_args<T>(env, pa, pb, update_atm, store_atm, store_phase);
    if (env->guide.set && pa.update_atm) {                         // the sensor's line of sight: the OPD toward the guide star, then
        GuideArgs<T> ga{};                                         // the phase kernel on a given OPD, as after aoenv_set_atm_opd
        ga.pa = pa;
        ga.dir = env->guide.dir;
        ga.opd_atm = pb.opd_atm;
        ga.R = env->R;
        ga.atm_scale = make_phase_kargs<T>(pa, pb, env->R, env->nAct, env->A, env->c.atm_wavelength, env->c.src_wavelength).atm_scale;
        AO_TRY(launch_guide_opd<T>(ga, st));
        pa.update_atm = 0;
    }
    AO_PROF(env, PHASE, st);
    // (a geometric shard: every phase path it can take writes the unmasked phase too -- launch_phase hands the target to whichever
    //  kernel it selects, there is none without the store)
    return launch_phase<T>(pa, pb, env->E, env->R, env->nAct, env->A, env->c.atm_wavelength, env->c.src_wavelength,
                           env->use_mfma, env->force_path, st, env->as<T>(env->phase_np));
}

// the WFS camera on the frame in HBM (detector.hpp); every measurement is a new frame of the noise streams
template <typename T>
int apply_detector(AoEnv* env, bool sh, hipStream_t st) {
    if (!env->det.active) return 0;
    env->det.frame_counter += 1;
    AO_PROF(env, DETECTOR, st);
    const int rc = launch_detector<T>(env->as<T>(env->frame), env->as<T>(env->wfs_max), sh ? env->valid2d : nullptr, env->E,
                                      env->c.cam_res, env->nSub, env->det, env->alias(), st);
    if (rc) env->det.frame_counter -= 1;                           // a refused frame is no frame of the noise streams
    return rc;
}

// Shack-Hartmann spots, then the camera on the frame (self*self.cam, OOPAO/ShackHartmann.py:539-576).  [Round 3 measured the camera
// INSIDE the spots kernel once more (16-wave workgroups, alias tables in LDS, the noisy frame written once, bit-identical): 1140 us
// against 611 + 463 us for the two kernels at the ELT size -- both are bound by vector instructions, not by the frame's round trip.]
template <typename T>
int run_spots_and_camera(AoEnv* env, const ShConst<T>& sc, hipStream_t st) {
    {
        AO_PROF(env, SH_SPOTS, st);
        if (env->lgs.on)                                           // elongated spots: every lenslet's own taps on the unbinned intensity
            AO_TRY(launch_sh_spots_lgs<T>(env->as<T>(env->phase), sc, env->star_env<T>().amp, env->as<T>(env->lgs.taps), env->lgs.tap_env,
                                          env->lgs.box, env->as<T>(env->frame), env->as<T>(env->wfs_max), env->E, env->R, env->nSub,
                                          env->nVal, st));
        else
        AO_TRY(launch_sh_spots<T>(env->as<T>(env->phase), sc, env->star_env<T>().amp, env->as<T>(env->frame), env->as<T>(env->wfs_max), env->E,
                                  env->R, env->nSub, env->nVal, st));
    }
    return apply_detector<T>(env, true, st);
}

template <typename T>
int run_wfs(AoEnv* env, hipStream_t st) {
    if (env->geometric()) {                                        // no spots, no camera: the frame stays zero, no noise frame is counted
        AO_PROF(env, SH_CENTROID, st);
        return launch_sh_geometric<T>(env->as<T>(env->phase_np), env->pupil, env->slot_of, env->units, env->as<T>(env->signal), env->E,
                                      env->R, env->nSub, env->nVal, st);
    }
    if (env->c.wfs_type == AOENV_WFS_PYRAMID) {
        if (!env->have[AOENV_C_PYR_MASK] || (env->c.pyr_n_theta > 1 && !env->have[AOENV_C_PYR_TT]))
            return fail("pyramid mask / modulation table has not been uploaded");
        PyrArgs<T> pa{};
        pa.phase = env->as<T>(env->phase);
        pa.amp = env->as<T>(env->amp);
        pa.amp_env = env->star_env<T>().amp;
        pa.tt = env->c.pyr_n_theta > 1 ? env->as<T>(env->pyr_tt) : nullptr;
        pa.mask = env->as<T>(env->pyr_mask);
        pa.tw = env->as<T>(env->pyr_tw);
        pa.t1 = reinterpret_cast<cx<T>*>(env->pyr_t1);
        pa.t2 = reinterpret_cast<cx<T>*>(env->pyr_t2);
        pa.frame = env->as<T>(env->frame);
        pa.plan = env->pyr_plan;
        pa.R = env->R;
        pa.N = env->c.pyr_n_res;
        pa.cam = env->c.cam_res;
        pa.off = env->c.pyr_n_res / 2 - env->R / 2;
        pa.centering = env->c.pyr_centering;
        pa.phasor_mult = env->c.pyr_centering ? env->c.pyr_n_res + 1 : 0;
        pa.n_env = env->E;
        pa.force_path = env->force_path;
        PyrSlopeArgs<T> sl{};
        sl.frame = env->as<T>(env->frame);
        sl.valid_idx = env->subap_idx;
        sl.ref = env->as<T>(env->sh_ref);
        sl.signal = env->as<T>(env->signal);
        sl.cam = env->c.cam_res;
        sl.n_sub = env->nSub;
        sl.n_valid = env->nVal;
        sl.q_lo = env->c.pyr_q_lo;
        sl.q_hi = env->c.pyr_q_hi;
        sl.norm_valid_mean = env->c.pyr_norm_valid;
        sl.units = (T)env->units;
        AO_PROF(env, PYRAMID, st);
        AO_TRY(launch_pyramid<T>(pa, env->c.pyr_n_theta, env->pyr_chunk, st));
        AO_TRY(apply_detector<T>(env, false, st));                 // self*self.cam (OOPAO/Pyramid.py:987-1006)
        return launch_pyramid_slopes<T>(sl, env->E, st);
    }
    const ShConst<T> sc = sh_const<T>(env);
    AO_TRY(run_spots_and_camera<T>(env, sc, st));                  // spots, self*self.cam (OOPAO/ShackHartmann.py:539-576)
    {
        AO_PROF(env, SH_CENTROID, st);
        AO_TRY(launch_sh_centroid<T>(env->as<T>(env->frame), env->as<T>(env->wfs_max), sc, env->star_env<T>().thr, env->as<T>(env->signal),
                                     env->E, env->R, env->nSub, env->nVal, env->c.max_group, st));
    }
    return 0;
}

// The one place that forms the DM surface of a shard that forms it ahead of the phase kernel (AoEnv::dm_surface_ahead).
// Actuator factor pairs: S_e = (Py_e diag(c_e)) Px_e^T per env (dm_pairs_kernels.hip).
// dm.OPD = modes @ coefs for a dense (non-separable, e.g. two chained mirrors) DM: [E][R^2] = coefs [E][A] . modes [R^2][A]^T
// With a sensor-arm static map (static_opd.hpp) every kind of mirror forms surface + S_w here: a separable mirror Gy C Gx^T + S_w in
// one product whose accumulators start from the map (k_dm_rows + k_dm_static_mfma, or k_coefs_image + k_dm_static<T>), a mirror that
// is formed ahead anyway by one trailing launch that adds the map into the buffer k_phase<T> reads (the mirror's own stays the
// mirror alone, aoenv_get_dm_surface).
template <typename T>
int refresh_mirror_surface(AoEnv* env, hipStream_t st);
template <typename T>
int refresh_dense_dm(AoEnv* env, hipStream_t st) {
    if (!env->dm_surface_ahead()) return 0;
    if (env->mirror_ahead()) AO_TRY(refresh_mirror_surface<T>(env, st));
    const AoEnv::Static& sa = env->stat;
    if (!sa.w) return 0;
    StaticDmArgs<T> a{};
    a.map = env->as<T>(sa.w);
    a.map_env = sa.map_env;
    a.out = env->as<T>(sa.surf);
    a.R = env->R;
    a.n_act = env->nAct;
    const int path = env->static_path();
    env->static_launches[path] += 1;
    if (path == 3) {
        a.base = env->as<T>(env->mirror_surface());
        return launch_static_add<T>(a, env->E, st);
    }
    const AoEnv::DmEnv& de = env->dm_env;                          // every env its own mirror: its tables, a block apart
    const DmLayout dl = env->dm_layout();
    if constexpr (std::is_same<T, float>::value) {
        if (path == 1) {
            const size_t ga_env = de.on ? dl.ga_elems() : 0;
            AO_TRY(launch_dm_rows(env->as<float>(env->cmd()), env->act_idx, de.on ? de.gya : env->gya, ga_env, sa.rows, env->E, env->R,
                                  env->nAct, env->A, env->ga_stride, st));
            a.s1a = sa.rows;
            a.gxa = de.on ? de.gxa : env->gxa;
            a.ga_env = ga_env;
            a.ga_stride = env->ga_stride;
            return launch_dm_static_mfma(a, env->E, st);
        }
    }
    AO_TRY(launch_coefs_image<T>(env->as<T>(env->cmd()), env->act_idx, env->as<T>(sa.cimg), env->E, env->nAct, env->A, st));
    a.coefs_img = env->as<T>(sa.cimg);
    a.gx = env->as<T>(de.on ? de.gx : env->gx);
    a.gy = env->as<T>(de.on ? de.gy : env->gy);
    a.g_env = de.on ? dl.g_elems() : 0;
    return launch_dm_static<T>(a, env->E, st);
}
template <typename T>
int refresh_mirror_surface(AoEnv* env, hipStream_t st) {
    if (env->dm_pairs.on) {
        const AoEnv::DmPairs& dp = env->dm_pairs;
        const PairsLayout pl = env->pairs_layout();
        PairsArgs<T> a{};
        a.coefs = env->as<T>(env->cmd());
        a.pyt = env->as<T>(dp.pyt);
        a.pxt = env->as<T>(dp.pxt);
        a.pya = dp.pya;
        a.pxa = dp.pxa;
        a.out = env->as<T>(dp.opd);
        a.R = env->R;
        a.A = env->A;
        a.ga_stride = pl.ga_stride();
        a.t_env = pl.t_elems();
        a.ga_env = pl.ga_elems();
        return launch_dm_pairs<T>(a, env->E, (env->force_path & AOENV_PATH_DM_PAIRS_GENERAL) != 0, st);
    }
    if (sizeof(T) == 4 && env->use_mfma)                           // one K slice: the product lands in dm_opd directly
        return launch_gemm_nt_mfma(reinterpret_cast<const float*>(env->cmd()), reinterpret_cast<const float*>(env->modes),
                                   reinterpret_cast<float*>(env->dm_opd), env->E, env->R * env->R, env->A, env->A, env->A, 1, st);
    return launch_gemm_nt<T>(env->as<T>(env->cmd()), env->as<T>(env->modes), env->as<T>(env->dm_opd), env->E,
                             env->R * env->R, env->A, env->A, env->A, env->R * env->R, st);
}

template <typename T>
FinishArgs<T> finish_args(AoEnv* env, const T* d_action, T* d_obs, T* d_reward, T* d_strehl, int telemetry_index,
                          int integrate, double gain, int splits) {
    FinishArgs<T> fa{};
    fa.v = env->as<T>(env->vbuf);
    fa.splits = splits;
    fa.act_idx = env->act_idx;
    fa.action = d_action;
    fa.coefs = env->as<T>(env->coefs);
    fa.dm_prev = env->as<T>(env->dm_prev);
    fa.obs = d_obs;
    fa.reward = d_reward;
    fa.ret = env->as<T>(env->ret_acc);
    fa.strehl = d_strehl;
    fa.scal = env->as<T>(env->scal);
    fa.total = env->as<T>(env->total);
    fa.residual = env->as<T>(env->residual);
    fa.part = env->part;
    fa.n_tiles = env->n_tiles;
    fa.n_pupil = env->n_pupil;
    fa.telemetry_index = telemetry_index;
    fa.n_act = env->nAct;
    fa.n_valid_act = env->A;
    fa.do_integrate = integrate;
    fa.leak = (T)env->c.leak;
    fa.gain_from_obs = (T)gain;
    fa.src_scale = 6.283185307179586476925286766559 / env->c.src_wavelength;
    return fa;
}

// v = R s.  With the factors of the reconstructor on the device (R = M2C calib.M, MAIN/OOPAOEnv/OOPAOEnv.py:295, 381) the
// product is chained, t = M s then v = M2C t: K (nSig + A) multiply-adds and bytes per env instead of A nSig -- 11x fewer at the
// ELT size (A = 5209, nSig = 10048, K = 300: 209 MB of dense reconstructor streamed per step), 4.5x at 40x40 Pyramid size.
template <typename T>
int recon_product(AoEnv* env, int* splits, hipStream_t st) {
    const int Kp = (env->n_modes + 3) & ~3;
    if (env->n_modes > 0 && env->use_factored_recon && env->fac_m2c && env->tbuf &&
        (size_t)Kp * (env->nSig + env->A) < (size_t)env->A * env->nSig) {
        T* t = env->as<T>(env->tbuf);
        if constexpr (std::is_same<T, float>::value) {
            if (env->use_mfma) {
                const int s1 = gemm_splits(env->E, Kp, env->nSig);
                AO_TRY(launch_gemm_nt_mfma(env->as<float>(env->signal), env->as<float>(env->fac_m), t, env->E, Kp, env->nSig, env->nSig,
                                           env->nSig, s1, st));
                // (32 and more column tiles of 64 actuators fill the chip for any shard: no split of the short K, one output slab instead of
                //  K / 64 of them -- at the ELT size 11 MB written and read back by the epilogue instead of 43; the choice does not depend on E)
                *splits = cdiv(env->A, 64) >= 32 ? 1 : gemm_splits(env->E, env->A, Kp);
                // a long chain read by many column tiles is summed once first (same order of the additions: same bits)
                int xs = s1;
                if (s1 > 1 && cdiv(env->A, 64) >= 8) {
                    AO_TRY(launch_sum_slabs(t, (size_t)env->E * Kp, s1, st));
                    xs = 1;
                }
                return launch_gemm_nt_mfma(t, env->as<float>(env->fac_m2c), env->as<float>(env->vbuf), env->E, env->A, Kp, Kp, Kp, *splits,
                                           st, xs, (size_t)env->E * Kp);
            }
        }
        *splits = 1;
        AO_TRY(launch_gemm_nt<T>(env->as<T>(env->signal), env->as<T>(env->fac_m), t, env->E, Kp, env->nSig, env->nSig, env->nSig, Kp, st));
        return launch_gemm_nt<T>(t, env->as<T>(env->fac_m2c), env->as<T>(env->vbuf), env->E, env->A, Kp, Kp, Kp, env->A, st);
    }
    return gemm_dispatch<T>(env, env->as<T>(env->signal), env->as<T>(env->recon), env->as<T>(env->vbuf), env->E, env->A, env->nSig,
                            splits, st);
}

template <typename T>
int run_recon(AoEnv* env, const T* d_action, T* d_obs, T* d_reward, T* d_strehl, int telemetry_index, int integrate,
              double gain, hipStream_t st) {
    int splits = 1;
    {
        AO_PROF(env, GEMM_RECON, st);
        AO_TRY(recon_product<T>(env, &splits, st));
    }
    {
        FinishArgs<T> fa = finish_args<T>(env, d_action, d_obs, d_reward, d_strehl, telemetry_index, integrate, gain, splits);
        AO_PROF(env, RECON_FINISH, st);
        AO_TRY(launch_recon_finish<T>(fa, env->E, st));
    }
    if (integrate) AO_TRY(refresh_dense_dm<T>(env, st));
    return 0;
}

// ---- the whole step as one kernel (step_kernel.hip) -------------------------------------------------------------
template <typename T>
bool fused_step_ok(const AoEnv*) { return false; }
template <>
bool fused_step_ok<float>(const AoEnv* env) {
    return env->use_fused_step && env->use_fast_wfs && env->use_mfma && env->use_fused_tail && env->c.wfs_type == AOENV_WFS_SH && !env->dm_surface_ahead() && !env->guide.set && !env->lgs.on && env->n_modes > 0 &&
           env->c.max_group == 1 && env->L > 0 && env->uniform && env->c.cam_res == env->R && (env->force_path & ~(AOENV_PATH_MODAL_GEMM | AOENV_PATH_SH_PLAIN | AOENV_PATH_WF_GENERAL | AOENV_PATH_SCI_GENERAL | AOENV_PATH_DM_PAIRS_GENERAL | AOENV_PATH_DM_STATIC_GENERAL)) == 0 &&
           step_fused_supported(env->R, env->nSub, env->nVal, env->nAct, env->n_modes) != 0;
}

template <typename T>
void fill_phase_args(AoEnv* env, PhaseArgs& pa, PhaseBuffers<T>& pb, int update_atm, int store_atm, int store_phase) {
    pa = PhaseArgs{};
    pa.n_layer = env->L;
    pa.S = env->layer[0].S;
    pa.foot = (env->layer[0].N / 2 - env->R / 2) + 1;
    pa.update_atm = (update_atm && env->L > 0 && !env->atm_user_defined) ? 1 : 0;
    pa.store_atm = store_atm;
    pa.store_phase = store_phase;
    for (int l = 0; l < env->L; ++l) {
        const Layer& y = env->layer[l];
        pa.S_l[l] = y.S;                                           // the R x R footprint of an on-axis source in the layer's grid
        pa.foot_l[l] = (y.N / 2 - env->R / 2) + 1;                 // (OOPAO/Atmosphere.py:226-232: centre N_l // 2)
        pa.screen[l] = env->screen_ptr(l);
        pa.minmax[l] = env->minmax_ptr(l);
        pa.minmax_dirty[l] = y.minmax_dirty ? 1 : 0;
        LayerTaps& t = pa.taps[l];
        t.oy = y.org[0];
        t.ox = y.org[1];
        taps_from_buff(y.clk.buff, t);
        t.weight = y.weight;
    }
    pa.env_taps = env->per_env_wind ? env->env_taps : nullptr;
    pa.n_env = env->E;
    pb = PhaseBuffers<T>{};
    pb.opd_atm = env->as<T>(env->opd_atm);
    pb.coefs = env->as<T>(env->cmd());
    pb.coefs_img = env->use_coefs_img && env->coefs_img ? env->as<T>(env->coefs_img) : nullptr;
    pb.s1a = env->use_coefs_img && !env->dm_surface_ahead() ? env->dm_rows : nullptr;
    pb.dm_opd = env->dm_surface_ahead() ? env->as<T>(env->surface()) : nullptr;
    const AoEnv::DmEnv& de = env->dm_env;                          // every env its own mirror: its tables, a block apart
    const DmLayout dl = env->dm_layout();
    pb.gx = env->as<T>(de.on ? de.gx : env->gx);
    pb.gy = env->as<T>(de.on ? de.gy : env->gy);
    pb.gxt = env->as<T>(de.on ? de.gxt : env->gxt);
    pb.gxa = de.on ? de.gxa : env->gxa;
    pb.gya = de.on ? de.gya : env->gya;
    pb.ga_stride = env->ga_stride;
    pb.g_env = de.on ? dl.g_elems() : 0;
    pb.gxt_env = de.on ? dl.gxt_elems() : 0;
    pb.ga_env = de.on ? dl.ga_elems() : 0;
    pb.act_idx = env->act_idx;
    pb.pupil = env->pupil;
    pb.phase = env->as<T>(env->phase);
    pb.part = env->part;
    pb.wfs_max = env->as<T>(env->wfs_max);
}

template <typename T>
int run_fused_step(AoEnv*, int, const void*, void*, void*, void*, double, bool, hipStream_t) { return fail("fused step: float32 only"); }
// observable: the phase and frame buffers may be read after this step (false: the next step overwrites them first, see StepArgs)
template <>
int run_fused_step<float>(AoEnv* env, int i, const void* d_action, void* d_obs, void* d_reward, void* d_strehl, double gain,
                          bool observable, hipStream_t st) {
    if (env->amp_pupil_dirty) {
        const size_t R2 = (size_t)env->R * env->R;
        if (env->h_pupil.size() != R2 || env->h_amp.size() != R2) return fail("pupil / WFS amplitude have not been uploaded");
        std::vector<float> t(R2);
        for (size_t q = 0; q < R2; ++q) t[q] = env->h_pupil[q] ? (float)env->h_amp[q] : -1.f;
        AO_HIP(hipMemcpyAsync(env->amp_pupil, t.data(), R2 * sizeof(float), hipMemcpyHostToDevice, st));
        AO_HIP(hipStreamSynchronize(st));
        env->amp_pupil_dirty = false;
    }
    StepArgs a{};
    PhaseArgs pa;
    PhaseBuffers<float> pb;
    // (a wavefront record reads the phase -- and the atmosphere, if it records it -- of EVERY step: both stores, not the frame's;
    // the long exposure reads the phase of every frame it accumulates)
    const int rec = env->wf.recorded();
    const bool oa = env->sci_reads_step(env->sci.accumulates(i));  // (the science arm reads both of every step it serves)
    fill_phase_args<float>(env, pa, pb, 1, (env->store_opd_atm || (rec & AOENV_WF_ATMOSPHERE) || oa) ? 1 : 0, 1);
    a.k = make_phase_kargs<float>(pa, pb, env->R, env->nAct, env->A, env->c.atm_wavelength, env->c.src_wavelength);
    a.sc = sh_const<float>(env);
    a.fa = finish_args<float>(env, static_cast<const float*>(d_action), static_cast<float*>(d_obs),
                              static_cast<float*>(d_reward), static_cast<float*>(d_strehl), i, 1, gain, 1);
    a.fa.n_tiles = 1;
    a.frame = env->as<float>(env->frame);
    // (atm.OPD written every step is the state-inspection mode: every step is then observable, there is no fast path to keep)
    a.store_frame = (observable || env->store_opd_atm) ? 1 : 0;
    a.store_phase = (a.store_frame || rec || oa || env->sci.accumulates(i)) ? 1 : 0;
    a.signal = env->as<float>(env->signal);
    a.wfs_max = env->as<float>(env->wfs_max);
    a.fac_m = env->as<float>(env->fac_m);
    a.fac_m2c_t = env->as<float>(env->fac_m2c_t);
    a.slot_of = env->slot_of;
    a.amp_pupil = env->amp_pupil;
    a.gxa = pb.gxa;                                                // (the env's own tables under aoenv_set_dm_env)
    a.gya = pb.gya;
    a.ga_env = pb.ga_env;
    if (env->det.active) env->det.frame_counter += 1;              // every measurement is a new frame of the noise streams
    a.det = env->det;
    a.pa = env->alias();
    take_rings(env, a);
    const Layer& y0 = env->layer[0];                               // (every layer's grid and ring tables: fused_step_ok)
    a.outer_idx = y0.outer_idx;
    a.n_outer = y0.nout;
    a.inner_idx = y0.inner_idx;
    a.n_inner = y0.nin;
    a.zx_ld = y0.K;
    a.n_modes = env->n_modes;
    a.n_subap = env->nSub;
    a.n_valid = env->nVal;
    a.n_env = env->E;
    const bool pair = env->pair.on;                                // (aoenv_run_integrator: the quiet step behind this one in the same launch)
    if (pair) {
        for (int l = 0; l < env->L; ++l) {
            a.taps2[l] = a.k.pa.taps[l];                           // origin and weight stand: nothing crosses
            taps_from_buff(env->pair.buff2[l], a.taps2[l]);
        }
    }
    {
        AO_PROF_N(env, ENV_STEP, st, pair ? 2 : 1);
        AO_TRY(pair ? launch_env_step_pair(a, st) : launch_env_step(a, env->star_env<float>(), st));
    }
    env->step_launches += 1;
    env->step_covered += pair ? 2 : 1;
    rings_written(env);
    if (pair) {                                                    // the covered step: the host clock and the noise streams follow
        for (int l = 0; l < env->L; ++l) {
            LayerClock& c = env->layer[l].clk;
            if (c.ratio[0] == 0 && c.ratio[1] == 0) continue;
            int bx, by;
            if (clock_rounds(c.ratio, 0, &bx, &by) > 0 || clock_subpixel(c.ratio, c.buff, &bx, &by))
                return fail("internal: a step covered by the launch before it crossed a pixel");
        }
        if (env->det.active) env->det.frame_counter += 1;
    }
    return 0;
}

// what plan_step_pair calls eligible, as far as it is the same for every step of a call of aoenv_run_integrator (delay.d == 0 and
// the long exposure's window are the caller's)
bool step_pair_eligible(AoEnv* env) {
    if (!env->use_step_pairs || env->esz != 4 || !fused_step_ok<float>(env) || env->per_env_wind) return false;
    if (env->disturb.set || env->wf.recorded() || env->oa.rec || env->store_opd_atm) return false;
    StepArgs a{};                                                  // what the choice of the instantiation reads
    a.sc = sh_const<float>(env);
    a.det = env->det;
    a.k.n_act = env->nAct;                                         // ... and the pair's LDS layout
    a.n_subap = env->nSub;
    a.n_valid = env->nVal;
    a.n_modes = env->n_modes;
    return env_step_pairable(a, env->star_env<float>());
}

// the measurement of frame i under a disturbance: seen = coefs + B v(t0 + i + 1) in a launch of its own; until the guard goes
// the phase kernels (and the dense DM's surface) read the command there
struct SeenCommand {
    AoEnv* env;
    ~SeenCommand() { env->step_cmd = nullptr; }
};
template <typename T>
int apply_disturbance(AoEnv* env, int i, hipStream_t st) {
    const AoEnv::Disturb& d = env->disturb;
    const size_t n = (size_t)env->E * d.M * d.J;
    DisturbArgs<T> a{};
    a.coefs = env->as<T>(env->coefs);
    a.seen = env->as<T>(env->coefs_seen);
    a.modes_t = env->as<T>(d.modes_t);
    a.amp = d.par;
    a.freq = d.par + n;
    a.phase = d.par + 2 * n;
    a.n_valid_act = env->A;
    a.n_modes = d.M;
    a.n_lines = d.J;
    a.tau = d.t0 + (int64_t)i + 1;
    AO_TRY(launch_disturb_apply<T>(a, env->E, st));
    env->step_cmd = env->coefs_seen;
    return refresh_dense_dm<T>(env, st);                           // (a dense DM's surface is formed ahead of the phase kernel)
}

// A delayed step (delay.hpp): the issued action -- the caller's image, or scale * src with scale != 0 (the integrator's gain * obs)
// -- goes into the ring in a launch of its own, and the step applies the oldest pending one from there.  The caller moves the
// index on (delay_after) once the step is enqueued.
template <typename T>
int delay_push(AoEnv* env, const void* src, double scale, hipStream_t st, const void** applied) {
    const size_t n = (size_t)env->E * env->nAct * env->nAct;
    AO_TRY(launch_delay_push<T>(env->as<T>(env->delay_ring), env->delay_stride, delay_write_slot(env->delay), static_cast<const T*>(src), n,
                                scale, st));
    *applied = env->delay_slot(delay_apply_slot(env->delay));
    return 0;
}

// step k of a recorded loop: the action it applies -- its own (no delay), trajectory slot k - d, or a pending row of the ring
template <typename T>
const T* delay_loop_action(const AoEnv* env, const T* d_action, int k) {
    const size_t n = (size_t)env->E * env->nAct * env->nAct;
    if (env->delay.d == 0) return d_action + (size_t)k * n;
    const DelaySource s = delay_loop_source(env->delay, k);
    return s.trajectory ? d_action + (size_t)s.slot * n : static_cast<const T*>(env->delay_slot(s.slot));
}

// behind a recorded loop of n_steps: the newest min(n_steps, d) actions into the ring, the index moved on
template <typename T>
int delay_loop_end(AoEnv* env, const T* d_action, int n_steps, hipStream_t st) {
    if (env->delay.d == 0) return 0;
    const DelayRefill r = delay_refill(env->delay, n_steps);
    AO_TRY(launch_delay_refill<T>(env->as<T>(env->delay_ring), env->delay_stride, delay_slots(env->delay), r.first_slot, d_action, r.first_traj,
                                  r.m, (size_t)env->E * env->nAct * env->nAct, st));
    env->delay = delay_after(env->delay, n_steps);
    return 0;
}

// ---- wavefront modes (wavefront.hpp, wavefront_kernels.hip) --------------------------------------------------------------------------
// K above which a float32 projection leaves k_wf_project_mfma for the split-K GEMM plus the finish kernel.
// profiles/wavefront_timing.json, measured by scripts/time_wavefront.py at C2 (256 envs, R^2 = 14400): the new tile wins at K = 10
// (11.8 us per call against 35.8), 30 (15.4 against 40.4) and 64 (22.0 against 41.3) and loses at K = 100 (43.7 against 41.9) and
// 500 (79.8 against 57.1); up to 64 modes a wave's tile takes every mode in one pass over X, above that X is read once per 64-mode tile.  The macro is for
// that script's A/B builds alone, which time either route at every K (make FLAGS_env=-D..., AOENV_LIB).
#ifndef AOENV_WF_GEMM_ABOVE_MODES
#define AOENV_WF_GEMM_ABOVE_MODES 64
#endif
constexpr int kWfGemmAboveModes = AOENV_WF_GEMM_ABOVE_MODES;
// the split-K slabs of that route, from (R^2, K) alone like the slices of wf_plan: gemm_splits as it cuts for a shard of 256 envs,
// whatever the shard's size, so that an env's sum has one order in every shard
static int wf_gemm_splits(int r2, int n_modes) { return gemm_splits(256, n_modes, r2); }

// The projection of the buffers as they stand: `what` bits in the order residual, atmosphere, into out [W][E][K].  Its launches are
// not attributed by aoenv_profile.
template <typename T>
int wf_project(AoEnv* env, int what, void* out, hipStream_t st) {
    const AoEnv::Wavefront& wf = env->wf;
    WfArgs<T> a{};
    int w = 0;
    if (what & (AOENV_WF_RESIDUAL | AOENV_WF_SCIENCE)) {            // (the residual toward the target: the caller has formed it)
        a.x[w] = env->as<T>((what & AOENV_WF_SCIENCE) ? env->sci_phase() : env->phase);
        a.scale[w] = (T)(env->c.src_wavelength / (2.0 * M_PI));
        a.use_scale[w] = 1;
        ++w;
    }
    if (what & AOENV_WF_ATMOSPHERE) {
        a.x[w] = env->as<T>(env->opd_atm);
        a.scale[w] = (T)1;
        a.use_scale[w] = 0;
        ++w;
    }
    a.n_w = w;
    a.p = env->as<T>(wf.p);
    a.slabs = env->as<T>(wf.slabs);
    a.out = static_cast<T*>(out);
    a.n_env = env->E;
    a.r2 = env->R * env->R;
    a.ld = wf_row_stride(a.r2);
    a.n_modes = wf.K;
    a.n_slices = wf.plan.n_slices;
    a.slice_len = wf.plan.slice_len;
    if constexpr (std::is_same<T, float>::value) {
        if (wf.K > kWfGemmAboveModes && !(env->force_path & AOENV_PATH_WF_GENERAL)) {
            // above one 64-mode tile: operand by operand through the 64 x 64 split-K tile of launch_gemm_nt_mfma into the slabs,
            // then the same finish kernel
            for (int v = 0; v < w; ++v) {
                WfArgs<T> b = a;
                b.n_w = 1;
                b.x[0] = a.x[v];
                b.scale[0] = a.scale[v];
                b.use_scale[0] = a.use_scale[v];
                b.out = a.out + (size_t)v * a.n_env * a.n_modes;
                b.n_slices = wf_gemm_splits(a.r2, a.n_modes);
                AO_TRY(launch_gemm_nt_mfma(b.x[0], b.p, b.slabs, b.n_env, b.n_modes, b.r2, b.r2, b.ld, b.n_slices, st));
                AO_TRY(launch_wf_finish<T>(b, st));
            }
            return 0;
        }
    }
    return launch_wf_project<T>(a, sizeof(T) == 8 || (env->force_path & AOENV_PATH_WF_GENERAL) != 0, st);
}

// frame i of a stepped loop into its slot of the record, if one is attached (the window was checked before the first launch)
template <typename T>
int wf_record_step(AoEnv* env, int i, hipStream_t st) {
    const AoEnv::Wavefront& wf = env->wf;
    if (!wf.rec) return 0;
    const int W = (wf.rec_what & AOENV_WF_RESIDUAL ? 1 : 0) + (wf.rec_what & AOENV_WF_ATMOSPHERE ? 1 : 0);
    if (i < wf.i_base || i - wf.i_base >= wf.n_slots) return fail("frame %d outside the wavefront record's window [%d, %d)", i, wf.i_base, wf.i_base + wf.n_slots);
    return wf_project<T>(env, wf.rec_what, static_cast<T*>(wf.rec) + (size_t)(i - wf.i_base) * W * env->E * wf.K, st);
}

// what every stepped call checks before its first launch: frames [i0, i0 + n) inside the window of an attached record
static int wf_window_check(const AoEnv* env, int i0, int n) {
    const AoEnv::Wavefront& wf = env->wf;
    const AoEnv::OffAxis& oa = env->oa;
    if (oa.rec && n > 0 && (i0 < oa.i_base || (int64_t)i0 + n > (int64_t)oa.i_base + oa.n_slots))
        return fail("frames [%d, %lld) leave the window [%d, %d) of the attached science-direction record", i0, (long long)i0 + n, oa.i_base,
                    oa.i_base + oa.n_slots);
    if (!wf.rec || n <= 0) return 0;
    if (i0 < wf.i_base || (int64_t)i0 + n > (int64_t)wf.i_base + wf.n_slots)
        return fail("frames [%d, %lld) leave the window [%d, %d) of the attached wavefront record", i0, (long long)i0 + n, wf.i_base,
                    wf.i_base + wf.n_slots);
    return 0;
}

// ---- off-axis science target (offaxis.hpp, offaxis_kernels.hip) -------------------------------------------------------------------
// The residual toward the target from the screens, AOENV_B_PHASE and the on-axis atmosphere OPD as they stand.  One launch, not
// attributed by aoenv_profile.  This is the one place the science arm's phase is formed: callers have checked AoEnv::sci_differs(),
// and without a direction it is AOENV_B_PHASE plus the static difference map (k_science_static; opd_atm_sci is then not written).
template <typename T>
int oa_residual(AoEnv* env, void* phase_sci, void* opd_atm_sci, void* rms_nm, void* strehl, hipStream_t st) {
    if (!env->oa.set) {                                            // a static difference map alone: no layer is walked
        SciStaticArgs<T> s{};
        s.pupil = env->pupil;
        s.phase = env->as<T>(env->phase);
        s.delta = env->as<T>(env->stat.delta);
        s.delta_env = env->stat.map_env;
        s.phase_sci = static_cast<T*>(phase_sci);
        s.rms_nm = static_cast<T*>(rms_nm);
        s.strehl = static_cast<T*>(strehl);
        s.R = env->R;
        s.n_pupil = env->n_pupil;
        s.src_scale = (T)(6.283185307179586476925286766559 / env->c.src_wavelength);
        s.src_scale_d = 6.283185307179586476925286766559 / env->c.src_wavelength;
        return launch_science_static<T>(s, env->E, st);
    }
    OaArgs<T> a{};
    a.delta = env->as<T>(env->stat.delta);
    a.delta_env = env->stat.map_env;
    PhaseBuffers<T> pb;
    fill_phase_args<T>(env, a.pa, pb, 1, 0, 0);
    const KArgs<T> k = make_phase_kargs<T>(a.pa, pb, env->R, env->nAct, env->A, env->c.atm_wavelength, env->c.src_wavelength);
    a.dir = env->oa.dir;
    a.pupil = env->pupil;
    a.phase = env->as<T>(env->phase);
    a.opd_atm = env->as<T>(env->opd_atm);
    a.phase_sci = static_cast<T*>(phase_sci);
    a.opd_atm_sci = static_cast<T*>(opd_atm_sci);
    a.rms_nm = static_cast<T*>(rms_nm);
    a.strehl = static_cast<T*>(strehl);
    a.R = env->R;
    a.n_pupil = env->n_pupil;
    a.atm_scale = k.atm_scale;
    a.src_scale = k.src_scale;
    a.src_scale_d = 6.283185307179586476925286766559 / env->c.src_wavelength;
    return launch_science_residual<T>(a, st);
}

// frame i of a stepped loop into its slot of the record, if one is attached (the window was checked before the first launch)
template <typename T>
int oa_record_step(AoEnv* env, int i, hipStream_t st) {
    const AoEnv::OffAxis& oa = env->oa;
    if (!oa.rec) return 0;
    if (i < oa.i_base || i - oa.i_base >= oa.n_slots) return fail("frame %d outside the science-direction record's window [%d, %d)", i, oa.i_base, oa.i_base + oa.n_slots);
    T* slot = static_cast<T*>(oa.rec) + (size_t)(i - oa.i_base) * 2 * env->E;
    return oa_residual<T>(env, nullptr, nullptr, slot, slot + env->E, st);
}

// on demand: the on-axis atmosphere OPD is not written by the step kernels unless asked to, and is re-derived from the screens
// first, as aoenv_download(AOENV_B_OPD_ATM) does
template <typename T>
int oa_residual_now(AoEnv* env, const char* who, void* phase_sci, void* opd_atm_sci, void* rms_nm, void* strehl, hipStream_t st) {
    if (!env->sci_differs()) return fail("%s: no science direction is set (aoenv_set_science_direction) and no static map makes the science arm differ (aoenv_set_static_opd)", who);
    if (!env->oa.set) {                                            // a static difference map alone: AOENV_B_PHASE as it stands
        if (opd_atm_sci) return fail("%s: no science direction is set (aoenv_set_science_direction): there is no atmosphere toward a target", who);
        return oa_residual<T>(env, phase_sci, nullptr, rms_nm, strehl, st);
    }
    if (env->atm_user_defined)
        return fail("%s: the atmosphere OPD is user-defined (aoenv_set_atm_opd): there are no layers to look through until the atmosphere advances", who);
    if (env->L < 1) return fail("%s: the shard has no layers", who);
    if (!env->store_opd_atm) AO_TRY(run_phase<T>(env, 1, 1, st, 0));
    return oa_residual<T>(env, phase_sci, opd_atm_sci, rms_nm, strehl, st);
}

// ---- science camera (science.hpp, science_kernels.hip) -----------------------------------------------------------------------------
// The window of the phase buffer as it stands (flat: of a zero phase), stored to `out` or -- out == null -- added to the attached
// accumulators.  One launch, not attributed by aoenv_profile.
template <typename T>
int sci_window(AoEnv* env, int flat, void* out, hipStream_t st) {
    const AoEnv::Science& sc = env->sci;
    SciArgs<T> a{};
    // (where the science arm differs from the sensor's the camera looks at phase_sci: the caller has formed it in the launch before
    //  this one)
    a.phase = env->as<T>(env->sci_differs() && !flat ? env->sci_phase() : env->phase);
    a.amp = env->as<T>(sc.amp);
    a.table = env->as<T>(sc.table);
    a.out = static_cast<T*>(out);
    if (!out) {
        a.sum = env->as<T>(sc.sum);
        a.sum_log10 = env->as<T>(sc.sum_log10);
        a.count = sc.count;
    }
    a.scale = sci_scale<T>(sc.g);
    a.n_env = env->E;
    a.R = env->R;
    a.W = sc.g.W;
    a.flat = flat ? 1 : 0;
    return launch_science_window<T>(a, (env->force_path & AOENV_PATH_SCI_GENERAL) != 0, st);
}

// frame i of a stepped loop into the long exposure, if accumulators are attached and the frame counts
template <typename T>
int sci_accumulate_step(AoEnv* env, int i, hipStream_t st) {
    if (!env->sci.accumulates(i)) return 0;
    if (env->sci_differs()) AO_TRY(oa_residual<T>(env, env->sci_phase(), nullptr, nullptr, nullptr, st));   // (the step stored what it reads)
    return sci_window<T>(env, 0, nullptr, st);
}

template <typename T>
int step_t(AoEnv* env, int i, const void* d_action, void* d_obs, void* d_frame, void* d_reward, void* d_strehl,
           double gain, bool observable, hipStream_t st) {
    const bool fused_step = fused_step_ok<T>(env);
    SeenCommand seen{env};                                         // (error paths: no later call sees the side buffer)
    if (env->disturb.set) AO_TRY(apply_disturbance<T>(env, i, st));
    AO_TRY(advance_atmosphere<T>(env, fused_step, st));
    env->atm_user_defined = false;
    if (fused_step) {
        AO_TRY(run_fused_step<T>(env, i, d_action, d_obs, d_reward, d_strehl, gain, observable, st));
        env->step_cmd = nullptr;
        AO_TRY(wf_record_step<T>(env, i, st));
        AO_TRY(oa_record_step<T>(env, i, st));
        AO_TRY(sci_accumulate_step<T>(env, i, st));
        if (d_frame)
            AO_HIP(hipMemcpyAsync(d_frame, env->frame, (size_t)env->E * env->c.cam_res * env->c.cam_res * sizeof(T),
                                  hipMemcpyDeviceToDevice, st));
        return 0;
    }
    AO_TRY(run_phase<T>(env, 1, (env->store_opd_atm || (env->wf.recorded() & AOENV_WF_ATMOSPHERE) || env->sci_reads_step(env->sci.accumulates(i))) ? 1 : 0, st));
    AO_TRY(wf_record_step<T>(env, i, st));                         // (the phase kernel has written what the sensor is about to see)
    AO_TRY(oa_record_step<T>(env, i, st));
    AO_TRY(sci_accumulate_step<T>(env, i, st));
    env->step_cmd = nullptr;                                       // the integration below, and a dense DM's next surface: the pure command
    // one workgroup per env re-reads the factors from L2: wins while launch latency dominates (measured: 19.5 us vs
    // 32.5 us at 256 envs, 96 us vs 75 us at 2048), the batched MFMA GEMM path takes over for large shards
    const bool fused = env->c.wfs_type == AOENV_WFS_SH && env->use_fused_tail && env->n_modes > 0 && env->E <= 1024;
    if (env->geometric()) {                                        // two launches: the phase above, slopes + tail here
        int rc = -1;
        // (the fit is decided before the profile scope opens: a step that takes the separate kernels counts nothing under sh_tail)
        if (env->use_fused_tail && env->n_modes > 0 && env->E <= 1024 &&
            geo_tail_band(env->R, env->nSub, env->nVal, env->nAct, env->n_modes, sizeof(T)) > 0) {
            FinishArgs<T> fa = finish_args<T>(env, static_cast<const T*>(d_action), static_cast<T*>(d_obs),
                                              static_cast<T*>(d_reward), static_cast<T*>(d_strehl), i, 1, gain, 1);
            AO_PROF(env, SH_TAIL, st);
            rc = launch_geo_tail<T>(env->as<T>(env->phase_np), env->pupil, env->slot_of, env->units, env->as<T>(env->signal),
                                    env->as<T>(env->fac_m), env->as<T>(env->fac_m2c_t), env->n_modes, fa, env->E, env->R, env->nSub,
                                    env->nVal, st);
        }
        if (rc > 0) return rc;
        if (rc == 0) {
            AO_TRY(refresh_dense_dm<T>(env, st));
        } else {                                                   // no fused tail, or it does not fit in LDS: the separate kernels
            AO_TRY(run_wfs<T>(env, st));
            AO_TRY(run_recon<T>(env, static_cast<const T*>(d_action), static_cast<T*>(d_obs), static_cast<T*>(d_reward),
                                static_cast<T*>(d_strehl), i, 1, gain, st));
        }
    } else if (fused) {
        const ShConst<T> sc = sh_const<T>(env);
        AO_TRY(run_spots_and_camera<T>(env, sc, st));
        FinishArgs<T> fa = finish_args<T>(env, static_cast<const T*>(d_action), static_cast<T*>(d_obs),
                                          static_cast<T*>(d_reward), static_cast<T*>(d_strehl), i, 1, gain, 1);
        int rc;
        {
            AO_PROF(env, SH_TAIL, st);
            rc = launch_sh_tail<T>(env->as<T>(env->frame), env->as<T>(env->wfs_max), sc, env->star_env<T>().thr, env->as<T>(env->signal),
                                   env->as<T>(env->fac_m), env->as<T>(env->fac_m2c_t), env->n_modes, fa, env->E, env->R,
                                   env->nSub, env->nVal, env->c.max_group, st);
        }
        if (rc > 0) return rc;
        if (rc == 0) {
            AO_TRY(refresh_dense_dm<T>(env, st));
        } else {                                                   // does not fit in LDS: the separate kernels
            {
                AO_PROF(env, SH_CENTROID, st);
                AO_TRY(launch_sh_centroid<T>(env->as<T>(env->frame), env->as<T>(env->wfs_max), sc, env->star_env<T>().thr, env->as<T>(env->signal),
                                             env->E, env->R, env->nSub, env->nVal, env->c.max_group, st));
            }
            AO_TRY(run_recon<T>(env, static_cast<const T*>(d_action), static_cast<T*>(d_obs), static_cast<T*>(d_reward),
                                static_cast<T*>(d_strehl), i, 1, gain, st));
        }
    } else {
        AO_TRY(run_wfs<T>(env, st));
        AO_TRY(run_recon<T>(env, static_cast<const T*>(d_action), static_cast<T*>(d_obs), static_cast<T*>(d_reward),
                            static_cast<T*>(d_strehl), i, 1, gain, st));
    }
    if (d_frame)
        AO_HIP(hipMemcpyAsync(d_frame, env->frame, (size_t)env->E * env->c.cam_res * env->c.cam_res * sizeof(T),
                              hipMemcpyDeviceToDevice, st));
    return 0;
}

// ---- the modal control surface (modal.hpp, modal_kernels.hip) ---------------------------------------------------------------------
// K n_signal above which the projection leaves the per-env kernel (every env re-reads cm from L2, every lane runs a chain of
// n_signal / 64 dependent fmas) for the batched GEMM plus the finish kernel.  profiles/modal_timing.json ("threshold"), measured by
// scripts/time_modal.py: at the C2 shape (256 envs, 632 slopes) the per-env kernel wins up to K = 50 (31 600: 7.5 us against 10.1)
// and loses from K = 100 (63 200: 11.4 against 10.2), the lines cross near 53 000; at the C4 shape (512 envs, 10 048 slopes) the
// GEMM path wins at every K measured from 5 (50 240: 55 us against 32) to 300 (3 014 400: 819 us against 61).  The macro is for
// that script's A/B build alone, which times the per-env kernel above the threshold too (make FLAGS_env=-D..., AOENV_LIB).
#ifndef AOENV_MODAL_GEMM_THRESHOLD
#define AOENV_MODAL_GEMM_THRESHOLD ((size_t)40000)
#endif
constexpr size_t kModalGemmThreshold = AOENV_MODAL_GEMM_THRESHOLD;

// o = -1e6 cm signal and the reward from AOENV_B_SIGNAL as it stands; `ret` is the return accumulator to add the reward to, or null
template <typename T>
int modal_project(AoEnv* env, void* d_obs, void* d_reward, void* ret, hipStream_t st) {
    const AoEnv::Modal& mo = env->modal;
    ModalObsArgs<T> a{};
    a.cm = env->as<T>(mo.cm);
    a.signal = env->as<T>(env->signal);
    a.obs = static_cast<T*>(d_obs);
    a.reward = static_cast<T*>(d_reward);
    a.ret = static_cast<T*>(ret);
    a.n_modes = mo.K;
    a.n_signal = env->nSig;
    const bool gemm = (env->force_path & AOENV_PATH_MODAL_GEMM) || (size_t)mo.K * env->nSig > kModalGemmThreshold ||
                      !modal_obs_fits(mo.K, env->nSig, sizeof(T));
    if (!gemm) return launch_modal_obs<T>(a, env->E, st);
    int splits = 1;
    AO_TRY(gemm_dispatch<T>(env, a.signal, a.cm, env->as<T>(mo.slabs), env->E, mo.K, env->nSig, &splits, st));
    a.slabs = env->as<T>(mo.slabs);
    a.splits = splits;
    return launch_modal_finish<T>(a, env->E, st);
}

// for the duration of a modal step the return accumulator is detached from the step kernel -- it receives the modal reward from the
// projection instead -- and is back in place whichever way the scope is left
struct DetachedReturn {
    AoEnv* env;
    void* ret;
    explicit DetachedReturn(AoEnv* e) : env(e), ret(e->ret_acc) { e->ret_acc = nullptr; }
    ~DetachedReturn() { env->ret_acc = ret; }
    DetachedReturn(const DetachedReturn&) = delete;
    DetachedReturn& operator=(const DetachedReturn&) = delete;
};

// One modal step: the action image from d_coef (the caller's coefficients, or with use_gain the previous observation times the
// gains) in one launch -- under a delay into the line's write slot, where aoenv_step would copy the caller's image -- then the
// explicit-action step of aoenv_step on it, then the projection.  The return accumulator is detached for the step itself: it
// receives the modal reward.
template <typename T>
int step_modal_t(AoEnv* env, int i, const void* d_coef, bool use_gain, void* d_obs, void* d_frame, void* d_reward, void* d_strehl,
                 bool observable, hipStream_t st) {
    AoEnv::Modal& mo = env->modal;
    ModalActionArgs<T> a{};
    a.m2c_t = env->as<T>(mo.m2c_t);
    a.act_idx = env->act_idx;
    a.coef = static_cast<const T*>(d_coef);
    a.gain = use_gain ? env->as<T>(mo.gain) : nullptr;
    a.gain_env = mo.gain_env;
    a.n_modes = mo.K;
    a.n_valid_act = env->A;
    a.img = env->nAct * env->nAct;
    const bool delayed = env->delay.d > 0;
    a.image = static_cast<T*>(delayed ? env->delay_slot(delay_write_slot(env->delay)) : mo.image);
    const void* applied = delayed ? env->delay_slot(delay_apply_slot(env->delay)) : mo.image;
    AO_TRY(launch_modal_action<T>(a, env->E, st));
    T* zs = env->as<T>(mo.zscal);
    void* ret = nullptr;
    {
        DetachedReturn detached(env);
        ret = detached.ret;
        AO_TRY(step_t<T>(env, i, applied, mo.zobs, d_frame, zs, d_strehl ? d_strehl : zs + env->E, 0.0, observable, st));
    }
    if (delayed) env->delay = delay_after(env->delay, 1);
    return modal_project<T>(env, d_obs, d_reward, ret, st);
}

template <typename T>
int reset_soft_t(AoEnv* env, void* d_obs, hipStream_t st) {
    return run_recon<T>(env, nullptr, static_cast<T*>(d_obs), nullptr, nullptr, -1, 0, 0.0, st);
}

template <typename T>
int reset_soft_modal_t(AoEnv* env, void* d_obs, hipStream_t st) {
    AO_TRY(run_recon<T>(env, nullptr, env->as<T>(env->modal.zobs), nullptr, nullptr, -1, 0, 0.0, st));
    return modal_project<T>(env, d_obs, nullptr, nullptr, st);
}

struct BufInfo {
    void* ptr;
    size_t bytes;
};

int buf_info(AoEnv* env, int which, BufInfo* b) {
    const size_t z = env->esz, E = env->E, R2 = (size_t)env->R * env->R;
    switch (which) {
        case AOENV_B_SCREEN: *b = {nullptr, env->scr_elems * z}; return 0;   // gathered per layer: [E][S_l^2] blocks, layer after layer
        case AOENV_B_OPD_ATM: *b = {env->opd_atm, E * R2 * z}; return 0;
        case AOENV_B_COEFS: *b = {env->coefs, E * env->A * z}; return 0;
        case AOENV_B_PHASE: *b = {env->phase, E * R2 * z}; return 0;
        case AOENV_B_FRAME: *b = {env->frame, E * (size_t)env->c.cam_res * env->c.cam_res * z}; return 0;
        case AOENV_B_SIGNAL: *b = {env->signal, E * env->nSig * z}; return 0;
        case AOENV_B_TOTAL: *b = {env->total, (size_t)env->c.n_loop * E * z}; return 0;
        case AOENV_B_RESIDUAL: *b = {env->residual, (size_t)env->c.n_loop * E * z}; return 0;
        case AOENV_B_WFS_MAX: *b = {env->wfs_max, E * z}; return 0;
        case AOENV_B_XI: *b = {env->last_zx ? const_cast<void*>(env->last_zx) : env->zx, E * env->layer[env->last_zx_layer].K * z}; return 0;
        case AOENV_B_MT_STATE: *b = {nullptr, (size_t)env->L * E * (kMtN + 1) * 4}; return 0;     // packed on the host
        case AOENV_B_COUNTERS: *b = {nullptr, 16}; return 0;
        case AOENV_B_DM_PREV: *b = {env->dm_prev, E * env->A * z}; return 0;
        case AOENV_B_COEFS_SEEN: *b = {env->coefs_seen, E * env->A * z}; return 0;
        default: return fail("unknown buffer id %d", which);
    }
}

}  // namespace

// Every entry point runs on the env's device and hands the calling thread's current device back on return: PyTorch shares
// this runtime, and an env on device k must not redirect the caller's later allocations and launches to k.
struct DeviceGuard {
    int prev = -1;
    bool ok = false;
    explicit DeviceGuard(int device) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        ok = prev == device || hipSetDevice(device) == hipSuccess;
        if (prev == device) prev = -1;                               // nothing to restore
    }
    ~DeviceGuard() { if (prev >= 0) (void)hipSetDevice(prev); }
    DeviceGuard(const DeviceGuard&) = delete;
    DeviceGuard& operator=(const DeviceGuard&) = delete;
};
#define AO_CHECK_ENV(env)                                                             \
    if (!(env)) return fail("null AoEnv");                                            \
    DeviceGuard ao_device_guard((env)->device);                                       \
    if (!ao_device_guard.ok) return fail("hipSetDevice(%d) failed", (env)->device)
// the ring tables of ONE layer: [A | B] (float64 [n_outer_l][n_inner_l + n_outer_l]) or the flat indices of its Z / X pixels
static int upload_layer_table(AoEnv* env, int kind, int l, const void* h, size_t bytes) {
    if (l < 0 || l >= env->L) return fail("layer %d outside [0, %d)", l, env->L);
    Layer& y = env->layer[l];
    const int S = y.S, N = y.N;
    auto need = [&](size_t n) { return bytes == n ? 0 : fail("ring table %d of layer %d: got %zu bytes, expected %zu", kind, l, bytes, n); };
    if (kind == AOENV_C_AB) {
        AO_TRY(need((size_t)y.nout * y.K * 8));
        for (int j = 0; j < env->L; ++j) forget_lookahead(env->layer[j]);   // a ring computed ahead used the old operators
        AO_TRY(upload_real(env, y.ab, static_cast<const double*>(h), (size_t)y.nout * y.K));
        y.have_ab = true;
        return 0;
    }
    if (kind != AOENV_C_INNER_IDX && kind != AOENV_C_OUTER_IDX) return fail("table %d is not a per-layer table", kind);
    const int cnt = kind == AOENV_C_INNER_IDX ? y.nin : y.nout;
    AO_TRY(need((size_t)cnt * 4));
    const int32_t* ix = static_cast<const int32_t*>(h);
    for (int i = 0; i < cnt; ++i)
        if (ix[i] < 0 || ix[i] >= S * S) return fail("ring index %d out of the %dx%d screen", ix[i], S, S);
    if (kind == AOENV_C_INNER_IDX)          // the gather reads idx - sy*S - sx with |s| <= 1
        for (int i = 0; i < cnt; ++i) {
            const int r = ix[i] / S, c = ix[i] % S;
            if (r < 1 || r > N || c < 1 || c > N) return fail("inner ring index %d is not interior", ix[i]);
        }
    AO_HIP(hipMemcpy(kind == AOENV_C_INNER_IDX ? y.inner_idx : y.outer_idx, h, (size_t)cnt * 4, hipMemcpyHostToDevice));
    (kind == AOENV_C_INNER_IDX ? y.have_in : y.have_out) = true;
    return 0;
}

template <typename T>
int atm_update_t(AoEnv* env, hipStream_t st) {
    AO_TRY(advance_atmosphere<T>(env, false, st));
    env->atm_user_defined = false;
    return run_phase<T>(env, 1, 1, st);
}

extern "C" {

const char* aoenv_last_error(void) { return g_err.c_str(); }
int aoenv_abi_version(void) { return AOENV_ABI_VERSION; }

int aoenv_create(const AoCfg* cfg, int device, AoEnv** out) {
    if (!cfg || !out) return fail("aoenv_create: null argument");
    if (cfg->abi_version != AOENV_ABI_VERSION) return fail("ABI version %d != %d", cfg->abi_version, AOENV_ABI_VERSION);
    if (cfg->dtype != AOENV_F32 && cfg->dtype != AOENV_F64) return fail("bad dtype %d", cfg->dtype);
    if (cfg->n_env < 1 || cfg->resolution < 2) return fail("bad n_env / resolution");
    if (cfg->n_layer < 0 || cfg->n_layer > kMaxLayer) return fail("n_layer %d out of range [0, %d]", cfg->n_layer, kMaxLayer);
    if (cfg->n_subap < 1 || cfg->resolution % cfg->n_subap) return fail("resolution %% n_subap != 0");
    if (cfg->n_layer > 0) {
        if (cfg->layer_res < cfg->resolution + 4) return fail("layer_res %d < R + 4", cfg->layer_res);
        if (cfg->n_inner != 8 * cfg->layer_res - 16 || cfg->n_outer != 4 * cfg->layer_res + 4)
            return fail("n_inner / n_outer do not match layer_res");
        for (int l = 0; l < cfg->n_layer; ++l)
            if (cfg->layer_res_l[l] != 0 && cfg->layer_res_l[l] < cfg->resolution + 4)
                return fail("layer_res_l[%d] = %d < R + 4", l, cfg->layer_res_l[l]);
    }
    if (cfg->n_signal != 2 * cfg->n_valid_subap) return fail("n_signal != 2 n_valid_subap");
    if (cfg->wfs_type != AOENV_WFS_SH && cfg->wfs_type != AOENV_WFS_PYRAMID && cfg->wfs_type != AOENV_WFS_SH_GEOMETRIC)
        return fail("unknown wfs_type %d", cfg->wfs_type);
    if (cfg->wfs_type == AOENV_WFS_SH_GEOMETRIC && cfg->cam_res < 1) return fail("geometric sensor: cam_res must be >= 1 (the frame is defined, and zero)");
    if (cfg->wfs_type == AOENV_WFS_PYRAMID) {
        if (cfg->pyr_n_res < cfg->resolution || cfg->pyr_n_res % 2 || cfg->cam_res < 1 || cfg->pyr_n_res % cfg->cam_res)
            return fail("pyramid: nRes %d must be even, >= R and a multiple of the camera size %d", cfg->pyr_n_res, cfg->cam_res);
        if (cfg->pyr_n_theta < 1) return fail("pyramid: n_theta must be >= 1");
        if (cfg->pyr_q_lo < 0 || cfg->pyr_q_hi + cfg->n_subap > cfg->cam_res) return fail("pyramid: quadrants outside the camera");
    }
    if (cfg->max_group < 1) return fail("max_group must be >= 1");
    int ndev = 0;
    AO_HIP(hipGetDeviceCount(&ndev));
    if (device < 0 || device >= ndev) return fail("device %d not in [0, %d)", device, ndev);
    DeviceGuard ao_device_guard(device);
    if (!ao_device_guard.ok) return fail("hipSetDevice(%d) failed", device);

    AoEnv* e = new (std::nothrow) AoEnv();
    if (!e) return fail("out of host memory");
    e->c = *cfg;
    e->device = device;
    e->esz = cfg->dtype == AOENV_F32 ? 4 : 8;
    e->R = cfg->resolution; e->A = cfg->n_valid_act; e->nAct = cfg->n_act; e->E = cfg->n_env; e->L = cfg->n_layer;
    e->nSig = cfg->n_signal; e->nSub = cfg->n_subap; e->nVal = cfg->n_valid_subap;
    e->p = e->R / e->nSub; e->n = 2 * e->p;
    e->layer[0].N = cfg->layer_res;                                // (the phase kernels' footprint without an atmosphere)
    e->layer[0].S = cfg->layer_res + 2;
    for (int l = 0; l < e->L; ++l) {
        Layer& y = e->layer[l];
        y.N = cfg->layer_res_l[l] ? cfg->layer_res_l[l] : cfg->layer_res;
        y.S = y.N + 2;
        y.nin = 8 * y.N - 16;
        y.nout = 4 * y.N + 4;
        y.K = y.nin + y.nout;
        y.scr_off = e->scr_elems;
        e->scr_elems += (size_t)e->E * y.S * y.S;
        e->Kmax = std::max(e->Kmax, y.K);
        e->noutmax = std::max(e->noutmax, y.nout);
        e->Smax = std::max(e->Smax, y.S);
        if (y.N != e->layer[0].N) e->uniform = false;
    }
    const size_t z = e->esz, E = e->E, R2 = (size_t)e->R * e->R;
    int rc = 0;
    auto A_ = [&](void** p, size_t bytes) { if (!rc) rc = dmalloc(e, p, bytes); };
    if (e->L > 0) {
        A_(&e->screen, e->scr_elems * z);
        A_(&e->minmax, (size_t)e->L * E * 2 * z);
        if (cfg->dtype == AOENV_F32) {                              // ring pipeline (fused float32 path)
            A_(&e->zx_pipe, (size_t)2 * e->L * E * e->Kmax * z);
        }
        A_(&e->zx, E * e->Kmax * z);
        A_(&e->xbuf, (size_t)e->L * kMaxSplits * E * e->noutmax * z);
        for (int l = 0; l < e->L; ++l) {
            Layer& y = e->layer[l];
            A_((void**)&y.mt_cur, E * kMtN * 4);
            A_((void**)&y.pos_cur, E * 4);
            A_((void**)&y.mt_alt, E * kMtN * 4);
            A_((void**)&y.pos_alt, E * 4);
            if (l > 0 && e->uniform) {                             // layers on one grid share one set of tables (non-uniform shards:
                y.ab = e->layer[0].ab;                             //  operators per layer -- r0 / L0 scale them alike, but the
                y.inner_idx = e->layer[0].inner_idx;               //  reference computes them per layer too when fov != 0)
                y.outer_idx = e->layer[0].outer_idx;
                continue;
            }
            A_(&y.ab, (size_t)y.nout * y.K * z);
            A_((void**)&y.inner_idx, (size_t)y.nin * 4);
            A_((void**)&y.outer_idx, (size_t)y.nout * 4);
        }
    }
    A_(&e->gx, (size_t)e->R * e->nAct * z);
    A_(&e->gy, (size_t)e->R * e->nAct * z);
    A_(&e->gxt, (size_t)((e->nAct + 3) & ~3) * (size_t)(cdiv(e->R, 128) * 128) * z);
    if (!cfg->dm_separable) {
        A_(&e->modes, R2 * e->A * z);
        A_(&e->dm_opd, E * R2 * z);
    }
    A_((void**)&e->act_idx, (size_t)e->A * 4);
    A_((void**)&e->pupil, R2);
    A_(&e->opd_atm, E * R2 * z);
    A_(&e->coefs, E * e->A * z);
    A_(&e->coefs_seen, E * e->A * z);                              // zero until a disturbed step writes it
    A_(&e->dm_prev, E * e->A * z);                                 // self.dm_prev = self.dm.coefs.copy() = 0 (OOPAOEnv.py:313-314)
    A_(&e->phase, E * R2 * z);
    if (cfg->wfs_type == AOENV_WFS_SH_GEOMETRIC) A_(&e->phase_np, E * R2 * z);
    A_(&e->scal, E * 4 * z);
    e->n_tiles = phase_tiles(e->R, e->nAct, e->esz);
    A_((void**)&e->part, E * (size_t)e->n_tiles * 4 * sizeof(double));
    A_(&e->total, (size_t)cfg->n_loop * E * z);
    A_(&e->residual, (size_t)cfg->n_loop * E * z);
    A_(&e->wfs_max, E * z);
    A_(&e->amp, R2 * z);
    A_((void**)&e->subap_idx, (size_t)e->nVal * 4);
    A_((void**)&e->valid2d, (size_t)e->nSub * e->nSub);
    A_((void**)&e->slot_of, (size_t)e->nSub * e->nSub * sizeof(short));
    A_((void**)&e->amp_pupil, R2 * sizeof(float));
    e->ga_stride = dm_ga_stride(e->nAct);
    A_((void**)&e->gxa, (size_t)(cdiv(e->R, 128) * 128) * 4 * e->ga_stride * sizeof(float));
    A_((void**)&e->gya, (size_t)(cdiv(e->R, 128) * 128) * 4 * e->ga_stride * sizeof(float));
    if (e->A > 1024 && !rc) { rc = alloc_dm_rows(e); e->use_coefs_img = true; }
    A_(&e->sh_ref, (size_t)2 * e->nVal * z);
    A_(&e->tw, (size_t)e->n * 2 * z);
    A_(&e->phs, (size_t)e->p * 2 * z);
    A_(&e->frame, E * (size_t)cfg->cam_res * cfg->cam_res * z);
    A_(&e->signal, E * e->nSig * z);
    A_(&e->recon, (size_t)e->A * e->nSig * z);
    A_(&e->fac_m, (size_t)kMaxModes * e->nSig * z);
    A_(&e->fac_m2c_t, (size_t)kMaxModes * e->A * z);
    if (cfg->wfs_type == AOENV_WFS_PYRAMID) {
        const size_t N = cfg->pyr_n_res;
        e->pyr_chunk = cfg->pyr_n_theta < 4 ? cfg->pyr_n_theta : 4;
        A_(&e->pyr_mask, N * N * 2 * z);
        A_(&e->pyr_tt, (size_t)cfg->pyr_n_theta * R2 * z);
        A_(&e->pyr_tw, N * 2 * z);
        A_(&e->pyr_t1, E * e->pyr_chunk * (size_t)e->R * N * 2 * z);
        A_(&e->pyr_t2, E * e->pyr_chunk * N * N * 2 * z);
    }
    A_(&e->vbuf, (size_t)kMaxSplits * E * e->A * z);
    {
        const PoissonAliasHost& ph = poisson_alias_host();
        int budget = (int)ph.tab.size();
        if (cfg->wfs_type == AOENV_WFS_SH && e->p == fast6::P && e->R <= 128 && e->nAct <= 32) budget = std::min(budget, step_alias_capacity(e->nAct));
        ph.prefix(budget, &e->alias_words, &e->alias_lmax);
        if (e->alias_lmax < palias::kCoarseStep && !rc) rc = fail("aoenv_create: no room for the photon-noise tables");
        A_((void**)&e->alias_tab, ph.tab.size() * 4);
        if (!rc && hipMemcpy(e->alias_tab, ph.tab.data(), ph.tab.size() * 4, hipMemcpyHostToDevice) != hipSuccess)
            rc = fail("aoenv_create: upload of the photon-noise tables failed");
    }
    if (rc) { aoenv_destroy(e); return rc; }
    // DFT twiddles w^k = exp(-2 pi i k / n) and the centring phasor exp(-i pi (n+1)/n x) at x = a + lo
    // (OOPAO/ShackHartmann.py:208-209), in float64 then converted
    if (cfg->wfs_type == AOENV_WFS_SH) {
        const int n = e->n, p = e->p, lo = n / 2 - p / 2;
        std::vector<double> tw(2 * n), ph(2 * p);
        const double pi = 3.14159265358979323846;
        for (int k = 0; k < n; ++k) { tw[2 * k] = std::cos(2 * pi * k / n); tw[2 * k + 1] = -std::sin(2 * pi * k / n); }
        for (int a = 0; a < p; ++a) {
            const double ang = pi * (n + 1) / n * (a + lo);
            ph[2 * a] = std::cos(ang); ph[2 * a + 1] = -std::sin(ang);
        }
        rc = upload_real(e, e->tw, tw.data(), tw.size());
        if (!rc) rc = upload_real(e, e->phs, ph.data(), ph.size());
        if (rc) { aoenv_destroy(e); return rc; }
    }
    if (cfg->wfs_type == AOENV_WFS_PYRAMID) {
        const int N = cfg->pyr_n_res;
        rc = make_fft_plan(N, &e->pyr_plan);
        std::vector<double> tw(2 * (size_t)N);
        const double pi = 3.14159265358979323846;
        for (int k = 0; k < N; ++k) { tw[2 * k] = std::cos(2 * pi * k / N); tw[2 * k + 1] = -std::sin(2 * pi * k / N); }
        if (!rc) rc = upload_real(e, e->pyr_tw, tw.data(), tw.size());
        if (rc) { aoenv_destroy(e); return rc; }
    }
    *out = e;
    return 0;
}

int aoenv_upload_layer(AoEnv* env, int kind, int layer, const void* h, size_t bytes) {
    AO_CHECK_ENV(env);
    if (!h) return fail("aoenv_upload_layer: null data");
    if (env->L == 0) return fail("no atmosphere in this shard");
    return upload_layer_table(env, kind, layer, h, bytes);
}

int aoenv_destroy(AoEnv* env) {
    if (!env) return 0;
    DeviceGuard ao_device_guard(env->device);
    for (auto& e : env->prof_ev) { (void)hipEventDestroy(e.a); (void)hipEventDestroy(e.b); }
    delete env;                                                    // every block frees itself, on the env's device
    return 0;
}

int aoenv_upload(AoEnv* env, int kind, const void* h, size_t bytes) {
    AO_CHECK_ENV(env);
    if (!h) return fail("aoenv_upload: null data");
    const size_t R2 = (size_t)env->R * env->R;
    auto need = [&](size_t n) { return bytes == n ? 0 : fail("aoenv_upload(kind=%d): got %zu bytes, expected %zu", kind, bytes, n); };
    const double* d = static_cast<const double*>(h);
    switch (kind) {
        case AOENV_C_PUPIL: {
            AO_TRY(need(R2));
            AO_HIP(hipMemcpy(env->pupil, h, R2, hipMemcpyHostToDevice));
            const uint8_t* pu = static_cast<const uint8_t*>(h);
            env->h_pupil.assign(pu, pu + R2);
            env->amp_pupil_dirty = true;
            env->n_pupil = 0;
            for (size_t i = 0; i < R2; ++i) env->n_pupil += pu[i] != 0;
            env->wf = AoEnv::Wavefront{};                           // a wavefront basis is indexed by the pupil's pixels
            env->sci = AoEnv::Science{};                            // ... and the science camera looks through it
            break;
        }
        case AOENV_C_AB:
        case AOENV_C_INNER_IDX:
        case AOENV_C_OUTER_IDX:
            // one set of ring tables for every layer: shards whose layers share one grid (fov = 0, or no layer above the ground)
            if (env->L == 0) return fail("no atmosphere in this shard");
            if (!env->uniform) return fail("the layers of this shard have grids of their own: upload the ring tables per layer (aoenv_upload_layer)");
            AO_TRY(upload_layer_table(env, kind, 0, h, bytes));
            for (int l = 1; l < env->L; ++l) {
                Layer& y = env->layer[l];
                (kind == AOENV_C_AB ? y.have_ab : kind == AOENV_C_INNER_IDX ? y.have_in : y.have_out) = true;
            }
            break;
        case AOENV_C_LAYER_WEIGHT:
            AO_TRY(need((size_t)env->L * 8));
            for (int l = 0; l < env->L; ++l) env->layer[l].weight = d[l];
            break;
        case AOENV_C_DM_GX:
        case AOENV_C_DM_GY:
            AO_TRY(need((size_t)env->R * env->nAct * 8));
            AO_TRY(upload_real(env, kind == AOENV_C_DM_GX ? env->gx : env->gy, d, (size_t)env->R * env->nAct));
            {                                                      // the other layouts of the table (dm_tables.hpp)
                const DmLayout dl = env->dm_layout();
                std::vector<float> t(dl.ga_elems());               // MFMA operand layout (float32 kernels): zero padded
                dm_fill_ga(dl, d, t.data());
                AO_HIP(hipMemcpy(kind == AOENV_C_DM_GX ? env->gxa : env->gya, t.data(), t.size() * sizeof(float), hipMemcpyHostToDevice));
                if (kind == AOENV_C_DM_GX) {
                    std::vector<double> tt(dl.gxt_elems());
                    dm_fill_gxt<double>(dl, d, tt.data());
                    AO_TRY(upload_real(env, env->gxt, tt.data(), tt.size()));
                }
            }
            break;
        case AOENV_C_DM_MODES:
            if (env->c.dm_separable) return fail("dense modes uploaded to a separable-DM shard");
            AO_TRY(need(R2 * env->A * 8));
            AO_TRY(upload_real(env, env->modes, d, R2 * env->A));
            break;
        case AOENV_C_ACT_IDX: {
            AO_TRY(need((size_t)env->A * 4));
            const int32_t* ix = static_cast<const int32_t*>(h);
            for (int i = 0; i < env->A; ++i)
                if (ix[i] < 0 || ix[i] >= env->nAct * env->nAct) return fail("actuator index %d out of range", ix[i]);
            AO_HIP(hipMemcpy(env->act_idx, h, (size_t)env->A * 4, hipMemcpyHostToDevice));
            env->h_act_idx.assign(ix, ix + env->A);
            env->act_slot_dirty = true;
            break;
        }
        case AOENV_C_WFS_AMP:
            AO_TRY(need(R2 * 8));
            AO_TRY(upload_real(env, env->amp, d, R2));
            env->h_amp.assign(d, d + R2);
            env->amp_pupil_dirty = true;
            env->sci = AoEnv::Science{};                            // the science camera holds a copy of the amplitude
            break;
        case AOENV_C_SH_SUBAP_IDX: {
            AO_TRY(need((size_t)env->nVal * 4));
            const int32_t* ix = static_cast<const int32_t*>(h);
            for (int i = 0; i < env->nVal; ++i)
                if (ix[i] < 0 || ix[i] >= env->nSub * env->nSub) return fail("lenslet index %d out of range", ix[i]);
            if (env->geometric() && env->nVal > 32767) return fail("geometric sensor: %d valid lenslets, at most 32767", env->nVal);
            AO_HIP(hipMemcpy(env->subap_idx, h, (size_t)env->nVal * 4, hipMemcpyHostToDevice));
            std::vector<uint8_t> v2((size_t)env->nSub * env->nSub, 0);
            for (int i = 0; i < env->nVal; ++i) v2[ix[i]] = 1;
            AO_HIP(hipMemcpy(env->valid2d, v2.data(), v2.size(), hipMemcpyHostToDevice));
            std::vector<short> so((size_t)env->nSub * env->nSub, (short)-1);
            if (env->nVal <= 32767)
                for (int i = 0; i < env->nVal; ++i) so[ix[i]] = (short)i;
            AO_HIP(hipMemcpy(env->slot_of, so.data(), so.size() * sizeof(short), hipMemcpyHostToDevice));
            break;
        }
        case AOENV_C_SH_REF:
            AO_TRY(need((size_t)2 * env->nVal * 8));
            AO_TRY(upload_real(env, env->sh_ref, d, (size_t)2 * env->nVal));
            break;
        case AOENV_C_WFS_UNITS:
            AO_TRY(need(8));
            if (!(d[0] != 0)) return fail("slopes units must be non-zero");
            env->units = d[0];
            break;
        case AOENV_C_RECON:
            AO_TRY(need((size_t)env->A * env->nSig * 8));
            AO_TRY(upload_real(env, env->recon, d, (size_t)env->A * env->nSig));
            env->n_modes = 0;                                      // factors must be re-uploaded for a new R
            break;
        case AOENV_C_RECON_FACTORS: {
            // [K*nSig] M then [A*K] M2C, K from the size
            const size_t per = (size_t)env->nSig + env->A;
            if (bytes % (8 * per)) return fail("aoenv_upload(RECON_FACTORS): %zu bytes is not K*(nSig+A) doubles", bytes);
            const int K = (int)(bytes / (8 * per));
            if (K < 1 || K > kMaxModes) return fail("reconstructor rank %d outside [1, %d]", K, kMaxModes);
            AO_TRY(upload_real(env, env->fac_m, d, (size_t)K * env->nSig));
            const double* m2c = d + (size_t)K * env->nSig;
            AO_TRY(upload_transposed(env, env->fac_m2c_t, m2c, env->A, K));
            // the same factors for the batched (non-fused) reconstruction: M with zero rows up to Kp, M2C as [A][Kp]
            const int Kp = (K + 3) & ~3;
            if ((size_t)Kp > env->fac_cap) {
                AO_TRY(block_alloc(env->fac_mem, {(size_t)env->A * Kp * env->esz, (size_t)kMaxSplits * env->E * Kp * env->esz}, true));
                env->fac_m2c = env->fac_mem.part(0);
                env->tbuf = env->fac_mem.part(1);
                env->fac_cap = (size_t)Kp;
            }
            if (Kp > K && Kp <= kMaxModes)
                AO_HIP(hipMemset(static_cast<char*>(env->fac_m) + (size_t)K * env->nSig * env->esz, 0, (size_t)(Kp - K) * env->nSig * env->esz));
            std::vector<double> mp((size_t)env->A * Kp, 0.0);
            for (int a = 0; a < env->A; ++a)
                for (int k = 0; k < K; ++k) mp[(size_t)a * Kp + k] = m2c[(size_t)a * K + k];
            AO_TRY(upload_real(env, env->fac_m2c, mp.data(), mp.size()));
            env->n_modes = K;
            break;
        }
        case AOENV_C_PYR_MASK: {
            if (env->c.wfs_type != AOENV_WFS_PYRAMID) return fail("not a pyramid shard");
            const size_t n = (size_t)env->c.pyr_n_res * env->c.pyr_n_res * 2;
            AO_TRY(need(n * 8));
            AO_TRY(upload_real(env, env->pyr_mask, d, n));
            break;
        }
        case AOENV_C_PYR_TT: {
            if (env->c.wfs_type != AOENV_WFS_PYRAMID) return fail("not a pyramid shard");
            const size_t n = (size_t)env->c.pyr_n_theta * R2;
            AO_TRY(need(n * 8));
            AO_TRY(upload_real(env, env->pyr_tt, d, n));
            break;
        }
        default: return fail("unknown constant id %d", kind);
    }
    env->have[kind] = true;
    return 0;
}

// ---- per-env clocks -----------------------------------------------------------------------------------------------------
static int alloc_env_clocks(AoEnv* env) {
    if (env->env_taps) return 0;
    const size_t n = (size_t)env->L * env->E;
    for (int b = 0; b < 2; ++b) AO_TRY(dmalloc(env, (void**)&env->env_clk[b], n * sizeof(EnvClock), false));
    return dmalloc(env, (void**)&env->env_taps, n * sizeof(LayerTaps), false);
}

// host copy of the clocks -> device (current buffer) + the taps they imply (no ring pending), and every layer's round count
static int push_env_clocks(AoEnv* env, const std::vector<EnvClock>& clk) {
    const size_t n = (size_t)env->L * env->E;
    std::vector<LayerTaps> taps(n);
    for (int l = 0; l < env->L; ++l) {
        env->layer[l].env_rounds = 0;                              // (the host holds every ratio here)
        for (int e = 0; e < env->E; ++e) {
            const EnvClock& c = clk[(size_t)l * env->E + e];
            int sx, sy;
            env->layer[l].env_rounds = std::max(env->layer[l].env_rounds, clock_rounds(c.ratio, 0, &sx, &sy));
            LayerTaps& t = taps[(size_t)l * env->E + e];
            t = LayerTaps{};
            t.oy = c.org[0];
            t.ox = c.org[1];
            taps_from_buff(c.buff, t);
            t.weight = env->layer[l].weight;
        }
    }
    AO_HIP(hipMemcpy(env->env_clk[env->clk_cur], clk.data(), n * sizeof(EnvClock), hipMemcpyHostToDevice));
    AO_HIP(hipMemcpy(env->env_taps, taps.data(), n * sizeof(LayerTaps), hipMemcpyHostToDevice));
    return 0;
}

static int pull_env_clocks(AoEnv* env, std::vector<EnvClock>& clk) {
    clk.resize((size_t)env->L * env->E);
    AO_HIP(hipMemcpy(clk.data(), env->env_clk[env->clk_cur], clk.size() * sizeof(EnvClock), hipMemcpyDeviceToHost));
    return 0;
}

int aoenv_set_wind_env(AoEnv* env, const double* h_ratio, int reset_buff, void* stream) {
    AO_CHECK_ENV(env);
    if (!h_ratio) return fail("null ratio");
    if (!env->uniform)
        return fail("aoenv_set_wind_env: layers on grids of their own (AoCfg.layer_res_l: fov != 0 with altitude layers) have no per-env clocks; "
                    "one wind for the shard (aoenv_set_wind)");
    const size_t n = (size_t)env->L * env->E;
    for (size_t i = 0; i < 2 * n; ++i)
        if (!(std::fabs(h_ratio[i]) < (double)env->wind_pixels))
            return fail("per-env wind: |ratio| = %g px/frame, must be < %d (%s)", std::fabs(h_ratio[i]), env->wind_pixels,
                        env->wind_pixels == 1 ? "an env extrudes at most one ring per step" : "AOENV_OPT_ENV_WIND_PIXELS");
    hipStream_t st = static_cast<hipStream_t>(stream);
    for (int l = 0; l < env->L; ++l) forget_lookahead(env->layer[l]);
    AO_TRY(AO_DISPATCH(env, flush_rings, env, st));                // a deferred ring of the clocks as they were
    AO_HIP(hipStreamSynchronize(st));
    AO_TRY(alloc_env_clocks(env));
    std::vector<EnvClock> clk;
    if (env->per_env_wind) {
        AO_TRY(pull_env_clocks(env, clk));
    } else {                                                       // from the shared clock: every env starts where the shard is
        clk.assign(n, EnvClock{});
        for (int l = 0; l < env->L; ++l)
            for (int e = 0; e < env->E; ++e) {
                EnvClock& c = clk[(size_t)l * env->E + e];
                const Layer& y = env->layer[l];
                c.buff[0] = y.clk.buff[0];
                c.buff[1] = y.clk.buff[1];
                c.org[0] = y.org[0];
                c.org[1] = y.org[1];
            }
    }
    for (size_t i = 0; i < n; ++i) {
        clk[i].ratio[0] = h_ratio[2 * i];
        clk[i].ratio[1] = h_ratio[2 * i + 1];
        if (reset_buff) clk[i].buff[0] = clk[i].buff[1] = 0;
    }
    env->per_env_wind = true;
    return push_env_clocks(env, clk);
}

int aoenv_get_clock_env(AoEnv* env, double* h_clock) {
    AO_CHECK_ENV(env);
    if (!h_clock) return fail("null argument");
    if (!env->per_env_wind) return fail("the shard runs the shared clock (aoenv_set_wind): use aoenv_get_buff");
    AO_HIP(hipDeviceSynchronize());
    std::vector<EnvClock> clk;
    AO_TRY(pull_env_clocks(env, clk));
    for (size_t i = 0; i < clk.size(); ++i) {
        h_clock[4 * i] = clk[i].ratio[0];
        h_clock[4 * i + 1] = clk[i].ratio[1];
        h_clock[4 * i + 2] = clk[i].buff[0];
        h_clock[4 * i + 3] = clk[i].buff[1];
    }
    return 0;
}

int aoenv_set_clock_env(AoEnv* env, const double* h_clock) {
    AO_CHECK_ENV(env);
    if (!h_clock) return fail("null argument");
    if (!env->per_env_wind) return fail("the shard runs the shared clock (aoenv_set_wind): use aoenv_set_buff");
    AO_HIP(hipDeviceSynchronize());
    std::vector<EnvClock> clk;
    AO_TRY(pull_env_clocks(env, clk));                             // (keeps the origins)
    for (size_t i = 0; i < clk.size(); ++i) {
        for (int d = 0; d < 2; ++d) {
            if (!(std::fabs(h_clock[4 * i + d]) < (double)env->wind_pixels)) return fail("per-env wind: |ratio| must be < %d px/frame", env->wind_pixels);
            if (!(std::fabs(h_clock[4 * i + 2 + d]) < 1.0)) return fail("|buff| must be < 1");
            clk[i].ratio[d] = h_clock[4 * i + d];
            clk[i].buff[d] = h_clock[4 * i + 2 + d];
        }
    }
    for (int l = 0; l < env->L; ++l) drop_ring(env->layer[l]);     // (aoenv_set_wind_env scatters it first instead)
    return push_env_clocks(env, clk);
}

// every env's clock back to the start of an episode: accumulators and origins zero (new screens / uploaded screens)
static int reset_env_clocks(AoEnv* env, bool reset_buff) {
    if (!env->per_env_wind) return 0;
    std::vector<EnvClock> clk;
    AO_TRY(pull_env_clocks(env, clk));
    for (auto& c : clk) {
        c.org[0] = c.org[1] = 0;
        if (reset_buff) c.buff[0] = c.buff[1] = 0;
    }
    return push_env_clocks(env, clk);
}

// The screens are replaced (new screens, an uploaded state): every torus restarts at origin 0; a deferred ring and a look-ahead of
// the old screens are moot; the min / max tables are stale.  reset_buff: the sub-pixel accumulators of the clocks restart too
// (notDoneOnce, OOPAO/Atmosphere.py:586, 359-364), else they are kept.
static int screens_replaced(AoEnv* env, bool reset_buff) {
    for (int l = 0; l < env->L; ++l) {
        Layer& y = env->layer[l];
        y.org[0] = y.org[1] = 0;
        drop_ring(y);
        forget_lookahead(y);
        y.minmax_dirty = true;
        if (reset_buff) y.clk.buff[0] = y.clk.buff[1] = 0;
    }
    env->atm_user_defined = false;
    return reset_env_clocks(env, reset_buff);
}

// one wind per layer ([L][2]) as the [L][E][2] of aoenv_set_wind_env: the same wind for every env
static std::vector<double> wind_for_every_env(const AoEnv* env, const double* ratio) {
    std::vector<double> r((size_t)env->L * env->E * 2);
    for (int l = 0; l < env->L; ++l)
        for (int e = 0; e < env->E; ++e) {
            r[2 * ((size_t)l * env->E + e)] = ratio[2 * l];
            r[2 * ((size_t)l * env->E + e) + 1] = ratio[2 * l + 1];
        }
    return r;
}

int aoenv_set_wind(AoEnv* env, const double* h_ratio, int reset_buff) {
    AO_CHECK_ENV(env);
    if (!h_ratio) return fail("null ratio");
    if (env->per_env_wind) {                                       // the shard keeps its per-env clocks: the same wind for every env
        const std::vector<double> r = wind_for_every_env(env, h_ratio);
        // (this entry point has no stream argument: the caller may be stepping on a non-blocking stream, whose pending ring /
        //  clock work must be through before the clocks are pulled, changed and pushed back on the null stream)
        AO_HIP(hipDeviceSynchronize());
        return aoenv_set_wind_env(env, r.data(), reset_buff, nullptr);
    }
    for (int l = 0; l < env->L; ++l) {
        LayerClock& k = env->layer[l].clk;
        k.ratio[0] = h_ratio[2 * l];
        k.ratio[1] = h_ratio[2 * l + 1];
        if (reset_buff) k.buff[0] = k.buff[1] = 0;
    }
    return 0;
}

// ---- per-env Fried parameter -------------------------------------------------------------------------------------------
int aoenv_set_r0_env(AoEnv* env, const double* h_r0, double r0_tables, void* stream) {
    AO_CHECK_ENV(env);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (!h_r0) {                                                   // back to one r0 for the shard
        if (!env->per_env_r0) return 0;
        for (int l = 0; l < env->L; ++l) forget_lookahead(env->layer[l]);   // drawn with the sigma that is going away
        env->per_env_r0 = false;
        env->h_r0.clear();
        return 0;
    }
    if (!(r0_tables > 0) || !std::isfinite(r0_tables)) return fail("aoenv_set_r0_env: r0_tables = %g, must be positive and finite", r0_tables);
    const size_t E = (size_t)env->E;
    for (size_t e = 0; e < E; ++e)
        if (!(h_r0[e] > 0) || !std::isfinite(h_r0[e])) return fail("aoenv_set_r0_env: r0[%zu] = %g, must be positive and finite", e, h_r0[e]);
    std::vector<double> sg(E);
    for (size_t e = 0; e < E; ++e) sg[e] = std::pow(r0_tables / h_r0[e], 5.0 / 6);
    if (!env->xi_scale) AO_TRY(dmalloc(env, (void**)&env->xi_scale, E * sizeof(double), false));
    // ordered on the stream behind the launches that read the old factors (a deferred ring was computed from them and is scattered
    // as it is)
    AO_HIP(hipMemcpyAsync(env->xi_scale, sg.data(), E * sizeof(double), hipMemcpyHostToDevice, st));
    AO_HIP(hipStreamSynchronize(st));
    for (int l = 0; l < env->L; ++l) forget_lookahead(env->layer[l]);       // an operand drawn ahead carries the old sigma
    env->h_r0.assign(h_r0, h_r0 + E);
    env->per_env_r0 = true;
    return 0;
}

int aoenv_get_r0_env(AoEnv* env, double* h_r0) {
    AO_CHECK_ENV(env);
    if (!h_r0) return fail("null argument");
    if (!env->per_env_r0) return fail("the shard has one r0 for all envs (aoenv_set_r0_env has not been called, or was cleared)");
    std::copy(env->h_r0.begin(), env->h_r0.end(), h_r0);
    return 0;
}

static int require_step_constants(AoEnv* env, bool atmosphere) {
    static const int base[] = {AOENV_C_PUPIL, AOENV_C_ACT_IDX, AOENV_C_WFS_AMP, AOENV_C_SH_SUBAP_IDX};
    for (int k : base)
        if (!env->have[k] && !(k == AOENV_C_WFS_AMP && env->geometric())) return fail("constant table %d has not been uploaded", k);
    if (env->c.dm_separable ? !(env->have[AOENV_C_DM_GX] && env->have[AOENV_C_DM_GY]) : !env->have[AOENV_C_DM_MODES])
        return fail("DM influence functions have not been uploaded");
    if (atmosphere && env->L > 0) {
        if (!env->have[AOENV_C_LAYER_WEIGHT]) return fail("atmosphere table %d has not been uploaded", (int)AOENV_C_LAYER_WEIGHT);
        for (int l = 0; l < env->L; ++l)
            if (!env->layer[l].have_ab || !env->layer[l].have_in || !env->layer[l].have_out) return fail("the ring tables of layer %d have not been uploaded", l);
    }
    return 0;
}

namespace {
// host arrays of 32-bit words (an index list, seeds) back to back in one scratch buffer, in one upload
int upload_words(TmpFree& tmp, std::initializer_list<std::pair<const void*, size_t>> parts, uint32_t** d_out) {
    std::vector<uint32_t> pack;
    for (const auto& p : parts) pack.insert(pack.end(), static_cast<const uint32_t*>(p.first), static_cast<const uint32_t*>(p.first) + p.second);
    AO_TRY(tmp.get({pack.size() * 4}));
    *d_out = tmp.part<uint32_t>(0);
    AO_HIP(hipMemcpy(*d_out, pack.data(), pack.size() * 4, hipMemcpyHostToDevice));
    return 0;
}

// Per-env Fried parameter: the factor of the new screens of the n envs of a reset generated at `r0`, (r0 / r0_e)^(5/6) in float64
// (the generator's amplitudes go as r0^(-5/6), vk_psd); row c belongs to env idx[c], or env c without a list.  Empty while the
// shard has one r0.
void screen_factors(const AoEnv* env, const int32_t* idx, int n, double r0, std::vector<double>& f) {
    f.clear();
    if (!env->per_env_r0) return;
    f.resize((size_t)n);
    for (int c = 0; c < n; ++c) f[c] = std::pow(r0 / env->h_r0[idx ? idx[c] : c], 5.0 / 6);
}
}  // namespace

extern "C++" {
// ring RandomState seeding, first ring X = A.Z + B.xi, atm.OPD: the part of generateNewPhaseScreen after the new interior is in
// mapShift (OOPAO/Atmosphere.py:579-592), for the n envs of the device list d_idx (null: the whole shard); d_ring_seeds is [n][L].
// The callers have put those envs at origin 0 with an empty accumulator (screens_replaced / k_reset_env_rows).
template <typename T>
static int finish_new_screens(AoEnv* env, const int* d_idx, int n, const uint32_t* d_ring_seeds, hipStream_t st) {
    for (int l = 0; l < env->L; ++l) {
        AO_TRY(launch_mt_seed(d_ring_seeds + l, env->L, d_idx, env->layer[l].mt_cur, env->layer[l].pos_cur, n, st));
        AO_TRY(first_ring<T>(env, l, d_idx, n, st));
    }
    env->atm_user_defined = false;
    return run_phase<T>(env, 1, 1, st);                            // fill_phase_support + set_OPD + atm*tel, from the screens as they are now
}
}  // extern "C++"

int aoenv_new_screens(AoEnv* env, const double* h_screens, const uint32_t* h_ring_seeds, void* stream) {
    AO_CHECK_ENV(env);
    if (env->L == 0) return fail("no atmosphere in this shard");
    AO_TRY(require_step_constants(env, true));
    if (!h_ring_seeds) return fail("null ring seeds");
    hipStream_t st = static_cast<hipStream_t>(stream);
    AO_HIP(hipStreamSynchronize(st));
    const int E = env->E, L = env->L;
    if (!h_screens) {
        if (env->per_env_wind) return fail("per-env clocks: the interior cannot be kept (every env has moved its own origin): hand the screens over");
        for (int l = 0; l < L; ++l)
            if (env->layer[l].org[0] || env->layer[l].org[1]) return fail("keeping the interior is only possible before the first shift");
    }
    AO_TRY(screens_replaced(env, true));
    if (h_screens) {
        // mapShift[~outerMask] = phase  (OOPAO/Atmosphere.py:585); the ring is drawn below
        std::vector<char> host;
        size_t layer_base = 0;                                     // (layers with grids of their own: layer-major blocks)
        for (int l = 0; l < L; ++l) {
            const int N = env->layer[l].N, S = env->layer[l].S;
            host.assign((size_t)E * S * S * env->esz, 0);
            for (int e = 0; e < E; ++e) {
                const double* src = env->uniform ? h_screens + ((size_t)e * L + l) * N * N : h_screens + layer_base + (size_t)e * N * N;
                for (int r = 0; r < N; ++r)
                    for (int c = 0; c < N; ++c) {
                        const size_t o = (size_t)e * S * S + (size_t)(r + 1) * S + (c + 1);
                        if (env->esz == 4) reinterpret_cast<float*>(host.data())[o] = (float)src[(size_t)r * N + c];
                        else reinterpret_cast<double*>(host.data())[o] = src[(size_t)r * N + c];
                    }
            }
            AO_HIP(hipMemcpy(env->screen_ptr(l), host.data(), host.size(), hipMemcpyHostToDevice));
            layer_base += (size_t)E * N * N;
        }
    }
    TmpFree tmp;
    uint32_t* d_ring_seeds = nullptr;
    AO_TRY(upload_words(tmp, {{h_ring_seeds, (size_t)E * L}}, &d_ring_seeds));
    return AO_DISPATCH(env, finish_new_screens, env, nullptr, E, d_ring_seeds, st);
}

namespace {
// von Karman spectrum of OOPAO/phaseStats.py:206-207 (l0 = 1e-10 m: the inner-scale roll-off is 1 in float64)
double vk_psd(double f, double r0, double L0) {
    const double fm = 5.92 / 1e-10 / (2 * 3.14159265358979323846), f0 = 1.0 / L0;
    return 0.023 * std::pow(r0, -5.0 / 3) * std::exp(-((f / fm) * (f / fm))) / std::pow(f * f + f0 * f0, 11.0 / 6);
}

// Tables and scratch of the device screen generator for one grid size N and up to n_env envs at a time (chunks of `ec`)
struct ScreenGen {
    ScreenArgs sa{};
    uint32_t* mt = nullptr;                        // [ec][624] the layers' own RandomState(seed + layer) ...
    int* pos = nullptr;                            // [ec]
    int ec = 1;
};
int make_screen_gen(TmpFree& tmp, int N, int n_env, double r0, double L0, double pixel_size, ScreenGen* g) {
    const double pi = 3.14159265358979323846;
    const size_t N2 = (size_t)N * N;
    // frequency-grid amplitude sqrt(PSD) del_f (phaseStats.py:209-222) and the 3 x 4 sub-harmonic terms (:277-309)
    std::vector<double> amp(N2), sub(36), tw(2 * (size_t)N);
    const double del_f = 1.0 / (N * pixel_size);
    for (int y = 0; y < N; ++y)
        for (int x = 0; x < N; ++x) {
            const double fx = (x - N / 2.0) * del_f, fy = (y - N / 2.0) * del_f;
            amp[(size_t)y * N + x] = std::sqrt(vk_psd(std::sqrt(fx * fx + fy * fy), r0, L0)) * del_f;
        }
    amp[(size_t)(N / 2) * N + N / 2] = 0;
    const double D = N * pixel_size;
    for (int p = 1; p <= 3; ++p) {
        const double df = 1.0 / (std::pow(3.0, p) * D);
        for (int i = 0; i < 2; ++i)
            for (int j = 0; j < 2; ++j) {
                const double fx = (j - 1) * df, fy = (i - 1) * df;
                double* t = &sub[3 * (4 * (p - 1) + 2 * i + j)];
                t[0] = (i == 1 && j == 1) ? 0.0 : std::sqrt(vk_psd(std::sqrt(fx * fx + fy * fy), r0, L0)) * df;
                t[1] = fx;
                t[2] = fy;
            }
    }
    for (int k = 0; k < N; ++k) { tw[2 * k] = std::cos(2 * pi * k / N); tw[2 * k + 1] = -std::sin(2 * pi * k / N); }
    ScreenArgs& sa = g->sa;
    sa = ScreenArgs{};
    AO_TRY(make_fft_plan(N, &sa.plan));
    sa.N = N;
    sa.delta = pixel_size;
    const size_t per_env = 40 * N2;                                // normals + complex scratch + real screen, float64
    const int EC = g->ec = (int)std::min<size_t>((size_t)n_env, std::max<size_t>(1, ((size_t)1 << 30) / per_env));
    AO_TRY(tmp.get({N2 * 8, 36 * 8, 2 * (size_t)N * 8, (size_t)EC * 2 * N2 * 8, (size_t)EC * N2 * 16, (size_t)EC * N2 * 8, (size_t)EC * kMtN * 4,
                    (size_t)EC * 4}));
    double *d_amp = tmp.part<double>(0), *d_sub = tmp.part<double>(1), *d_tw = tmp.part<double>(2);
    AO_HIP(hipMemcpy(d_amp, amp.data(), N2 * 8, hipMemcpyHostToDevice));
    AO_HIP(hipMemcpy(d_sub, sub.data(), 36 * 8, hipMemcpyHostToDevice));
    AO_HIP(hipMemcpy(d_tw, tw.data(), tw.size() * 8, hipMemcpyHostToDevice));
    sa.amp = d_amp; sa.sub = d_sub; sa.tw = d_tw; sa.nrm = tmp.part<double>(3); sa.hi = tmp.part<double>(5);
    sa.scratch = tmp.part<cx<double>>(4);
    g->mt = tmp.part<uint32_t>(6);
    g->pos = tmp.part<int>(7);
    return 0;
}
}  // namespace

extern "C++" {
// New interiors (OOPAO/Atmosphere.py:568-578) for the n envs of the device list d_idx (null: env c is row c, the whole shard), every
// layer: RandomState(seed + layer) seeded on the device from d_screen_seeds [n][L], normal(size=(N, N)) drawn twice (real, imaginary
// parts), the screen written into the env's map.  The generator works on a compact scratch of at most g.ec envs, reused chunk after
// chunk in stream order (no host wait in between); its tables are rebuilt whenever a layer is on a grid of another size.
// d_scale [n] (per-env Fried parameter, else null): the finished float64 screen of row c is multiplied by d_scale[c].
template <typename T>
static int draw_screens(AoEnv* env, const int* d_idx, int n, const uint32_t* d_screen_seeds, const double* d_scale, double r0, double L0,
                        double pixel_size, TmpFree& tmp, hipStream_t st) {
    const int L = env->L;
    ScreenGen g;
    for (int l = 0; l < L; ++l) {
        const int N = env->layer[l].N, S = env->layer[l].S;
        const int n2 = 2 * N * N;
        if (N != g.sa.N) AO_TRY(make_screen_gen(tmp, N, n, r0, L0, pixel_size, &g));   // (every layer's tables when fov = 0)
        for (int c0 = 0; c0 < n; c0 += g.ec) {
            const int nc = std::min(g.ec, n - c0);
            AO_TRY(launch_mt_seed(d_screen_seeds + (size_t)c0 * L + l, L, nullptr, g.mt, g.pos, nc, st));
            AO_TRY(launch_mt_normal<double>(g.mt, g.pos, const_cast<double*>(g.sa.nrm), nc, n2, 0, n2, nullptr, st));
            g.sa.n_env = nc;
            g.sa.scale = d_scale ? d_scale + c0 : nullptr;
            T* map = env->as<T>(env->screen_ptr(l));
            if (d_idx) AO_TRY(launch_screen<T>(g.sa, map, S, st, d_idx + c0));
            else AO_TRY(launch_screen<T>(g.sa, map + (size_t)c0 * S * S, S, st));
        }
    }
    return 0;
}

// An episode reset on the device, everything on the stream: the full one (d_idx null, n = n_env, behind screens_replaced) and the
// partial one (aoenv_reset_envs, behind its validation and the switch to per-env clocks) are this sequence; the listed envs' state
// rows are cleared first, which the full reset leaves alone.
template <typename T>
static int reset_on_device(AoEnv* env, const int* d_idx, int n, const uint32_t* d_screen_seeds, const uint32_t* d_ring_seeds,
                           const double* d_scale, double r0, double L0, double pixel_size, TmpFree& tmp, hipStream_t st) {
    if (d_idx) {
        AO_TRY(launch_reset_env_rows<T>(d_idx, n, env->as<T>(env->coefs), env->as<T>(env->dm_prev), env->A, env->env_clk[env->clk_cur],
                                        env->env_taps, env->L, env->E, st));
        if (env->delay.d > 0)                                      // their pending actions too (TimeDelayEnv.reset_envs clears those rows)
            AO_TRY(launch_delay_zero_rows<T>(env->as<T>(env->delay_ring), env->delay_stride, delay_slots(env->delay), d_idx, n,
                                             env->nAct * env->nAct, st));
        AO_TRY(refresh_dense_dm<T>(env, st));
    }
    AO_TRY(draw_screens<T>(env, d_idx, n, d_screen_seeds, d_scale, r0, L0, pixel_size, tmp, st));
    return finish_new_screens<T>(env, d_idx, n, d_ring_seeds, st);
}
}  // extern "C++"

int aoenv_new_screens_device(AoEnv* env, const uint32_t* h_screen_seeds, const uint32_t* h_ring_seeds, double r0,
                             double L0, double pixel_size, void* stream) {
    AO_CHECK_ENV(env);
    if (env->L == 0) return fail("no atmosphere in this shard");
    AO_TRY(require_step_constants(env, true));
    if (!h_screen_seeds || !h_ring_seeds) return fail("null seeds");
    if (!(r0 > 0) || !(L0 > 0) || !(pixel_size > 0)) return fail("r0, L0 and the pixel size must be positive");
    hipStream_t st = static_cast<hipStream_t>(stream);
    AO_HIP(hipStreamSynchronize(st));
    AO_TRY(screens_replaced(env, true));
    TmpFree tmp;
    const size_t ns = (size_t)env->E * env->L;                     // [E][L] screen seeds, [E][L] ring seeds
    std::vector<double> fac;                                       // (first in the pack: 8-byte aligned)
    screen_factors(env, nullptr, env->E, r0, fac);
    const size_t nf = 2 * fac.size();
    uint32_t* d_pack = nullptr;
    AO_TRY(upload_words(tmp, {{fac.data(), nf}, {h_screen_seeds, ns}, {h_ring_seeds, ns}}, &d_pack));
    const uint32_t* d_seeds = d_pack + nf;
    const double* d_scale = nf ? reinterpret_cast<const double*>(d_pack) : nullptr;
    return AO_DISPATCH(env, reset_on_device, env, nullptr, env->E, d_seeds, d_seeds + ns, d_scale, r0, L0, pixel_size, tmp, st);
}

int aoenv_reset_envs(AoEnv* env, const int32_t* h_env_idx, int n_idx, const uint32_t* h_screen_seeds, const uint32_t* h_ring_seeds,
                     double r0, double L0, double pixel_size, void* stream) {
    AO_CHECK_ENV(env);
    if (n_idx < 0) return fail("aoenv_reset_envs: n_idx = %d", n_idx);
    if (n_idx == 0) return 0;
    if (!h_env_idx || !h_screen_seeds || !h_ring_seeds) return fail("aoenv_reset_envs: null index list / seeds");
    if (env->L == 0) return fail("no atmosphere in this shard");
    if (!env->uniform)
        return fail("aoenv_reset_envs: layers on grids of their own (AoCfg.layer_res_l: fov != 0 with altitude layers) have no per-env clocks; "
                    "reset the whole shard (aoenv_new_screens_device)");
    AO_TRY(require_step_constants(env, true));
    if (!(r0 > 0) || !(L0 > 0) || !(pixel_size > 0)) return fail("r0, L0 and the pixel size must be positive");
    const int E = env->E, L = env->L;
    std::vector<char> seen((size_t)E, 0);
    for (int c = 0; c < n_idx; ++c) {
        const int e = h_env_idx[c];
        if (e < 0 || e >= E) return fail("aoenv_reset_envs: env index %d outside [0, n_env=%d)", e, E);
        if (seen[e]) return fail("aoenv_reset_envs: env index %d is listed twice", e);
        seen[e] = 1;
    }
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (!env->per_env_wind) {
        // One env restarted at origin 0 cannot share an origin with the others: per-env clocks from here on, every env where the shard
        // is (origin, accumulator) with the shard's wind.  aoenv_set_wind_env forgets the look-aheads and scatters a pending ring first.
        double shard[2 * kMaxLayer];
        for (int l = 0; l < L; ++l) {
            const LayerClock& k = env->layer[l].clk;
            if (!(std::fabs(k.ratio[0]) < (double)env->wind_pixels) || !(std::fabs(k.ratio[1]) < (double)env->wind_pixels))
                return fail("aoenv_reset_envs: the shard's wind is %g px/frame in layer %d; per-env clocks take < %d", std::max(std::fabs(k.ratio[0]), std::fabs(k.ratio[1])), l, env->wind_pixels);
            shard[2 * l] = k.ratio[0];
            shard[2 * l + 1] = k.ratio[1];
        }
        AO_TRY(aoenv_set_wind_env(env, wind_for_every_env(env, shard).data(), 0, stream));
    } else {
        for (int l = 0; l < L; ++l) forget_lookahead(env->layer[l]);
        AO_TRY(AO_DISPATCH(env, flush_rings, env, st));            // a deferred ring of the clocks as they were
        AO_HIP(hipStreamSynchronize(st));
    }
    // the list and the seeds in one upload: (per-env r0: [n_idx] float64 screen factors, first: 8-byte aligned,) [n_idx] indices,
    // [n_idx][L] screen seeds, [n_idx][L] ring seeds
    TmpFree tmp;
    const size_t ns = (size_t)n_idx * L;
    std::vector<double> fac;
    screen_factors(env, h_env_idx, n_idx, r0, fac);
    const size_t nf = 2 * fac.size();
    uint32_t* d_pack = nullptr;
    AO_TRY(upload_words(tmp, {{fac.data(), nf}, {h_env_idx, (size_t)n_idx}, {h_screen_seeds, ns}, {h_ring_seeds, ns}}, &d_pack));
    const int* d_idx = reinterpret_cast<const int*>(d_pack + nf);
    const uint32_t* d_seeds = d_pack + nf + n_idx;
    const double* d_scale = nf ? reinterpret_cast<const double*>(d_pack) : nullptr;
    return AO_DISPATCH(env, reset_on_device, env, d_idx, n_idx, d_seeds, d_seeds + ns, d_scale, r0, L0, pixel_size, tmp, st);
}

int aoenv_set_atm_opd(AoEnv* env, const double* h_opd, void* stream) {
    AO_CHECK_ENV(env);
    hipStream_t st = static_cast<hipStream_t>(stream);
    AO_HIP(hipStreamSynchronize(st));
    const size_t n = (size_t)env->E * env->R * env->R;
    env->atm_user_defined = true;
    if (!h_opd) { AO_HIP(hipMemset(env->opd_atm, 0, n * env->esz)); return 0; }
    return upload_real(env, env->opd_atm, h_opd, n);
}

int aoenv_set_coefs(AoEnv* env, const double* h_coefs, void* stream) {
    AO_CHECK_ENV(env);
    hipStream_t st = static_cast<hipStream_t>(stream);
    AO_HIP(hipStreamSynchronize(st));
    const size_t n = (size_t)env->E * env->A;
    if (!h_coefs) AO_HIP(hipMemset(env->coefs, 0, n * env->esz));
    else AO_TRY(upload_real(env, env->coefs, h_coefs, n));
    return AO_DISPATCH(env, refresh_dense_dm, env, st);
}

int aoenv_measure(AoEnv* env, void* stream) {
    AO_CHECK_ENV(env);
    AO_TRY(require_step_constants(env, false));
    hipStream_t st = static_cast<hipStream_t>(stream);
    AO_TRY(AO_DISPATCH(env, run_phase, env, 1, 1, st));            // atmosphere re-derived from the screens at the current buff
    return AO_DISPATCH(env, run_wfs, env, st);
}

int aoenv_atm_update(AoEnv* env, void* stream) {
    AO_CHECK_ENV(env);
    AO_TRY(require_step_constants(env, true));
    hipStream_t st = static_cast<hipStream_t>(stream);
    return AO_DISPATCH(env, atm_update_t, env, st);
}

int aoenv_reset_soft(AoEnv* env, void* d_obs, void* stream) {
    AO_CHECK_ENV(env);
    if (!d_obs) return fail("null obs");
    if (!env->have[AOENV_C_RECON]) return fail("the reconstructor has not been uploaded");
    hipStream_t st = static_cast<hipStream_t>(stream);
    return AO_DISPATCH(env, reset_soft_t, env, d_obs, st);
}

int aoenv_step(AoEnv* env, int i, const void* d_action, void* d_obs, void* d_frame, void* d_reward, void* d_strehl,
               void* stream) {
    AO_CHECK_ENV(env);
    if (!d_action || !d_obs) return fail("aoenv_step: null action / obs");
    if (i < 0 || i >= env->c.n_loop) return fail("frame index %d outside [0, n_loop=%d)", i, env->c.n_loop);
    AO_TRY(require_step_constants(env, true));
    if (!env->have[AOENV_C_RECON]) return fail("the reconstructor has not been uploaded");
    AO_TRY(wf_window_check(env, i, 1));
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (env->delay.d == 0) return AO_DISPATCH(env, step_t, env, i, d_action, d_obs, d_frame, d_reward, d_strehl, 0.0, true, st);
    const void* applied = nullptr;                                 // the caller's tensor may be reused at once: it is copied
    AO_TRY(AO_DISPATCH(env, delay_push, env, d_action, 0.0, st, &applied));
    AO_TRY(AO_DISPATCH(env, step_t, env, i, applied, d_obs, d_frame, d_reward, d_strehl, 0.0, true, st));
    env->delay = delay_after(env->delay, 1);
    return 0;
}

int aoenv_run_integrator(AoEnv* env, int i0, int n_steps, double gain, void* d_obs, void* d_frame, void* d_reward,
                         void* d_strehl, void* stream) {
    AO_CHECK_ENV(env);
    if (!d_obs) return fail("aoenv_run_integrator: null obs");
    if (gain == 0) return fail("aoenv_run_integrator: gain must be non-zero");
    if (i0 < 0 || n_steps < 0 || i0 + n_steps > env->c.n_loop) return fail("frames [%d, %d) outside [0, n_loop=%d)", i0, i0 + n_steps, env->c.n_loop);
    AO_TRY(require_step_constants(env, true));
    if (!env->have[AOENV_C_RECON]) return fail("the reconstructor has not been uploaded");
    AO_TRY(wf_window_check(env, i0, n_steps));
    hipStream_t st = static_cast<hipStream_t>(stream);
    // only the last step's residual phase and camera frame can be read afterwards (aoenv_buffer, aoenv_download, aoenv_compute_psf,
    // d_frame, checkpoints: all of them between calls): the fused step leaves the stores of the other steps out
    // ... and takes the step behind it along where that one is quiet (plan_step_pair): its arguments are then that step's
    if (env->delay.d == 0) {
        const bool eligible = n_steps > 1 && step_pair_eligible(env);   // (nothing a step of this loop does changes it)
        double ratio[kMaxLayer][2], buff[kMaxLayer][2];
        for (int l = 0; eligible && l < env->L; ++l)
            for (int d = 0; d < 2; ++d) ratio[l][d] = env->layer[l].clk.ratio[d];
        for (int k = 0; k < n_steps;) {
            for (int l = 0; eligible && l < env->L; ++l)
                for (int d = 0; d < 2; ++d) buff[l][d] = env->layer[l].clk.buff[d];
            const bool pair = plan_step_pair(eligible && !env->sci.accumulates(i0 + k + 1), k, n_steps, env->L, ratio, buff, env->pair.buff2);
            const int last = k + (pair ? 1 : 0);
            env->pair.on = pair;
            const int rc = AO_DISPATCH(env, step_t, env, i0 + k, d_obs /*unused*/, d_obs, last == n_steps - 1 ? d_frame : nullptr, d_reward,
                                       d_strehl, gain, last == n_steps - 1, st);
            env->pair.on = false;
            if (rc) return rc;
            k = last + 1;
        }
        return 0;
    }
    // under a delay the action formed now is applied d steps later: gain * obs goes into the ring (one small launch per step, one
    // multiply in the env dtype as k_rollout_action forms it at sigma 0) and the step is the explicit-action step of aoenv_step
    for (int k = 0; k < n_steps; ++k) {
        const void* applied = nullptr;
        AO_TRY(AO_DISPATCH(env, delay_push, env, d_obs, gain, st, &applied));
        AO_TRY(AO_DISPATCH(env, step_t, env, i0 + k, applied, d_obs, k == n_steps - 1 ? d_frame : nullptr, d_reward, d_strehl, 0.0,
                           k == n_steps - 1, st));
        env->delay = delay_after(env->delay, 1);
    }
    return 0;
}

int aoenv_set_noise_filter(AoEnv* env, const double* h_factors, int K, void* stream) {
    AO_CHECK_ENV(env);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (!h_factors || K == 0) {
        env->noise_K = 0;
        return 0;
    }
    const int A = env->A;
    if (K < 1 || K > A) return fail("aoenv_set_noise_filter: rank %d outside [1, A=%d]", K, A);
    const size_t n = (size_t)K * A;
    if (const size_t i = first_not_finite(h_factors, 2 * n); i < 2 * n) return fail("aoenv_set_noise_filter: entry %zu is not finite", i);
    AO_HIP(hipStreamSynchronize(st));                              // a rollout in flight reads the factors in place
    if (n > env->noise_cap) {
        AO_TRY(block_alloc(env->noise_mem, {n * env->esz, n * env->esz}, false));
        env->noise_fr = env->noise_mem.part(0); env->noise_fl_t = env->noise_mem.part(1); env->noise_cap = n;
    }
    env->noise_K = 0;                                              // (a failed copy leaves no half-written filter in use)
    AO_TRY(upload_real(env, env->noise_fr, h_factors, n));
    AO_TRY(upload_transposed(env, env->noise_fl_t, h_factors + n, A, K));   // Fl [A][K] -> [K][A]
    env->noise_K = K;
    return 0;
}

int aoenv_set_disturbance(AoEnv* env, const AoDisturbance* cfg, void* stream) {
    AO_CHECK_ENV(env);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (!cfg) {
        env->disturb.set = false;                                  // (the tables stay allocated for the next one)
        return 0;
    }
    const int M = cfg->n_modes, J = cfg->n_lines, A = env->A;
    if (M < 1 || M > kDisturbMaxModes) return fail("aoenv_set_disturbance: n_modes %d outside [1, %d]", M, kDisturbMaxModes);
    if (J < 1 || J > kDisturbMaxLines) return fail("aoenv_set_disturbance: n_lines %d outside [1, %d]", J, kDisturbMaxLines);
    if (!cfg->h_modes || !cfg->h_amp || !cfg->h_freq || !cfg->h_phase) return fail("aoenv_set_disturbance: null modes / amp / freq / phase");
    const size_t nb = (size_t)A * M, np = (size_t)env->E * M * J;
    if (const size_t i = first_not_finite(cfg->h_modes, nb); i < nb) return fail("aoenv_set_disturbance: modes[%zu] is not finite", i);
    const struct { const double* p; const char* name; } arrays[] = {{cfg->h_amp, "amp"}, {cfg->h_freq, "freq"}, {cfg->h_phase, "phase"}};
    for (const auto& a : arrays)
        if (const size_t i = first_not_finite(a.p, np); i < np) return fail("aoenv_set_disturbance: %s[%zu] is not finite", a.name, i);
    for (size_t i = 0; i < np; ++i)
        if (cfg->h_amp[i] < 0) return fail("aoenv_set_disturbance: amp[%zu] is negative", i);
    AO_HIP(hipStreamSynchronize(st));                              // a loop in flight reads the tables in place
    AoEnv::Disturb& d = env->disturb;
    if (nb > d.modes_cap || np > d.par_cap) {                      // (neither table ever shrinks)
        const size_t cb = std::max(nb, d.modes_cap), cp = std::max(np, d.par_cap);
        AO_TRY(block_alloc(d.mem, {cb * env->esz, 3 * cp * sizeof(double)}, false));
        d.modes_t = d.mem.part(0); d.modes_cap = cb;
        d.par = static_cast<double*>(d.mem.part(1)); d.par_cap = cp;
    }
    d.set = false;                                                 // (a failed copy leaves no half-written disturbance in use)
    AO_TRY(upload_transposed(env, d.modes_t, cfg->h_modes, A, M));  // B [A][M] -> [M][A]
    AO_HIP(hipMemcpy(d.par, cfg->h_amp, np * sizeof(double), hipMemcpyHostToDevice));
    AO_HIP(hipMemcpy(d.par + np, cfg->h_freq, np * sizeof(double), hipMemcpyHostToDevice));
    AO_HIP(hipMemcpy(d.par + 2 * np, cfg->h_phase, np * sizeof(double), hipMemcpyHostToDevice));
    d.M = M; d.J = J; d.t0 = cfg->t0;
    d.set = true;
    return 0;
}

// ---- per-env mirrors (dm_tables.hpp) -----------------------------------------------------------------------------------------
extern "C++" {
namespace {
template <typename T>
int set_dm_env_t(AoEnv* env, const double* h_gx, const double* h_gy, hipStream_t st) {
    const DmLayout dl = env->dm_layout();
    const size_t E = (size_t)env->E;
    const size_t bg = E * dl.g_elems() * sizeof(T), bt = E * dl.gxt_elems() * sizeof(T), ba = E * dl.ga_elems() * sizeof(float);
    const std::initializer_list<size_t> parts = {bg, bg, bt, ba, ba};
    DmHostTables<T> h;
    dm_relayout<T>(dl, env->E, h_gx, h_gy, h);
    AO_HIP(hipStreamSynchronize(st));                              // a step in flight reads the tables in place
    AoEnv::DmEnv& de = env->dm_env;
    if (!de.mem) {
        if (de.mem.alloc(parts, false))
            return fail("aoenv_set_dm_env: no device memory for %zu bytes of per-env DM tables (%d envs x %zu)", dev_layout(parts).total, env->E, dl.bytes(sizeof(T)));
        de.gx = de.mem.part(0);
        de.gy = de.mem.part(1);
        de.gxt = de.mem.part(2);
        de.gxa = static_cast<float*>(de.mem.part(3));
        de.gya = static_cast<float*>(de.mem.part(4));
    }
    de.on = false;                                                 // (a failed copy leaves no half-written mirror in use)
    AO_HIP(hipMemcpy(de.gx, h.gx.data(), h.gx.size() * sizeof(T), hipMemcpyHostToDevice));
    AO_HIP(hipMemcpy(de.gy, h.gy.data(), h.gy.size() * sizeof(T), hipMemcpyHostToDevice));
    AO_HIP(hipMemcpy(de.gxt, h.gxt.data(), h.gxt.size() * sizeof(T), hipMemcpyHostToDevice));
    AO_HIP(hipMemcpy(de.gxa, h.gxa.data(), h.gxa.size() * sizeof(float), hipMemcpyHostToDevice));
    AO_HIP(hipMemcpy(de.gya, h.gya.data(), h.gya.size() * sizeof(float), hipMemcpyHostToDevice));
    de.on = true;
    return env->stat.w ? refresh_dense_dm<T>(env, st) : 0;         // (a sensor-arm static map: mirror + map on the new tables)
}
}  // namespace
}  // extern "C++"

int aoenv_set_dm_env(AoEnv* env, const double* h_gx, const double* h_gy, void* stream) {
    AO_CHECK_ENV(env);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (!h_gx != !h_gy) return fail("aoenv_set_dm_env: one of gx / gy is null (both, or neither for the shared tables)");
    if (h_gx && !env->c.dm_separable) return fail("aoenv_set_dm_env: this shard's DM is dense (dm_separable == 0): it has no factors");
    if (h_gx && env->dm_pairs.on)
        return fail("aoenv_set_dm_env: actuator factor pairs are in force (aoenv_set_dm_pairs): clear them first (two NULLs)");
    if (!h_gx) {
        if (env->dm_env.mem) AO_HIP(hipStreamSynchronize(st));
        env->dm_env = AoEnv::DmEnv{};
        return env->stat.w ? AO_DISPATCH(env, refresh_dense_dm, env, st) : 0;   // (a sensor-arm static map: mirror + map on the shared tables)
    }
    const size_t n = (size_t)env->E * env->R * env->nAct;
    const size_t ix = first_not_finite(h_gx, n), iy = first_not_finite(h_gy, n);   // (the lower index is reported, gx first)
    if (ix < n && ix <= iy) return fail("aoenv_set_dm_env: gx[%zu] is not finite", ix);
    if (iy < n) return fail("aoenv_set_dm_env: gy[%zu] is not finite", iy);
    return AO_DISPATCH(env, set_dm_env_t, env, h_gx, h_gy, st);
}

int aoenv_get_dm_env(AoEnv* env, double* h_gx, double* h_gy, void* stream) {
    AO_CHECK_ENV(env);
    if (!h_gx || !h_gy) return fail("aoenv_get_dm_env: null destination");
    if (!env->dm_env.on) return fail("aoenv_get_dm_env: the shard shares one mirror (aoenv_set_dm_env has not been called)");
    AO_HIP(hipStreamSynchronize(static_cast<hipStream_t>(stream)));
    const size_t n = (size_t)env->E * env->dm_layout().g_elems();
    AO_TRY(download_real(env, h_gx, env->dm_env.gx, n));
    return download_real(env, h_gy, env->dm_env.gy, n);
}

// ---- per-env actuator factor pairs (dm_pairs.hpp) ----------------------------------------------------------------------------------
extern "C++" {
namespace {
template <typename T>
int set_dm_pairs_t(AoEnv* env, const double* h_py, const double* h_px, hipStream_t st) {
    const PairsLayout pl = env->pairs_layout();
    const size_t E = (size_t)env->E;
    const size_t bt = E * pl.t_elems() * sizeof(T), ba = E * pl.ga_elems() * sizeof(float), bo = E * env->R * env->R * sizeof(T);
    const std::initializer_list<size_t> parts = {bt, bt, ba, ba, bo};
    PairsHostTables<T> h;
    pairs_relayout<T>(pl, env->E, h_py, h_px, h);
    AO_HIP(hipStreamSynchronize(st));                              // a step in flight reads the tables in place
    AoEnv::DmPairs& dp = env->dm_pairs;
    if (!dp.mem) {
        if (dp.mem.alloc(parts, false))
            return fail("aoenv_set_dm_pairs: no device memory for %zu bytes of actuator factor pairs (%d envs x %zu, and the surfaces)", dev_layout(parts).total, env->E, pl.bytes(sizeof(T)));
        dp.pyt = dp.mem.part(0);
        dp.pxt = dp.mem.part(1);
        dp.pya = static_cast<float*>(dp.mem.part(2));
        dp.pxa = static_cast<float*>(dp.mem.part(3));
        dp.opd = dp.mem.part(4);
    }
    dp.on = false;                                                 // (a failed copy leaves no half-written mirror in use)
    AO_HIP(hipMemcpy(dp.pyt, h.pyt.data(), h.pyt.size() * sizeof(T), hipMemcpyHostToDevice));
    AO_HIP(hipMemcpy(dp.pxt, h.pxt.data(), h.pxt.size() * sizeof(T), hipMemcpyHostToDevice));
    AO_HIP(hipMemcpy(dp.pya, h.pya.data(), h.pya.size() * sizeof(float), hipMemcpyHostToDevice));
    AO_HIP(hipMemcpy(dp.pxa, h.pxa.data(), h.pxa.size() * sizeof(float), hipMemcpyHostToDevice));
    dp.on = true;
    return refresh_dense_dm<T>(env, st);                           // the surface of the command held, on the new mirror
}
template <typename T>
int get_dm_pairs_t(AoEnv* env, double* h_py, double* h_px) {
    const PairsLayout pl = env->pairs_layout();
    const size_t n = (size_t)env->E * pl.t_elems();
    std::vector<T> ty(n), tx(n);
    AO_HIP(hipMemcpy(ty.data(), env->dm_pairs.pyt, n * sizeof(T), hipMemcpyDeviceToHost));
    AO_HIP(hipMemcpy(tx.data(), env->dm_pairs.pxt, n * sizeof(T), hipMemcpyDeviceToHost));
    for (int e = 0; e < env->E; ++e) {
        pairs_read_t<T>(pl, ty.data() + (size_t)e * pl.t_elems(), h_py + (size_t)e * pl.t_elems());
        pairs_read_t<T>(pl, tx.data() + (size_t)e * pl.t_elems(), h_px + (size_t)e * pl.t_elems());
    }
    return 0;
}
}  // namespace
}  // extern "C++"

int aoenv_set_dm_pairs(AoEnv* env, const double* h_py, const double* h_px, void* stream) {
    AO_CHECK_ENV(env);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (!h_py != !h_px) return fail("aoenv_set_dm_pairs: one of py / px is null (both, or neither to clear the pairs)");
    if (!h_py) {
        if (env->dm_pairs.mem) AO_HIP(hipStreamSynchronize(st));
        env->dm_pairs = AoEnv::DmPairs{};
        return env->stat.w ? AO_DISPATCH(env, refresh_dense_dm, env, st) : 0;   // (a sensor-arm static map: mirror + map of the separable mirror)
    }
    if (!env->c.dm_separable) return fail("aoenv_set_dm_pairs: this shard's DM is dense (dm_separable == 0): upload its modes instead");
    if (env->dm_env.on)
        return fail("aoenv_set_dm_pairs: per-env factor tables are in force (aoenv_set_dm_env): clear them first (two NULLs)");
    const size_t n = (size_t)env->E * env->R * env->A;
    const size_t iy = first_not_finite(h_py, n), ix = first_not_finite(h_px, n);   // (the lower index is reported, py first)
    if (iy < n && iy <= ix) return fail("aoenv_set_dm_pairs: py[%zu] is not finite", iy);
    if (ix < n) return fail("aoenv_set_dm_pairs: px[%zu] is not finite", ix);
    return AO_DISPATCH(env, set_dm_pairs_t, env, h_py, h_px, st);
}

int aoenv_get_dm_pairs(AoEnv* env, double* h_py, double* h_px, void* stream) {
    AO_CHECK_ENV(env);
    if (!h_py || !h_px) return fail("aoenv_get_dm_pairs: null destination");
    if (!env->dm_pairs.on) return fail("aoenv_get_dm_pairs: no actuator factor pairs are in force (aoenv_set_dm_pairs has not been called)");
    AO_HIP(hipStreamSynchronize(static_cast<hipStream_t>(stream)));
    return AO_DISPATCH(env, get_dm_pairs_t, env, h_py, h_px);
}

int aoenv_get_dm_surface(AoEnv* env, double* h_surface, void* stream) {
    AO_CHECK_ENV(env);
    if (!h_surface) return fail("aoenv_get_dm_surface: null destination");
    if (!env->mirror_ahead())                                      // (a static map's buffer holds mirror + map: not the mirror's surface)
        return fail("aoenv_get_dm_surface: this shard forms its mirror surface inside the phase kernel and has no surface buffer "
                    "(a dense DM or aoenv_set_dm_pairs has one)");
    hipStream_t st = static_cast<hipStream_t>(stream);
    AO_TRY(AO_DISPATCH(env, refresh_dense_dm, env, st));            // (outside a step: the pure command)
    AO_HIP(hipStreamSynchronize(st));
    return download_real(env, h_surface, env->mirror_surface(), (size_t)env->E * env->R * env->R);
}

// ---- per-env guide stars (star_env.hpp) ------------------------------------------------------------------------------------------
extern "C++" {
namespace {
// one [E] array of the env dtype in a block of its own: `h` (already validated) through `fill`, or freed when h is null
template <typename T, typename Fill>
int set_star_row_t(AoEnv* env, Block& mem, void*& slot, const double* h, Fill fill, const char* who, hipStream_t st) {
    std::vector<T> t((size_t)env->E);
    fill(h, env->E, t.data());
    AO_HIP(hipStreamSynchronize(st));                              // a step in flight reads the array in place
    Block fresh;
    if (!mem && fresh.alloc({t.size() * sizeof(T)}, false)) return fail("%s: no device memory for %d values", who, env->E);
    if ((mem ? mem : fresh).upload(0, t.data(), t.size() * sizeof(T)))
        return fail("%s: the copy to the device failed", who);     // (an array already held keeps being used: same size, same place)
    if (!mem) mem = std::move(fresh);
    slot = mem.part(0);
    return 0;
}
int clear_star_row(Block& mem, void*& slot, hipStream_t st) {
    if (mem) AO_HIP(hipStreamSynchronize(st));
    mem.reset();
    slot = nullptr;
    return 0;
}
}  // namespace
}  // extern "C++"

int aoenv_set_flux_env(AoEnv* env, const double* h_scale, void* stream) {
    AO_CHECK_ENV(env);
    hipStream_t st = static_cast<hipStream_t>(stream);
    AoEnv::StarDev& s = env->star;
    if (!h_scale) return clear_star_row(s.amp_mem, s.amp, st);
    if (env->geometric()) return fail("aoenv_set_flux_env: a geometric sensor has neither photons nor a threshold");
    char msg[96];
    if (star_flux_check(h_scale, env->E, msg, sizeof msg)) return fail("aoenv_set_flux_env: %s", msg);
    const auto fill = [](const double* h, int n, auto* out) { star_amp_factors(h, n, out); };
    return AO_DISPATCH(env, set_star_row_t, env, s.amp_mem, s.amp, h_scale, fill, "aoenv_set_flux_env", st);
}

int aoenv_get_flux_env(AoEnv* env, double* h_amp, void* stream) {
    AO_CHECK_ENV(env);
    if (!h_amp) return fail("aoenv_get_flux_env: null destination");
    if (!env->star.amp) return fail("aoenv_get_flux_env: the shard has one star (aoenv_set_flux_env has not been called)");
    AO_HIP(hipStreamSynchronize(static_cast<hipStream_t>(stream)));
    return download_real(env, h_amp, env->star.amp, (size_t)env->E);
}

int aoenv_set_threshold_env(AoEnv* env, const double* h_thr, void* stream) {
    AO_CHECK_ENV(env);
    hipStream_t st = static_cast<hipStream_t>(stream);
    AoEnv::StarDev& s = env->star;
    if (!h_thr) return clear_star_row(s.thr_mem, s.thr, st);
    if (env->geometric()) return fail("aoenv_set_threshold_env: a geometric sensor has neither photons nor a threshold");
    if (const char* why = star_threshold_refusal(env->c.wfs_type == AOENV_WFS_PYRAMID, env->c.max_group)) return fail("aoenv_set_threshold_env: %s", why);
    char msg[96];
    if (star_threshold_check(h_thr, env->E, msg, sizeof msg)) return fail("aoenv_set_threshold_env: %s", msg);
    const auto fill = [](const double* h, int n, auto* out) { star_thresholds(h, n, out); };
    return AO_DISPATCH(env, set_star_row_t, env, s.thr_mem, s.thr, h_thr, fill, "aoenv_set_threshold_env", st);
}

int aoenv_get_threshold_env(AoEnv* env, double* h_thr, void* stream) {
    AO_CHECK_ENV(env);
    if (!h_thr) return fail("aoenv_get_threshold_env: null destination");
    if (!env->star.thr) return fail("aoenv_get_threshold_env: the shard has one threshold (aoenv_set_threshold_env has not been called)");
    AO_HIP(hipStreamSynchronize(static_cast<hipStream_t>(stream)));
    return download_real(env, h_thr, env->star.thr, (size_t)env->E);
}

// ---- the modal control surface (modal.hpp) ----------------------------------------------------------------------------------------
int aoenv_set_modal(AoEnv* env, const AoModal* cfg, void* stream) {
    AO_CHECK_ENV(env);
    hipStream_t st = static_cast<hipStream_t>(stream);
    AoEnv::Modal& mo = env->modal;
    if (!cfg) {
        AO_HIP(hipStreamSynchronize(st));                          // a step in flight reads the tables in place
        mo = AoEnv::Modal{};
        return 0;
    }
    const int K = cfg->n_modes, A = env->A;
    if (K < 1 || K > A) return fail("aoenv_set_modal: n_modes %d outside [1, A=%d]", K, A);
    if (!cfg->h_m2c || !cfg->h_cm) return fail("aoenv_set_modal: null m2c / cm");
    const size_t nm = (size_t)A * K, nc = (size_t)K * env->nSig, E = (size_t)env->E, img = (size_t)env->nAct * env->nAct;
    if (const size_t i = first_not_finite(cfg->h_m2c, nm); i < nm) return fail("aoenv_set_modal: m2c[%zu] is not finite", i);
    if (const size_t i = first_not_finite(cfg->h_cm, nc); i < nc) return fail("aoenv_set_modal: cm[%zu] is not finite", i);
    const size_t z = env->esz, n_slab = (z == 4 ? (size_t)kMaxSplits : 1) * E * K;
    const std::initializer_list<size_t> parts = {nm * z, nc * z, E * K * z, E * img * z, E * img * z, 2 * E * z, n_slab * z};
    AO_HIP(hipStreamSynchronize(st));                              // a step in flight reads the tables in place
    Block mem;                                                     // zeroed whole
    if (mem.alloc(parts, true)) return fail("aoenv_set_modal: no device memory for %zu bytes of modal tables and scratch", dev_layout(parts).total);
    mo = AoEnv::Modal{};                                           // (frees the basis held so far)
    mo.mem = std::move(mem);
    void** field[] = {&mo.m2c_t, &mo.cm, &mo.gain, &mo.image, &mo.zobs, &mo.zscal, &mo.slabs};
    for (int k = 0; k < 7; ++k) *field[k] = mo.mem.part(k);
    AO_TRY(upload_transposed(env, mo.m2c_t, cfg->h_m2c, A, K));    // M2C [A][K] -> [K][A]
    AO_TRY(upload_real(env, mo.cm, cfg->h_cm, nc));
    mo.K = K;
    mo.set = true;
    return 0;
}

int aoenv_set_modal_gain(AoEnv* env, const double* h_gain, int per_env, void* stream) {
    AO_CHECK_ENV(env);
    AoEnv::Modal& mo = env->modal;
    if (!mo.set) return fail("aoenv_set_modal_gain: no modal basis is set (aoenv_set_modal)");
    if (!h_gain) return fail("aoenv_set_modal_gain: null gains");
    const size_t n = (size_t)(per_env ? env->E : 1) * mo.K;
    for (size_t i = 0; i < n; ++i)
        if (!std::isfinite(h_gain[i]) || h_gain[i] < 0) return fail("aoenv_set_modal_gain: gain[%zu] is not finite or negative", i);
    AO_HIP(hipStreamSynchronize(static_cast<hipStream_t>(stream)));   // a loop in flight reads the gains in place
    mo.have_gain = false;                                          // (a failed copy leaves no half-written gains in use)
    AO_TRY(upload_real(env, mo.gain, h_gain, n));
    mo.gain_env = per_env ? (size_t)mo.K : 0;
    mo.have_gain = true;
    return 0;
}

int aoenv_reset_soft_modal(AoEnv* env, void* d_obs, void* stream) {
    AO_CHECK_ENV(env);
    if (!env->modal.set) return fail("aoenv_reset_soft_modal: no modal basis is set (aoenv_set_modal)");
    if (!d_obs) return fail("aoenv_reset_soft_modal: null obs");
    if (!env->have[AOENV_C_RECON]) return fail("the reconstructor has not been uploaded");
    return AO_DISPATCH(env, reset_soft_modal_t, env, d_obs, static_cast<hipStream_t>(stream));
}

int aoenv_step_modal(AoEnv* env, int i, const void* d_action, void* d_obs, void* d_frame, void* d_reward, void* d_strehl,
                     void* stream) {
    AO_CHECK_ENV(env);
    if (!env->modal.set) return fail("aoenv_step_modal: no modal basis is set (aoenv_set_modal)");
    if (!d_action || !d_obs) return fail("aoenv_step_modal: null action / obs");
    if (i < 0 || i >= env->c.n_loop) return fail("frame index %d outside [0, n_loop=%d)", i, env->c.n_loop);
    AO_TRY(require_step_constants(env, true));
    if (!env->have[AOENV_C_RECON]) return fail("the reconstructor has not been uploaded");
    AO_TRY(wf_window_check(env, i, 1));
    return AO_DISPATCH(env, step_modal_t, env, i, d_action, false, d_obs, d_frame, d_reward, d_strehl, true, static_cast<hipStream_t>(stream));
}

int aoenv_run_integrator_modal(AoEnv* env, int i0, int n_steps, void* d_obs, void* d_frame, void* d_reward, void* d_strehl,
                               void* stream) {
    AO_CHECK_ENV(env);
    if (!env->modal.set) return fail("aoenv_run_integrator_modal: no modal basis is set (aoenv_set_modal)");
    if (!env->modal.have_gain) return fail("aoenv_run_integrator_modal: no modal gains are set (aoenv_set_modal_gain)");
    if (!d_obs) return fail("aoenv_run_integrator_modal: null obs");
    if (i0 < 0 || n_steps < 0 || i0 + n_steps > env->c.n_loop) return fail("frames [%d, %d) outside [0, n_loop=%d)", i0, i0 + n_steps, env->c.n_loop);
    AO_TRY(require_step_constants(env, true));
    if (!env->have[AOENV_C_RECON]) return fail("the reconstructor has not been uploaded");
    AO_TRY(wf_window_check(env, i0, n_steps));
    hipStream_t st = static_cast<hipStream_t>(stream);
    // (only the last step's residual phase and camera frame can be read afterwards, as after aoenv_run_integrator)
    for (int k = 0; k < n_steps; ++k)
        AO_TRY(AO_DISPATCH(env, step_modal_t, env, i0 + k, d_obs, true, d_obs, k == n_steps - 1 ? d_frame : nullptr, d_reward, d_strehl,
                           k == n_steps - 1, st));
    return 0;
}

// ---- wavefront modes (wavefront.hpp) ----------------------------------------------------------------------------------------------
static_assert(kWfMaxModes == AOENV_MAX_WF_MODES, "wavefront.hpp and aoenv.h disagree");
constexpr int kWfSlabsAtLeast = kMaxSplits;                        // (the GEMM route writes up to kMaxSplits slabs)

extern "C++" {
template <typename T>
static int wf_set_basis(AoEnv* env, const AoWavefrontBasis* cfg, hipStream_t st) {
    const int R2 = env->R * env->R;
    const bool have_pupil = env->h_pupil.size() == (size_t)R2;
    size_t where = 0;
    switch (wf_validate<T>(cfg->n_modes, cfg->n_pix, have_pupil ? env->h_pupil.data() : nullptr, R2, cfg->h_opd2m, &where)) {
        case kWfOk: break;
        case kWfPix: return fail("aoenv_set_wavefront_basis: n_pix %d is not positive", cfg->n_pix);
        case kWfModes: return fail("aoenv_set_wavefront_basis: n_modes %d outside [1, min(n_pix=%d, %d)]", cfg->n_modes, cfg->n_pix, kWfMaxModes);
        case kWfNoPupil: return fail("aoenv_set_wavefront_basis: the pupil has not been uploaded");
        case kWfPupilCount: return fail("aoenv_set_wavefront_basis: n_pix %d, the pupil has %d pixels", cfg->n_pix, env->n_pupil);
        case kWfNullTable: return fail("aoenv_set_wavefront_basis: null opd2m");
        case kWfNotFinite: return fail("aoenv_set_wavefront_basis: opd2m[%zu] is not finite in the env dtype", where);
    }
    const int K = cfg->n_modes;
    const WfPlan pl = wf_plan(R2, K);
    const size_t ld = (size_t)wf_row_stride(R2), np = (size_t)K * ld, ns = (size_t)std::max(pl.n_slices, kWfSlabsAtLeast) * 2 * env->E * K;
    const std::initializer_list<size_t> parts = {np * sizeof(T), ns * sizeof(T)};
    std::vector<T> table(np);
    wf_scatter<T>(cfg->h_opd2m, K, cfg->n_pix, env->h_pupil.data(), R2, table.data());
    AO_HIP(hipStreamSynchronize(st));                              // a projection in flight reads the table in place
    Block mem;                                                     // (built whole before the basis in use is given up)
    if (mem.alloc(parts, false)) return fail("aoenv_set_wavefront_basis: no device memory for %zu bytes of projector and slabs", dev_layout(parts).total);
    if (mem.upload(0, table.data(), np * sizeof(T))) return fail("aoenv_set_wavefront_basis: the copy of the projector failed");
    AoEnv::Wavefront& wf = env->wf;
    wf = AoEnv::Wavefront{};                                       // (a new basis detaches the record of the previous one)
    wf.mem = std::move(mem);
    wf.p = wf.mem.part(0);
    wf.slabs = wf.mem.part(1);
    wf.K = K;
    wf.plan = pl;
    wf.set = true;
    return 0;
}
}  // extern "C++"

int aoenv_set_wavefront_basis(AoEnv* env, const AoWavefrontBasis* cfg, void* stream) {
    AO_CHECK_ENV(env);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (!cfg) {
        AO_HIP(hipStreamSynchronize(st));
        env->wf = AoEnv::Wavefront{};
        return 0;
    }
    return AO_DISPATCH(env, wf_set_basis, env, cfg, st);
}

static int wf_one_or_two_bits(int what) { return what != 0 && (what & ~(AOENV_WF_RESIDUAL | AOENV_WF_ATMOSPHERE)) == 0; }

int aoenv_project_wavefront(AoEnv* env, int what, void* d_out, void* stream) {
    AO_CHECK_ENV(env);
    if (!env->wf.set) return fail("aoenv_project_wavefront: no wavefront basis is set (aoenv_set_wavefront_basis)");
    if (what != AOENV_WF_RESIDUAL && what != AOENV_WF_ATMOSPHERE && what != AOENV_WF_SCIENCE)
        return fail("aoenv_project_wavefront: what = %d is not exactly one of AOENV_WF_RESIDUAL, AOENV_WF_ATMOSPHERE, AOENV_WF_SCIENCE", what);
    if (!d_out) return fail("aoenv_project_wavefront: null output");
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (what == AOENV_WF_SCIENCE) {                                // the residual toward the target, formed now
        if (!env->sci_differs())
            return fail("aoenv_project_wavefront: what = %d is not exactly one of AOENV_WF_RESIDUAL, AOENV_WF_ATMOSPHERE (AOENV_WF_SCIENCE: no science direction is set, aoenv_set_science_direction, and no static map makes the science arm differ, aoenv_set_static_opd)", what);
        AO_TRY(require_step_constants(env, false));
        AO_TRY(AO_DISPATCH(env, oa_residual_now, env, "aoenv_project_wavefront", env->sci_phase(), nullptr, nullptr, nullptr, st));
    }
    if (what == AOENV_WF_ATMOSPHERE && env->L > 0 && !env->atm_user_defined && !env->store_opd_atm) {
        // not written by the step kernels unless asked to: re-derived from the screens now, as aoenv_download(AOENV_B_OPD_ATM) does
        AO_TRY(require_step_constants(env, false));
        AO_TRY(AO_DISPATCH(env, run_phase, env, 1, 1, st, 0));
    }
    return AO_DISPATCH(env, wf_project, env, what, d_out, st);
}

int aoenv_set_wavefront_record(AoEnv* env, int what, void* d_rec, int i_base, int n_slots) {
    AO_CHECK_ENV(env);
    AoEnv::Wavefront& wf = env->wf;
    if (!d_rec) {
        wf.rec = nullptr;
        wf.rec_what = wf.i_base = wf.n_slots = 0;
        return 0;
    }
    if (!wf.set) return fail("aoenv_set_wavefront_record: no wavefront basis is set (aoenv_set_wavefront_basis)");
    if (what & AOENV_WF_SCIENCE)
        return fail("aoenv_set_wavefront_record: what = %d is no combination of AOENV_WF_RESIDUAL, AOENV_WF_ATMOSPHERE: AOENV_WF_SCIENCE is projected on demand only (aoenv_project_wavefront), the record does not take it", what);
    if (!wf_one_or_two_bits(what)) return fail("aoenv_set_wavefront_record: what = %d is no combination of AOENV_WF_RESIDUAL, AOENV_WF_ATMOSPHERE", what);
    if (i_base < 0 || n_slots < 1) return fail("aoenv_set_wavefront_record: window [%d, %d + %d) is empty or negative", i_base, i_base, n_slots);
    wf.rec = d_rec;
    wf.rec_what = what;
    wf.i_base = i_base;
    wf.n_slots = n_slots;
    return 0;
}

// ---- science camera (science.hpp) --------------------------------------------------------------------------------------------------
static_assert(kSciLog10 == AOENV_SCI_LOG10, "science.hpp and aoenv.h disagree");

extern "C++" {
template <typename T>
static int sci_set(AoEnv* env, const AoScience* cfg, hipStream_t st) {
    const int R = env->R;
    const size_t R2 = (size_t)R * R;
    size_t where = 0;
    switch (sci_validate<T>(R, cfg->zero_padding, cfg->window, cfg->first_frame, cfg->flags, cfg->h_dft, &where)) {
        case kSciOk: break;
        case kSciZp: return fail("aoenv_set_science: zeroPaddingFactor %d outside [1, %d]", cfg->zero_padding, kSciMaxZp);
        case kSciOddImage: return fail("aoenv_set_science: odd image sizes are not built (zero_padding %d x resolution %d)", cfg->zero_padding, R);
        case kSciWindowOdd: return fail("aoenv_set_science: window %d is odd", cfg->window);
        case kSciWindowRange: return fail("aoenv_set_science: window %d outside [2, zero_padding * resolution = %d]", cfg->window, cfg->zero_padding * R);
        case kSciFirstFrame: return fail("aoenv_set_science: first_frame %d is negative", cfg->first_frame);
        case kSciFlags: return fail("aoenv_set_science: flags %d: only AOENV_SCI_LOG10 is known", cfg->flags);
        case kSciNotFinite: return fail("aoenv_set_science: dft[%zu] is not finite in the env dtype", where);
    }
    if (env->h_amp.size() != R2) return fail("aoenv_set_science: the WFS amplitude has not been uploaded");
    const SciGeom g = sci_geom(R, cfg->zero_padding, cfg->window);
    const SciPlan pl = sci_plan(R, cfg->window);
    const size_t nt = sci_table_elems(pl);
    const std::initializer_list<size_t> parts = {nt * sizeof(T), R2 * sizeof(T)};
    std::vector<T> table(nt), amp(R2);
    sci_fill_table<T>(g, pl, cfg->h_dft, table.data());
    // the amplitude of aoenv_compute_psf: pupil * sqrt(src.fluxMap), all modulation points of a Pyramid together
    const double scale = env->c.wfs_type == AOENV_WFS_PYRAMID ? std::sqrt((double)env->c.pyr_n_theta) : 1.0;
    for (size_t q = 0; q < R2; ++q) amp[q] = (T)(env->h_amp[q] * scale);
    AO_HIP(hipStreamSynchronize(st));                              // a window in flight reads the table in place
    Block mem;                                                     // (built whole before the configuration in use is given up)
    if (mem.alloc(parts, false)) return fail("aoenv_set_science: no device memory for %zu bytes of table and amplitude", dev_layout(parts).total);
    if (mem.upload(0, table.data(), nt * sizeof(T)) || mem.upload(1, amp.data(), R2 * sizeof(T)))
        return fail("aoenv_set_science: the copy of the table failed");
    AoEnv::Science& sc = env->sci;
    sc = AoEnv::Science{};                                         // (a new configuration detaches the accumulators of the previous one)
    sc.mem = std::move(mem);
    sc.table = sc.mem.part(0);
    sc.amp = sc.mem.part(1);
    sc.g = g;
    sc.first_frame = cfg->first_frame;
    sc.flags = cfg->flags;
    sc.set = true;
    return 0;
}
}  // extern "C++"

int aoenv_set_science(AoEnv* env, const AoScience* cfg, void* stream) {
    AO_CHECK_ENV(env);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (!cfg) {
        AO_HIP(hipStreamSynchronize(st));
        env->sci = AoEnv::Science{};
        return 0;
    }
    return AO_DISPATCH(env, sci_set, env, cfg, st);
}

int aoenv_science_psf(AoEnv* env, int flat, void* d_out, void* stream) {
    AO_CHECK_ENV(env);
    if (!env->sci.set) return fail("aoenv_science_psf: no science camera is set (aoenv_set_science)");
    if (!d_out) return fail("aoenv_science_psf: null output");
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (env->sci_differs() && !flat) {                             // the camera looks at the target, through its own arm
        AO_TRY(require_step_constants(env, false));
        AO_TRY(AO_DISPATCH(env, oa_residual_now, env, "aoenv_science_psf", env->sci_phase(), nullptr, nullptr, nullptr, st));
    }
    return AO_DISPATCH(env, sci_window, env, flat, d_out, st);
}

int aoenv_set_science_accumulator(AoEnv* env, void* d_sum, void* d_sum_log10, int32_t* d_count) {
    AO_CHECK_ENV(env);
    AoEnv::Science& sc = env->sci;
    if (!d_sum) {
        sc.sum = sc.sum_log10 = nullptr;
        sc.count = nullptr;
        return 0;
    }
    if (!sc.set) return fail("aoenv_set_science_accumulator: no science camera is set (aoenv_set_science)");
    if (!d_count) return fail("aoenv_set_science_accumulator: null count");
    if ((sc.flags & AOENV_SCI_LOG10) && !d_sum_log10) return fail("aoenv_set_science_accumulator: AOENV_SCI_LOG10 is set and d_sum_log10 is null");
    if (!(sc.flags & AOENV_SCI_LOG10) && d_sum_log10) return fail("aoenv_set_science_accumulator: d_sum_log10 given without AOENV_SCI_LOG10");
    sc.sum = d_sum;
    sc.sum_log10 = d_sum_log10;
    sc.count = d_count;
    return 0;
}

// ---- off-axis science target (offaxis.hpp) -----------------------------------------------------------------------------------------
int aoenv_set_field(AoEnv* env, double diameter, double fov_arcsec, const double* h_altitude) {
    AO_CHECK_ENV(env);
    if (!(std::isfinite(diameter) && diameter > 0)) return fail("aoenv_set_field: diameter %g is not positive", diameter);
    if (!(std::isfinite(fov_arcsec) && fov_arcsec >= 0)) return fail("aoenv_set_field: field of view %g arcsec is negative or not finite", fov_arcsec);
    if (env->L > 0 && !h_altitude) return fail("aoenv_set_field: null altitudes");
    for (int l = 0; l < env->L; ++l)
        if (!(std::isfinite(h_altitude[l]) && h_altitude[l] >= 0)) return fail("aoenv_set_field: altitude %g of layer %d is negative or not finite", h_altitude[l], l);
    if (env->oa.set) return fail("aoenv_set_field: a science direction is set; forget it first (aoenv_set_science_direction with NULL)");
    if (env->guide.set) return fail("aoenv_set_field: a guide direction is set; forget it first (aoenv_set_guide_direction with NULL)");
    AoEnv::OffAxis& oa = env->oa;
    oa.D = diameter;
    oa.fov = fov_arcsec;
    for (int l = 0; l < env->L; ++l) oa.altitude[l] = h_altitude[l];
    oa.have_field = true;
    return 0;
}

// what aoenv_set_science_direction and aoenv_set_guide_direction check, with `who` in every message, and the table [L][E] they upload
static int oa_plan_direction(const AoEnv* env, const char* who, const double* h_zenith_arcsec, const double* h_azimuth_deg,
                             std::vector<OaShift>& dir) {
    const AoEnv::OffAxis& oa = env->oa;
    if (!h_zenith_arcsec || !h_azimuth_deg) return fail("%s: one of the two arrays is null", who);
    if (env->L < 1) return fail("%s: the shard has no layers to look through", who);
    if (!oa.have_field) return fail("%s: the field is not set (aoenv_set_field)", who);
    const int E = env->E, L = env->L;
    int N_l[kMaxLayer], we = 0, wl = 0;
    for (int l = 0; l < L; ++l) N_l[l] = env->layer[l].N;
    dir.resize((size_t)L * E);
    switch (oa_make(L, E, env->R, oa.D, oa.fov, oa.altitude, N_l, h_zenith_arcsec, h_azimuth_deg, dir.data(), &we, &wl)) {
        case kOaOk: break;
        case kOaNoLayers: return fail("%s: the shard has no layers to look through", who);
        case kOaNull: return fail("%s: null argument", who);
        case kOaGeometry: return fail("%s: the field is not valid (aoenv_set_field)", who);
        case kOaZenith:
            return fail("%s: zenith %g arcsec of env %d is negative, not finite or above fov / 2 = %g", who, h_zenith_arcsec[we], we, oa.fov / 2);
        case kOaAzimuth: return fail("%s: azimuth of env %d is not finite", who, we);
        case kOaPlan:
            return fail("%s: the footprint of env %d in layer %d (grid %d) would read beyond the layer's screen", who, we, wl, N_l[wl]);
    }
    return 0;
}

int aoenv_set_science_direction(AoEnv* env, const double* h_zenith_arcsec, const double* h_azimuth_deg, void* stream) {
    AO_CHECK_ENV(env);
    hipStream_t st = static_cast<hipStream_t>(stream);
    AoEnv::OffAxis& oa = env->oa;
    if (!h_zenith_arcsec && !h_azimuth_deg) {                      // forget the direction; the record goes with it, the field stays
        AO_HIP(hipStreamSynchronize(st));
        oa.mem = Block{};
        oa.dir = nullptr;
        oa.phase_sci = nullptr;
        oa.rec = nullptr;
        oa.i_base = oa.n_slots = 0;
        oa.zenith.clear();
        oa.azimuth.clear();
        oa.set = false;
        return 0;
    }
    const int E = env->E;
    std::vector<OaShift> dir;
    AO_TRY(oa_plan_direction(env, "aoenv_set_science_direction", h_zenith_arcsec, h_azimuth_deg, dir));
    const size_t R2 = (size_t)env->R * env->R;
    const std::initializer_list<size_t> parts = {dir.size() * sizeof(OaShift), (size_t)E * R2 * env->esz};
    AO_HIP(hipStreamSynchronize(st));                              // a launch in flight reads the table in place
    Block mem;                                                     // (built whole before the direction in use is given up)
    if (mem.alloc(parts, true)) return fail("aoenv_set_science_direction: no device memory for %zu bytes", dev_layout(parts).total);
    if (mem.upload(0, dir.data(), dir.size() * sizeof(OaShift))) return fail("aoenv_set_science_direction: the copy of the footprints failed");
    oa.mem = std::move(mem);
    oa.dir = static_cast<OaShift*>(oa.mem.part(0));
    oa.phase_sci = oa.mem.part(1);
    oa.zenith.assign(h_zenith_arcsec, h_zenith_arcsec + E);
    oa.azimuth.assign(h_azimuth_deg, h_azimuth_deg + E);
    oa.set = true;                                                 // (an attached record stays: it is [n_slots][2][E] whatever the direction)
    return 0;
}

int aoenv_get_science_direction(AoEnv* env, double* h_zenith_arcsec, double* h_azimuth_deg) {
    if (!env || !h_zenith_arcsec || !h_azimuth_deg) return fail("aoenv_get_science_direction: null argument");
    if (!env->oa.set) return fail("aoenv_get_science_direction: no science direction is set (aoenv_set_science_direction)");
    std::copy(env->oa.zenith.begin(), env->oa.zenith.end(), h_zenith_arcsec);
    std::copy(env->oa.azimuth.begin(), env->oa.azimuth.end(), h_azimuth_deg);
    return 0;
}

int aoenv_science_residual(AoEnv* env, void* d_phase_sci, void* d_opd_atm_sci, void* d_rms_nm, void* d_strehl, void* stream) {
    AO_CHECK_ENV(env);
    if (!env->sci_differs()) return fail("aoenv_science_residual: no science direction is set (aoenv_set_science_direction) and no static map makes the science arm differ (aoenv_set_static_opd)");
    AO_TRY(require_step_constants(env, false));
    return AO_DISPATCH(env, oa_residual_now, env, "aoenv_science_residual", d_phase_sci, d_opd_atm_sci, d_rms_nm, d_strehl, static_cast<hipStream_t>(stream));
}

int aoenv_set_science_direction_record(AoEnv* env, void* d_rec, int i_base, int n_slots) {
    AO_CHECK_ENV(env);
    AoEnv::OffAxis& oa = env->oa;
    if (!d_rec) {
        oa.rec = nullptr;
        oa.i_base = oa.n_slots = 0;
        return 0;
    }
    if (!env->sci_differs()) return fail("aoenv_set_science_direction_record: no science direction is set (aoenv_set_science_direction) and no static map makes the science arm differ (aoenv_set_static_opd)");
    if (i_base < 0 || n_slots < 1) return fail("aoenv_set_science_direction_record: window [%d, %d + %d) is empty or negative", i_base, i_base, n_slots);
    oa.rec = d_rec;
    oa.i_base = i_base;
    oa.n_slots = n_slots;
    return 0;
}

// ---- off-axis guide star (offaxis.hpp, k_guide_opd) ----------------------------------------------------------------------------------
int aoenv_set_guide_direction(AoEnv* env, const double* h_zenith_arcsec, const double* h_azimuth_deg, void* stream) {
    AO_CHECK_ENV(env);
    hipStream_t st = static_cast<hipStream_t>(stream);
    AoEnv::Guide& gd = env->guide;
    if (!h_zenith_arcsec && !h_azimuth_deg) {                      // forget the direction: the sensor looks along the axis again
        AO_HIP(hipStreamSynchronize(st));
        gd = AoEnv::Guide{};
        return 0;
    }
    std::vector<OaShift> dir;
    AO_TRY(oa_plan_direction(env, "aoenv_set_guide_direction", h_zenith_arcsec, h_azimuth_deg, dir));
    const std::initializer_list<size_t> parts = {dir.size() * sizeof(OaShift)};
    AO_HIP(hipStreamSynchronize(st));                              // a launch in flight reads the table in place
    Block mem;                                                     // (built whole before the direction in use is given up)
    if (mem.alloc(parts, true)) return fail("aoenv_set_guide_direction: no device memory for %zu bytes", dev_layout(parts).total);
    if (mem.upload(0, dir.data(), dir.size() * sizeof(OaShift))) return fail("aoenv_set_guide_direction: the copy of the footprints failed");
    gd.mem = std::move(mem);
    gd.dir = static_cast<OaShift*>(gd.mem.part(0));
    gd.zenith.assign(h_zenith_arcsec, h_zenith_arcsec + env->E);
    gd.azimuth.assign(h_azimuth_deg, h_azimuth_deg + env->E);
    gd.set = true;
    return 0;
}

int aoenv_get_guide_direction(AoEnv* env, double* h_zenith_arcsec, double* h_azimuth_deg) {
    if (!env || !h_zenith_arcsec || !h_azimuth_deg) return fail("aoenv_get_guide_direction: null argument");
    if (!env->guide.set) return fail("aoenv_get_guide_direction: no guide direction is set (aoenv_set_guide_direction)");
    std::copy(env->guide.zenith.begin(), env->guide.zenith.end(), h_zenith_arcsec);
    std::copy(env->guide.azimuth.begin(), env->guide.azimuth.end(), h_azimuth_deg);
    return 0;
}

// ---- static aberrations (static_opd.hpp) -------------------------------------------------------------------------------------------
extern "C++" {
namespace {
// one arm, or the difference of the two, in the env dtype: h_a - h_b element by element in float64 (a null array is zeros), rounded
// once.  Returns the index of the first value that is not finite in the env dtype, n if there is none; *nonzero: any value != 0
template <typename T>
size_t static_round(const double* h_a, const double* h_b, size_t n, std::vector<T>& out, bool* nonzero) {
    out.resize(n);
    *nonzero = false;
    for (size_t i = 0; i < n; ++i) {
        const double d = (h_a ? h_a[i] : 0.0) - (h_b ? h_b[i] : 0.0);
        out[i] = (T)d;
        if (!std::isfinite((double)out[i])) return i;
        if (out[i] != (T)0) *nonzero = true;
    }
    return n;
}
template <typename T>
int set_static_t(AoEnv* env, const double* h_wfs, const double* h_sci, int per_env, hipStream_t st) {
    const size_t E = (size_t)env->E, R2 = (size_t)env->R * env->R, nm = (per_env ? E : 1) * R2;
    std::vector<T> tw, td;
    bool nz_w = false, nz_d = false;
    if (h_wfs)
        if (const size_t i = static_round<T>(h_wfs, nullptr, nm, tw, &nz_w); i < nm)
            return fail("aoenv_set_static_opd: wfs[%zu] = %g is not finite in the env dtype", i, h_wfs[i]);
    if (const size_t i = static_round<T>(h_sci, h_wfs, nm, td, &nz_d); i < nm)
        return fail("aoenv_set_static_opd: science[%zu] - wfs[%zu] is not finite in the env dtype", i, i);
    // (the sensor arm's map is held as given, zeros included: the shard then runs the path of a shard with a map; a difference that
    //  is zero everywhere is not held: the science arm IS the sensor's)
    const bool have_w = h_wfs != nullptr, have_d = nz_d, sep = env->c.dm_separable != 0;
    if (have_w) AO_TRY(require_step_constants(env, false));        // (the surface is formed before this call returns)
    const size_t z = sizeof(T), surf = E * R2 * z;
    const size_t rows = have_w && sep && sizeof(T) == 4 && env->nAct <= 128 ? E * env->dm_layout().ga_elems() * sizeof(float) : 0;
    const size_t cimg = have_w && sep ? E * env->nAct * env->nAct * z : 0;
    const std::initializer_list<size_t> parts = {have_w ? nm * z : 0, have_d ? nm * z : 0, have_w ? surf : 0, rows, cimg, have_d ? surf : 0};
    AO_HIP(hipStreamSynchronize(st));                              // a launch in flight reads the maps in place
    Block mem;                                                     // (built whole before the maps in use are given up; zeroed: the
    if (mem.alloc(parts, true))                                    //  padding of Gy C stays zero from here on)
        return fail("aoenv_set_static_opd: no device memory for %zu bytes of maps, surface and scratch", dev_layout(parts).total);
    if ((have_w && mem.upload(0, tw.data(), nm * z)) || (have_d && mem.upload(1, td.data(), nm * z)))
        return fail("aoenv_set_static_opd: the copy of the maps failed");
    AoEnv::Static& sa = env->stat;
    sa = AoEnv::Static{};
    sa.mem = std::move(mem);
    sa.on = true;
    sa.w = sa.mem.part(0);
    sa.delta = sa.mem.part(1);
    sa.map_env = per_env ? R2 : 0;
    sa.surf = sa.mem.part(2);
    sa.rows = static_cast<float*>(sa.mem.part(3));
    sa.cimg = sa.mem.part(4);
    sa.phase_sci = sa.mem.part(5);
    if (h_wfs) sa.h_w.assign(h_wfs, h_wfs + nm);
    if (h_sci) sa.h_s.assign(h_sci, h_sci + nm);
    if (!env->sci_differs()) {                                     // (no science arm of its own any more: its record goes with it)
        env->oa.rec = nullptr;
        env->oa.i_base = env->oa.n_slots = 0;
    }
    return refresh_dense_dm<T>(env, st);                           // the surface of the command held, with the map
}
}  // namespace
}  // extern "C++"

int aoenv_set_static_opd(AoEnv* env, const double* h_wfs, const double* h_sci, int per_env, void* stream) {
    AO_CHECK_ENV(env);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (!h_wfs && !h_sci) {                                        // no maps: the shard launches what it launched before
        if (env->stat.on) AO_HIP(hipStreamSynchronize(st));
        env->stat = AoEnv::Static{};
        if (!env->sci_differs()) {
            env->oa.rec = nullptr;
            env->oa.i_base = env->oa.n_slots = 0;
        }
        return 0;
    }
    if (per_env != 0 && per_env != env->E)
        return fail("aoenv_set_static_opd: per_env = %d maps, the shard has %d envs (0: one map for the shard)", per_env, env->E);
    const size_t nm = (size_t)(per_env ? env->E : 1) * env->R * env->R;
    const struct { const double* p; const char* name; } arms[] = {{h_wfs, "wfs"}, {h_sci, "science"}};
    for (const auto& a : arms)
        if (a.p)
            if (const size_t i = first_not_finite(a.p, nm); i < nm) return fail("aoenv_set_static_opd: %s[%zu] is not finite", a.name, i);
    return AO_DISPATCH(env, set_static_t, env, h_wfs, h_sci, per_env, st);
}

int aoenv_static_surface_path(AoEnv* env, int64_t* h_launches) {
    if (!env) return -1;
    if (h_launches) std::copy(env->static_launches, env->static_launches + 4, h_launches);
    return env->static_path();
}

int aoenv_get_static_opd(AoEnv* env, double* h_wfs, double* h_sci) {
    AO_CHECK_ENV(env);
    const AoEnv::Static& sa = env->stat;
    if (!sa.on) return fail("aoenv_get_static_opd: no static map is set (aoenv_set_static_opd)");
    const size_t R2 = (size_t)env->R * env->R;
    const struct { double* dst; const std::vector<double>& src; } arms[] = {{h_wfs, sa.h_w}, {h_sci, sa.h_s}};
    for (const auto& a : arms) {
        if (!a.dst) continue;
        for (size_t e = 0; e < (size_t)env->E; ++e)
            for (size_t q = 0; q < R2; ++q) a.dst[e * R2 + q] = a.src.empty() ? 0.0 : a.src[(sa.map_env ? e * R2 : 0) + q];
    }
    return 0;
}

// ---- laser-guide-star spots (sh_lgs.hpp) -------------------------------------------------------------------------------------------
extern "C++" {
namespace {
template <typename T>
int set_lgs_t(AoEnv* env, const double* h_taps, size_t count, int per_env, const int32_t box[4], hipStream_t st) {
    std::vector<T> t(count);
    for (size_t q = 0; q < count; ++q) t[q] = (T)h_taps[q];
    AO_HIP(hipStreamSynchronize(st));                              // a launch in flight reads the table in place
    Block mem;                                                     // (built whole before the table in use is given up)
    if (mem.alloc({count * sizeof(T)}, false)) return fail("aoenv_set_lgs_spots: no device memory for %zu bytes of taps", count * sizeof(T));
    if (mem.upload(0, t.data(), count * sizeof(T))) return fail("aoenv_set_lgs_spots: the copy of the taps failed");
    AoEnv::Lgs& g = env->lgs;
    g = AoEnv::Lgs{};
    g.mem = std::move(mem);
    g.on = true;
    g.taps = g.mem.part(0);
    g.tap_env = per_env ? count / (size_t)env->E : 0;
    std::copy(box, box + 4, g.box);
    g.h_taps.assign(h_taps, h_taps + count);
    return 0;
}
}  // namespace
}  // extern "C++"

int aoenv_set_lgs_spots(AoEnv* env, const double* h_taps, size_t bytes, int per_env, const int32_t box[4], void* stream) {
    AO_CHECK_ENV(env);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (!h_taps) {                                                 // no table: the shard launches what it launched before
        if (env->lgs.on) AO_HIP(hipStreamSynchronize(st));
        env->lgs = AoEnv::Lgs{};
        return 0;
    }
    if (env->c.wfs_type != AOENV_WFS_SH)
        return fail("aoenv_set_lgs_spots: elongated spots belong to the diffractive Shack-Hartmann; this shard's sensor is %s",
                    env->c.wfs_type == AOENV_WFS_PYRAMID ? "a Pyramid" : "the geometric Shack-Hartmann (no spots)");
    if (!box) return fail("aoenv_set_lgs_spots: null box");
    if (per_env != 0 && per_env != env->E)
        return fail("aoenv_set_lgs_spots: per_env = %d tables, the shard has %d envs (0: one table for the shard)", per_env, env->E);
    const int p = env->R / env->nSub, n = 2 * p;
    if (lgs_lenslets_per_group(p, env->esz) == 0)
        return fail("aoenv_set_lgs_spots: %d px per lenslet needs %zu B of LDS for one lenslet", p, lgs_lds_bytes(p, 1, env->esz));
    const int n_tab = per_env ? env->E : 1;
    const LgsCheck c = lgs_validate(h_taps, bytes, n_tab, env->nVal, n, box, env->esz == 4);
    switch (c.verdict) {
    case kLgsOk: break;
    case kLgsBytes:
        return fail("aoenv_set_lgs_spots: %zu bytes, expected %zu = [%d][%d][%d] float64 (per_env = %d, the shard has %d envs)", bytes,
                    (size_t)n_tab * env->nVal * n * n * sizeof(double), n_tab, env->nVal, n * n, per_env, env->E);
    case kLgsBox:
        return fail("aoenv_set_lgs_spots: box {x0 %d, y0 %d, nx %d, ny %d} is not inside [0, %d)", box[0], box[1], box[2], box[3], n);
    case kLgsNotFinite:
        return fail("aoenv_set_lgs_spots: tap [%zu][%zu][%zu] is not finite in the env dtype", c.table, c.lenslet, c.tap);
    case kLgsNegative:
        return fail("aoenv_set_lgs_spots: tap [%zu][%zu][%zu] is negative", c.table, c.lenslet, c.tap);
    case kLgsOutside:
        return fail("aoenv_set_lgs_spots: tap [%zu][%zu][%zu] is not zero and lies outside the box", c.table, c.lenslet, c.tap);
    case kLgsZeroSum:
        return fail("aoenv_set_lgs_spots: the taps of lenslet [%zu][%zu] sum to zero in the env dtype", c.table, c.lenslet);
    }
    return AO_DISPATCH(env, set_lgs_t, env, h_taps, bytes / sizeof(double), per_env, box, st);
}

int aoenv_get_lgs_spots(AoEnv* env, double* h_taps, int32_t* per_env, int32_t box[4]) {
    AO_CHECK_ENV(env);
    const AoEnv::Lgs& g = env->lgs;
    if (!g.on) return fail("aoenv_get_lgs_spots: no table is set (aoenv_set_lgs_spots)");
    if (per_env) *per_env = g.tap_env ? env->E : 0;
    if (box) std::copy(g.box, g.box + 4, box);
    if (h_taps) std::copy(g.h_taps.begin(), g.h_taps.end(), h_taps);
    return 0;
}

// ---- the control delay (delay.hpp) ------------------------------------------------------------------------------------------------
static_assert(kMaxDelay == AOENV_MAX_DELAY, "delay.hpp and aoenv.h disagree");
int aoenv_set_delay(AoEnv* env, int delay, void* stream) {
    AO_CHECK_ENV(env);
    if (delay < 0 || delay > AOENV_MAX_DELAY) return fail("aoenv_set_delay: delay %d outside [0, %d]", delay, AOENV_MAX_DELAY);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (delay > 0) {
        if (!env->delay_ring) {                                    // storage grows once: every delay fits from then on
            const size_t per16 = 16 / env->esz, n = (size_t)env->E * env->nAct * env->nAct;
            const size_t stride = (n + per16 - 1) / per16 * per16;
            AO_HIP(hipStreamSynchronize(st));
            void* p = nullptr;
            AO_TRY(dmalloc(env, &p, (size_t)(kMaxDelay + 1) * stride * env->esz, false));
            env->delay_ring = p;
            env->delay_stride = stride;
        }
        AO_HIP(hipMemsetAsync(env->delay_ring, 0, (size_t)(delay + 1) * env->delay_stride * env->esz, st));
    }
    env->delay = DelayLine{delay, 0};
    return 0;
}

int aoenv_get_delay(AoEnv* env, int* delay) {
    if (!env || !delay) return fail("aoenv_get_delay: null argument");
    *delay = env->delay.d;
    return 0;
}

// the line on the host in logical order, [d][E][nAct^2]: pending row j is ring slot delay_pending_slot(j)
static int delay_line_check(AoEnv* env, const void* h, size_t bytes, const char* who) {
    if (!h) return fail("%s: null host pointer", who);
    if (env->delay.d == 0) return fail("%s: no delay is set (aoenv_set_delay)", who);
    const size_t want = (size_t)env->delay.d * env->E * env->nAct * env->nAct * env->esz;
    if (bytes != want) return fail("%s: got %zu bytes, expected %zu", who, bytes, want);
    return 0;
}

int aoenv_get_delay_line(AoEnv* env, void* h_dst, size_t bytes, void* stream) {
    AO_CHECK_ENV(env);
    AO_TRY(delay_line_check(env, h_dst, bytes, "aoenv_get_delay_line"));
    AO_HIP(hipStreamSynchronize(static_cast<hipStream_t>(stream)));
    const size_t row = (size_t)env->E * env->nAct * env->nAct * env->esz;
    for (int j = 0; j < env->delay.d; ++j)
        AO_HIP(hipMemcpy(static_cast<char*>(h_dst) + (size_t)j * row, env->delay_slot(delay_pending_slot(env->delay, j)), row, hipMemcpyDeviceToHost));
    return 0;
}

int aoenv_set_delay_line(AoEnv* env, const void* h_src, size_t bytes, void* stream) {
    AO_CHECK_ENV(env);
    AO_TRY(delay_line_check(env, h_src, bytes, "aoenv_set_delay_line"));
    AO_HIP(hipStreamSynchronize(static_cast<hipStream_t>(stream)));
    const size_t row = (size_t)env->E * env->nAct * env->nAct * env->esz;
    for (int j = 0; j < env->delay.d; ++j)
        AO_HIP(hipMemcpy(env->delay_slot(delay_pending_slot(env->delay, j)), static_cast<const char*>(h_src) + (size_t)j * row, row, hipMemcpyHostToDevice));
    return 0;
}

extern "C++" {
template <typename T>
static int run_rollout_t(AoEnv* env, const AoRollout* cfg, void* d_obs, void* d_action, void* d_reward, void* d_strehl, void* d_frame,
                         uint32_t counter, hipStream_t st) {
    const size_t img = (size_t)env->nAct * env->nAct, E = env->E;
    T* scratch = env->as<T>(env->rollout_scratch);
    RolloutActionArgs<T> a{};
    a.fr = env->noise_K ? env->as<T>(env->noise_fr) : nullptr;
    a.fl_t = env->noise_K ? env->as<T>(env->noise_fl_t) : nullptr;
    a.act_slot = env->act_slot;
    a.sigma_env = static_cast<const T*>(cfg->d_sigma_env);
    a.gain = (T)cfg->gain;
    a.sigma = (T)cfg->sigma;
    a.n_act = env->nAct;
    a.n_valid_act = env->A;
    a.n_filter = env->noise_K;
    a.seed_lo = (uint32_t)(cfg->seed & 0xffffffffu);
    a.seed_hi = (uint32_t)(cfg->seed >> 32);
    a.env_offset = (uint32_t)cfg->env_index_offset;
    for (int k = 0; k < cfg->n_steps; ++k) {
        const bool last = k == cfg->n_steps - 1;
        a.obs = static_cast<const T*>(d_obs) + (size_t)k * E * img;
        a.action = static_cast<T*>(d_action) + (size_t)k * E * img;
        a.counter = counter + (uint32_t)k;
        AO_TRY(launch_rollout_action<T>(a, env->E, st));
        // the explicit-action step of aoenv_step; only the last step's residual phase and frame can be read afterwards
        // (under a delay the trajectory is the delay line: the action of step k - d, or a pending row of the ring; delay.hpp)
        AO_TRY(step_t<T>(env, cfg->i0 + k, delay_loop_action<T>(env, static_cast<const T*>(d_action), k),
                         static_cast<T*>(d_obs) + (size_t)(k + 1) * E * img, last ? d_frame : nullptr,
                         d_reward ? static_cast<T*>(d_reward) + (size_t)k * E : scratch,
                         d_strehl ? static_cast<T*>(d_strehl) + (size_t)k * E : scratch + E, 0.0, last, st));
    }
    return delay_loop_end<T>(env, static_cast<const T*>(d_action), cfg->n_steps, st);
}
}  // extern "C++"

// what the two recorded rollouts (aoenv_run_rollout, aoenv_run_policy_rollout) refuse alike
static int rollout_check(AoEnv* env, const AoRollout* cfg, const void* d_obs, const void* d_action, const char* who) {
    if (!cfg || !d_obs || !d_action) return fail("%s: null cfg / obs / action", who);
    if (cfg->i0 < 0 || cfg->n_steps < 0 || (int64_t)cfg->i0 + cfg->n_steps > env->c.n_loop)
        return fail("frames [%d, %lld) outside [0, n_loop=%d)", cfg->i0, (long long)cfg->i0 + cfg->n_steps, env->c.n_loop);
    if (!(cfg->sigma >= 0) || !std::isfinite(cfg->sigma)) return fail("%s: sigma must be finite and >= 0", who);
    if (!(cfg->gain >= 0) || !std::isfinite(cfg->gain)) return fail("%s: gain must be finite and >= 0", who);
    AO_TRY(require_step_constants(env, true));
    if (!env->have[AOENV_C_RECON]) return fail("the reconstructor has not been uploaded");
    return wf_window_check(env, cfg->i0, cfg->n_steps);
}

// the inverse of AOENV_C_ACT_IDX on the device
static int ensure_act_slot(AoEnv* env, hipStream_t st) {
    if (!env->act_slot_dirty) return 0;
    const size_t img = (size_t)env->nAct * env->nAct;
    std::vector<int> slot(img, -1);
    for (int i = 0; i < env->A; ++i) slot[env->h_act_idx[i]] = i;
    if (!env->act_slot) AO_TRY(dmalloc(env, (void**)&env->act_slot, img * sizeof(int), false));
    AO_HIP(hipStreamSynchronize(st));
    AO_HIP(hipMemcpy(env->act_slot, slot.data(), img * sizeof(int), hipMemcpyHostToDevice));
    env->act_slot_dirty = false;
    return 0;
}

// the tables a rollout needs, and the position of the exploration stream: it goes on from call to call, only another seed starts
// it again.  Returns the counter of the call's first step and leaves counter + n_steps behind.
static int rollout_begin(AoEnv* env, const AoRollout* cfg, hipStream_t st, uint32_t* counter) {
    AO_TRY(ensure_act_slot(env, st));
    if (!env->rollout_scratch) AO_TRY(dmalloc(env, &env->rollout_scratch, (size_t)2 * env->E * env->esz));
    *counter = (env->explore_seeded && env->explore_seed != cfg->seed) ? 0 : env->explore_counter;
    env->explore_seed = cfg->seed;
    env->explore_seeded = true;
    env->explore_counter = *counter + (uint32_t)cfg->n_steps;
    return 0;
}

int aoenv_run_rollout(AoEnv* env, const AoRollout* cfg, void* d_obs, void* d_action, void* d_reward, void* d_strehl, void* d_frame,
                      void* stream) {
    AO_CHECK_ENV(env);
    AO_TRY(rollout_check(env, cfg, d_obs, d_action, "aoenv_run_rollout"));
    if (rollout_action_lds(env->A, env->noise_K, env->esz) > kRolloutLdsMax)
        return fail("aoenv_run_rollout: %d actuators and filter rank %d need %zu bytes of LDS, a workgroup has %zu", env->A, env->noise_K,
                    rollout_action_lds(env->A, env->noise_K, env->esz), kRolloutLdsMax);
    if (cfg->n_steps == 0) return 0;
    hipStream_t st = static_cast<hipStream_t>(stream);
    uint32_t counter = 0;
    AO_TRY(rollout_begin(env, cfg, st, &counter));
    return AO_DISPATCH(env, run_rollout_t, env, cfg, d_obs, d_action, d_reward, d_strehl, d_frame, counter, st);
}

// ---- the policy (policy.hpp) ---------------------------------------------------------------------------------------------------
int aoenv_set_policy(AoEnv* env, const AoPolicy* cfg, void* stream) {
    AO_CHECK_ENV(env);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (!cfg) {
        AO_HIP(hipStreamSynchronize(st));
        env->policy = AoEnv::Policy{};
        return 0;
    }
    const int H = cfg->n_history, F = cfg->n_filt, Kp = cfg->proj_rank, A = env->A;
    if (H < 1 || H > kPolicyMaxHistory) return fail("aoenv_set_policy: n_history %d outside [1, %d]", H, kPolicyMaxHistory);
    if (F < 1 || F > kPolicyMaxFilt) return fail("aoenv_set_policy: n_filt %d outside [1, %d]", F, kPolicyMaxFilt);
    if (Kp < 0 || Kp > A) return fail("aoenv_set_policy: proj_rank %d outside [0, A=%d]", Kp, A);
    if (cfg->path != 0 && cfg->path != 1) return fail("aoenv_set_policy: path %d is neither 0 nor 1", cfg->path);
    if (!std::isfinite(cfg->negative_slope)) return fail("aoenv_set_policy: negative_slope is not finite");
    if (!(cfg->clamp_abs > 0)) return fail("aoenv_set_policy: clamp_abs must be > 0");
    if (!cfg->h_w1 || !cfg->h_b1 || !cfg->h_w2 || !cfg->h_b2 || !cfg->h_w3 || !cfg->h_b3 || (Kp > 0 && !cfg->h_proj))
        return fail("aoenv_set_policy: null weights");
    const int C1 = 2 * H - 1;
    const size_t n1 = (size_t)F * C1 * 9, n2 = (size_t)F * F * 9, n3 = (size_t)F * 9, np = (size_t)Kp * A;
    const struct { const double* p; size_t n; const char* name; } arrays[] = {
        {cfg->h_w1, n1, "w1"}, {cfg->h_b1, (size_t)F, "b1"}, {cfg->h_w2, n2, "w2"}, {cfg->h_b2, (size_t)F, "b2"},
        {cfg->h_w3, n3, "w3"}, {cfg->h_b3, 1, "b3"}, {cfg->h_proj, 2 * np, "proj"}};
    for (const auto& a : arrays)
        if (const size_t i = first_not_finite(a.p, a.n); i < a.n) return fail("aoenv_set_policy: %s[%zu] is not finite", a.name, i);
    AO_HIP(hipStreamSynchronize(st));                              // an evaluation in flight reads the old policy in place
    AoEnv::Policy p;                                               // (a failed build frees it on return: the policy in use stays)
    p.H = H; p.F = F; p.Kp = Kp;
    p.slope = cfg->negative_slope; p.clamp_abs = cfg->clamp_abs; p.b3 = cfg->h_b3[0];
    p.mfma = policy_uses_mfma(env->esz, cfg->path, F, env->nAct, C1);
    const size_t z = env->esz, hid = (size_t)env->E * F * env->nAct * env->nAct * z;
    std::vector<float> t1, t2;                                     // the wide layers re-laid; absent off the MFMA path
    if (p.mfma) {
        policy_relayout(cfg->h_w1, F, C1, t1);
        policy_relayout(cfg->h_w2, F, F, t2);
    }
    AO_TRY(block_alloc(p.mem, {n1 * z, F * z, n2 * z, F * z, n3 * z, t1.size() * 4, t2.size() * 4, np * z, np * z, hid, hid}, false));
    void** field[] = {&p.w1, &p.b1, &p.w2, &p.b2, &p.w3, &p.wt1, &p.wt2, &p.proj_fr, &p.proj_fl_t, &p.hid1, &p.hid2};
    for (int k = 0; k < 11; ++k) *field[k] = p.mem.part(k);
    AO_TRY(upload_real(env, p.w1, cfg->h_w1, n1));
    AO_TRY(upload_real(env, p.b1, cfg->h_b1, F));
    AO_TRY(upload_real(env, p.w2, cfg->h_w2, n2));
    AO_TRY(upload_real(env, p.b2, cfg->h_b2, F));
    AO_TRY(upload_real(env, p.w3, cfg->h_w3, n3));
    if (p.mfma) {
        AO_HIP(hipMemcpy(p.wt1, t1.data(), t1.size() * 4, hipMemcpyHostToDevice));
        AO_HIP(hipMemcpy(p.wt2, t2.data(), t2.size() * 4, hipMemcpyHostToDevice));
    }
    if (Kp > 0) {
        AO_TRY(upload_real(env, p.proj_fr, cfg->h_proj, np));
        AO_TRY(upload_transposed(env, p.proj_fl_t, cfg->h_proj + np, A, Kp));   // Fl [A][K] -> [K][A], as aoenv_set_noise_filter
    }
    p.set = true;
    env->policy = std::move(p);
    return 0;
}

extern "C++" {
// one evaluation: two wide convolutions and the last stage; `in` names the first layer's channels, `aa` carries the noise
template <typename T>
static int policy_eval_t(AoEnv* env, ConvIn<T> in, PolicyActionArgs<T> aa, hipStream_t st) {
    const AoEnv::Policy& p = env->policy;
    const int F = p.F, E = env->E, nAct = env->nAct, img = nAct * nAct;
    T *h1 = env->as<T>(p.hid1), *h2 = env->as<T>(p.hid2);
    in.plain = nullptr; in.H = p.H; in.C = 2 * p.H - 1; in.E = E; in.img = img;
    ConvIn<T> in2{};
    in2.plain = h1; in2.C = F; in2.E = E; in2.img = img;
    bool done = false;
    if constexpr (sizeof(T) == 4) {
        if (p.mfma) {
            AO_TRY(launch_policy_conv_mfma(in, env->as<float>(p.wt1), env->as<float>(p.b1), h1, nAct, F, (float)p.slope, E, st));
            AO_TRY(launch_policy_conv_mfma(in2, env->as<float>(p.wt2), env->as<float>(p.b2), h2, nAct, F, (float)p.slope, E, st));
            done = true;
        }
    }
    if (!done) {
        AO_TRY(launch_policy_conv_general<T>(in, env->as<T>(p.w1), env->as<T>(p.b1), h1, nAct, F, (T)p.slope, E, st));
        AO_TRY(launch_policy_conv_general<T>(in2, env->as<T>(p.w2), env->as<T>(p.b2), h2, nAct, F, (T)p.slope, E, st));
    }
    aa.hidden = h2;
    aa.w3 = env->as<T>(p.w3);
    aa.b3 = (T)p.b3;
    aa.clamp_abs = (T)p.clamp_abs;
    aa.proj_fr = p.Kp ? env->as<T>(p.proj_fr) : nullptr;
    aa.proj_fl_t = p.Kp ? env->as<T>(p.proj_fl_t) : nullptr;
    aa.act_slot = env->act_slot;
    aa.n_act = nAct; aa.n_valid_act = env->A; aa.n_filt = F; aa.proj_rank = p.Kp;
    return launch_policy_action<T>(aa, E, st);
}

template <typename T>
static int policy_forward_t(AoEnv* env, const void* d_obs, const void* d_past_obs, const void* d_past_act, void* d_action, hipStream_t st) {
    ConvIn<T> in{};
    in.obs = static_cast<const T*>(d_obs);
    in.past_obs = static_cast<const T*>(d_past_obs);
    in.past_act = static_cast<const T*>(d_past_act);
    in.k = 0;                                                      // every past channel from the caller's windows
    PolicyActionArgs<T> aa{};
    aa.action = static_cast<T*>(d_action);                         // sigma = 0: no noise
    return policy_eval_t<T>(env, in, aa, st);
}

template <typename T>
static int run_policy_rollout_t(AoEnv* env, const AoRollout* cfg, void* d_obs, void* d_action, void* d_reward, void* d_strehl,
                                void* d_frame, void* d_past_obs, void* d_past_act, uint32_t counter, hipStream_t st) {
    const size_t img = (size_t)env->nAct * env->nAct, E = env->E;
    T* scratch = env->as<T>(env->rollout_scratch);
    ConvIn<T> in{};
    in.obs = static_cast<const T*>(d_obs);
    in.act = static_cast<const T*>(d_action);
    in.past_obs = static_cast<const T*>(d_past_obs);
    in.past_act = static_cast<const T*>(d_past_act);
    PolicyActionArgs<T> aa{};
    aa.fr = env->noise_K ? env->as<T>(env->noise_fr) : nullptr;
    aa.fl_t = env->noise_K ? env->as<T>(env->noise_fl_t) : nullptr;
    aa.sigma_env = static_cast<const T*>(cfg->d_sigma_env);
    aa.sigma = (T)cfg->sigma;
    aa.n_filter = env->noise_K;
    aa.seed_lo = (uint32_t)(cfg->seed & 0xffffffffu);
    aa.seed_hi = (uint32_t)(cfg->seed >> 32);
    aa.env_offset = (uint32_t)cfg->env_index_offset;
    for (int k = 0; k < cfg->n_steps; ++k) {
        const bool last = k == cfg->n_steps - 1;
        in.k = k;
        aa.action = static_cast<T*>(d_action) + (size_t)k * E * img;
        aa.counter = counter + (uint32_t)k;
        AO_TRY(policy_eval_t<T>(env, in, aa, st));
        AO_TRY(step_t<T>(env, cfg->i0 + k, delay_loop_action<T>(env, static_cast<const T*>(d_action), k),
                         static_cast<T*>(d_obs) + (size_t)(k + 1) * E * img, last ? d_frame : nullptr,
                         d_reward ? static_cast<T*>(d_reward) + (size_t)k * E : scratch,
                         d_strehl ? static_cast<T*>(d_strehl) + (size_t)k * E : scratch + E, 0.0, last, st));
    }
    AO_TRY(delay_loop_end<T>(env, static_cast<const T*>(d_action), cfg->n_steps, st));
    // the windows n_steps iterations of mbrl.py:80-81 leave (the trajectory is complete: stream order)
    AO_TRY(launch_policy_roll<T>(static_cast<T*>(d_past_obs), static_cast<const T*>(d_obs), cfg->n_steps, env->policy.H, env->E, (int)img, st));
    return launch_policy_roll<T>(static_cast<T*>(d_past_act), static_cast<const T*>(d_action), cfg->n_steps, env->policy.H, env->E, (int)img, st);
}
}  // extern "C++"

static int policy_ready(AoEnv* env, const char* who) {
    if (!env->policy.set) return fail("%s: no policy has been set (aoenv_set_policy)", who);
    if (!env->have[AOENV_C_ACT_IDX]) return fail("constant table %d has not been uploaded", (int)AOENV_C_ACT_IDX);
    if (policy_action_lds(env->A, env->policy.Kp, env->noise_K, env->esz) > kPolicyLdsMax)
        return fail("%s: %d actuators and ranks %d / %d need %zu bytes of LDS, a workgroup has %zu", who, env->A, env->policy.Kp,
                    env->noise_K, policy_action_lds(env->A, env->policy.Kp, env->noise_K, env->esz), kPolicyLdsMax);
    return 0;
}

int aoenv_policy_forward(AoEnv* env, const void* d_obs, const void* d_past_obs, const void* d_past_act, void* d_action, void* stream) {
    AO_CHECK_ENV(env);
    AO_TRY(policy_ready(env, "aoenv_policy_forward"));
    if (!d_obs || !d_action) return fail("aoenv_policy_forward: null obs / action");
    if (env->policy.H > 1 && (!d_past_obs || !d_past_act)) return fail("aoenv_policy_forward: null history with n_history = %d", env->policy.H);
    hipStream_t st = static_cast<hipStream_t>(stream);
    AO_TRY(ensure_act_slot(env, st));
    return AO_DISPATCH(env, policy_forward_t, env, d_obs, d_past_obs, d_past_act, d_action, st);
}

int aoenv_run_policy_rollout(AoEnv* env, const AoRollout* cfg, void* d_obs, void* d_action, void* d_reward, void* d_strehl,
                             void* d_frame, void* d_past_obs, void* d_past_act, void* stream) {
    AO_CHECK_ENV(env);
    AO_TRY(policy_ready(env, "aoenv_run_policy_rollout"));
    AO_TRY(rollout_check(env, cfg, d_obs, d_action, "aoenv_run_policy_rollout"));
    if (cfg->gain != 0) return fail("aoenv_run_policy_rollout: gain must be 0 (a residual controller is out of scope), got %g", cfg->gain);
    if (env->policy.H > 1 && (!d_past_obs || !d_past_act))
        return fail("aoenv_run_policy_rollout: null history with n_history = %d", env->policy.H);
    if (cfg->n_steps == 0) return 0;
    hipStream_t st = static_cast<hipStream_t>(stream);
    uint32_t counter = 0;
    AO_TRY(rollout_begin(env, cfg, st, &counter));
    return AO_DISPATCH(env, run_policy_rollout_t, env, cfg, d_obs, d_action, d_reward, d_strehl, d_frame, d_past_obs, d_past_act, counter, st);
}

extern "C++" {
// Odd R: the reference pads ceil((2 M - R) / 2) pixels on both sides and transforms at 2 M + 1 (Telescope.py:320-325), a length
// the transform below (2 M points, the field centred on one of them) does not take.  The whole image is then the science window
// with W = M (science.hpp: the DFT rows as a table, two products per env), from scratch of this call.
template <typename T>
static int compute_psf_odd_t(AoEnv* env, int zp, void* d_psf, hipStream_t st) {
    const int R = env->R, M = zp * R;
    const size_t R2 = (size_t)R * R;
    if (env->h_amp.size() != R2) return fail("the WFS amplitude has not been uploaded");
    const SciGeom g = sci_geom(R, zp, M);
    const SciPlan pl = sci_plan(R, M);
    const size_t nt = sci_table_elems(pl);
    std::vector<T> host(nt + R2);
    sci_fill_table<T>(g, pl, nullptr, host.data());
    const double scale = env->c.wfs_type == AOENV_WFS_PYRAMID ? std::sqrt((double)env->c.pyr_n_theta) : 1.0;
    for (size_t q = 0; q < R2; ++q) host[nt + q] = (T)(env->h_amp[q] * scale);
    Block tmp;
    AO_TRY(block_alloc(tmp, {host.size() * sizeof(T)}, false));
    T* d_tab = static_cast<T*>(tmp.part(0));
    AO_HIP(hipMemcpyAsync(d_tab, host.data(), host.size() * sizeof(T), hipMemcpyHostToDevice, st));
    SciArgs<T> a{};
    a.phase = env->as<T>(env->phase);
    a.table = d_tab;
    a.amp = d_tab + nt;
    a.out = static_cast<T*>(d_psf);
    a.scale = sci_scale<T>(g);
    a.n_env = env->E;
    a.R = R;
    a.W = M;
    AO_TRY(launch_science_window<T>(a, (env->force_path & AOENV_PATH_SCI_GENERAL) != 0, st));
    AO_HIP(hipStreamSynchronize(st));                              // the scratch is released on return
    return 0;
}

template <typename T>
static int compute_psf_t(AoEnv* env, int zp, void* d_psf, hipStream_t st) {
    if (env->R % 2) return compute_psf_odd_t<T>(env, zp, d_psf, st);
    // the reference runs the transform at oversampling 2 for every even image size and sum-bins |.|^2 2 x 2 (Telescope.py:303-305)
    const int R = env->R, N = 2 * zp * R;
    const size_t R2 = (size_t)R * R;
    // scratch of one call: amplitude pupil * sqrt(src.fluxMap) (= the SH field amplitude; the Pyramid's is per modulation
    // point), twiddles, first-pass output
    Block tmp;
    AO_TRY(block_alloc(tmp, {R2 * sizeof(T), (size_t)2 * N * sizeof(T), (size_t)env->E * R * N * 2 * sizeof(T)}, false));
    T *d_amp = static_cast<T*>(tmp.part(0)), *d_tw = static_cast<T*>(tmp.part(1));
    void* d_t1 = tmp.part(2);
    if (env->h_amp.size() != R2) return fail("the WFS amplitude has not been uploaded");
    const double scale = env->c.wfs_type == AOENV_WFS_PYRAMID ? std::sqrt((double)env->c.pyr_n_theta) : 1.0;
    std::vector<T> amp(R2), tw(2 * (size_t)N);
    for (size_t q = 0; q < R2; ++q) amp[q] = (T)(env->h_amp[q] * scale);
    const double pi = 3.14159265358979323846;
    for (int k = 0; k < N; ++k) { tw[2 * k] = (T)std::cos(2 * pi * k / N); tw[2 * k + 1] = (T)(-std::sin(2 * pi * k / N)); }
    AO_HIP(hipMemcpyAsync(d_amp, amp.data(), R2 * sizeof(T), hipMemcpyHostToDevice, st));
    AO_HIP(hipMemcpyAsync(d_tw, tw.data(), tw.size() * sizeof(T), hipMemcpyHostToDevice, st));
    PyrArgs<T> pa{};
    AO_TRY(make_fft_plan(N, &pa.plan));
    pa.phase = env->as<T>(env->phase);
    pa.amp = d_amp;
    pa.tt = nullptr;
    pa.tw = d_tw;
    pa.t1 = reinterpret_cast<cx<T>*>(d_t1);
    pa.R = R;
    pa.N = N;
    pa.off = N / 2 - R / 2;                                        // pad_width = (N - R) / 2
    pa.phasor_mult = 1;                                            // exp(-i pi / N (x + y)): even image sizes (Telescope.py:316)
    pa.n_env = env->E;
    AO_TRY(launch_psf<T>(pa, static_cast<T*>(d_psf), st));
    AO_HIP(hipStreamSynchronize(st));                              // the scratch is released on return
    return 0;
}
}  // extern "C++"

int aoenv_compute_psf(AoEnv* env, int zero_padding, void* d_psf, void* stream) {
    AO_CHECK_ENV(env);
    if (!d_psf) return fail("null psf");
    if (zero_padding < 1 || zero_padding > 8) return fail("zeroPaddingFactor %d outside [1, 8]", zero_padding);
    if ((zero_padding * env->R) % 2) return fail("odd image sizes are not built");
    if (2 * zero_padding * env->R > 8192) return fail("PSF transform length %d too long", 2 * zero_padding * env->R);
    hipStream_t st = static_cast<hipStream_t>(stream);
    return AO_DISPATCH(env, compute_psf_t, env, zero_padding, d_psf, st);
}

int aoenv_set_detector(AoEnv* env, const AoDetector* cfg, void* stream) {
    AO_CHECK_ENV(env);
    hipStream_t st = static_cast<hipStream_t>(stream);
    DetectorCfg d{};
    if (cfg) {
        if (cfg->bits < 0 || cfg->bits > 24) return fail("detector: bits %d outside [0, 24]", cfg->bits);
        if (cfg->bits > 0 && !(cfg->fwc > 0)) return fail("detector: the ADC needs a full-well capacity (FWC = None with bits set is not built)");
        if (!(cfg->qe > 0) || !(cfg->gain > 0) || cfg->dark_electrons < 0 || cfg->readout_noise < 0 || cfg->fwc < 0)
            return fail("detector: QE and gain must be positive, dark current / read-out noise / FWC non-negative");
        d.active = 1;
        d.photon_noise = cfg->photon_noise != 0;
        d.bits = cfg->bits;
        d.emccd = cfg->emccd != 0;
        d.qe = (float)cfg->qe;
        d.dark_e = (float)cfg->dark_electrons;
        d.fwc = (float)cfg->fwc;
        d.gain = (float)cfg->gain;
        d.readout_noise = (float)cfg->readout_noise;
        d.seed_lo = (uint32_t)(cfg->seed & 0xffffffffu);
        d.seed_hi = (uint32_t)(cfg->seed >> 32);
        d.env_offset = (uint32_t)cfg->env_index_offset;
        // the noise streams keep counting frames across camera changes: only a new seed starts them again
        d.frame_counter = (env->det_seeded && env->det.seed_lo == d.seed_lo && env->det.seed_hi == d.seed_hi) ? env->det.frame_counter : 0;
        // identity settings are the ideal camera: keep the fast paths
        if (!d.photon_noise && d.bits == 0 && d.qe == 1.f && d.dark_e == 0.f && d.fwc == 0.f && d.gain == 1.f && d.readout_noise == 0.f)
            d.active = 0;
    }
    if (env->geometric()) return 0;                                // checked and accepted, no effect: no frame, no noise, no frame counted
    if (env->det.active)                                           // no stale noise outside the valid lenslets (the new camera may not write there)
        AO_HIP(hipMemsetAsync(env->frame, 0, (size_t)env->E * env->c.cam_res * env->c.cam_res * env->esz, st));
    if (!cfg) {                                                    // ideal detector: the stream position and its seed are kept
        d.seed_lo = env->det.seed_lo; d.seed_hi = env->det.seed_hi; d.frame_counter = env->det.frame_counter;
        d.env_offset = env->det.env_offset;
    } else {
        env->det_seeded = true;
    }
    env->det = d;
    return 0;
}

int aoenv_set_return_accumulator(AoEnv* env, void* d_return) {
    AO_CHECK_ENV(env);
    env->ret_acc = d_return;
    return 0;
}

int aoenv_buffer(AoEnv* env, int which, void** d_ptr, size_t* bytes) {
    AO_CHECK_ENV(env);
    BufInfo b{};
    AO_TRY(buf_info(env, which, &b));
    if (which == AOENV_B_SCREEN || which == AOENV_B_MT_STATE || which == AOENV_B_COUNTERS)
        return fail("buffer %d has no flat device image (tori / host-side state): use aoenv_download / aoenv_upload_state", which);
    if (d_ptr) *d_ptr = b.ptr;
    if (bytes) *bytes = b.bytes;
    return 0;
}

int aoenv_download(AoEnv* env, int which, void* h_dst, size_t bytes, void* stream) {
    AO_CHECK_ENV(env);
    BufInfo b{};
    AO_TRY(buf_info(env, which, &b));
    if (bytes != b.bytes) return fail("aoenv_download(%d): got %zu bytes, expected %zu", which, bytes, b.bytes);
    hipStream_t st = static_cast<hipStream_t>(stream);
    AO_HIP(hipStreamSynchronize(st));
    if (which == AOENV_B_SCREEN) {
        AO_TRY(AO_DISPATCH(env, flush_rings, env, st));
        AO_HIP(hipStreamSynchronize(st));
        // the device keeps every screen as a torus: hand back the logical layer.mapShift
        const size_t z = env->esz;
        std::vector<char> tmp;
        std::vector<EnvClock> clk_h;
        if (env->per_env_wind) AO_TRY(pull_env_clocks(env, clk_h));
        for (int l = 0; l < env->L; ++l) {
            const Layer& y = env->layer[l];
            const int S = y.S;
            const size_t per = (size_t)env->E * S * S * z;
            tmp.resize(per);
            AO_HIP(hipMemcpy(tmp.data(), env->screen_ptr(l), per, hipMemcpyDeviceToHost));
            char* dst = static_cast<char*>(h_dst) + y.scr_off * z;
            for (int e = 0; e < env->E; ++e) {
                const int* org = env->per_env_wind ? clk_h[(size_t)l * env->E + e].org : y.org;
                const int oy = org[0], ox = org[1];
                for (int r = 0; r < S; ++r) {
                    const char* srow = tmp.data() + ((size_t)e * S * S + (size_t)((r + oy) % S) * S) * z;
                    char* drow = dst + ((size_t)e * S * S + (size_t)r * S) * z;
                    std::memcpy(drow, srow + (size_t)ox * z, (size_t)(S - ox) * z);
                    std::memcpy(drow + (size_t)(S - ox) * z, srow, (size_t)ox * z);
                }
            }
        }
        return 0;
    }
    if (which == AOENV_B_MT_STATE) {
        const size_t n = (size_t)env->L * env->E;
        std::vector<uint32_t> st_(n * kMtN);
        std::vector<int> pos(n);
        for (int l = 0; l < env->L; ++l) {                         // the committed copy of every layer (a look-ahead writes the other)
            AO_HIP(hipMemcpy(&st_[(size_t)l * env->E * kMtN], env->layer[l].mt_cur, (size_t)env->E * kMtN * 4, hipMemcpyDeviceToHost));
            AO_HIP(hipMemcpy(&pos[(size_t)l * env->E], env->layer[l].pos_cur, (size_t)env->E * 4, hipMemcpyDeviceToHost));
        }
        uint32_t* out = static_cast<uint32_t*>(h_dst);
        for (size_t i = 0; i < n; ++i) {
            std::memcpy(out + i * (kMtN + 1), &st_[i * kMtN], kMtN * 4);
            out[i * (kMtN + 1) + kMtN] = (uint32_t)pos[i];
        }
        return 0;
    }
    if (which == AOENV_B_COUNTERS) {
        uint32_t* out = static_cast<uint32_t*>(h_dst);
        out[0] = env->det.frame_counter; out[1] = env->explore_counter; out[2] = out[3] = 0;
        return 0;
    }
    if (which == AOENV_B_OPD_ATM && env->L > 0 && !env->atm_user_defined && !env->store_opd_atm) {
        // not written by the step kernels unless AOENV_OPT_STORE_ATM_OPD: re-derive it from the screens now
        // (same kernel, same sampling constants; the residual phase it rewrites is identical)
        AO_TRY(AO_DISPATCH(env, run_phase, env, 1, 1, st, 0));
        AO_HIP(hipStreamSynchronize(st));
    }
    AO_HIP(hipMemcpy(h_dst, b.ptr, bytes, hipMemcpyDeviceToHost));
    return 0;
}

int aoenv_get_phase_no_pupil(AoEnv* env, void* h_dst, size_t bytes, void* stream) {
    AO_CHECK_ENV(env);
    if (!h_dst) return fail("aoenv_get_phase_no_pupil: null destination");
    if (!env->phase_np) return fail("aoenv_get_phase_no_pupil: the unmasked phase is kept by geometric shards only (AOENV_WFS_SH_GEOMETRIC)");
    const size_t want = (size_t)env->E * env->R * env->R * env->esz;
    if (bytes != want) return fail("aoenv_get_phase_no_pupil: got %zu bytes, expected %zu", bytes, want);
    AO_HIP(hipStreamSynchronize(static_cast<hipStream_t>(stream)));
    AO_HIP(hipMemcpy(h_dst, env->phase_np, bytes, hipMemcpyDeviceToHost));
    return 0;
}

int aoenv_upload_state(AoEnv* env, int which, const void* h_src, size_t bytes, void* stream) {
    AO_CHECK_ENV(env);
    BufInfo b{};
    AO_TRY(buf_info(env, which, &b));
    if (bytes != b.bytes) return fail("aoenv_upload_state(%d): got %zu bytes, expected %zu", which, bytes, b.bytes);
    hipStream_t st = static_cast<hipStream_t>(stream);
    AO_HIP(hipStreamSynchronize(st));
    if (which == AOENV_B_SCREEN) {
        // logical layer.mapShift of every env: the tori restart at origin 0; the clip range is re-derived by its next consumer
        AO_TRY(screens_replaced(env, false));                      // (the clocks' accumulators are kept)
        for (int l = 0; l < env->L; ++l) {
            const Layer& y = env->layer[l];
            const size_t per = (size_t)env->E * y.S * y.S * env->esz;
            AO_HIP(hipMemcpy(env->screen_ptr(l), static_cast<const char*>(h_src) + y.scr_off * env->esz, per, hipMemcpyHostToDevice));
        }
        return 0;
    }
    if (which == AOENV_B_MT_STATE) {
        const size_t n = (size_t)env->L * env->E;
        std::vector<uint32_t> st_(n * kMtN);
        std::vector<int> pos(n);
        const uint32_t* in = static_cast<const uint32_t*>(h_src);
        for (size_t i = 0; i < n; ++i) {
            std::memcpy(&st_[i * kMtN], in + i * (kMtN + 1), kMtN * 4);
            pos[i] = (int)in[i * (kMtN + 1) + kMtN];
            if (pos[i] < 0 || pos[i] > kMtN || pos[i] % 4) return fail("MT19937 position %d is not a multiple of 4 in [0, 624]", pos[i]);
        }
        for (int l = 0; l < env->L; ++l) {
            forget_lookahead(env->layer[l]);
            AO_HIP(hipMemcpy(env->layer[l].mt_cur, &st_[(size_t)l * env->E * kMtN], (size_t)env->E * kMtN * 4, hipMemcpyHostToDevice));
            AO_HIP(hipMemcpy(env->layer[l].pos_cur, &pos[(size_t)l * env->E], (size_t)env->E * 4, hipMemcpyHostToDevice));
        }
        return 0;
    }
    if (which == AOENV_B_COUNTERS) {
        env->det.frame_counter = static_cast<const uint32_t*>(h_src)[0];
        env->explore_counter = static_cast<const uint32_t*>(h_src)[1];
        env->explore_seeded = false;                               // the uploaded position belongs to the seed of the next rollout
        return 0;
    }
    AO_HIP(hipMemcpy(b.ptr, h_src, bytes, hipMemcpyHostToDevice));
    if (which == AOENV_B_COEFS) return AO_DISPATCH(env, refresh_dense_dm, env, st);
    return 0;
}

int aoenv_get_buff(AoEnv* env, double* h_buff) {
    if (!env || !h_buff) return fail("null argument");
    if (env->per_env_wind) return fail("the shard runs per-env clocks (aoenv_set_wind_env): use aoenv_get_clock_env");
    for (int l = 0; l < env->L; ++l) { h_buff[2 * l] = env->layer[l].clk.buff[0]; h_buff[2 * l + 1] = env->layer[l].clk.buff[1]; }
    return 0;
}

int aoenv_set_buff(AoEnv* env, const double* h_buff) {
    if (!env || !h_buff) return fail("null argument");
    if (env->per_env_wind) return fail("the shard runs per-env clocks (aoenv_set_wind_env): use aoenv_set_clock_env");
    for (int l = 0; l < env->L; ++l) {
        if (std::fabs(h_buff[2 * l]) >= 1 || std::fabs(h_buff[2 * l + 1]) >= 1) return fail("|buff| must be < 1");
        env->layer[l].clk.buff[0] = h_buff[2 * l]; env->layer[l].clk.buff[1] = h_buff[2 * l + 1];
    }
    return 0;
}

int aoenv_fused_step_active(AoEnv* env) {
    if (!env) return 0;
    return env->c.dtype == AOENV_F32 && fused_step_ok<float>(env) ? 1 : 0;
}

int aoenv_set_option(AoEnv* env, int option, int value) {
    AO_CHECK_ENV(env);
    switch (option) {
        case AOENV_OPT_FAST_WFS: env->use_fast_wfs = value != 0; return 0;
        case AOENV_OPT_MFMA_GEMM: env->use_mfma = value != 0; return 0;
        case AOENV_OPT_FAST_TRIG: env->use_fast_trig = value != 0; return 0;
        case AOENV_OPT_STORE_ATM_OPD: env->store_opd_atm = value != 0; return 0;
        case AOENV_OPT_FUSED_TAIL: env->use_fused_tail = value != 0; return 0;
        case AOENV_OPT_FUSED_STEP: env->use_fused_step = value != 0; return 0;
        case AOENV_OPT_STEP_PAIRS: env->use_step_pairs = value != 0; return 0;
        case AOENV_OPT_DEFER_RING: env->defer_ring = value != 0; return 0;
        case AOENV_OPT_FACTORED_RECON: env->use_factored_recon = value != 0; return 0;
        case AOENV_OPT_RING_LOOKAHEAD:
            if (!value)
                for (int l = 0; l < env->L; ++l) forget_lookahead(env->layer[l]);
            env->use_lookahead = value != 0;
            return 0;
        case AOENV_OPT_COEFS_IMAGE:
            if (value) AO_TRY(alloc_dm_rows(env));
            env->use_coefs_img = value != 0;
            return 0;
        case AOENV_OPT_ENV_WIND_PIXELS:
            if (value < 1 || value > 8) return fail("AOENV_OPT_ENV_WIND_PIXELS: %d outside [1, 8]", value);
            if (env->per_env_wind)                                 // (Layer::env_rounds is the largest floor |ratio| the clocks hold)
                for (int l = 0; l < env->L; ++l)
                    if (env->layer[l].env_rounds >= value)
                        return fail("AOENV_OPT_ENV_WIND_PIXELS: layer %d holds a per-env wind of %d px/frame or more, the ceiling cannot go to %d",
                                    l, env->layer[l].env_rounds, value);
            env->wind_pixels = value;
            return 0;
        case AOENV_OPT_FORCE_PATH:
            if (value & ~(AOENV_PATH_PHASE_DWORD | AOENV_PATH_GENERIC | AOENV_PATH_PYR_ROUND_ROBIN | AOENV_PATH_MODAL_GEMM | AOENV_PATH_SH_PLAIN |
                          AOENV_PATH_WF_GENERAL | AOENV_PATH_SCI_GENERAL | AOENV_PATH_DM_PAIRS_GENERAL | AOENV_PATH_DM_STATIC_GENERAL))
                return fail("AOENV_OPT_FORCE_PATH: %d is not a combination of AOENV_PATH_* bits", value);
            env->force_path = value;
            return 0;
        default: return fail("unknown option %d", option);
    }
}

int aoenv_profile(AoEnv* env, int enable) {
    AO_CHECK_ENV(env);
    for (auto& e : env->prof_ev) { (void)hipEventDestroy(e.a); (void)hipEventDestroy(e.b); }
    env->prof_ev.clear();
    env->prof_on = enable != 0;
    if (enable) env->step_launches = env->step_covered = 0;
    return 0;
}

int aoenv_step_counters(AoEnv* env, int64_t* h_out) {
    AO_CHECK_ENV(env);
    if (!h_out) return fail("null argument");
    h_out[0] = env->step_launches;
    h_out[1] = env->step_covered;
    return 0;
}

int aoenv_profile_read(AoEnv* env, double* h_ms, int32_t* h_count, void* stream) {
    AO_CHECK_ENV(env);
    if (!h_ms || !h_count) return fail("null argument");
    AO_HIP(hipStreamSynchronize(static_cast<hipStream_t>(stream)));
    for (int k = 0; k < AOENV_K_COUNT; ++k) { h_ms[k] = 0; h_count[k] = 0; }
    for (auto& e : env->prof_ev) {
        float ms = 0;
        AO_HIP(hipEventElapsedTime(&ms, e.a, e.b));
        h_ms[e.stage] += ms;
        h_count[e.stage] += e.n;
    }
    return 0;
}

int aoenv_test_normal(int device, uint32_t seed, int n, int n_calls, double* h_out) {
    if (n < 2 || n % 2 || n_calls < 1 || !h_out) return fail("aoenv_test_normal: bad arguments");
    DeviceGuard ao_device_guard(device);
    if (!ao_device_guard.ok) return fail("hipSetDevice(%d) failed", device);
    Block mem;                                                     // state, position, one call's draws, the seed
    AO_TRY(block_alloc(mem, {kMtN * 4, 4, (size_t)n * 8, 4}, false));
    uint32_t* st = static_cast<uint32_t*>(mem.part(0));
    int* pos = static_cast<int*>(mem.part(1));
    double* zx = static_cast<double*>(mem.part(2));
    uint32_t* d_seed = static_cast<uint32_t*>(mem.part(3));
    AO_HIP(hipMemcpy(d_seed, &seed, 4, hipMemcpyHostToDevice));
    int rc = launch_mt_seed(d_seed, 1, nullptr, st, pos, 1, nullptr);                  // RandomState(seed)
    for (int c = 0; c < n_calls && !rc; ++c) {
        rc = launch_mt_normal<double>(st, pos, zx, 1, n, 0, n, nullptr, nullptr);
        if (!rc && hipMemcpy(h_out + (size_t)c * n, zx, (size_t)n * 8, hipMemcpyDeviceToHost) != hipSuccess) rc = fail("copy back failed");
    }
    return rc;
}

}  // extern "C"
