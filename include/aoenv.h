/*
 * aoenv.h -- C ABI of the MI355X-native batched adaptive-optics environment (libaoenv.so).
 *
 * The reference (artiom-matvei/RLAO) is pure Python: there is no native FFI to mirror.  Each entry
 * point below names the reference *Python* interface it replaces, so that a maintainer can bind the
 * library behind drl4ao's gym-style env (INTEGRATION.md shows the ctypes stub):
 *
 *   OOPAO/  = drl4ao/AO_OOPAO/OOPAO/          MAIN/ = drl4ao/MAIN_CODE/
 *
 * Conventions
 *   - plain C types only; every function returns 0 on success, non-zero on error and never throws or
 *     aborts; aoenv_last_error() returns a thread-local description of the last failure.
 *   - "d_" pointers are DEVICE pointers owned by the caller (PyTorch tensors, hipMalloc, ...), laid
 *     out contiguously, element type = the environment's dtype (AOENV_F32 float / AOENV_F64 double).
 *   - "h_" pointers are HOST pointers; constants are always handed over as float64 / int32 / uint8 and
 *     converted to the environment's dtype on upload.
 *   - stream arguments are hipStream_t passed as void* (NULL = the default stream).  All work of a
 *     call is enqueued on that stream; no call synchronises the device except aoenv_download().
 *   - one host thread per AoEnv; one AoEnv per GPU shard of independent AO loops ("envs").
 */
#ifndef AOENV_H
#define AOENV_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define AOENV_ABI_VERSION 7

enum { AOENV_F32 = 0, AOENV_F64 = 1 };
/* AOENV_WFS_SH_GEOMETRIC replaces ShackHartmann(..., is_geometric=True) (OOPAO/ShackHartmann.py:382-394, 676-695; the reference's
 * own SH initialisation calibrates in this mode, OOPAO/calibration/initialization_AO_SHWFS.py:114-127).  With phi = src.phase_no_pupil
 * = (atm.OPD_no_pupil + dm.OPD) 2 pi / lambda_src, NOT pupil-masked, and p = R / n_subap:
 *     gx = np.gradient(phi, axis=0) * pupil;  gy = np.gradient(phi, axis=1) * pupil      central differences, one-sided on the edges
 *     signal = [bin(gy) | bin(gx)][valid lenslets] / units,    bin = the sum over a lenslet's p x p pixels
 * No spots, no camera, no threshold, no reference slopes, no noise (:712-713).  Such a shard uses n_subap, n_valid_subap, n_signal,
 * AOENV_C_SH_SUBAP_IDX (at most 32767 valid lenslets) and AOENV_C_WFS_UNITS as a Shack-Hartmann does and ignores AOENV_C_SH_REF,
 * AOENV_C_WFS_AMP, threshold_cog and max_group; cam_res is kept so that AOENV_B_FRAME and d_frame are defined: they are zero.
 * AoCfg has no diameter: the HOST folds the gradient's 1 / pixelSize into the uploaded units, AOENV_C_WFS_UNITS = slopes_units *
 * pixelSize (rlao_amd keeps env.slopes_units the reference's value).
 * The phase kernels of such a shard also store the unmasked phase (aoenv_get_phase_no_pupil); a step is the phase kernel and one launch
 * for slopes + reconstruction + integrator (k_geo_tail) where the fused tail applies (AOENV_OPT_FUSED_TAIL, reconstructor factors,
 * <= 1024 envs, the LDS plan of rlao_amd/csrc/sh_geometric.hpp), otherwise the stand-alone slopes kernel (k_sh_geometric, also
 * aoenv_measure's) and the reconstruction kernels; the signal is the same bits either way.  The fused step kernel and the step
 * pairs never run: aoenv_fused_step_active is 0.  aoenv_set_detector is accepted and has no effect (frame zero, no noise frame
 * counted); aoenv_set_flux_env and aoenv_set_threshold_env with an array are refused: there are neither photons nor a threshold.
 * The new launches count under AOENV_K_SH_CENTROID (stand-alone) and AOENV_K_SH_TAIL (fused) in aoenv_profile.
 * Additive: a shard of the other two kinds runs what it ran, and the ABI version stays. */
enum { AOENV_WFS_SH = 0, AOENV_WFS_PYRAMID = 1, AOENV_WFS_SH_GEOMETRIC = 2 };

/* Geometry and loop constants of one shard.  Filled by the host (rlao_amd/calib.py) from the same
 * parameter-file keys the reference uses (MAIN/Conf/parameterFile_oopao_parser.py:19-79). */
typedef struct AoEnv AoEnv;   /* opaque */

typedef struct AoCfg {
    int32_t abi_version;     /* = AOENV_ABI_VERSION */
    int32_t dtype;           /* AOENV_F32 | AOENV_F64: arithmetic type of device state and kernels */
    int32_t n_env;           /* independent AO loops stepped in lock-step on this GPU */
    int32_t resolution;      /* R: telescope pupil pixels across the diameter (OOPAO/Telescope.py:138) */
    int32_t n_layer;         /* turbulence layers; 0 = no atmosphere (calibration shards) */
    int32_t layer_res;       /* N: interior size of a layer screen, N = R + 4 for fov 0 (OOPAO/Atmosphere.py:216-218) */
    int32_t n_inner;         /* 8N-16 : conditioning ring pixels Z (OOPAO/Atmosphere.py:267-274) */
    int32_t n_outer;         /* 4N+4  : regenerated ring pixels X */
    int32_t n_act;           /* actuators across the diameter, nSubap+1 (OOPAO/DeformableMirror.py:288) */
    int32_t n_valid_act;     /* A: controlled actuators */
    int32_t dm_separable;    /* 1: OPD = Gy C Gx^T (Cartesian Gaussian DM, no rotation); 0: dense modes GEMM */
    int32_t wfs_type;        /* AOENV_WFS_SH | AOENV_WFS_PYRAMID | AOENV_WFS_SH_GEOMETRIC */
    int32_t n_subap;         /* lenslets (SH) / pupil samples (Pyramid) across the diameter */
    int32_t n_valid_subap;   /* SH: valid lenslets;  Pyramid: valid pixels per quadrant */
    int32_t n_signal;        /* length of wfs.signal */
    int32_t cam_res;         /* WFS camera frame is cam_res x cam_res */
    int32_t n_loop;          /* length of the total[] / residual[] telemetry (param['nLoop']) */
    int32_t max_group;       /* envs in consecutive groups of max_group share the centroid-threshold
                                maximum (1 in the loop; nMeasurements when emulating the batched
                                interaction-matrix measurement, OOPAO/ShackHartmann.py:605-672) */
    int32_t pyr_n_res;       /* Pyramid: padded FFT size nRes (OOPAO/Pyramid.py:251) */
    int32_t pyr_n_theta;     /* Pyramid: modulation points (1 = unmodulated, OOPAO/Pyramid.py:955, 976) */
    int32_t pyr_centering;   /* Pyramid: 1 = psfCentering (mask on 4 pixels, phasor), 0 = fftshift + 1-pixel mask */
    int32_t pyr_norm_valid;  /* Pyramid: 0 = 'slopesMaps_incidence_flux' (norm = frame.mean()), 1 = 'slopesMaps' */
    int32_t pyr_q_lo;        /* Pyramid: first row/column of quadrants 1 (and of the low side of 2, 4) in the frame */
    int32_t pyr_q_hi;        /* Pyramid: first row/column of the high-side quadrants (grabQuadrant, OOPAO/Pyramid.py:774-790) */
    int32_t layer_res_l[8];  /* per-layer N: 0 = layer_res.  With a field of view (the reference env builds its telescope with
                                fov = 1 arcsec, MAIN/OOPAOEnv/OOPAOEnv.py:129) a layer at altitude h lives on a grid of
                                N_l = ceil(R / D (D + 2 tan(fov / 2) h)) + 4 pixels with ring operators of its own
                                (OOPAO/Atmosphere.py:216-218, 277-286); its n_inner / n_outer are 8 N_l - 16 / 4 N_l + 4.  Layers on
                                different grids run the batched kernels (the fused step kernel needs one grid) */
    double  atm_wavelength;  /* 500e-9: wavelength the screens are expressed at (OOPAO/Atmosphere.py:134) */
    double  src_wavelength;  /* guide-star wavelength (OOPAO/Source.py:102) */
    double  leak;            /* leaky-integrator factor (MAIN/OOPAOEnv/OOPAOEnv.py:69) */
    double  threshold_cog;   /* SH centre-of-gravity threshold (OOPAO/ShackHartmann.py:42) */
} AoCfg;

/* Constant tables, uploaded once per geometry (aoenv_upload).  Element type on the host side in []. */
enum AoConst {
    AOENV_C_PUPIL = 0,       /* [u8  R*R]            Telescope.pupil                                  */
    AOENV_C_AB,              /* [f64 n_outer*(n_inner+n_outer)] rows = [A | B] (OOPAO/Atmosphere.py:284-286) */
    AOENV_C_INNER_IDX,       /* [i32 n_inner]  flat index into the (N+2)^2 screen of each Z pixel, mask order */
    AOENV_C_OUTER_IDX,       /* [i32 n_outer]  flat index of each X pixel, mask order                  */
    AOENV_C_LAYER_WEIGHT,    /* [f64 n_layer]  sqrt(fractionalR0) (OOPAO/Atmosphere.py:450)            */
    AOENV_C_DM_GX,           /* [f64 R*n_act]  separable influence factor along x                      */
    AOENV_C_DM_GY,           /* [f64 R*n_act]  separable influence factor along y                      */
    AOENV_C_DM_MODES,        /* [f64 R*R*A]    dense influence matrix dm.modes (only if !dm_separable)  */
    AOENV_C_ACT_IDX,         /* [i32 A]        iy*n_act+ix of each valid actuator (xvalid,yvalid)       */
    AOENV_C_WFS_AMP,         /* [f64 R*R]      sqrt(src.fluxMap) (x pupilReflectivity)                  */
    AOENV_C_SH_SUBAP_IDX,    /* [i32 n_valid_subap] SH: i*n_subap+j of each valid lenslet;
                                                    Pyramid: r*n_subap+c of each valid pixel of a quadrant (validI4Q) */
    AOENV_C_SH_REF,          /* [f64 2*n_valid_subap] SH: reference centroids (x block then y block);
                                                      Pyramid: referenceSignal_2D at the valid pixels             */
    AOENV_C_WFS_UNITS,       /* [f64 1]        slopes_units                                             */
    AOENV_C_RECON,           /* [f64 A*n_signal] reconstructor = M2C @ calib.M (MAIN/OOPAOEnv/OOPAOEnv.py:381) */
    AOENV_C_PYR_MASK,        /* [f64 nRes*nRes*2] exp(i m) of the pyramid mask, rounded to complex64 (OOPAO/Pyramid.py:323) */
    AOENV_C_PYR_TT,          /* [f64 n_theta*R*R] modulation tip/tilt phases, float32-rounded (OOPAO/Pyramid.py:964-970) */
    AOENV_C_RECON_FACTORS,   /* [f64 K*n_signal + A*K] optional: calib.M (K x nSig) then M2C (A x K) with reconstructor = M2C @ M
                                (MAIN/OOPAOEnv/OOPAOEnv.py:295, 381); enables the fused low-rank tail.  Upload after AOENV_C_RECON */
    AOENV_C_COUNT
};

/* Device buffers that can be inspected / overwritten (aoenv_download / aoenv_upload_state): the
 * environment state of SURVEY.md section 5 "checkpoint / resume" plus the stage boundaries the parity
 * tests compare.  Shapes are per shard, leading dimension n_env unless noted. */
enum AoBuf {
    AOENV_B_SCREEN = 0,      /* [n_layer][n_env][(N_l+2)^2]  layer.mapShift, layer after layer (stored as a torus: no flat device image) */
    AOENV_B_OPD_ATM,         /* [n_env][R*R]   atm.OPD_no_pupil                                          */
    AOENV_B_COEFS,           /* [n_env][A]     dm.coefs                                                  */
    AOENV_B_PHASE,           /* [n_env][R*R]   tel.src.phase (residual, pupil-masked, rad @ src)          */
    AOENV_B_FRAME,           /* [n_env][cam^2] wfs.cam.frame                                             */
    AOENV_B_SIGNAL,          /* [n_env][n_signal] wfs.signal                                             */
    AOENV_B_TOTAL,           /* [n_loop][n_env] env.total  (nm rms)                                      */
    AOENV_B_RESIDUAL,        /* [n_loop][n_env] env.residual (nm rms)                                    */
    AOENV_B_WFS_MAX,         /* [n_env]        max of the valid spot intensities (threshold reference)   */
    AOENV_B_XI,              /* [n_env][n_inner+n_outer] last [Z | xi] operand of the ring extrusion      */
    AOENV_B_MT_STATE,        /* [n_layer][n_env][625] uint32 (whatever the env dtype): the 624 MT19937 state words of
                                the layer's ring RandomState and its position (OOPAO/Atmosphere.py:201, 308)         */
    AOENV_B_COUNTERS,        /* [4] uint32: frame counter of the camera noise streams, step counter of the exploration
                                stream (aoenv_run_rollout), 2 reserved                                              */
    AOENV_B_DM_PREV,         /* [n_env][A]     env.dm_prev: the leaky integrator's state.  aoenv_step computes
                                dm.coefs = dm_prev * leak + action and copies it back to dm_prev; aoenv_set_coefs (dm.coefs = ...
                                from outside) leaves it alone, as in the reference (MAIN/OOPAOEnv/OOPAOEnv.py:314, 508-509), so
                                the trainers' episode prologue `env.dm.coefs = 0` (MAIN/PO4AO/mbrl.py:50) does not clear it */
    AOENV_B_COEFS_SEEN,      /* [n_env][A]     the command the last stepped measurement saw under a disturbance (aoenv_set_disturbance):
                                dm.coefs + B v(tau), what the reference calls dm.coefs = vibration_state + correction_state
                                (MAIN/OOPAOEnv/vibrationEnv.py:197-202).  Zero until a disturbed step has written it; not loop state */
    AOENV_B_COUNT
};

const char* aoenv_last_error(void);
int aoenv_abi_version(void);

/* Replaces: OOPAO() + the object construction half of set_params() (MAIN/OOPAOEnv/OOPAOEnv.py:19-73,
 * 121-246): allocates all device state for cfg->n_env loops on HIP device `device`.  The DM starts
 * flat (dm.coefs = 0), the atmosphere OPD at zero, the WFS reference at zero and units at 1. */
int aoenv_create(const AoCfg* cfg, int device, AoEnv** out);
int aoenv_destroy(AoEnv* env);

/* Replaces: the constant members the reference objects compute in their constructors (pupil, layer.A /
 * layer.B, dm.modes, wfs flux / reference / units, env.reconstructor ...).  `kind` is an AoConst;
 * `bytes` must match the table size implied by the AoCfg.  May be called again at any time (e.g. the
 * r0 setter re-uploads [A|B], OOPAO/Atmosphere.py:792-807). */
int aoenv_upload(AoEnv* env, int kind, const void* h_data, size_t bytes);

/* The ring tables AOENV_C_AB / AOENV_C_INNER_IDX / AOENV_C_OUTER_IDX of ONE layer, sized by that layer's grid (AoCfg.layer_res_l):
 * layer.A / layer.B and the masks of OOPAO/Atmosphere.py:262-286.  aoenv_upload() with these kinds serves every layer at once and
 * is only accepted when all layers share one grid. */
int aoenv_upload_layer(AoEnv* env, int kind, int layer, const void* h_data, size_t bytes);

/* Replaces: the windSpeed / windDirection setters (OOPAO/Atmosphere.py:829-873): per layer
 * ratio = (vX, vY) * samplingTime / pixel_size in pixels per frame (OOPAO/Atmosphere.py:362-363).
 * h_ratio is [n_layer][2] float64, shared by all envs of the shard.  `reset_buff` != 0 also clears the
 * sub-pixel accumulator (what notDoneOnce does after generateNewPhaseScreen). */
int aoenv_set_wind(AoEnv* env, const double* h_ratio, int reset_buff);

/* The same setters when every env has its OWN wind (a trainer that draws wind speed / direction per run, e.g.
 * MAIN/integrator_oopao_razor.py:41-44, batched): h_ratio is [n_layer][n_env][2] float64, |ratio| < n pixels per frame on each
 * axis, n the ceiling AOENV_OPT_ENV_WIND_PIXELS (default 1); a larger ratio is refused with nothing changed, and so is a shard with
 * layers on grids of their own (AoCfg.layer_res_l), which has no per-env clocks.
 * The shard switches to per-env clocks for good: accumulators, torus origins and warp taps of every (env, layer) live on
 * the device and are advanced there, by the same arithmetic as the shared host clock (an env stepped by its own clock is
 * bit-identical to a shard stepped with that wind); on every step one launch per layer advances the clocks and prepares the
 * ring operands of the envs that cross a pixel, and the ring GEMM runs over the whole shard.  A layer in which some env's wind is
 * a pixel per frame or more first makes max over the envs of max(floor |rx|, floor |ry|) whole-pixel rounds (scatter of the round
 * before, one launch for the operands of the envs that take part, the GEMM over the whole shard), in the order of the shared
 * clock: all whole pixels, then the sub-pixel crossing, from the env's one stream.  aoenv_set_wind keeps working
 * afterwards (the same wind for every env); new screens reset accumulators and origins as for the shared clock.
 * Clock state for checkpoints: h_clock [n_layer][n_env][4] float64 = {ratio x, ratio y, buff x, buff y}; aoenv_set_clock_env
 * takes |ratio| below the same ceiling and |buff| < 1, and changes nothing when it refuses. */
int aoenv_set_wind_env(AoEnv* env, const double* h_ratio, int reset_buff, void* stream);
int aoenv_get_clock_env(AoEnv* env, double* h_clock);
int aoenv_set_clock_env(AoEnv* env, const double* h_clock);

/* Replaces: the r0 setter (OOPAO/Atmosphere.py:792-807) when every env has its OWN Fried parameter (a trainer that sweeps the
 * seeing, one value per run, batched).  h_r0 is [n_env] float64, metres at 500 nm; r0_tables is the r0 the uploaded AOENV_C_AB
 * was built at.  No tables per env and no second product: with s = (r0_def / r0)^(5/3), A = (zx s)^T (zz^-1 / s) does not depend
 * on r0 and B = chol(xx s - A zx s) goes as r0^(-5/6), so X = A Z + B(r0_e) xi = A Z + B(r0_tables) (sigma_e xi) with
 * sigma_e = (r0_tables / r0_e)^(5/6).  The library keeps h_r0 on the host (aoenv_get_r0_env, the resets) and sigma_e, computed on
 * the host as pow(r0_tables / h_r0[e], 5.0 / 6), as float64 [n_env] on the device; every kernel that writes innovations into
 * [Z | xi] multiplies them by sigma_e in float64 before converting to the env dtype.  The MT19937 streams are untouched
 * (AOENV_B_MT_STATE is what it is without the feature), and sigma_e == 1 exactly for h_r0[e] == r0_tables.  It takes effect from
 * each env's next ring extrusion: screens on the device are not rescaled (the reference's setter does not either), a deferred ring
 * already computed is scattered as it is, a ring look-ahead drawn with the old factors is forgotten.  Works with shared and per-env
 * clocks, both sensors, and layers on grids of their own (sigma_e is the same for every layer).  While it is active,
 * aoenv_new_screens_device and aoenv_reset_envs give env e the screens of their `r0` argument multiplied by (r0 / r0_e)^(5/6)
 * (computed on the host in float64, applied once to the finished float64 screen); aoenv_new_screens takes the host's screens as
 * they are.  Re-uploading AOENV_C_AB at another r0 needs a new call with that r0_tables.
 * h_r0 == NULL: back to one r0 for all envs (the factors are absent, not ones).  The stream is waited for once.
 * Refused, with nothing changed: a null env, an entry that is not finite and positive, such an r0_tables.
 * aoenv_get_r0_env fills h_r0 [n_env]; it fails while the shard has one r0. */
int aoenv_set_r0_env(AoEnv* env, const double* h_r0, double r0_tables, void* stream);
int aoenv_get_r0_env(AoEnv* env, double* h_r0);

/* Replaces: atm.generateNewPhaseScreen(seed) (OOPAO/Atmosphere.py:560-592) for every env of the shard.
 *   h_screens [n_env][n_layer][N*N] float64: the new layer.phase screens (rad @ 500 nm), or NULL to keep
 *             the current interior (not with per-env clocks).  Layers on grids of their own (layer_res_l): layer-major
 *             blocks, layer l = [n_env][N_l*N_l];
 *   h_ring_seeds [n_env][n_layer] uint32: seeds of the per-layer ring RandomState (seed + 1000*layer);
 * seeds every MT19937 stream, draws the first ring X = A.Z + B.xi on the device, rebuilds mapShift,
 * clears the sub-pixel accumulators and refreshes atm.OPD (fill_phase_support + set_OPD). */
int aoenv_new_screens(AoEnv* env, const double* h_screens, const uint32_t* h_ring_seeds, void* stream);

/* Same, with the screens themselves generated on the device (OOPAO/phaseStats.py:190-318 ft_sh_phase_screen:
 * FFT screen + 3 sub-harmonic grids, both seeded with the same RandomState as the reference does):
 *   h_screen_seeds [n_env][n_layer] uint32: seed + layer of each layer's own RandomState (OOPAO/Atmosphere.py:574);
 *   r0 [m @ 500 nm], L0 [m], pixel_size = layer.D / layer.resolution [m] (= telescope pixel size for fov 0).
 * MT19937 + legacy Gaussian stream, float64 FFT: agrees with the NumPy generator to ~1e-12 rad. */
int aoenv_new_screens_device(AoEnv* env, const uint32_t* h_screen_seeds, const uint32_t* h_ring_seeds, double r0,
                             double L0, double pixel_size, void* stream);

/* Replaces: atm.generateNewPhaseScreen(seed) (OOPAO/Atmosphere.py:560-592) plus the trainers' episode prologue (dm.coefs = 0,
 * dm_prev = 0: MAIN/PO4AO/mbrl.py:49-52, OOPAOEnv_VPG.py:120-121) for SOME envs of the shard: the restart of single loops that a
 * batched RL environment needs (a diverged loop, staggered episodes, autoreset).
 *   h_env_idx [n_idx] int32: the envs to restart, each in [0, n_env), none twice, in any order;
 *   h_screen_seeds / h_ring_seeds [n_idx][n_layer] uint32: row c belongs to env h_env_idx[c]; as for aoenv_new_screens_device;
 *   r0, L0, pixel_size: as for aoenv_new_screens_device.
 * For every listed env, and only for those: new layer screens drawn on the device (the generator and streams of
 * aoenv_new_screens_device), ring RandomStates reseeded, the first ring X = A.Z + B.xi drawn, the clock restarted (accumulator and
 * torus origin 0, the wind ratio kept), min / max refreshed, dm.coefs and dm_prev zeroed; atm.OPD and the residual phase are then
 * re-derived from the screens (a user-defined OPD of aoenv_set_atm_opd ends here, as with new screens).  Afterwards a listed env is
 * indistinguishable, bit for bit, from the same env of a shard of the same size that was reset as a whole with those seeds and had
 * its commands zeroed; screens, streams, clocks, commands and telemetry of every other env stay bit for bit as they were.
 * The shard switches to per-env clocks FOR GOOD, exactly as aoenv_set_wind_env does (a shared origin cannot describe one env
 * restarted at origin 0): from the shared clock every env starts at the shared origin and accumulator with the shard's wind, which
 * must be below the ceiling AOENV_OPT_ENV_WIND_PIXELS (default: < 1 pixel per frame) and is handed to every env's clock; a
 * deferred ring is scattered and a ring look-ahead forgotten first.  From then on the shard pays the
 * cost of per-env clocks on every step (the ring kernels run on every step: about 26 % at the 8 m Shack-Hartmann geometry,
 * DESIGN.md section 4.2).  The screen generation and the ring operands are work for n_idx envs, driven by a device index list;
 * the ring product itself runs once per layer over the whole shard, so that it sums in the order of the full reset.
 * With a per-env Fried parameter (aoenv_set_r0_env) a listed env restarts with ITS r0: its screens are those of `r0` times
 * (r0 / r0_e)^(5/6) -- row c of the factors belongs to env h_env_idx[c] -- and its first ring is drawn with sigma_e; to restart an
 * env at a new seeing, call aoenv_set_r0_env first.
 * n_idx == 0 succeeds and does nothing (the clocks stay as they are).  Refused, with nothing changed: null pointers, n_idx < 0,
 * an index outside [0, n_env), a duplicate index, n_layer == 0, missing ring tables, non-positive r0 / L0 / pixel_size, a shared
 * wind at or above the ceiling AOENV_OPT_ENV_WIND_PIXELS (default: a pixel per frame or more), and shards with layers on grids of their own (AoCfg.layer_res_l), which have no per-env
 * clocks.  Host synchronisation as in aoenv_new_screens_device (the stream is waited for once, before the clocks are switched). */
int aoenv_reset_envs(AoEnv* env, const int32_t* h_env_idx, int n_idx, const uint32_t* h_screen_seeds,
                     const uint32_t* h_ring_seeds, double r0, double L0, double pixel_size, void* stream);

/* Replaces: atm.update(OPD) with a user-defined OPD (OOPAO/Atmosphere.py:421-425) and
 * tel.OPD = ... in the WFS calibration (OOPAO/ShackHartmann.py:296-297).  h_opd [n_env][R*R] float64
 * (no pupil applied); only meaningful while n_layer == 0 or until the next aoenv_step. */
int aoenv_set_atm_opd(AoEnv* env, const double* h_opd, void* stream);

/* Replaces: dm.coefs = v (OOPAO/DeformableMirror.py:534-570).  h_coefs [n_env][A] float64 or NULL for
 * dm.coefs = 0 (MAIN/PO4AO/mbrl.py:50).  env.dm_prev (AOENV_B_DM_PREV) is not touched. */
int aoenv_set_coefs(AoEnv* env, const double* h_coefs, void* stream);

/* Replaces: tel*dm*wfs with no atmosphere update (MAIN/PO4AO/mbrl.py:52; OOPAO/Telescope.py:533-544,
 * 476-485): residual phase = (atm.OPD_no_pupil + dm.OPD) * pupil, WFS measurement, signal. */
int aoenv_measure(AoEnv* env, void* stream);

/* Replaces: atm.update() on its own (OOPAO/Atmosphere.py:439-477; the open-loop scripts call it between propagations):
 * every layer moves by one frame -- ring extrusions included -- and atm.OPD_no_pupil (AOENV_B_OPD_ATM) and the residual
 * phase are re-derived.  No WFS measurement, no controller.  aoenv_step = this + aoenv_measure + the glue. */
int aoenv_atm_update(AoEnv* env, void* stream);

/* Replaces: env.reset_soft() (MAIN/OOPAOEnv/OOPAOEnv.py:82-86): obs = vec_to_img(-R @ wfs.signal) * 1e6.
 * d_obs [n_env][n_act][n_act]. */
int aoenv_reset_soft(AoEnv* env, void* d_obs, void* stream);

/* Replaces: env.step(i, action) (MAIN/OOPAOEnv/OOPAOEnv.py:485-536; Razor twin OOPAOEnvRazor.py:474-514).
 *   i        frame index: total[i], residual[i] are written (i < n_loop)
 *   d_action [n_env][n_act][n_act]  DM increment image in micrometres
 *   d_obs    [n_env][n_act][n_act]  out: reconstructed residual image (micrometres)
 *   d_frame  [n_env][cam][cam] or NULL  out: wfs.cam.frame (Papyrus 6-tuple) / NULL (Razor 5-tuple)
 *   d_reward [n_env]  out: -||obs||_2        d_strehl [n_env]  out: exp(-var(phase[pupil]))
 * Order of effects as in the reference: turbulence advances, the WFS sees the command latched by the
 * previous call, then dm.coefs <- leak * dm_prev + 1e-6 * img_to_vec(action) and dm_prev <- dm.coefs. */
int aoenv_step(AoEnv* env, int i, const void* d_action, void* d_obs, void* d_frame, void* d_reward,
               void* d_strehl, void* stream);

/* Closed-loop driver of MAIN/integrator_oopao_razor.py:66-91 kept on the device: n_steps iterations of
 * action = gain * obs; obs, reward, strehl = step(i0 + k, action).  d_obs is in/out. */
int aoenv_run_integrator(AoEnv* env, int i0, int n_steps, double gain, void* d_obs, void* d_frame,
                         void* d_reward, void* d_strehl, void* stream);

/* Replaces: env.sample_noise's filter F = M2C_CL @ pinv(M2C_CL) (MAIN/OOPAOEnv/OOPAOEnv.py:383, 566-570), for aoenv_run_rollout.
 * F = Fl @ Fr in factored form.  h_factors = [f64 K*A] Fr then [f64 A*K] Fl;  K in [1, A].
 * NULL / K == 0: no filter (n = z: the reference's F = 1 before set_params).  Refused with nothing changed: K out of range,
 * non-finite entries.  The stream is waited for once. */
int aoenv_set_noise_filter(AoEnv* env, const double* h_factors, int K, void* stream);

/* Replaces: the command-space disturbance of the reference's vibration envs (MAIN/OOPAOEnv/vibrationEnv.py:119-123, 146-167,
 * 197-202: three sine lines each on tip and tilt with random phases per episode, dm.coefs = vibration_state + correction_state, so
 * that the integrator state holds the correction alone; SinEnv.py / modalAOSinEnv.py, CRL_twoSin.py, twoSin_hpOptim.py are of the
 * same family), for the loops that run inside the library, every env with its own lines.  The model is rlao_amd/csrc/disturb.hpp:
 * for env e, mode m < M, line j < J at the integer measurement time tau
 *     x = fma(freq[e][m][j], (double)tau, phase[e][m][j]);   v[e][m] = sum_j amp[e][m][j] sin(2 pi (x - floor(x)))     (float64)
 *     seen[e][a] = coefs[e][a] + sum_m modes[a][m] (T)v[e][m]                                             (env dtype, fma chain)
 * every sum in index order, whatever the shard size or the env's place in it.  While a disturbance is set, aoenv_step,
 * aoenv_run_integrator, aoenv_run_rollout and aoenv_run_policy_rollout -- and only those -- launch one kernel in front of each step that
 * writes `seen` into AOENV_B_COEFS_SEEN with that step's tau = t0 + i + 1 (i the frame index; the reference shows vibration[:, t]
 * with t incremented before use), and the step's measurement shows THAT command on the mirror, on the fused and the batched path, for
 * both sensors and dtypes.  The step goes on writing the pure command to AOENV_B_COEFS / AOENV_B_DM_PREV.  aoenv_measure,
 * aoenv_reset_soft, the calibration and aoenv_compute_psf after a bare aoenv_measure never see the disturbance, because a calibration
 * must not: unlike vibrationEnv.reset, whose first observation shows sample 0, the first disturbed observation here is that of step 0.
 * With every amp == 0 `seen` equals dm.coefs in value; with no disturbance set there is no extra launch and no changed argument.
 * t0 lets a vibration run on across episodes.  Everything is copied before the call returns; the stream is waited for once.
 * The configuration is NOT loop state: it is in neither aoenv_get_buff nor the checkpoint buffers, and a caller that restores a
 * state sets it again.  Refused, with nothing changed: n_modes / n_lines out of range, a null array, a non-finite entry, a negative amp. */
typedef struct AoDisturbance {
    int32_t n_modes, n_lines;      /* M in [1, 64], J in [1, 8] */
    int64_t t0;                    /* tau = t0 + i + 1 at the measurement of frame i */
    const double *h_modes;         /* [A][M] dimensionless, e.g. columns of M2C_CL; A covers both DMs of a two-DM shard */
    const double *h_amp, *h_freq, *h_phase;   /* [n_env][M][J] each: metres of command, cycles per frame, cycles */
} AoDisturbance;
int aoenv_set_disturbance(AoEnv* env, const AoDisturbance* cfg, void* stream);   /* NULL cfg: forget it */

/* Replaces: a mis-registered deformable mirror per run (OOPAO/DeformableMirror.py:326-351: the actuator positions from
 * misReg.shiftX, shiftY, rotationAngle, radialScaling, tangentialScaling; :494-514: the Gaussian widths from the two scalings;
 * MAIN/OOPAOEnv/OOPAOEnv.py:214-226 feeds param['MisReg_shiftX' | 'MisReg_shiftY' | 'MisReg_rotationAngle'] into the mirror), for
 * every env of a shard at once: a tolerance study over n_env offsets is one shard and one calibration.
 * The model: a shift or a scaling along the axes keeps the influence function of actuator (iy, ix) a product
 * gy[:, iy] (x) gx[:, ix], so the surface of env e stays Gy_e C_e Gx_e^T and only the operand tables differ from env to env.
 * h_gx, h_gy: [n_env][R][n_act] float64, per env the meaning and element order of AOENV_C_DM_GX / _GY (a two-DM shard: the composite
 * [gx1 | gx2]).  Each env's pair is written in every layout the shared tables have (rlao_amd/csrc/dm_tables.hpp): gx, gy and the
 * transpose of gx in the env dtype, and the two float32 matrix-core operand tables, zero padded to R rounded up to 128.  Device
 * memory of a per-env set: n_env times
 *     (2 R n_act + (n_act pad 4)(R pad 128)) sizeof(dtype) + 2 (R pad 128) 4 ga_stride sizeof(float),  ga_stride = max(8, n_act / 4 pad 4)
 * (the transpose, the second term, is kept as the shared one is, though no kernel reads either at present)
 * -- 64 KB per env at R = 120, n_act = 21 in float32.  Every kernel that forms the DM surface from the factors (the fused step kernel,
 * the phase kernels of every path, k_dm_rows) offsets its table pointers by env x stride; the stride is 0 while the tables are
 * shared, and the addresses, loads and results are then those of a shard that never made the call.  Everything that steps or
 * measures follows without a new argument: aoenv_step, aoenv_measure, aoenv_reset_soft, aoenv_run_integrator, both recorded
 * rollouts, a disturbance (`seen` goes through the env's own mirror), a delay; aoenv_compute_psf through the phase it reads.  The
 * reconstructor stays that of the calibrated mirror: that is the experiment.
 * Both pointers NULL: back to the shared tables (AOENV_C_DM_GX / _GY as uploaded), the per-env ones are freed.
 * Everything is copied before the call returns; the stream is waited for once, because a step in flight reads the tables in place.
 * The tables are configuration, as the disturbance is: not loop state, not in the checkpoint buffers; aoenv_reset_envs and
 * aoenv_new_screens* leave them alone.
 * Refused, with nothing changed: exactly one of the two pointers null, a non-finite entry, a shard with dm_separable == 0 (a dense
 * mirror has no factors), an allocation that fails (the message states the bytes).
 * A rotation or an anamorphosis angle is not a product of two factors and has no entry here.
 * aoenv_get_dm_env fills h_gx, h_gy [n_env][R][n_act] with the values as held: rounded to the env dtype, widened to float64.
 * It fails while the tables are shared. */
int aoenv_set_dm_env(AoEnv* env, const double* h_gx, const double* h_gy, void* stream);
int aoenv_get_dm_env(AoEnv* env, double* h_gx, double* h_gy, void* stream);

/* Replaces: a MisRegistration with rotationAngle != 0 on the mirror of one env (OOPAO/DeformableMirror.py:326-351 moves the actuator
 * positions, :494-510 evaluates the Gaussians).  A rotated grid is not Gy C Gx^T, but at anamorphosis angle 0 every actuator's
 * Gaussian is still a product of a y factor and an x factor, so env e's surface is
 *     S_e[y][x] = sum_k c_e[k] py_e[y][k] px_e[x][k],   k over the n_valid_act valid actuators.
 * h_py, h_px: [n_env][R][n_valid_act] float64 (rlao_amd.calib.dm_actuator_pairs computes them; a dead actuator is a zero column).
 * While pairs are in force the shard forms the surface ahead of the phase kernel, as a dense mirror's shard does, in one launch
 * wherever the command changes: on the fp32 matrix cores for float32 shards (k_dm_pairs_mfma), as one fma chain per pixel for
 * float64 shards and under AOENV_PATH_DM_PAIRS_GENERAL (k_dm_pairs).  Both add c[k] py[y][k] * px[x][k] in ascending k: the order
 * depends on (R, n_valid_act) alone, there are no atomics, and an env has the same bits in any shard and at any place in it.  The
 * shard then runs the batched kernels (k_phase<T> reads the surface); aoenv_fused_step_active is 0 until the pairs are cleared.
 * Device memory of a set (rlao_amd/csrc/dm_pairs.hpp): n_env times
 *     2 R A sizeof(dtype) + 2 (R pad 128) 4 ga_stride sizeof(float) + R^2 sizeof(dtype),   ga_stride = max(8, A / 4 pad 4)
 * (the tables in the env dtype, the two float32 operand tables, the surface).  Both pointers NULL: the pairs are cleared and the
 * memory freed; the shard launches what it launched before.
 * Configuration like the per-env factor tables: copied before the call returns (the stream is waited for once), not loop state,
 * not in the checkpoint buffers; aoenv_reset_envs and aoenv_new_screens* leave them alone.
 * Refused, with nothing changed: exactly one pointer null, a non-finite entry (the index is reported), a shard with
 * dm_separable == 0, per-env factor tables in force (aoenv_set_dm_env: clear them first; aoenv_set_dm_env with tables is likewise
 * refused while pairs are in force), an allocation that fails.
 * aoenv_get_dm_pairs fills h_py, h_px with the values as held: rounded to the env dtype, widened to float64. */
int aoenv_set_dm_pairs(AoEnv* env, const double* h_py, const double* h_px, void* stream);
int aoenv_get_dm_pairs(AoEnv* env, double* h_py, double* h_px, void* stream);

/* Replaces: reading dm.OPD.  h_surface [n_env][R*R]: the mirror surface, in metres, of the command currently held
 * (AOENV_B_COEFS, without a disturbance), formed first on the stream.  For shards that keep a surface buffer: a dense mirror
 * (dm_separable == 0) and actuator factor pairs.  Refused on a shard that forms its surface inside the phase kernel. */
int aoenv_get_dm_surface(AoEnv* env, double* h_surface, void* stream);

/* Replaces: OOPAOEnvRazor.change_mag (MAIN/OOPAOEnvRazor/OOPAOEnvRazor.py:644-647: source.nPhoton = zeroPoint 10^(-0.4 mag), then
 * source * tel * wfs) and the assignment env.wfs.threshold_cog = t, as the noise study makes them between its serial runs
 * (MAIN/OOPAOEnvRazor/integrator_threshold.py:34-106: six thresholds for each of six magnitudes) -- for the envs of ONE shard: every
 * env its own guide-star flux and its own centroid threshold, one calibration.
 * The model (OOPAO/Source.py:109, 151; OOPAO/ShackHartmann.py:327-338, 515-517; rlao_amd/csrc/star_env.hpp): fluxMap is linear in
 * nPhoton and the WFS amplitude is sqrt(fluxMap); the valid lenslets / pixels are chosen relative to the maximum and the reference
 * slopes and slope units are measured on ideal intensities, so none of them moves with the flux.  Env e is therefore the calibrated
 * shard with every WFS amplitude multiplied by a_e = sqrt(h_scale[e]): one multiply in the env dtype where a kernel loads the
 * amplitude (both Shack-Hartmann spot kernels, both Pyramid row kernels, the fused step kernel), the product rounded once -- the bits
 * of a shard whose AOENV_C_WFS_AMP was replaced by the rounded product.  The reconstructor, the modal basis, the photon-noise tables
 * and their range stay those of the calibration, as change_mag leaves them.  The env's threshold takes the place of
 * AoCfg.threshold_cog in  I < thr max -> 0  (ShackHartmann.py:314-324) in the centroid kernel, the fused tail and the fused step kernel.
 * h_scale [n_env]: flux relative to the uploaded AOENV_C_WFS_AMP, finite and > 0; the host forms sqrt in float64 and stores it in the
 * env dtype, h_scale[e] == 1 gives exactly 1.  h_thr [n_env]: finite and >= 0, stored in the env dtype.
 * NULL: back to one value for the shard; the array is then absent (freed), not filled with ones, and the kernels are handed a null
 * pointer: a shard that never made the call, and one that returned, run what they ran before.  With either array present a shard in
 * the fused step kernel's envelope runs an instantiation of that kernel of its own; aoenv_fused_step_active stays 1.
 * Both are configuration, as the per-env mirrors are: copied before the call returns (the stream is waited for once), not loop state,
 * not in the checkpoint buffers, no buffer id; aoenv_reset_envs and aoenv_new_screens* leave them alone.  Everything that steps or
 * measures follows without a new argument: aoenv_step, aoenv_measure, aoenv_reset_soft, aoenv_run_integrator, both recorded
 * rollouts, the modal surface, a delay, a disturbance.  aoenv_compute_psf keeps the calibrated star: the PSF's flux is not per env.
 * Refused, with nothing changed: a non-finite entry, a scale <= 0, a threshold < 0; aoenv_set_threshold_env on a Pyramid shard (no
 * centre of gravity) and on a shard with max_group > 1 (the envs of a batch share the threshold maximum: the interaction-matrix
 * emulation); an allocation that fails.
 * aoenv_get_flux_env fills h_amp [n_env] with the amplitude factors a_e as held (env dtype widened to float64), aoenv_get_threshold_env
 * h_thr [n_env] likewise.  Each fails while its array is absent. */
int aoenv_set_flux_env(AoEnv* env, const double* h_scale, void* stream);
int aoenv_get_flux_env(AoEnv* env, double* h_amp, void* stream);
int aoenv_set_threshold_env(AoEnv* env, const double* h_thr, void* stream);
int aoenv_get_threshold_env(AoEnv* env, double* h_thr, void* stream);

/* Replaces: TimeDelayEnv (MAIN/PO4AO/util_simple.py:25-52, the contract is :46-52: append the action, apply action_buffer[0], drop
 * it), which both trainer mains put around the env with delay = 1 (MAIN/mbrl_main.py:46, MAIN/mbrl_main_network.py:41,
 * MAIN/PO4AO/mbrl_funcsRAZOR.py:32-33), and the action_buffer every gymnasium env of the reference carries (OOPAOEnv_VPG.py:562-566,
 * modalAOEnv.py:150-154, IM_delayEnv.py:164-165, vibrationEnv.py) -- "can also be done inside OOPAO or OOPAO_env", as the docstring
 * of TimeDelayEnv says -- for the loops that run inside the library.
 * With a delay of d frames the library keeps the d actions issued but not yet applied, oldest first: the delay line.  A step that is
 * given (aoenv_step) or forms (aoenv_run_integrator, aoenv_run_rollout, aoenv_run_policy_rollout) action a_k appends it, applies the
 * oldest entry and drops it: step k of an episode applies a_(k-d), or zero for k < d.  Nothing else in the step changes: the order of
 * effects, dm_prev and the leak, telemetry, the return accumulator, the disturbance (tau = t0 + i + 1 whatever the delay).  The
 * recorded trajectories keep the action ISSUED in step k, and so do the policy windows (d_past_act), as mbrl.py:80-81 rolls them.
 * The line is a ring of d + 1 image slots (rlao_amd/csrc/delay.hpp).  aoenv_step copies the caller's action into it in one launch
 * in front of the step (the tensor may be reused at once); aoenv_run_integrator writes gain * obs there with the same kernel (one
 * multiply in the env dtype: the bits a caller forms) and steps as aoenv_step does, its fused-gain epilogue being the path of
 * delay 0; the recorded rollouts use their trajectory as the line -- step k is handed trajectory slot k - d, or a pending row of
 * the ring for k < d, no launch per step -- and one launch at the end of the call copies the newest min(n_steps, d) actions into
 * the ring, so that the line is what n_steps appends would have left, for n_steps < d and across calls of any kind too.
 * aoenv_reset_envs zeroes the rows of the listed envs in every slot; aoenv_reset_soft, aoenv_measure, aoenv_new_screens* and
 * aoenv_set_coefs leave the line alone.
 * aoenv_set_delay sets the delay and zeroes the line; with the delay in force it is the "clear" of TimeDelayEnv.reset /
 * reset_soft (util_simple.py:36-44).  The work is enqueued on `stream`, which is waited for only by the first call with a delay
 * > 0 (the ring is allocated then, for every delay).  delay == 0: every call does exactly what it did without the feature, no
 * extra launch and no changed argument.  Refused, with nothing changed: a null env, a delay outside [0, AOENV_MAX_DELAY]. */
#define AOENV_MAX_DELAY 8
int aoenv_set_delay(AoEnv* env, int delay, void* stream);
int aoenv_get_delay(AoEnv* env, int* delay);
/* The delay line as loop state (TimeDelayEnv.action_buffer, util_simple.py:29-31): host arrays of the env dtype,
 * [delay][n_env][nAct][nAct] in logical order, oldest first, whatever the ring's position.  Both synchronise the stream as
 * aoenv_download / aoenv_upload_state do.  Refused: a null pointer, bytes other than that size, delay == 0. */
int aoenv_get_delay_line(AoEnv* env, void* h_dst, size_t bytes, void* stream);
int aoenv_set_delay_line(AoEnv* env, const void* h_src, size_t bytes, void* stream);

/* Replaces: the modal environments of the reference (MAIN/OOPAOEnv/modalAOEnv.py, modalAOSinEnv.py, OOPAOEnvModal.py, driven by the
 * trainers under MAIN/RL/ and MAIN/VPG/), whose action is a vector of nModes modal coefficients and whose observation is the modal
 * reconstruction:
 *     dm.coefs = dm_prev * leak + (M2C_tt @ a) * 1e-6                    (modalAOEnv.py:150-157)
 *     obs = -(reconstructor_tt @ wfs.signal) * 1e6                       (:165-171; reconstructor_tt = CalibrationVault(D @ M2C[:, :nModes]).M,
 *                                                                         :410, 447-449)
 *     reward = -||obs||^2                                                (:190)
 * as a second surface BESIDE the actuator images of aoenv_step: nothing of the zonal calls changes.  The model is
 * rlao_amd/csrc/modal.hpp.  With K modes, A valid actuators and T the env dtype:
 *     expansion   img[e][act_px[k]] = sum_m m2c[k][m] a[e][m]    micrometres of command; an fma chain in T over m in index order; every
 *                                                                pixel that is no actuator is 0 (vec_to_img); the bits depend on
 *                                                                neither the shard size nor the env's place in it
 *     projection  o[e][m] = -1e6 sum_{j < n_signal} cm[m][j] signal[e][j],   reward[e] = -sum_m o[e][m]^2 (summed in float64)
 *     integrator  a[e][m] = g[e][m] * o_prev[e][m]               one multiply in T
 * aoenv_set_modal hands over the basis: both tables are converted to the env dtype (m2c is kept transposed, [K][A]) and the internal
 * action image [n_env][nAct^2] and the modal scratch are allocated; everything is copied before the call returns and the stream is
 * waited for once.  A NULL cfg forgets the basis and the gains and frees all of it.  Like the disturbance, the basis is
 * configuration: it is NOT loop state, it is in no checkpoint buffer, and a caller that restores a state sets it again.  A new basis
 * forgets the gains of the previous one.  Refused, with nothing changed: n_modes outside [1, A], a null table, a non-finite entry. */
typedef struct AoModal {
    int32_t n_modes;               /* K in [1, A] */
    const double* h_m2c;           /* [A][K] metres of command per unit coefficient BEFORE the step's 1e-6 (M2C_CL[:, :K]) */
    const double* h_cm;            /* [K][n_signal] modal command matrix (calib_tt.M) */
} AoModal;
int aoenv_set_modal(AoEnv* env, const AoModal* cfg, void* stream);
/* The gains of the modal integrator: h_gain [K], or [n_env][K] with per_env != 0 (a gain sweep is then ONE shard; an env whose gains
 * are 0 runs open loop).  Needs a basis.  The stream is waited for once.  Refused, with nothing changed: no basis, a null pointer,
 * a non-finite or negative entry. */
int aoenv_set_modal_gain(AoEnv* env, const double* h_gain, int per_env, void* stream);
/* aoenv_reset_soft (a measurement's reconstruction: no disturbance, the delay line left alone) followed by the projection:
 * d_obs [n_env][K].  The zonal observation goes to internal scratch. */
int aoenv_reset_soft_modal(AoEnv* env, void* d_obs, void* stream);
/* env.step(action) of the modal envs (modalAOEnv.py:139-200).  d_action [n_env][K] modal coefficients, d_obs [n_env][K] out,
 * d_reward [n_env] out: -||o||^2 (may be NULL); d_frame / d_strehl as in aoenv_step.
 * One launch in front of the step forms the action image (k_modal_action) -- under a control delay straight into the delay line's
 * write slot, in place of the copy aoenv_step makes, otherwise into the internal image; the caller's tensor may be reused at once.
 * The step is then EXACTLY the explicit-action step of aoenv_step on that image: the same order of effects (the atmosphere
 * advances, the sensor sees the command latched by the previous call, then the command is updated), the same telemetry,
 * disturbance, delay and per-env mirror, fused or batched as aoenv_step would run it; d_strehl is the step's own.  The zonal
 * observation the step produces goes to internal scratch.  One launch behind the step writes d_obs and d_reward (two launches on
 * the GEMM path of the projection, taken above a size threshold or with AOENV_PATH_MODAL_GEMM); the return accumulator, if
 * attached, receives THIS reward, not the zonal one.
 * Order of effects against the reference: modalAOEnv.step updates the command, measures, then advances the atmosphere (:150-200)
 * with an action_buffer of d entries; the library advances, measures the command of the previous call, then updates.  The loop
 * latency is the same when aoenv_set_delay is d - 1: the reference's default d = 1 is delay 0 here.  The only difference is that
 * the reference's step 0 measures the frame of reset a second time.  (INTEGRATION.md works this through.)
 * aoenv_get_delay_line / aoenv_set_delay_line keep returning IMAGES: the line holds expanded actions.  aoenv_run_rollout,
 * aoenv_run_policy_rollout and the policy stay zonal.
 * Refused: no basis, a null action / obs, a frame index outside [0, n_loop), missing constants. */
int aoenv_step_modal(AoEnv* env, int i, const void* d_action, void* d_obs, void* d_frame, void* d_reward, void* d_strehl,
                     void* stream);
/* The modal integrator kept on the device, the baseline a learned modal controller is compared with: n_steps iterations of
 * a = g * o;  o, reward, strehl = step_modal(i0 + k, a), with the gain multiply fused into the expansion launch.  d_obs
 * [n_env][K] is in/out.  Bit for bit what n_steps calls of aoenv_step_modal give on a = g * o formed by the caller in the env
 * dtype.  Needs aoenv_set_modal_gain.  Only the last step's frame and residual phase can be read afterwards, as after
 * aoenv_run_integrator. */
int aoenv_run_integrator_modal(AoEnv* env, int i0, int n_steps, void* d_obs, void* d_frame, void* d_reward, void* d_strehl,
                               void* stream);

/* Replaces: the modal read-out of the wavefront that the reference forms on the host, always as
 *     opd2m @ tel.OPD[xpupil, ypupil]            with opd2m = pinv(M2OPD)
 * (MAIN_CODE/OOPAOEnv/SinEnv.py:150-204, MultiAtmEnv: the observation is the first modes of the open-loop atmosphere OPD;
 * MAIN_CODE/predictiveControl/EOF/EOF_POL.py:105-123, EOF_OPD.py, linear_extrap/le_OPD.py: time series of the true coefficients;
 * MAIN_CODE/make_dataset.py:84-103: the modal fit of a screen; MAIN_CODE/Plots/AO_plots.py zernike_dist: the modal spectrum of
 * recorded residual frames).  The model is rlao_amd/csrc/wavefront.hpp.  With K modes, R^2 pixels and T the env dtype:
 *     c[e][m] = s * sum_q P[m][q] X[e][q]
 *     P            opd2m scattered to the full grid in T (pixel p of the table = the p-th pixel of np.where(tel.pupil == 1)), zero
 *                  outside the pupil
 *     residual     X = AOENV_B_PHASE (rad at the source wavelength), s = (T)(lambda_src / 2 pi) applied once after the sum: the
 *                  coefficients of tel.OPD in metres
 *     atmosphere   X = what aoenv_download(AOENV_B_OPD_ATM) would return at that moment, s = 1: those of the pupil-masked atm.OPD
 * The sum runs over slices of [0, R^2) whose count and bounds depend on (R^2, K) alone, added in slice order without atomics: an
 * env with the same buffers has the same bits in any shard and at any place in it.  float32 shards sum a slice on the matrix
 * cores, float64 shards and AOENV_PATH_WF_GENERAL as one fma chain; the two orders have the bound of any summation order in common.
 * aoenv_set_wavefront_basis hands over the projector; it is copied (and the slab scratch allocated) before the call returns, the
 * stream is waited for once.  Like the modal basis it is configuration: in no checkpoint buffer, and a caller that restores a
 * state sets it again.  A NULL cfg forgets it and detaches the record; so do a new basis and an upload of AOENV_C_PUPIL.
 * Refused, with nothing changed: n_modes outside [1, min(n_pix, AOENV_MAX_WF_MODES)], n_pix different from the number of pupil
 * pixels or no pupil uploaded, a null table, an entry that is not finite in the env dtype.  No buffer id, no profiled kernel and
 * no ABI version go with it: the coefficients have these accessors of their own, and aoenv_profile does not attribute the
 * projection's launches (the re-derivation of the atmosphere OPD in front of an on-demand atmosphere projection is a launch of the
 * phase kernel and counts under AOENV_K_PHASE, as it does for aoenv_download).  float32 shards take the matrix-core tile of
 * wavefront_kernels.hip up to 64 modes and the split-K GEMM of the reconstruction above (measured: profiles/wavefront_timing.json);
 * the split count of that route is a function of (R^2, K) too. */
#define AOENV_MAX_WF_MODES 1024
enum AoWavefront { AOENV_WF_RESIDUAL = 1, AOENV_WF_ATMOSPHERE = 2,
                   AOENV_WF_SCIENCE = 4 /* the residual toward the science target (aoenv_set_science_direction): X = phase_sci, s as the
                                           residual's; aoenv_project_wavefront alone takes it, one more launch in front; the record refuses it */ };
typedef struct AoWavefrontBasis {
    int32_t n_modes;               /* K in [1, min(n_pix, AOENV_MAX_WF_MODES)] */
    int32_t n_pix;                 /* must equal the number of pupil pixels of the uploaded pupil */
    const double* h_opd2m;         /* [K][n_pix], pixel p = the p-th pixel of np.where(tel.pupil == 1), row-major */
} AoWavefrontBasis;
int aoenv_set_wavefront_basis(AoEnv* env, const AoWavefrontBasis* cfg, void* stream);
/* The coefficients of the buffers as they are now -- after aoenv_reset_soft, aoenv_measure, aoenv_set_atm_opd, an
 * aoenv_upload_state(AOENV_B_PHASE) or a step of the per-call API -- into d_out [n_env][K] (env dtype).  `what` is exactly one
 * AoWavefront bit.  Two launches (the slices, then their sum); the atmosphere is first re-derived from the screens where
 * aoenv_download would do so.  Refused: no basis, zero or two bits, a null d_out. */
int aoenv_project_wavefront(AoEnv* env, int what, void* d_out, void* stream);
/* A per-step record that every stepped call honours: while attached, stepped frame i of aoenv_step, aoenv_step_modal,
 * aoenv_run_integrator, aoenv_run_integrator_modal, aoenv_run_rollout and aoenv_run_policy_rollout writes slot i - i_base of the
 * caller-owned d_rec [n_slots][W][n_env][K] (env dtype; W = the number of bits in `what`, residual first; with both, one pass over
 * P serves the two).  The recorded residual is the one the sensor saw in that step -- the atmosphere after its advance minus the
 * command latched by the previous call, under the delay and with the disturbance: the content AOENV_B_PHASE has after that step,
 * bit for bit what aoenv_project_wavefront gives after the same step of the per-call API.  A loop step then stores the phase (and
 * the atmosphere OPD, with that bit) it otherwise skips, not the camera frame; the loop's state and every output of the loop are
 * bit for bit what they are without the record.  A call whose frames do not all lie in [i_base, i_base + n_slots) is refused
 * before anything is launched.  NULL d_rec detaches; no stream is waited for (the caller keeps d_rec alive until the work
 * enqueued so far is done).  Refused: no basis, no or unknown bits, i_base < 0, n_slots < 1. */
int aoenv_set_wavefront_record(AoEnv* env, int what, void* d_rec, int i_base, int n_slots);

/* Replaces: the exploration episodes of the trainers (MAIN/PO4AO/mbrl.py:64-89), kept on the device and recorded:
 *     action = gain * obs + env.sample_noise(sigma);  next_obs, _, reward, strehl, done, _ = env.step(i, action)
 * for the frames [i0, i0 + n_steps), every observation, action, reward and Strehl ratio written into the caller's trajectory buffers
 * (what replay.append takes).  One extra launch per step forms the action; the step is the explicit-action step of aoenv_step, so a
 * twin env stepped with the recorded actions reproduces the trajectory bit for bit, on every kind of shard.
 * The noise is sigma_e * vec_to_img(Fl (Fr z)), z ~ N(0, 1)^A from a counter-based Philox4x32-7 stream (rlao_amd/csrc/explore.hpp)
 * keyed by `seed` and indexed by (quad of valid actuators, env_index_offset + env, exploration step counter): reproducible, and the
 * same for an env wherever it sits in a batch.  Step k of a call uses counter + k and the call leaves counter + n_steps behind; the
 * counter restarts at 0 only when `seed` differs from the previous call's, and it is word 1 of AOENV_B_COUNTERS (a counter
 * uploaded with aoenv_upload_state belongs to the seed of the next call).  gain * obs is one multiply in the env dtype: at
 * sigma == 0 the action is bit for bit the gain * obs a caller forms.
 * Refused: a null cfg / d_obs / d_action, frames outside [0, n_loop), a negative or non-finite sigma or gain, (A + K) elements that do
 * not fit in a workgroup's LDS, and what aoenv_step refuses.  d_sigma_env is not inspected (it lives on the device).
 * A return accumulator, if attached, receives every step's reward. */
typedef struct AoRollout {
    int32_t  i0, n_steps;          /* frames [i0, i0 + n_steps) within n_loop; n_steps == 0 succeeds and does nothing */
    int32_t  env_index_offset;     /* global index of env 0 of this shard */
    int32_t  reserved;
    double   gain;                 /* may be 0: open-loop exploration */
    double   sigma;                /* >= 0, used when d_sigma_env is NULL */
    const void* d_sigma_env;       /* [n_env] env dtype, caller-owned, or NULL */
    uint64_t seed;
} AoRollout;

/* d_obs    [n_steps+1][n_env][nAct][nAct]  slot 0 = the current observation (in); slot k+1 = obs after step k (out)
 * d_action [n_steps][n_env][nAct][nAct]    out: the action applied in step k
 * d_reward, d_strehl [n_steps][n_env]      out, either may be NULL
 * d_frame  [n_env][cam][cam] or NULL       out: the LAST step's frame, as aoenv_run_integrator */
int aoenv_run_rollout(AoEnv* env, const AoRollout* cfg, void* d_obs, void* d_action, void* d_reward,
                      void* d_strehl, void* d_frame, void* stream);

/* Replaces: ConvPolicy (MAIN/PO4AO/conv_models_simple.py:56-111), the trainer's policy, evaluated inside the library:
 *     out = net(cat([obs, past_obs, past_act], dim=1));  out = out.clamp(-1, 1);  action = vec_to_img(F @ out[valid])
 * net = Conv2d(2H-1, n_filt, 3, padding=1), LeakyReLU, Conv2d(n_filt, n_filt, 3, padding=1), LeakyReLU, Conv2d(n_filt, 1, 3, padding=1).
 * The weights are host float64 arrays in torch's Conv2d layout, so a state_dict of the reference trainer loads unchanged; they are
 * copied (and, for the float32 matrix-core kernel, re-laid) before the call returns.  F = Fl @ Fr in factored form, as
 * aoenv_set_noise_filter takes it.  The two hidden images ([n_env][n_filt][nAct^2], env dtype) are allocated here and freed when
 * the policy is forgotten or replaced.  float32 shards with n_filt % 16 == 0 run the two wide convolutions on the matrix cores;
 * float64 shards, any other n_filt and path = 1 take the general kernel (same sums in the same order, on the vector unit).
 * Refused with nothing changed: n_history / n_filt / proj_rank out of range, a path other than 0 / 1, null or non-finite weights,
 * a non-finite slope, clamp_abs <= 0 (or NaN).  The stream is waited for once. */
typedef struct AoPolicy {
    int32_t n_history;      /* H in [1, 32]; input channels C_in = 2H - 1 */
    int32_t n_filt;         /* filters of the two hidden layers, in [1, 128] */
    int32_t proj_rank;      /* K of the projection factors, 0 = no projection */
    int32_t path;           /* 0 = default kernels, 1 = force the general kernel (parity tests) */
    double  negative_slope; /* LeakyReLU, torch default 0.01 */
    double  clamp_abs;      /* > 0, may be +inf */
    const double *h_w1, *h_b1;  /* [n_filt][C_in][3][3], [n_filt]   torch Conv2d layout */
    const double *h_w2, *h_b2;  /* [n_filt][n_filt][3][3], [n_filt] */
    const double *h_w3, *h_b3;  /* [1][n_filt][3][3], [1] */
    const double *h_proj;       /* as aoenv_set_noise_filter: [K*A] Fr then [A*K] Fl, or NULL */
} AoPolicy;
int aoenv_set_policy(AoEnv* env, const AoPolicy* cfg, void* stream);   /* NULL cfg: forget the policy */

/* Replaces: policy(obs, torch.cat([past_obs, past_act], dim=1)) (MAIN/PO4AO/mbrl.py:73; ConvPolicy.forward,
 * conv_models_simple.py:83-111).  d_obs [n_env][nAct][nAct]; d_past_obs, d_past_act [n_env][H-1][nAct][nAct], OLDEST FIRST, the
 * order mbrl.py:80-81 rolls them in (not read when H == 1); d_action [n_env][nAct][nAct] out, zero off the valid actuators.
 * All in the env dtype.  Channel order [obs, past_obs.., past_act..] (conv_models_simple.py:89).
 * Refused: no policy set, a null obs / action, a null history with H > 1. */
int aoenv_policy_forward(AoEnv* env, const void* d_obs, const void* d_past_obs, const void* d_past_act,
                         void* d_action, void* stream);

/* Replaces: the policy episodes of the trainers (MAIN/PO4AO/mbrl.py:64-89, the branch of :72-74), on the device and recorded as
 * aoenv_run_rollout records the warm-up episodes:
 *     action = policy(obs, cat([past_obs, past_act])) + env.sample_noise(sigma);  step;  roll past_obs, past_act (:80-81)
 * Buffers, cfg, noise stream, counter and refusals as aoenv_run_rollout; cfg->gain must be 0.  At sigma == 0 (the reference adds
 * no noise after the warm-up) the action is bit for bit what aoenv_policy_forward returns for the same windows.
 * No history ring lives in the library: at step k past channel c is trajectory slot k - (H-1) + c of d_obs / d_action when that
 * is >= 0 and row k + c of d_past_obs / d_past_act otherwise.  On return d_past_obs / d_past_act (in/out, [n_env][H-1][nAct][nAct],
 * oldest first, not read when H == 1) hold the windows n_steps iterations of mbrl.py:80-81 leave.  A caller that restarts some
 * envs (aoenv_reset_envs) clears their rows itself.
 * Three launches per step in front of the step: the two wide convolutions and the last stage. */
int aoenv_run_policy_rollout(AoEnv* env, const AoRollout* cfg, void* d_obs, void* d_action, void* d_reward,
                             void* d_strehl, void* d_frame, void* d_past_obs, void* d_past_act, void* stream);

/* Replaces: tel.computePSF(zeroPaddingFactor) (OOPAO/Telescope.py:258-357) of the current residual phase (tel.src.phase):
 * d_psf [n_env][M][M], M = zero_padding * R (even), env dtype: the short-exposure PSF of every env.  As the reference does for even
 * image sizes (oversampling 2, :303-305), the field is transformed at N = 2 M and |fftshift(fft2(E phasor)) / N|^2 is sum-binned 2 x 2.
 * For odd R (M still even) the reference pads ceil((2 M - R) / 2) on both sides and transforms at 2 M + 1 (:320-325): the image is then
 * formed as the science window below with W = M, not by the 2 M-point transform.
 * Science-path rendering (MAIN/OOPAOEnv/OOPAOEnv.py:473-482, integrator_network.py:93-95); not part of the step. */
int aoenv_compute_psf(AoEnv* env, int zero_padding, void* d_psf, void* stream);

/* Replaces: the long-exposure PSF and its Strehl ratio as the reference's evaluation scripts form them on the host from one full
 * render per step,
 *     env.tel.computePSF(4); SE_PSFs.append(env.tel.PSF[175:-175, 175:-175]); LE_SR = max(mean(SE_PSFs)) / psf_model_max
 * (MAIN_CODE/predictiveControl/POL_error_CL.py; MAIN_CODE/integrator_network.py:134-138), and the mean of log10(PSF) over the frames
 * current_i > 15 of render4plot (MAIN_CODE/OOPAOEnv/OOPAOEnv.py:473-482).  The model is rlao_amd/csrc/science.hpp: the W x W window
 * around the core of tel.computePSF(zero_padding) -- output pixel (a, b) is pixel (M/2 - W/2 + a, M/2 - W/2 + b) of the M x M image,
 * M = zero_padding * R -- without the full transform: the 2 W oversampled rows the window needs are the rows of a table F [2W][R],
 * into which the reference's padding offset, ifftshift and even-size phasor fold (OOPAO/Telescope.py:320-332), and
 *     window = bin2x2(|F E F^T|^2) / n_fft^2,   E = amp * exp(i phase)   (R x R),
 * two small complex products per env: on the fp32 matrix cores for float32 shards (k_science_window_mfma), as fma chains for
 * float64 shards, under AOENV_PATH_SCI_GENERAL and where the matrix-core plan refuses (k_science_window).  n_fft is the reference's
 * transform length, 2 M for even R and 2 M + 1 for odd R (its padding is ceil((2 M - R) / 2) on both sides).  The order of every sum
 * depends on (R, W) alone and there are no atomics: an env has the same bits in any shard and at any place in it.
 * aoenv_set_science copies the table (evaluated in float64 on the reduced integer angle, rounded once to the env dtype; or h_dft
 * in its place) and the amplitude to the device before it returns and waits for the stream once.  The amplitude is that of
 * aoenv_compute_psf: AOENV_C_WFS_AMP, times sqrt(pyr_n_theta) on a Pyramid shard; per-env flux does not enter.  Like the wavefront
 * basis it is configuration: in no checkpoint buffer.  A NULL cfg forgets it and detaches the accumulators; so do a new
 * configuration and an upload of AOENV_C_PUPIL or AOENV_C_WFS_AMP.
 * Refused, with nothing changed: zero_padding outside [1, 8], zero_padding * R odd, window odd or outside [2, zero_padding * R],
 * first_frame < 0, an unknown flag, an entry of h_dft that is not finite in the env dtype, no amplitude uploaded.
 * No buffer id, no profiled kernel and no ABI version go with it. */
enum AoScienceFlag { AOENV_SCI_LOG10 = 1 };
typedef struct AoScience {
    int32_t zero_padding;   /* zp */
    int32_t window;         /* W */
    int32_t first_frame;    /* stepped frames i >= first_frame are accumulated (reference: current_i > 15 -> 16) */
    int32_t flags;
    const double* h_dft;    /* NULL: the library's table; else [2W][R][2] (re, im), used in its place */
} AoScience;
int aoenv_set_science(AoEnv* env, const AoScience* cfg, void* stream);
/* The window of AOENV_B_PHASE as it is now (flat != 0: of a zero phase, the diffraction-limited PSF the Strehl ratio divides by)
 * into d_out [n_env][W][W], env dtype.  One launch, no scratch, no wait.  Refused: nothing set, a null d_out. */
int aoenv_science_psf(AoEnv* env, int flat, void* d_out, void* stream);
/* The long exposure.  d_sum and d_sum_log10 [n_env][W][W] (env dtype) and d_count [n_env] are caller-owned device buffers, zeroed
 * by the caller; the library holds the pointers only.  While attached, every stepped frame i >= first_frame of aoenv_step,
 * aoenv_step_modal, aoenv_run_integrator, aoenv_run_integrator_modal, aoenv_run_rollout and aoenv_run_policy_rollout adds the
 * window of the residual the sensor saw in that step (the content AOENV_B_PHASE has after it) to d_sum, its log10 to d_sum_log10,
 * and 1 to d_count: one extra launch per accumulated step.  Such a loop step stores the phase it otherwise skips, not the
 * camera frame; the loop's state and every output are bit for bit what they are without it, and a fused shard stays fused.
 * d_sum_log10 must be non-null exactly when AOENV_SCI_LOG10 is set.  NULL d_sum detaches; no stream is waited for. */
int aoenv_set_science_accumulator(AoEnv* env, void* d_sum, void* d_sum_log10, int32_t* d_count);

/* Replaces: the reference env's second source, put off axis "to simulate anisoplanetism" (MAIN_CODE/OOPAOEnv/OOPAOEnv.py:140-146,
 * 303-304, 335-336: self.src.coordinates = [0.4, 0]; atm * src, OOPAO/Atmosphere.py:313-334, 439-450, 643-647): per env, a science
 * target at [zenith arcsec, azimuth deg] seen through the same layers and the same mirror as the guide star.  The model is
 * rlao_amd/csrc/offaxis.hpp.  For a layer at altitude h on its N x N grid
 *     [x_z, y_z] = pol2cart(h tan(zenith / 206265) R / D, deg2rad(azimuth))    pixels; y_z moves rows, x_z columns
 * and the target's R x R footprint reads layer.phase (the wind's clipped bicubic warp) at (row + N//2 - R//2 + y_z, column + N//2 -
 * R//2 + x_z), bilinearly, exactly where the reference translates: unless both offsets are whole pixels.  The host computes floor
 * and fraction of every (layer, env) in float64; the blend runs in the env dtype.  The mirror is conjugated to the pupil:
 *     OPD_sci = (OPD_no_pupil_sci + dm.OPD) * pupil,  phase_sci = OPD_sci 2 pi / lambda_src,
 *     rms_sci = std(OPD_sci[pupil]) 1e9,  strehl_sci = exp(-var(phase_sci[pupil]))
 * with the surface the sensor saw in that step (delay, disturbance, per-env mirrors included); the library forms it as
 * AOENV_B_PHASE + (OPD_no_pupil_sci - OPD_no_pupil) 2 pi / lambda_src.  The pupil sums are float64 in a fixed order, no atomics: an
 * env has the same bits in any shard and at any place in it; at zenith 0 OPD_no_pupil_sci and phase_sci are bit for bit
 * AOENV_B_OPD_ATM and AOENV_B_PHASE.
 * aoenv_set_field tells the library what it is otherwise never told: the telescope's diameter [m], its field of view [arcsec] and
 * the n_layer altitudes [m].  Refused: values that are negative or not finite, and any call while a direction is set.
 * aoenv_set_science_direction takes [n_env] arrays; it copies the footprints (and allocates phase_sci scratch) before it returns and
 * waits for the stream once.  Configuration: in no checkpoint buffer.  Both arrays NULL forget the direction and detach its record.
 * Refused, with nothing changed: no field set, a shard without layers, a zenith that is negative, not finite or above fov / 2, an
 * azimuth that is not finite, and a footprint whose interpolation taps would leave the layer's screen (with the reference's grid
 * rule N = ceil(R / D (D + 2 tan(fov / 2) h)) + 4 no zenith <= fov / 2 does).  Every zenith 0 is legal.
 * No buffer id, no profiled kernel and no ABI version go with it. */
int aoenv_set_field(AoEnv* env, double diameter, double fov_arcsec, const double* h_altitude);
int aoenv_set_science_direction(AoEnv* env, const double* h_zenith_arcsec, const double* h_azimuth_deg, void* stream);
int aoenv_get_science_direction(AoEnv* env, double* h_zenith_arcsec, double* h_azimuth_deg);
/* The residual toward the target of the buffers as they are now -- after aoenv_reset_soft, aoenv_measure or a step of the per-call
 * API: d_phase_sci [n_env][R*R] (rad at the source wavelength), d_opd_atm_sci [n_env][R*R] (OPD_no_pupil toward the target, m),
 * d_rms_nm and d_strehl [n_env], all in the env dtype, any of them NULL.  One launch, after the re-derivation of the on-axis
 * atmosphere OPD where aoenv_download(AOENV_B_OPD_ATM) would re-derive it.  Refused: no direction set, a user-defined atmosphere OPD
 * (aoenv_set_atm_opd: there are no layers to look through until the atmosphere advances again). */
int aoenv_science_residual(AoEnv* env, void* d_phase_sci, void* d_opd_atm_sci, void* d_rms_nm, void* d_strehl, void* stream);
/* A per-step record by the rules of aoenv_set_wavefront_record: while attached, stepped frame i of every stepped call writes slot
 * i - i_base of the caller-owned d_rec [n_slots][2][n_env] (env dtype): rms nm, then Strehl, toward the target.  One extra launch
 * per recorded step; such a step stores the phase and the on-axis atmosphere OPD it otherwise skips; the loop's state and outputs
 * are bit for bit what they are without it; a fused shard stays fused; AOENV_OPT_STEP_PAIRS stands down.  A call whose frames do
 * not all lie in the window is refused before anything is launched.  NULL detaches.  Refused: no direction, i_base < 0, n_slots < 1.
 * While a direction is set, aoenv_science_psf(flat = 0) and the long exposure form their window from phase_sci (one more launch in
 * front of the window's); aoenv_compute_psf keeps the guide star's direction. */
int aoenv_set_science_direction_record(AoEnv* env, void* d_rec, int i_base, int n_slots);

/* Replaces: a guide star off axis, `ngs.coordinates = [zenith arcsec, azimuth deg]` with `atm * ngs` and then `tel * dm * wfs`
 * (OOPAO/Atmosphere.py:313-334, 439-450): per env, the SENSOR's line of sight through the layers.  The model, the host plan and the
 * refusals are the science direction's (rlao_amd/csrc/offaxis.hpp): [n_env] arrays, the footprints copied before the call returns,
 * the stream waited for once; both arrays NULL forget the direction.  Refused, with nothing changed: no field set, a shard without
 * layers, one array NULL, a zenith that is negative, not finite or above fov / 2, an azimuth that is not finite, a footprint whose
 * taps would leave the layer's screen.  aoenv_set_field is refused while a guide direction is set.
 * While a direction is set, wherever the library derives the atmosphere from the screens -- aoenv_step, aoenv_measure,
 * aoenv_atm_update, aoenv_reset_soft, aoenv_run_integrator, both rollouts, the modal calls, aoenv_download(AOENV_B_OPD_ATM),
 * aoenv_project_wavefront(AOENV_WF_ATMOSPHERE), aoenv_get_phase_no_pupil, aoenv_science_residual -- one launch (a workgroup per
 * 16 x 64 pixel tile and env, no sums, no atomics) writes OPD_no_pupil toward every env's guide star into AOENV_B_OPD_ATM, and the
 * phase kernel takes it from there, as it takes a user-defined OPD.  Everything behind it -- the mirror of any kind, the delay, a
 * disturbance, the sensor of any kind, the camera, reward, Strehl and telemetry -- follows without a change.  A user-defined OPD
 * (aoenv_set_atm_opd) still wins until the atmosphere advances.  An env has the same bits in any shard and at any place in it; at
 * zenith 0 every output is bit for bit that of the batched kernels without a direction.
 * The shard leaves the fused step kernel while a direction is set (aoenv_fused_step_active reports 0; the batched kernels run, as
 * for a rotated mirror) and returns to it, bit-identical to an untouched shard, when the direction is forgotten.
 * The science arm differences against the OPD the sensor saw: phase_sci = AOENV_B_PHASE + (OPD_no_pupil_sci - AOENV_B_OPD_ATM) 2 pi /
 * lambda_src.  So with no science direction the science camera keeps looking at the guide star, wherever it is; with a science
 * direction of zenith 0 it looks along the axis while the sensor looks off it (classical anisoplanatism); with both directions
 * equal OPD_no_pupil_sci and phase_sci are bit for bit AOENV_B_OPD_ATM and AOENV_B_PHASE.
 * Configuration: in no checkpoint buffer, untouched by aoenv_reset_envs and aoenv_new_screens*.  No buffer id, no profiled kernel
 * and no ABI version go with it. */
int aoenv_set_guide_direction(AoEnv* env, const double* h_zenith_arcsec, const double* h_azimuth_deg, void* stream);
int aoenv_get_guide_direction(AoEnv* env, double* h_zenith_arcsec, double* h_azimuth_deg);

/* Replaces: a static optical-path map in the optical train, the reference's OPD_map and NCPA objects (OOPAO/OPD_map.py,
 * OOPAO/NCPA.py; `ngs*tel*map*dm*wfs`, applied as tel.OPD += obj.OPD, tel.OPD_no_pupil += obj.OPD, OOPAO/Telescope.py:502-512) -- for
 * the envs of ONE shard, one map per env and per arm.  h_wfs is the map S_w the wavefront sensor sees, h_sci the map S_s the
 * science camera sees: float64, metres, unmasked.  per_env is the number of maps in each array: n_env for [n_env][R*R], one map
 * per env, or 0 for ONE map [R*R] for the whole shard (one copy is held and read with stride 0).  A NULL arm is a zero arm; both NULL clear the feature and free its memory.  A common-path
 * aberration is the same map in both arms; the classic non-common-path case is h_wfs = N, h_sci = NULL: the loop drives the
 * sensor's residual to zero and prints -N into the science image.
 * Sensor arm:  OPD_no_pupil = atm + S_w + dm,  OPD = that times the pupil.  Observation, reward, Strehl, residual rms,
 * AOENV_B_PHASE and a geometric shard's unmasked phase (S_w unmasked there) include S_w; the atmosphere's own numbers
 * (AOENV_B_OPD_ATM, the `total` telemetry, aoenv_project_wavefront(AOENV_WF_ATMOSPHERE)) do not.  The map is added on the mirror
 * side of the sum: while S_w is set the shard forms mirror surface + S_w ahead of the phase kernel, wherever the command changes,
 * and k_phase<T> reads it (as for actuator factor pairs and a dense mirror): the batched kernels run, aoenv_fused_step_active
 * reports 0 and the step pairs stand down until the map is cleared, when the shard launches what it launched before.  A separable
 * mirror (shared tables, aoenv_set_dm_env's, the composite two-mirror tables) forms Gy C Gx^T + S_w on the fp32 matrix cores on
 * float32 shards up to 128 actuators across (k_dm_rows, then k_dm_static_mfma, whose accumulators start from the map), and as one
 * fma chain per pixel on float64 shards, above 128 actuators across and under AOENV_PATH_DM_STATIC_GENERAL (k_dm_static); the order
 * of either sum depends on (R, n_act) alone, there are no atomics, and an env has the same bits in any shard and at any place in
 * it.  A shard that forms its surface ahead anyway (actuator pairs, a dense mirror) gets one trailing launch that adds the map into
 * a buffer of its own; aoenv_get_dm_surface keeps returning the mirror alone (and stays refused on a separable mirror).
 * Science arm:  phase_sci = AOENV_B_PHASE + ((OPD_no_pupil_sci - AOENV_B_OPD_ATM) + (S_s - S_w)) 2 pi / lambda_src inside the pupil, 0
 * outside; the first bracket only while a science direction is set.  The host forms D = S_s - S_w in float64 and the device holds
 * S_w and D in the env dtype; S_w is held whenever h_wfs is not NULL (zeros included: the shard then takes the path
 * of a shard with a map), D only where it is not zero everywhere in the env dtype (a common-path aberration leaves the science arm
 * on the sensor's phase).  While D is held, "the science arm differs from the sensor's"
 * exactly as under a science direction: aoenv_science_psf(flat = 0), the long exposure, aoenv_science_residual,
 * aoenv_project_wavefront(AOENV_WF_SCIENCE) and aoenv_set_science_direction_record look at phase_sci, formed by one light launch
 * that walks no layer (k_science_static; pupil sums in float64 in a fixed order) or, under a direction, by k_science_residual with D
 * as one more term.  Without a direction aoenv_science_residual's d_opd_atm_sci must be NULL.
 * Calibration never sees the maps (set them after the tables are uploaded): a sensor-arm map is an offset in the slopes.
 * Configuration like the guide direction: copied before the call returns (the stream is waited for once), in no checkpoint buffer,
 * untouched by aoenv_reset_envs and aoenv_new_screens*.  No buffer id, no profiled kernel and no ABI version go with it.
 * Device memory (ONE block): the maps held, R^2 sizeof(dtype) each per env (or once); with S_w n_env R^2 sizeof(dtype) of surface
 * and, on a separable mirror, n_env (R pad 128) 4 ga_stride sizeof(float) of Gy C or n_env n_act^2 sizeof(dtype) of command images;
 * with D n_env R^2 sizeof(dtype) of phase_sci.
 * Refused, with nothing changed and nothing launched: per_env that is neither 0 nor the shard's n_env (arrays made for a shard of
 * another size), a non-finite entry or one that is not finite in the env dtype (the arm and index are reported), an allocation
 * that fails.
 * aoenv_get_static_opd fills h_wfs and h_sci ([n_env][R*R] float64 each, either may be NULL) with the maps as given (a shared map
 * repeated for every env, a zero arm as zeros); refused while no map is set. */
int aoenv_set_static_opd(AoEnv* env, const double* h_wfs, const double* h_sci, int per_env, void* stream);
int aoenv_get_static_opd(AoEnv* env, double* h_wfs, double* h_sci);
/* Which launch forms mirror surface + S_w with the maps, tables and options as they are now (an answer, not a status, like
 * aoenv_fused_step_active): 0 = no sensor-arm map, 1 = k_dm_rows + k_dm_static_mfma, 2 = k_coefs_image + k_dm_static<T>, 3 = the
 * trailing k_static_add behind actuator pairs or a dense mirror; -1 for a null env.  h_launches, if not NULL, receives int64 [4]:
 * how often each of these has refreshed a surface since the shard was created (index 0 is never counted). */
int aoenv_static_surface_path(AoEnv* env, int64_t* h_launches);

/* Replaces: the spot elongation of a laser guide star in the diffractive Shack-Hartmann (OOPAO/ShackHartmann.py:189-192, 239-240,
 * 396-503, 554-556: behind a Source with a sodium profile and an up-link FWHM the sensor convolves every valid lenslet's unbinned
 * n x n spot intensity, n = 2 p, with a kernel of that lenslet's own, I = fftshift(abs(ifft2(fft2(I) * C))), before the 2 x 2
 * binning, the camera and the centroid) -- for the envs of ONE shard, one table per env or one for the shard.
 * h_taps is float64 [per_env ? n_env : 1][n_valid_subap][n*n]: the kernels K = real(ifft2(C)) with the shift and the binning folded in,
 *     Kb[x][y]     = K[x][y] + K[x+1][y] + K[x][y+1] + K[x+1][y+1]                                  (indices mod n)
 *     camera[P][Q] = sum_{s,t} I[s][t] Kb[(2 P + n/2 - s) mod n][(2 Q + n/2 - t) mod n]              (I = |FFT2(E) / n|^2, unbinned)
 * (rlao_amd/calib.py: lgs_spot_kernels restates get_convolution_spot, lgs_binned_taps forms Kb and the box).  `bytes` is the size
 * of h_taps; per_env is n_env for a table per env or 0 for ONE table (one copy is held and read with a per-env stride of 0, as the
 * per-env mirror tables are).  box = {x0, y0, nx, ny}: every non-zero tap of every lenslet of the table lies in rows x0 .. x0 + nx - 1
 * and columns y0 .. y0 + ny - 1 (mod n) of its n x n array; the kernel's tap loop runs over the box alone ({0, 0, n, n}: all taps).
 * While a table is set the spots come from k_sh_spots_lgs<T> (sh_lgs_kernels.hip; timed under AOENV_K_SH_SPOTS): k_sh_spots'
 * transform with the unbinned intensity kept in LDS, then the tap sum in ascending tap order, whatever the box -- a zero tap adds
 * exactly nothing, so an env has the same bits under any box that holds its taps, beside any other envs' tables and at any place in
 * the shard.  Everything behind the frame (camera and noise streams, centroid, thresholds, every loop) is what it was; the guide
 * star's flux per env applies.  The shard leaves the fused step kernel (aoenv_fused_step_active reports 0; the batched kernels
 * run) and returns to it, bit-identical to an untouched shard, when the table is forgotten: h_taps = NULL (bytes, per_env and box are
 * then ignored).  Calibration shards are handed the table like any other (the reference calibrates behind the LGS source).
 * Configuration like the mirror tables: copied before the call returns (the stream is waited for once), rounded once to the env
 * dtype, in no checkpoint buffer, untouched by aoenv_reset_envs and aoenv_new_screens*.  No buffer id, no profiled kernel and no ABI
 * version go with it.  Device memory (ONE block): the table in the env dtype.
 * Refused, with nothing changed and nothing launched: a Pyramid or geometric shard; a per_env that is neither 0 nor n_env; a byte count
 * that is not the table's; a box outside [0, n) (x0, y0 in [0, n), nx, ny in [1, n]); a tap that is negative, not
 * finite (also once rounded to the env dtype) or non-zero outside the box; a lenslet whose taps sum to zero; a lenslet size whose
 * LDS image does not fit; an allocation that fails.
 * aoenv_get_lgs_spots returns the table as given (h_taps sized as it was set), *per_env (n_env or 0) and the box; any may be NULL;
 * refused while no table is set. */
int aoenv_set_lgs_spots(AoEnv* env, const double* h_taps, size_t bytes, int per_env, const int32_t box[4], void* stream);
int aoenv_get_lgs_spots(AoEnv* env, double* h_taps, int32_t* per_env, int32_t box[4]);

/* Replaces: the WFS camera settings wfs.cam.{photonNoise, readoutNoise, QE, darkCurrent, integrationTime, FWC, bits, gain,
 * sensor} (OOPAO/Detector.py:19-60; Papyrus: photonNoise = True, MAIN/OOPAOEnv/OOPAOEnv.py:379; Razor:
 * OOPAOEnvRazor.py:243-250, 333).  The frame of every measurement then goes through integrate() + readout()
 * (Detector.py:232-301) before the slopes are computed.  The reference seeds its noise generators from the wall clock;
 * here every pixel of every frame draws from a counter-based stream keyed by `seed` and indexed by (pixel, env_index_offset
 * + env, frame number): reproducible, and the same for an env wherever it sits in a batch.  NULL = ideal detector.
 * The frame number keeps counting across calls (a camera setting changed in mid-run does not replay earlier noise frames); it
 * restarts at 0 only when `seed` changes, and it is part of the checkpoint (AOENV_B_COUNTERS).  Work is enqueued on `stream`. */
typedef struct AoDetector {
    int32_t photon_noise;    /* cam.photonNoise */
    int32_t bits;            /* ADC bits, 0 = None (needs fwc > 0 when set) */
    int32_t emccd;           /* sensor == 'EMCCD': gain before the read-out noise; CCD / CMOS: after */
    int32_t env_index_offset; /* global index of env 0 of this shard (multi-GPU sharding) */
    double  qe;              /* cam.QE */
    double  dark_electrons;  /* cam.darkCurrent * cam.integrationTime */
    double  fwc;             /* cam.FWC, 0 = None */
    double  gain;            /* cam.gain */
    double  readout_noise;   /* cam.readoutNoise [e- rms] */
    uint64_t seed;
} AoDetector;
int aoenv_set_detector(AoEnv* env, const AoDetector* cfg, void* stream);

/* Episode return on the device (the sum of rewards the trainers accumulate on the host, MAIN/PO4AO/mbrl.py:64-89):
 * d_return [n_env] is a caller-owned device buffer of the env dtype; every aoenv_step / integrator step adds its reward
 * to it.  NULL detaches it.  The caller zeroes it at the start of an episode. */
int aoenv_set_return_accumulator(AoEnv* env, void* d_return);

/* State access (get_state / set_state = checkpoint / resume of the env; also the stage boundaries
 * compared by the parity tests).  The complete loop state is {AOENV_B_SCREEN, aoenv_get_buff, AOENV_B_MT_STATE,
 * AOENV_B_COEFS, AOENV_B_DM_PREV, AOENV_B_COUNTERS}, under a control delay {aoenv_get_delay, aoenv_get_delay_line} (no AoBuf: the
 * line has functions of its own), plus the caller's last observation; aoenv_upload_state(AOENV_B_SCREEN) takes the
 * logical layer.mapShift (as aoenv_download returns it) and re-derives the clip range.  `which` is an AoBuf.  aoenv_buffer returns the device pointer and size in bytes;
 * aoenv_download copies to a host buffer of the env dtype and synchronises the stream. */
int aoenv_buffer(AoEnv* env, int which, void** d_ptr, size_t* bytes);
int aoenv_download(AoEnv* env, int which, void* h_dst, size_t bytes, void* stream);
int aoenv_upload_state(AoEnv* env, int which, const void* h_src, size_t bytes, void* stream);
/* Replaces: reading src.phase_no_pupil (OOPAO/Telescope.py:404-412) on a geometric shard (AOENV_WFS_SH_GEOMETRIC): h_dst [n_env][R*R]
 * in the env dtype, the unmasked phase (atm.OPD_no_pupil + dm.OPD) 2 pi / lambda_src the last phase kernel wrote -- inside the pupil
 * AOENV_B_PHASE bit for bit (the same add and the same multiply).  Derived, not checkpoint state, and no AoBuf: the buffer exists on
 * geometric shards only.  Synchronises the stream.  Refused: any other shard, a null pointer, bytes other than that size. */
int aoenv_get_phase_no_pupil(AoEnv* env, void* h_dst, size_t bytes, void* stream);
/* host-side atmosphere clock: h_buff [n_layer][2] float64 (layer.buff, OOPAO/Atmosphere.py:392-404) */
int aoenv_get_buff(AoEnv* env, double* h_buff);
int aoenv_set_buff(AoEnv* env, const double* h_buff);

/* Implementation switches (parity tests compare the specialised kernels with the generic ones). */
enum AoOption {
    AOENV_OPT_FAST_WFS = 0,  /* 1 (default): register-resident 6 px/lenslet SH kernel; 0: generic LDS kernel */
    AOENV_OPT_MFMA_GEMM = 1, /* 1 (default): float32 split-K MFMA contractions; 0: generic tiled VALU kernel */
    AOENV_OPT_STORE_ATM_OPD = 3, /* 1: every step also writes atm.OPD_no_pupil to AOENV_B_OPD_ATM; 0 (default): it is
                                re-derived from the screens when it is downloaded */
    AOENV_OPT_FUSED_TAIL = 4, /* 1 (default): when AOENV_C_RECON_FACTORS is uploaded, SH centroid + low-rank R.s + epilogue run as
                                 one per-env kernel; 0: separate centroid / MFMA GEMM / epilogue kernels */
    AOENV_OPT_FUSED_STEP = 5, /* 1 (default): float32 SH shards with 6 px per lenslet, <= 336 valid lenslets, R <= 128 and uploaded
                                 AOENV_C_RECON_FACTORS run the whole step as ONE kernel, one workgroup per env, every intermediate in LDS;
                                 0: the separate phase / spots / tail kernels */
    AOENV_OPT_DEFER_RING = 6, /* 1 (default): on a step where a layer crosses a pixel, the fused step kernel itself writes the new
                                 border ring of the screen (sum of the ring GEMM's slabs); 0: a separate scatter launch */
    AOENV_OPT_COEFS_IMAGE = 7, /* 1: the per-env part of the DM surface is formed once per step by a small kernel instead of once per
                                 tile of the separate phase kernel: float32 shards Gy.C on the matrix cores (MFMA operand layout),
                                 float64 shards the scattered command image (always on above 1024 actuators: ELT-size DMs);
                                 0 (default below): every tile workgroup does it itself */
    AOENV_OPT_FACTORED_RECON = 8, /* 1 (default): with AOENV_C_RECON_FACTORS uploaded, the batched (non-fused) reconstruction is the
                                 chained product v = M2C (M s) instead of the dense reconstructor; 0: dense */
    AOENV_OPT_RING_LOOKAHEAD = 9, /* 1 (default): float32 fused step, shared clock: the ring pipeline -- the operand [Z | xi] of a layer's NEXT
                                 pixel crossing is put together while the current one is served: xi by extra workgroups of the ring GEMM's
                                 launch, Z by the step kernel once it has written the ring; a crossing step then launches the GEMM and
                                 nothing else in front of the step kernel (bit-identical results).  0: gather + draw in a launch of
                                 their own in front of the GEMM.  [Round-2 note: the same work one crossing ahead on a SECOND STREAM was
                                 slower -- with one 1024-lane workgroup per CU the side stream finds no free CU (5.59 -> 4.97 M env-steps/s)] */
    AOENV_OPT_FAST_TRIG = 2, /* 1 (default): v_sin/v_cos after Cody-Waite reduction in the float32 SH kernel; 0: sincosf */
    AOENV_OPT_ENV_WIND_PIXELS = 10, /* n in [1, 8] (default 1): per-env clocks (aoenv_set_wind_env, aoenv_set_clock_env, the switch
                                 inside aoenv_reset_envs) take |ratio| < n pixels per frame on each axis; a step then makes up to n - 1
                                 whole-pixel ring rounds per layer in front of the sub-pixel one.  Other values are rejected, and so is
                                 lowering n to or below a ratio the shard's clocks hold, with nothing changed.  Raising it costs a shard
                                 whose winds stay below one pixel per frame nothing: the same launches */
    AOENV_OPT_STEP_PAIRS = 11, /* 1 (default): aoenv_run_integrator without a delay, float32 fused step, shared clock, a specialised
                                 instantiation of the step kernel whose camera gives whole-number pixels (photon noise alone, or any camera with an ADC; not the
                                 ideal detector, nor read-out noise, gain or quantum efficiency without an ADC), and no disturbance, wavefront record, long exposure, atmosphere
                                 store or modal loop: a step takes the step behind it along in its launch where no layer makes a
                                 whole-pixel round or crosses a pixel in that one (two steps, one workgroup per env, nothing read back
                                 from global memory in between; bit-identical results).  0: one launch per step */
    AOENV_OPT_FORCE_PATH = 99 /* AoPath bits (default 0): force the general kernel where a specialised one applies; any bit set
                                 other than AOENV_PATH_MODAL_GEMM, AOENV_PATH_SH_PLAIN, AOENV_PATH_WF_GENERAL, AOENV_PATH_SCI_GENERAL, AOENV_PATH_DM_PAIRS_GENERAL and AOENV_PATH_DM_STATIC_GENERAL also keeps the shard off the fused step
                                 kernel; other bits are rejected */
};
/* Bits of AOENV_OPT_FORCE_PATH: each selects another correct implementation (parity tests compare it with the default). */
enum AoPath {
    AOENV_PATH_PHASE_DWORD = 256,      /* float32 phase kernel with dword accesses instead of the 16-byte one (R % 4 == 0) */
    AOENV_PATH_GENERIC = 512,          /* the Stockham Pyramid passes at nRes 528 / 288, the tiled 16-byte phase kernel instead of its
                                          one-layer band form */
    AOENV_PATH_PYR_ROUND_ROBIN = 1024, /* nRes 528 / 288 Pyramid column pass: blocks dealt round-robin over the XCDs */
    AOENV_PATH_MODAL_GEMM = 2048,      /* the projection of the modal surface (aoenv_step_modal) as a batched GEMM plus a finish kernel
                                          whatever its size, instead of the per-env kernel below the threshold.  It touches nothing
                                          inside the step, so unlike the other bits it leaves the shard on the fused step kernel: the
                                          loop state is the same bit for bit, only the order of the projection's sum differs */
    AOENV_PATH_WF_GENERAL = 8192,      /* the wavefront projection (aoenv_project_wavefront, the record) as one fma chain per (env, mode,
                                          slice) on float32 shards too, instead of the matrix-core kernel.  Like AOENV_PATH_MODAL_GEMM
                                          it touches nothing inside the step and leaves the shard on the fused step kernel */
    AOENV_PATH_SCI_GENERAL = 16384,    /* the science window (aoenv_science_psf, the long exposure) as fma chains on float32 shards
                                          too, instead of the matrix-core kernel.  Like AOENV_PATH_WF_GENERAL it touches nothing
                                          inside the step and leaves the shard on the fused step kernel */
    AOENV_PATH_DM_PAIRS_GENERAL = 32768, /* the surface of actuator factor pairs (aoenv_set_dm_pairs) as one fma chain per pixel on float32
                                          shards too, instead of the matrix-core kernel.  It touches nothing of a shard without pairs,
                                          which stays on the fused step kernel */
    AOENV_PATH_DM_STATIC_GENERAL = 65536, /* the surface of a separable mirror with a sensor-arm static map (aoenv_set_static_opd) as
                                          one fma chain per pixel on float32 shards too, instead of the matrix-core kernel.  It touches
                                          nothing of a shard without such a map, which stays on the fused step kernel */
    AOENV_PATH_SH_PLAIN = 4096         /* the general instantiation of the fused step kernel (run-time camera and trig tests, the
                                          pixel-by-pixel stage A epilogue) and the plain C++ lenslet transform, there and in the
                                          batched spots kernel, instead of the forms specialised for the launch and the register-pair
                                          transform.  The shard stays on the fused step kernel; every output is the same bit for bit */
};
int aoenv_set_option(AoEnv* env, int option, int value);

/* Which path aoenv_step would take with the tables, options and camera as they are now: 1 = the whole step as one kernel
 * (float32 Shack-Hartmann, 6 pixels per lenslet, <= 336 valid lenslets, R <= 128, <= 32 actuators across, <= 52 modes, reconstructor
 * factors uploaded), 0 = the batched kernels (3-5 launches per step, roughly half the speed at small geometries).  A caller
 * outside the envelope is told instead of finding out from a profile. */
int aoenv_fused_step_active(AoEnv* env);

/* Per-kernel timing (bench.py roofline leg).  While enabled, every kernel launch of aoenv_step /
 * aoenv_measure is bracketed by a hipEvent pair recorded on the launch stream; aoenv_profile_read
 * synchronises the stream and returns the summed elapsed milliseconds and the launch count of each
 * AoKernel.  aoenv_profile(env, 0|1) also clears the recorded events.
 * AOENV_K_ENV_STEP counts the steps covered, not the launches: a launch of two steps (AOENV_OPT_STEP_PAIRS) counts two, its
 * elapsed time once.  aoenv_step_counters: h_out[0] = launches of the fused step kernel, h_out[1] = steps they covered, since the
 * last aoenv_profile(env, 1) (or the shard's creation); counted whether or not the timing is enabled. */
enum AoKernel {
    AOENV_K_SHIFT_GATHER = 0, AOENV_K_MT_NORMAL, AOENV_K_GEMM_RING, AOENV_K_SCATTER, AOENV_K_PHASE,
    AOENV_K_SH_SPOTS, AOENV_K_SH_CENTROID, AOENV_K_GEMM_RECON, AOENV_K_RECON_FINISH, AOENV_K_PYRAMID, AOENV_K_SH_TAIL, AOENV_K_ENV_STEP,
    AOENV_K_DETECTOR, AOENV_K_COUNT
};
int aoenv_profile(AoEnv* env, int enable);
int aoenv_profile_read(AoEnv* env, double* h_ms, int32_t* h_count, void* stream);
int aoenv_step_counters(AoEnv* env, int64_t* h_out);

/* Test hook: draw `n` (even) values of RandomState(seed).normal(size=n) with the device MT19937 +
 * legacy polar generator into h_out (float64), to pin the stream against NumPy. */
int aoenv_test_normal(int device, uint32_t seed, int n, int n_calls, double* h_out);

/* Test hooks of the camera's photon-noise sampler (rlao_amd/csrc/poisson_alias.hpp; replaces the NumPy draw of
 * OOPAO/Detector.py:204-206, whose law -- not whose stream -- is what can be matched: the reference seeds it from the wall clock).
 * aoenv_test_poisson_table: the alias tables as the kernels read them (host only, no GPU needed): h_words = size in 32-bit
 *   words; h_out (cap_words >= that) receives header {fine rows, coarse rows, words, 0}, row descriptors {first entry, kmin << 16 |
 *   cells} and entries {23-bit threshold << 9 | alias}.  A CPU test rebuilds every row's outcome probabilities from them.
 * aoenv_test_poisson: h_out[i] = one draw of Poisson(h_lambda[i]) by the cameras' code path, stream (seed, frame); lmax > 0 lowers
 *   the photon count from which PTRS takes over (a multiple of 32, at least 32), 0 = the table's own end (1024). */
int aoenv_test_poisson_table(uint32_t* h_out, size_t cap_words, size_t* h_words);
int aoenv_test_poisson(int device, const float* h_lambda, int n, uint64_t seed, uint32_t frame, float lmax, float* h_out);

/* Test hook of the fused step kernel's LDS layouts (rlao_amd/csrc/step_kernel.hip; host only, no GPU needed), for a geometry of
 * n_act actuators across, n_subap lenslets across, n_valid valid lenslets and n_modes modes:
 *   h_out[0] = words (4 bytes) of a launch of one step, h_out[1] = of a launch of two steps (AOENV_OPT_STEP_PAIRS), which has words
 *   of its own for the first step's slopes, from h_out[2], and modal coefficients, from h_out[3]; h_out[4] = the bytes a workgroup
 *   has for either; h_out[5] = 1 if a photon-noise launch of this geometry may cover two steps, 0 if it runs one launch per step. */
int aoenv_test_step_lds(int n_act, int n_subap, int n_valid, int n_modes, int32_t* h_out);

#ifdef __cplusplus
}
#endif
#endif
