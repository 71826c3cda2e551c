"""ctypes binding of libaoenv.so (include/aoenv.h).  There is no CPU fallback: if the HIP library is
missing or does not load, importing the binding raises."""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("AOENV_LIB") or os.path.join(_HERE, "csrc", "libaoenv.so")   # AOENV_LIB: A/B kernel builds

ABI_VERSION = 7
F32, F64 = 0, 1
WFS_SH, WFS_PYRAMID, WFS_SH_GEOMETRIC = 0, 1, 2

# enum AoConst
(C_PUPIL, C_AB, C_INNER_IDX, C_OUTER_IDX, C_LAYER_WEIGHT, C_DM_GX, C_DM_GY, C_DM_MODES, C_ACT_IDX, C_WFS_AMP,
 C_SH_SUBAP_IDX, C_SH_REF, C_WFS_UNITS, C_RECON, C_PYR_MASK, C_PYR_TT, C_RECON_FACTORS) = range(17)
# enum AoBuf
(B_SCREEN, B_OPD_ATM, B_COEFS, B_PHASE, B_FRAME, B_SIGNAL, B_TOTAL, B_RESIDUAL, B_WFS_MAX, B_XI, B_MT_STATE,
 B_COUNTERS, B_DM_PREV, B_COEFS_SEEN) = range(14)


(OPT_FAST_WFS, OPT_MFMA_GEMM, OPT_FAST_TRIG, OPT_STORE_ATM_OPD, OPT_FUSED_TAIL, OPT_FUSED_STEP, OPT_DEFER_RING, OPT_COEFS_IMAGE,
 OPT_FACTORED_RECON, OPT_RING_LOOKAHEAD, OPT_ENV_WIND_PIXELS, OPT_STEP_PAIRS) = range(12)
OPT_FORCE_PATH = 99
MAX_DELAY = 8                                                      # AOENV_MAX_DELAY
# enum AoPath: bits of OPT_FORCE_PATH
PATH_PHASE_DWORD, PATH_GENERIC, PATH_PYR_ROUND_ROBIN, PATH_MODAL_GEMM, PATH_SH_PLAIN, PATH_WF_GENERAL = 256, 512, 1024, 2048, 4096, 8192
PATH_SCI_GENERAL = 16384
PATH_DM_PAIRS_GENERAL = 32768
PATH_DM_STATIC_GENERAL = 65536
SCI_LOG10 = 1                                                      # enum AoScienceFlag
WF_RESIDUAL, WF_ATMOSPHERE, WF_SCIENCE = 1, 2, 4                   # enum AoWavefront
MAX_WF_MODES = 1024                                                # AOENV_MAX_WF_MODES
KERNEL_NAMES = ("ring_prepare", "mt_normal", "gemm_ring", "ring_scatter", "phase", "sh_spots", "sh_centroid",
                "gemm_recon", "recon_finish", "pyramid", "sh_tail", "env_step", "detector")


class AoCfg(C.Structure):
    _fields_ = [(n, C.c_int32) for n in (
        "abi_version", "dtype", "n_env", "resolution", "n_layer", "layer_res", "n_inner", "n_outer", "n_act",
        "n_valid_act", "dm_separable", "wfs_type", "n_subap", "n_valid_subap", "n_signal", "cam_res", "n_loop",
        "max_group", "pyr_n_res", "pyr_n_theta", "pyr_centering", "pyr_norm_valid", "pyr_q_lo", "pyr_q_hi")] + [
            ("layer_res_l", C.c_int32 * 8)] + [(n, C.c_double) for n in (
            "atm_wavelength", "src_wavelength", "leak", "threshold_cog")]


class AoDetector(C.Structure):
    _fields_ = [("photon_noise", C.c_int32), ("bits", C.c_int32), ("emccd", C.c_int32), ("env_index_offset", C.c_int32),
                ("qe", C.c_double), ("dark_electrons", C.c_double), ("fwc", C.c_double), ("gain", C.c_double),
                ("readout_noise", C.c_double), ("seed", C.c_uint64)]


class AoRollout(C.Structure):
    _fields_ = [("i0", C.c_int32), ("n_steps", C.c_int32), ("env_index_offset", C.c_int32), ("reserved", C.c_int32),
                ("gain", C.c_double), ("sigma", C.c_double), ("d_sigma_env", C.c_void_p), ("seed", C.c_uint64)]


class AoPolicy(C.Structure):
    _fields_ = [("n_history", C.c_int32), ("n_filt", C.c_int32), ("proj_rank", C.c_int32), ("path", C.c_int32),
                ("negative_slope", C.c_double), ("clamp_abs", C.c_double)] + [
                    (n, C.c_void_p) for n in ("h_w1", "h_b1", "h_w2", "h_b2", "h_w3", "h_b3", "h_proj")]


class AoDisturbance(C.Structure):
    _fields_ = [("n_modes", C.c_int32), ("n_lines", C.c_int32), ("t0", C.c_int64)] + [
        (n, C.c_void_p) for n in ("h_modes", "h_amp", "h_freq", "h_phase")]


class AoModal(C.Structure):
    _fields_ = [("n_modes", C.c_int32), ("h_m2c", C.c_void_p), ("h_cm", C.c_void_p)]


class AoWavefrontBasis(C.Structure):
    _fields_ = [("n_modes", C.c_int32), ("n_pix", C.c_int32), ("h_opd2m", C.c_void_p)]


class AoScience(C.Structure):
    _fields_ = [("zero_padding", C.c_int32), ("window", C.c_int32), ("first_frame", C.c_int32), ("flags", C.c_int32),
                ("h_dft", C.c_void_p)]


EXPORTS = {
    # name: (restype, argtypes)
    "aoenv_last_error": (C.c_char_p, []),
    "aoenv_abi_version": (C.c_int, []),
    "aoenv_create": (C.c_int, [C.POINTER(AoCfg), C.c_int, C.POINTER(C.c_void_p)]),
    "aoenv_destroy": (C.c_int, [C.c_void_p]),
    "aoenv_upload": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t]),
    "aoenv_upload_layer": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_size_t]),
    "aoenv_set_wind": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int]),
    "aoenv_new_screens": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "aoenv_new_screens_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, C.c_double, C.c_double,
                                           C.c_void_p]),
    "aoenv_reset_envs": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_double, C.c_double, C.c_double,
                                   C.c_void_p]),
    "aoenv_set_atm_opd": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "aoenv_set_coefs": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "aoenv_measure": (C.c_int, [C.c_void_p, C.c_void_p]),
    "aoenv_fused_step_active": (C.c_int, [C.c_void_p]),
    "aoenv_atm_update": (C.c_int, [C.c_void_p, C.c_void_p]),
    "aoenv_reset_soft": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "aoenv_step": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                             C.c_void_p]),
    "aoenv_run_integrator": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_double, C.c_void_p, C.c_void_p,
                                       C.c_void_p, C.c_void_p, C.c_void_p]),
    "aoenv_set_noise_filter": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "aoenv_set_disturbance": (C.c_int, [C.c_void_p, C.POINTER(AoDisturbance), C.c_void_p]),
    "aoenv_set_modal": (C.c_int, [C.c_void_p, C.POINTER(AoModal), C.c_void_p]),
    "aoenv_set_modal_gain": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "aoenv_reset_soft_modal": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "aoenv_step_modal": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                   C.c_void_p]),
    "aoenv_run_integrator_modal": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                             C.c_void_p]),
    "aoenv_set_wavefront_basis": (C.c_int, [C.c_void_p, C.POINTER(AoWavefrontBasis), C.c_void_p]),
    "aoenv_project_wavefront": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "aoenv_set_wavefront_record": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int]),
    "aoenv_set_dm_env": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "aoenv_get_dm_env": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "aoenv_set_dm_pairs": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "aoenv_get_dm_pairs": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "aoenv_get_dm_surface": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "aoenv_set_flux_env": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "aoenv_get_flux_env": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "aoenv_set_threshold_env": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "aoenv_get_threshold_env": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "aoenv_set_delay": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p]),
    "aoenv_get_delay": (C.c_int, [C.c_void_p, C.POINTER(C.c_int)]),
    "aoenv_get_delay_line": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "aoenv_set_delay_line": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "aoenv_run_rollout": (C.c_int, [C.c_void_p, C.POINTER(AoRollout), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                    C.c_void_p]),
    "aoenv_set_policy": (C.c_int, [C.c_void_p, C.POINTER(AoPolicy), C.c_void_p]),
    "aoenv_policy_forward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "aoenv_run_policy_rollout": (C.c_int, [C.c_void_p, C.POINTER(AoRollout), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                           C.c_void_p, C.c_void_p, C.c_void_p]),
    "aoenv_compute_psf": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "aoenv_set_science": (C.c_int, [C.c_void_p, C.POINTER(AoScience), C.c_void_p]),
    "aoenv_science_psf": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "aoenv_set_science_accumulator": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "aoenv_set_field": (C.c_int, [C.c_void_p, C.c_double, C.c_double, C.c_void_p]),
    "aoenv_set_science_direction": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "aoenv_get_science_direction": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "aoenv_science_residual": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "aoenv_set_science_direction_record": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int]),
    "aoenv_set_guide_direction": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "aoenv_get_guide_direction": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "aoenv_set_static_opd": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "aoenv_get_static_opd": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "aoenv_static_surface_path": (C.c_int, [C.c_void_p, C.c_void_p]),
    "aoenv_set_lgs_spots": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p, C.c_void_p]),
    "aoenv_get_lgs_spots": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "aoenv_set_detector": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "aoenv_set_return_accumulator": (C.c_int, [C.c_void_p, C.c_void_p]),
    "aoenv_buffer": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]),
    "aoenv_download": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p]),
    "aoenv_upload_state": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p]),
    "aoenv_get_phase_no_pupil": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "aoenv_set_wind_env": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "aoenv_get_clock_env": (C.c_int, [C.c_void_p, C.c_void_p]),
    "aoenv_set_clock_env": (C.c_int, [C.c_void_p, C.c_void_p]),
    "aoenv_set_r0_env": (C.c_int, [C.c_void_p, C.c_void_p, C.c_double, C.c_void_p]),
    "aoenv_get_r0_env": (C.c_int, [C.c_void_p, C.c_void_p]),
    "aoenv_get_buff": (C.c_int, [C.c_void_p, C.c_void_p]),
    "aoenv_set_buff": (C.c_int, [C.c_void_p, C.c_void_p]),
    "aoenv_set_option": (C.c_int, [C.c_void_p, C.c_int, C.c_int]),
    "aoenv_profile": (C.c_int, [C.c_void_p, C.c_int]),
    "aoenv_profile_read": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "aoenv_step_counters": (C.c_int, [C.c_void_p, C.c_void_p]),
    "aoenv_test_normal": (C.c_int, [C.c_int, C.c_uint32, C.c_int, C.c_int, C.c_void_p]),
    "aoenv_test_poisson_table": (C.c_int, [C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]),
    "aoenv_test_poisson": (C.c_int, [C.c_int, C.c_void_p, C.c_int, C.c_uint64, C.c_uint32, C.c_float, C.c_void_p]),
    "aoenv_test_step_lds": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]),
}


_LATER_ENTRIES = ("aoenv_step_counters", "aoenv_set_field", "aoenv_set_science_direction", "aoenv_get_science_direction",
                  "aoenv_science_residual", "aoenv_set_science_direction_record", "aoenv_test_step_lds", "aoenv_get_phase_no_pupil",
                  "aoenv_set_guide_direction", "aoenv_get_guide_direction", "aoenv_set_static_opd", "aoenv_get_static_opd",
                  "aoenv_static_surface_path", "aoenv_set_lgs_spots", "aoenv_get_lgs_spots")


class AoEnvError(RuntimeError):
    pass


_lib = None


def load():
    """Load libaoenv.so and declare every entry point of include/aoenv.h.  Raises if it is missing."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise AoEnvError(f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                         "(there is no CPU fallback)")
    # One HIP runtime per process: PyTorch-ROCm bundles its own libamdhip64.so.7 / libhsa-runtime64.so.1.
    # Importing torch first makes the dynamic loader resolve libaoenv's dependency (same SONAMEs) to the
    # copies torch already mapped, so torch streams / device pointers and libaoenv kernels share one runtime.
    import torch  # noqa: F401
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in EXPORTS.items():
        if name in _LATER_ENTRIES and os.environ.get("AOENV_LIB") and not hasattr(lib, name):
            continue                       # an A/B run of a library built before these entries (AOENV_LIB): same ABI without them
        fn = getattr(lib, name)            # AttributeError if the symbol is not exported
        fn.restype = res
        fn.argtypes = args
    if lib.aoenv_abi_version() != ABI_VERSION:
        raise AoEnvError(f"libaoenv ABI {lib.aoenv_abi_version()} != binding ABI {ABI_VERSION}")
    _lib = lib
    return lib


def check(rc: int, lib=None):
    if rc != 0:
        raise AoEnvError((lib or load()).aoenv_last_error().decode("utf-8", "replace"))


def _pointer(a):
    """One argument of an entry point in the form the library object is handed: a struct by reference, host and device memory
    as ``c_void_p`` (an empty tensor has no address: None), everything else -- None, numbers, ready-made ctypes objects -- as it
    is.  Only an object becomes a pointer here; the dtype an entry reads is the caller's business.  An array is never copied (it
    may be an output), so one that is not C-contiguous is refused."""
    if a is None or isinstance(a, (int, float)):
        return a
    if isinstance(a, np.ndarray):
        if not a.flags.c_contiguous:
            raise ValueError("an array handed to libaoenv must be C-contiguous (it is passed by address, never copied)")
        return a.ctypes.data_as(C.c_void_p)
    if isinstance(a, C.Structure):
        return C.byref(a)
    if hasattr(a, "data_ptr"):                                     # a torch tensor, host or device
        return C.c_void_p(a.data_ptr()) if a.numel() else None
    return a


def address(a):
    """The same memory as the integer a struct's pointer field takes (None: a null pointer)."""
    p = _pointer(a)
    return None if p is None else p.value


def invoke(owner, name: str, *args):
    """``owner.lib.<name>(owner.h, *args)`` with every argument through ``_pointer``; the entry's own return value.  ``owner``: a
    ``Shard``, or anything else with ``.lib`` and ``.h``."""
    return getattr(owner.lib, name)(owner.h, *[_pointer(a) for a in args])


def call(owner, name: str, *args):
    """The one way into the library for an entry point that returns a status: ``invoke``, and ``AoEnvError`` with the library's
    message unless it is 0."""
    check(invoke(owner, name, *args), owner.lib)
