"""ctypes binding of libpnpadmm.so (include/pnpadmm.h).  No fallback: if the HIP library is
missing or a call fails, this raises - the product path never routes through CPU code."""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("PNP_LIB_PATH") or os.path.join(_HERE, "csrc", "libpnpadmm.so")   # override: kernel experiments

PNP_FLAG_PROFILE = 1
PNP_FLAG_NO_DENOISER = 2
PNP_FLAG_KEEP_STAGES = 4
PNP_FLAG_BF16_CONVS = 8
PNP_FLAG_PROFILE_LAYERS = 16
PNP_SSIM_CLAMP_X = 1
PNP_RES_COLS = 6
PNP_RES_DELTA = 1
PNP_RES_DC = 2
RESIDUAL_COLUMNS = ("primal", "dx", "dz", "du", "delta", "dc")      # columns of pnp_residuals' [N, 6] output
PNP_MC_MAX_COILS = 32
PNP_MC_MAX_CG = 64
PNP_CC_MAX_COILS = 64
PNP_PW_MAX_COILS = 64
PNP_ESPIRIT_MAX_COILS = 16
PNP_ESPIRIT_MAX_KSIZE = 8
PNP_ESPIRIT_MAX_N = 512
PNP_GRAPPA_MAX_COILS = 32
PNP_GRAPPA_MAX_ACCEL = 8
PNP_GRAPPA_MAX_SRC = 512
PNP_TV_MAX_ITERS = 64
PNP_PRIOR_UNET = 0
PNP_PRIOR_TV = 1
PRIORS = {"unet": PNP_PRIOR_UNET, "tv": PNP_PRIOR_TV}      # prior names of pnp_set_prior
PNP_PRIOR_HAAR = 2                                         # set by pnp_set_prior_haar, never by pnp_set_prior
PRIOR_NAMES = {PNP_PRIOR_UNET: "unet", PNP_PRIOR_TV: "tv", PNP_PRIOR_HAAR: "haar"}      # what pnp_get_prior can report
PNP_HAAR_TI = 0
PNP_HAAR_ORTHO = 1
PNP_HAAR_MAX_LEVELS = 4
HAAR_MODES = {"ti": PNP_HAAR_TI, "ortho": PNP_HAAR_ORTHO}      # mode names of pnp_haar_denoise / pnp_set_prior_haar
PNP_SENS_BOX = 0
PNP_SENS_HANN = 1
SENS_WINDOWS = {"box": PNP_SENS_BOX, "hann": PNP_SENS_HANN}      # window names of pnp_estimate_sens
PROFILE_CLASSES = 6
PROFILE_CLASS_NAMES = ("conv3x3_mfma", "conv_first", "conv_last", "fft_rows", "fft_cols_prox", "other")
N_LAYERS = 28


class pnp_config(C.Structure):
    _fields_ = [("n", C.c_int32), ("h", C.c_int32), ("w", C.c_int32), ("device", C.c_int32), ("flags", C.c_int32)]


_vp, _fp, _u8p = C.c_void_p, C.c_void_p, C.c_void_p   # device pointers travel as integers

# name -> (restype, argtypes); every symbol include/pnpadmm.h declares
SIGNATURES = {
    "pnp_create": (C.c_int, [C.POINTER(pnp_config), C.POINTER(C.c_void_p)]),
    "pnp_destroy": (C.c_int, [C.c_void_p]),
    "pnp_last_error": (C.c_char_p, []),
    "pnp_version": (C.c_char_p, []),
    "pnp_load_unet_weights": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t]),
    "pnp_reset": (C.c_int, [C.c_void_p, _fp, _fp, _u8p, C.c_int, _fp, _fp, _fp, _vp]),
    "pnp_set_kspace": (C.c_int, [C.c_void_p, _fp, _u8p, C.c_int, _vp]),
    "pnp_step": (C.c_int, [C.c_void_p, _fp, _fp, _fp, _fp, _fp, _fp, _fp, _u8p, _vp]),
    "pnp_denoise": (C.c_int, [C.c_void_p, _fp, _fp, _fp, _vp]),
    "pnp_tv_denoise": (C.c_int, [C.c_void_p, _fp, _fp, C.c_int, _fp, _vp]),
    "pnp_set_prior": (C.c_int, [C.c_void_p, C.c_int, C.c_double, C.c_int]),
    "pnp_get_prior": (C.c_int, [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_double), C.POINTER(C.c_int)]),
    "pnp_haar_denoise": (C.c_int, [C.c_void_p, _fp, _fp, C.c_int, C.c_int, _fp, _vp]),
    "pnp_set_prior_haar": (C.c_int, [C.c_void_p, C.c_double, C.c_int, C.c_int]),
    "pnp_get_prior_haar": (C.c_int, [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "pnp_fft2c": (C.c_int, [C.c_void_p, _fp, _fp, C.c_int, C.c_int, C.c_int, C.c_int, _vp]),
    "pnp_prox_dual": (C.c_int, [C.c_void_p, _fp, _fp, _fp, _fp, _fp, _vp]),
    "pnp_psnr": (C.c_int, [C.c_void_p, _fp, _fp, _fp, _vp]),
    "pnp_ssim": (C.c_int, [C.c_void_p, _fp, _fp, C.c_float, C.c_float, C.c_float, C.c_int, C.c_int, _fp, _fp, _vp]),
    "pnp_residuals": (C.c_int, [C.c_void_p, _fp, _fp, _fp, _vp, C.c_int, _fp, _vp]),
    "pnp_acquire": (C.c_int, [C.c_void_p, _fp, _u8p, C.c_int, C.c_double, C.c_uint64, C.c_int, _fp, _fp, _fp, _vp]),
    "pnp_set_kspace_mc": (C.c_int, [C.c_void_p, _fp, _fp, C.c_int, C.c_int, _u8p, C.c_int, C.c_int, _vp]),
    "pnp_reset_mc": (C.c_int, [C.c_void_p, _fp, _fp, _fp, C.c_int, C.c_int, _u8p, C.c_int, C.c_int, _fp, _fp, _fp, _vp]),
    "pnp_mc_coils": (C.c_int, [C.c_void_p]),
    "pnp_mc_cg_residual": (C.c_int, [C.c_void_p, _fp, _vp]),
    "pnp_mc_normal": (C.c_int, [C.c_void_p, _fp, _fp, _fp, _vp]),
    "pnp_acquire_mc": (C.c_int, [C.c_void_p, _fp, _fp, C.c_int, C.c_int, _u8p, C.c_int, C.c_double, C.c_uint64, C.c_int, _fp, _fp, _fp, _vp]),
    "pnp_nufft_plan": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int]),
    "pnp_nufft_samples": (C.c_int64, [C.c_void_p]),
    "pnp_nufft_grid": (C.c_int, [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "pnp_nufft_forward": (C.c_int, [C.c_void_p, _fp, C.c_int, _fp, _vp]),
    "pnp_nufft_adjoint": (C.c_int, [C.c_void_p, _fp, _fp, C.c_int, _fp, _vp]),
    "pnp_set_kspace_nc": (C.c_int, [C.c_void_p, _fp, _fp, C.c_int, _vp]),
    "pnp_reset_nc": (C.c_int, [C.c_void_p, _fp, _fp, _fp, C.c_int, _fp, _fp, _fp, _vp]),
    "pnp_nc_cg_residual": (C.c_int, [C.c_void_p, _fp, _vp]),
    "pnp_nc_normal": (C.c_int, [C.c_void_p, _fp, _fp, _fp, _vp]),
    "pnp_acquire_nc": (C.c_int, [C.c_void_p, _fp, _fp, C.c_double, C.c_uint64, C.c_int, _fp, _fp, _fp, _vp]),
    "pnp_estimate_sens": (C.c_int, [C.c_void_p, _fp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, C.c_int, _fp, _fp, _vp]),
    "pnp_coil_compress_matrix": (C.c_int, [C.c_void_p, _fp, C.c_int, C.c_int, C.c_int, C.c_int, _fp, _fp, _fp, _vp]),
    "pnp_coil_compress_apply": (C.c_int, [C.c_void_p, _fp, C.c_int, _fp, C.c_int, C.c_int, _fp, _vp]),
    "pnp_noise_cov": (C.c_int, [C.c_void_p, _fp, C.c_int, C.c_int, C.c_int, C.c_int, _fp, _vp]),
    "pnp_whiten_matrix": (C.c_int, [C.c_void_p, _fp, C.c_int, C.c_int, C.c_int, _fp, _fp, _fp, _vp]),
    "pnp_whiten_apply": (C.c_int, [C.c_void_p, _fp, C.c_int, _fp, C.c_int, _fp, _vp]),
    "pnp_espirit_sens": (C.c_int, [C.c_void_p, _fp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, C.c_double, C.c_int, C.c_int, C.c_double,
                                  C.c_int, _fp, _fp, _fp, _vp, _vp]),
    "pnp_grappa_weights": (C.c_int, [C.c_void_p, _fp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, C.c_int, _fp, _vp, _fp,
                                    _vp]),
    "pnp_grappa_apply": (C.c_int, [C.c_void_p, _fp, C.c_int, _u8p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _fp, C.c_int, _fp, _vp]),
    "pnp_snapshot_bytes": (C.c_size_t, [C.c_void_p]),
    "pnp_snapshot": (C.c_int, [C.c_void_p, _fp, _fp, _fp, _fp, _vp, _vp]),
    "pnp_restore": (C.c_int, [C.c_void_p, _vp, _fp, _fp, _fp, _fp, _vp]),
    "pnp_unet_read_stage": (C.c_int, [C.c_void_p, C.c_int, _fp, C.POINTER(C.c_int), C.POINTER(C.c_int),
                                      C.POINTER(C.c_int), _vp]),
    "pnp_profile_reset": (C.c_int, [C.c_void_p]),
    "pnp_profile_collect": (C.c_int, [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_int64)]),
    "pnp_profile_layers": (C.c_int, [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_int64)]),
    "pnp_conv_algorithms": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32)]),
    "pnp_conv_schedules": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32)]),
    "pnp_bf16_weight_terms": (C.c_int, [C.c_void_p]),
    "pnp_workspace_bytes": (C.c_size_t, [C.c_void_p]),
}

# name -> (restype, argtypes); every symbol include/pnpadmm_ncsense.h declares (non-Cartesian SENSE: the extension header of the same library)
SIGNATURES_NCSENSE = {
    "pnp_nufft_forward_mc": (C.c_int, [C.c_void_p, _fp, _fp, C.c_int, C.c_int, C.c_int, _fp, _vp]),
    "pnp_nufft_adjoint_mc": (C.c_int, [C.c_void_p, _fp, _fp, _fp, C.c_int, C.c_int, C.c_int, _fp, _vp]),
    "pnp_set_kspace_ncsense": (C.c_int, [C.c_void_p, _fp, _fp, C.c_int, C.c_int, _fp, C.c_int, _vp]),
    "pnp_reset_ncsense": (C.c_int, [C.c_void_p, _fp, _fp, _fp, C.c_int, C.c_int, _fp, C.c_int, _fp, _fp, _fp, _vp]),
    "pnp_ncsense_coils": (C.c_int, [C.c_void_p]),
    "pnp_ncsense_cg_residual": (C.c_int, [C.c_void_p, _fp, _vp]),
    "pnp_ncsense_normal": (C.c_int, [C.c_void_p, _fp, _fp, _fp, _vp]),
    "pnp_acquire_ncsense": (C.c_int, [C.c_void_p, _fp, _fp, C.c_int, C.c_int, _fp, C.c_double, C.c_uint64, C.c_int, _fp, _fp, _fp, _vp]),
}

# name -> (restype, argtypes); every symbol include/pnpadmm_toeplitz.h declares (the Toeplitz normal operator of the non-Cartesian CG stages)
SIGNATURES_TOEPLITZ = {
    "pnp_toeplitz_plan": (C.c_int, [C.c_void_p, _fp, C.c_int, _vp]),
    "pnp_toeplitz_planned": (C.c_int, [C.c_void_p]),
    "pnp_toeplitz_live": (C.c_int, [C.c_void_p]),
    "pnp_toeplitz_spectrum": (C.c_int, [C.c_void_p, _fp, _vp]),
    "pnp_toeplitz_apply": (C.c_int, [C.c_void_p, _fp, C.c_int, _fp, _vp]),
    "pnp_toeplitz_apply_mc": (C.c_int, [C.c_void_p, _fp, _fp, C.c_int, C.c_int, C.c_int, _fp, _vp]),
    "pnp_set_kspace_nc_tz": (C.c_int, [C.c_void_p, _fp, C.c_int, _vp]),
    "pnp_reset_nc_tz": (C.c_int, [C.c_void_p, _fp, _fp, C.c_int, _fp, _fp, _fp, _vp]),
    "pnp_set_kspace_ncsense_tz": (C.c_int, [C.c_void_p, _fp, _fp, C.c_int, C.c_int, C.c_int, _vp]),
    "pnp_reset_ncsense_tz": (C.c_int, [C.c_void_p, _fp, _fp, _fp, C.c_int, C.c_int, C.c_int, _fp, _fp, _fp, _vp]),
}
PNP_TOEPLITZ_MAX_SIDE = 512

# name -> (restype, argtypes); every symbol include/pnpadmm_dcf.h declares (density weights for any trajectory: Pipe and Menon's iteration)
SIGNATURES_DCF = {
    "pnp_nufft_psi": (C.c_int, [C.c_void_p, _fp, _fp, _vp]),
    "pnp_nufft_dcf": (C.c_int, [C.c_void_p, _fp, C.c_int, C.c_int, _fp, _fp, _vp]),
}
PNP_DCF_MAX_ITERS = 256

# name -> (restype, argtypes); every symbol include/pnpadmm_offres.h declares (off-resonance correction by time segmentation)
SIGNATURES_OFFRES = {
    "pnp_offres_plan": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int]),
    "pnp_offres_segments": (C.c_int, [C.c_void_p]),
    "pnp_offres_maps": (C.c_int, [C.c_void_p, _fp, C.c_int, _fp, _vp]),
    "pnp_offres_forward": (C.c_int, [C.c_void_p, _fp, _fp, C.c_int, C.c_int, _fp, _vp]),
    "pnp_offres_adjoint": (C.c_int, [C.c_void_p, _fp, _fp, _fp, C.c_int, C.c_int, _fp, _vp]),
    "pnp_set_kspace_offres": (C.c_int, [C.c_void_p, _fp, _fp, C.c_int, _fp, C.c_int, _vp]),
    "pnp_reset_offres": (C.c_int, [C.c_void_p, _fp, _fp, _fp, C.c_int, _fp, C.c_int, _fp, _fp, _fp, _vp]),
    "pnp_offres_live": (C.c_int, [C.c_void_p]),
    "pnp_offres_cg_residual": (C.c_int, [C.c_void_p, _fp, _vp]),
    "pnp_offres_normal": (C.c_int, [C.c_void_p, _fp, _fp, _fp, _vp]),
    "pnp_acquire_offres": (C.c_int, [C.c_void_p, _fp, _fp, C.c_int, _fp, C.c_double, C.c_uint64, C.c_int, _fp, _fp, _fp, _vp]),
}

# name -> (restype, argtypes); every symbol include/pnpadmm_offres_ls.h declares (the least-squares temporal interpolator)
SIGNATURES_OFFRES_LS = {
    "pnp_offres_plan_ls": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_double, C.c_int]),
    "pnp_offres_interpolator": (C.c_int, [C.c_void_p]),
    "pnp_offres_ls_coeffs": (C.c_int, [C.c_void_p, C.c_void_p]),
}
OFFRES_INTERPOLATORS = {"linear": 1, "ls": 2}

# name -> (restype, argtypes); every symbol include/pnpadmm_offres_mc.h declares (off-resonance correction for multi-coil data)
SIGNATURES_OFFRES_MC = {
    "pnp_offres_forward_mc": (C.c_int, [C.c_void_p, _fp, _fp, C.c_int, _fp, C.c_int, C.c_int, C.c_int, _fp, _vp]),
    "pnp_offres_adjoint_mc": (C.c_int, [C.c_void_p, _fp, _fp, _fp, C.c_int, _fp, C.c_int, C.c_int, C.c_int, _fp, _vp]),
    "pnp_set_kspace_offres_mc": (C.c_int, [C.c_void_p, _fp, _fp, C.c_int, C.c_int, _fp, C.c_int, _fp, C.c_int, _vp]),
    "pnp_reset_offres_mc": (C.c_int, [C.c_void_p, _fp, _fp, _fp, C.c_int, C.c_int, _fp, C.c_int, _fp, C.c_int, _fp, _fp, _fp, _vp]),
    "pnp_offres_mc_coils": (C.c_int, [C.c_void_p]),
    "pnp_offres_mc_cg_residual": (C.c_int, [C.c_void_p, _fp, _vp]),
    "pnp_offres_mc_normal": (C.c_int, [C.c_void_p, _fp, _fp, _fp, _vp]),
    "pnp_acquire_offres_mc": (C.c_int, [C.c_void_p, _fp, _fp, C.c_int, C.c_int, _fp, C.c_int, _fp, C.c_double, C.c_uint64, C.c_int, _fp, _fp, _fp,
                                       _vp]),
}
PNP_OFFRES_MC_COIL_BLOCK = 4     # default coils per block under a least-squares plan, and 2 under a linear one (the environment variable of the
PNP_OFFRES_MC_COIL_BLOCK_LINEAR = 2   # first name, read at pnp_create, overrides both)

# name -> (restype, argtypes); every symbol include/pnpadmm_offres_tz.h declares (the Toeplitz form of the off-resonance normal operator)
SIGNATURES_OFFRES_TZ = {
    "pnp_offres_tz_plan": (C.c_int, [C.c_void_p, _fp, C.c_int, _vp]),
    "pnp_offres_tz_planned": (C.c_int, [C.c_void_p]),
    "pnp_offres_tz_live": (C.c_int, [C.c_void_p]),
    "pnp_offres_tz_spectra": (C.c_int, [C.c_void_p]),
    "pnp_offres_tz_spectrum": (C.c_int, [C.c_void_p, _fp, _vp]),
    "pnp_offres_tz_apply": (C.c_int, [C.c_void_p, _fp, _fp, C.c_int, C.c_int, _fp, _vp]),
    "pnp_offres_tz_apply_mc": (C.c_int, [C.c_void_p, _fp, _fp, C.c_int, _fp, C.c_int, C.c_int, C.c_int, _fp, _vp]),
    "pnp_set_kspace_offres_tz": (C.c_int, [C.c_void_p, _fp, _fp, C.c_int, C.c_int, _vp]),
    "pnp_reset_offres_tz": (C.c_int, [C.c_void_p, _fp, _fp, _fp, C.c_int, C.c_int, _fp, _fp, _fp, _vp]),
    "pnp_set_kspace_offres_mc_tz": (C.c_int, [C.c_void_p, _fp, _fp, C.c_int, C.c_int, _fp, C.c_int, C.c_int, _vp]),
    "pnp_reset_offres_mc_tz": (C.c_int, [C.c_void_p, _fp, _fp, _fp, C.c_int, C.c_int, _fp, C.c_int, C.c_int, _fp, _fp, _fp, _vp]),
}
PNP_OFFRES_TZ_MAX_PAIRS = 136    # spectra of one plan: 16 segments under a least-squares plan, 32 under a linear one
PNP_OFFRES_TZ_PLANES = 512       # planes (slices x segments) in flight in the pass buffers

# name -> (restype, argtypes); every symbol include/pnpadmm_fieldmap.h declares (the B0 field map from two echo images)
SIGNATURES_FIELDMAP = {
    "pnp_fieldmap_estimate": (C.c_int, [C.c_void_p, _fp, _fp, C.c_int, C.c_double, C.c_float, C.c_int, C.c_int, _fp, _fp, _vp]),
    "pnp_fieldmap_cost": (C.c_int, [C.c_void_p, _fp, _fp, C.c_int, C.c_double, C.c_float, _fp, _fp, _vp]),
}
PNP_FIELDMAP_MAX_ITERS = 4096
PNP_FIELDMAP_T = 10          # sweeps per launch of the fused kernel


def toeplitz_size_error(fn: str, h: int, w: int):
    """The library's refusal of a slice too large for the Toeplitz operator, word for word (pnp_capi.hip: tz_check_sizes), or None: for a
    caller that knows the size before it has a handle."""
    if h <= PNP_TOEPLITZ_MAX_SIDE and w <= PNP_TOEPLITZ_MAX_SIDE:
        return None
    return f"{fn}: the Toeplitz operator transforms a 2h x 2w grid, so it takes h, w up to {PNP_TOEPLITZ_MAX_SIDE} (got {int(h)}x{int(w)})"

def offres_tz_pairs(interpolator: str, segments: int) -> int:
    """P, the spectra the Toeplitz form of the off-resonance operator stores for a plan: the band under the linear interpolator, the upper
    triangle under least squares."""
    L = int(segments)
    return 2 * L - 1 if interpolator == "linear" else L * (L + 1) // 2


def offres_tz_pairs_error(fn: str, interpolator: str, segments: int):
    """The library's refusal of a plan with too many spectra, word for word (offres_tz_plan.hip: plan_offres_tz), or None: for a caller that
    knows the plan before it has a handle."""
    pairs = offres_tz_pairs(interpolator, segments)
    if pairs <= PNP_OFFRES_TZ_MAX_PAIRS:
        return None
    kind = "linear" if interpolator == "linear" else "least-squares"
    return (f"{fn}: {int(segments)} segments under a {kind} plan need {pairs} spectra, more than the limit of {PNP_OFFRES_TZ_MAX_PAIRS} "
            f"(16 segments least squares, 32 linear)")


_lib = None


class PnPError(RuntimeError):
    pass


def load() -> C.CDLL:
    """Load the shared library (once).  Raises PnPError with build instructions if absent."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise PnPError(f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                       f"or `make -C {os.path.dirname(LIB_PATH)}`; there is no CPU fallback")
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in {**SIGNATURES, **SIGNATURES_NCSENSE, **SIGNATURES_TOEPLITZ, **SIGNATURES_DCF, **SIGNATURES_OFFRES,
                              **SIGNATURES_OFFRES_LS, **SIGNATURES_OFFRES_MC, **SIGNATURES_FIELDMAP, **SIGNATURES_OFFRES_TZ}.items():
        fn = getattr(lib, name)          # AttributeError here = header/library mismatch
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def check(rc: int, what: str) -> None:
    if rc != 0:
        msg = load().pnp_last_error()
        raise PnPError(f"{what} failed ({rc}): {msg.decode() if msg else '?'}")
