"""ctypes binding of ``csrc/librawformer_hip.so`` (the C ABI in ``include/rawformer_hip.h``).

There is no fallback: if the library is missing or a call fails, a ``RuntimeError`` is raised
(the reference's own error convention is Python exceptions).
"""
from __future__ import annotations

import ctypes as C
import os

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("RF_LIB_PATH") or os.path.join(_HERE, "csrc", "librawformer_hip.so")  # override: diagnostic builds

RF_VARIANT_FLCA = 0
RF_VARIANT_PLAIN = 1
RF_VARIANT_TRUECOLOR = 2
RF_VARIANT_MULTILVL = 3
RF_VARIANT_WFB = 4
RF_PARAM_BUFFER = 1
RF_PARAM_UNUSED = 2


class RfConfig(C.Structure):
    _fields_ = [("dim", C.c_int32), ("heads", C.c_int32 * 4), ("inp_channels", C.c_int32),
                ("out_channels", C.c_int32), ("ffn_expansion", C.c_int32), ("variant", C.c_int32),
                ("branch_lrelu", C.c_int32), ("clamp_io", C.c_int32), ("flca_levels", C.c_int32)]


_vp, _i, _f, _sz = C.c_void_p, C.c_int, C.c_float, C.c_size_t
# rf_allreduce_fn (include/rawformer_hip.h): void (*)(void* user, float* buf, size_t n, int op, void* stream); buf arrives as an integer address
ALLREDUCE_FN = C.CFUNCTYPE(None, C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p)
_psz = C.POINTER(C.c_size_t)
# rf_grad_ready_fn: void (*)(void* user, size_t offset, size_t count, void* stream)
GRAD_READY_FN = C.CFUNCTYPE(None, C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p)

# name -> (restype, argtypes); mirrors include/rawformer_hip.h one to one
SIGNATURES = {
    "rf_last_error": (C.c_char_p, []),
    "rf_version": (_i, []),
    "rf_profile_begin": (_i, []),
    "rf_profile_end": (_i, [C.c_char_p, _sz]),
    "rf_create": (_i, [C.POINTER(RfConfig), C.POINTER(_vp)]),
    "rf_destroy": (None, [_vp]),
    "rf_param_count": (_i, [_vp]),
    "rf_param_info": (_i, [_vp, _i, C.POINTER(C.c_char_p), C.POINTER(C.c_int64 * 4), C.POINTER(_i)]),
    "rf_param_flags": (_i, [_vp, _i, C.POINTER(_i)]),
    "rf_set_param": (_i, [_vp, C.c_char_p, _vp, C.POINTER(C.c_int64), _i]),
    "rf_packed_bytes": (_i, [_vp, _psz]),
    "rf_pack_params": (_i, [_vp, _vp, _sz, _vp]),
    "rf_workspace_bytes": (_i, [_vp, _i, _i, _i, _psz]),
    "rf_forward": (_i, [_vp, _vp, _vp, _vp, _sz, _i, _i, _i, _i, _vp]),
    "rf_forward_stage": (_i, [_vp, _i, _vp, _vp, _vp, _vp, _sz, _i, _i, _i, _vp]),
    "rf_tc_guidance": (_i, [_vp, _vp, _i, _vp, _vp, _vp, _vp, _vp, _sz, _i, _i, _i, _vp]),
    "rf_ml_guidance": (_i, [_vp, _vp, _i, _vp, _vp, _vp, _sz, _i, _i, _i, _vp]),
    "rf_ml_tail": (_i, [_vp, _vp, _vp, _i, _vp, _sz, _i, _i, _i, _vp]),
    "rf_set_shard": (_i, [_vp, _i, _i, _i, ALLREDUCE_FN, _vp]),
    "rf_set_shard_grid": (_i, [_vp, _i, _i, _i, _i, _i, _i, ALLREDUCE_FN, _vp]),
    "rf_flat_param_floats": (_i, [_vp, _psz]),
    "rf_flat_offset": (_i, [_vp, _i, _psz]),
    "rf_train_workspace_bytes": (_i, [_vp, _i, _i, _i, _psz]),
    "rf_set_grad_ready": (_i, [_vp, GRAD_READY_FN, _vp]),
    "rf_set_loss_clamp": (_i, [_vp, _i]),
    "rf_grad_range_count": (_i, [_vp, C.POINTER(_i)]),
    "rf_grad_range": (_i, [_vp, _i, _psz, _psz]),
    "rf_train_step": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _i, _i, _i, _i, _f, _vp]),
    "rf_adam_step": (_i, [_vp, _vp, _vp, _vp, _sz, _f, _f, _f, _f, _f, _i, _i, _f, _vp]),
    "rf_optim_state_bytes": (_i, [_i, _sz, _psz]),
    "rf_optim_init": (_i, [_psz, _psz, _i, _sz, _vp, _sz, _vp]),
    "rf_grad_stats": (_i, [_vp, _sz, _i, _vp, _sz, _vp]),
    "rf_adam_step_guarded": (_i, [_vp, _vp, _vp, _vp, _sz, _f, _f, _f, _f, _f, _i, _f, _f, _i, _i, _vp, _sz, _vp]),
    "rf_optim_set_steps": (_i, [_vp, _sz, C.c_longlong, _vp]),
    "rf_pixel_unshuffle2": (_i, [_vp, _vp, _i, _i, _i, _i, _vp]),
    "rf_pixel_shuffle2": (_i, [_vp, _vp, _i, _i, _i, _i, _vp]),
    "rf_dwt_haar": (_i, [_vp, _vp, _i, _i, _i, _i, _vp]),
    "rf_idwt_haar": (_i, [_vp, _vp, _i, _i, _i, _i, _vp]),
    "rf_dwt_custom": (_i, [_vp, _vp, C.POINTER(C.c_float), _i, _i, _i, _i, _i, _vp]),
    "rf_idwt_custom": (_i, [_vp, _vp, C.POINTER(C.c_float), _i, _i, _i, _i, _i, _vp]),
    "rf_haar_dwt": (_i, [_vp, _vp, _i, _i, _i, _i, _vp]),
    "rf_layernorm2d": (_i, [_vp, _vp, _vp, _vp, _f, _i, _i, _i, _i, _vp]),
    "rf_conv1x1_scratch_bytes": (_i, [_i, _i, _psz]),
    "rf_conv1x1": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _vp]),
    "rf_conv1x1_group_grid": (_i, [_i, _i, C.POINTER(_i)]),
    "rf_conv1x1_group_map": (_i, [_i, _i, _i, C.POINTER(_i), C.POINTER(_i)]),
    "rf_dwconv3x3": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _vp]),
    "rf_conv3x3_scratch_bytes": (_i, [_i, _i, _psz]),
    "rf_conv3x3": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _vp]),
    "rf_conv3x3_plan": (_i, [_i] * 8 + [_sz, C.c_char_p, _sz, C.POINTER(_i), C.POINTER(_i), C.POINTER(_i), C.POINTER(_i)]),
    "rf_convT2x2_scratch_bytes": (_i, [_i, _i, _psz]),
    "rf_convT2x2": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _vp]),
    "rf_conv1x1_plan": (_i, [_i] * 10 + [C.c_char_p, _sz, C.POINTER(_i), C.POINTER(_i), _psz, C.POINTER(_i)]),
    "rf_conv1x1_dw3_plan": (_i, [_i] * 5 + [C.c_char_p, _sz, C.POINTER(_i), C.POINTER(_i), C.POINTER(_i)]),
    "rf_chan_attn_scratch_bytes": (_i, [_i, _i, _i, _i, _i, _psz]),
    "rf_chan_attn": (_i, [_vp] * 10 + [_i] * 5 + [_vp]),
    "rf_transformer_block_scratch_bytes": (_i, [_i, _i, _i, _i, _i, _i, _psz]),
    "rf_transformer_block": (_i, [_vp, _vp, C.POINTER(_vp), _vp, _i, _i, _i, _i, _i, _i, _vp]),
    "rf_transformer_block_window": (_i, [_vp, _vp, C.POINTER(_vp), _vp, _i, _i, _i, _i, _i, _i, _i, _i, _i, _i, _vp]),
    "rf_attn_front_plan": (_i, [_i, _i, _i, _i, _i, C.POINTER(C.c_longlong)]),
    "rf_flca_scratch_bytes": (_i, [_i, _i, _i, _i, _psz]),
    "rf_flca": (_i, [_vp, _vp, _vp, C.POINTER(_vp), _vp, _i, _i, _i, _i, _vp]),
    "rf_guidance_scratch_bytes": (_i, [_i, _i, _i, _psz]),
    "rf_flca_guidance": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _i, _vp]),
    "rf_to_uint8_hwc": (_i, [_vp, _vp, _i, _i, _i, _i, _vp]),
    "rf_u8_sse": (_i, [_vp, _vp, _vp, _i, _sz, _vp]),
    "rf_u8_channel_sums": (_i, [_vp, _vp, _i, _i, _sz, _vp]),
    "rf_u8_ssim_scratch_bytes": (_i, [_i, _i, _i, _i, _psz]),
    "rf_u8_ssim": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp]),
    "rf_sid_pack": (_i, [_vp, _vp, _i, _i, _i, _i, _i, C.c_double, _i, _vp]),
    "rf_sid_check_desc": (_i, [C.POINTER(C.c_int), _i, _i, _i, _i, _i, _i]),
    "rf_sid_sample": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _i, _vp]),
    "rf_mcr_sample": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _vp]),
    "rf_token_attn": (_i, [_vp, _vp, _vp, _vp, C.c_longlong, C.c_longlong, _i, _i, _i, _i, _f, _vp]),
    "rf_bayer_luma_scratch_bytes": (_i, [_i, _i, _i, _psz]),
    "rf_bayer_luma": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _vp]),
    "rf_luma_film_scratch_bytes": (_i, [_i, _i, _i, _psz]),
    "rf_luma_film": (_i, [_vp, _vp, _vp, C.c_longlong, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp]),
    "rf_dwgate3x3": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp]),
    "rf_dwconv5x5": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp]),
    "rf_wfb_ffn_nblk": (_i, [_i, _i]),
    "rf_wfb_ffn_train_workspace_bytes": (C.c_longlong, [_i, _i, _i, _i, _i]),
    "rf_wfb_ffn_train_forward": (_i, [_vp, _vp, C.POINTER(_vp), _vp, _vp, _sz, _i, _i, _i, _i, _i, _f, _f, _i, _vp]),
    "rf_wfb_ffn_backward_workspace_bytes": (C.c_longlong, [_i, _i, _i, _i, _i]),
    "rf_wfb_ffn_backward": (_i, [_vp, _vp, _vp, C.POINTER(_vp), C.POINTER(_vp), _vp, _sz, _i, _i, _i, _i, _i, _i, _f, _i, _vp]),
    "rf_rfft2_polar_scratch_bytes": (_i, [_i, _i, _i, _psz]),
    "rf_rfft2_polar": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _vp]),
    "rf_polar_irfft2": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _vp]),
    "rf_fft_plan": (_i, [_i, _i, _i, C.POINTER(_i)]),
    "rf_feb_scratch_bytes": (_i, [_i, _i, _i, _i, _psz]),
    "rf_feb": (_i, [_vp, _vp, C.POINTER(_vp), _vp, _i, _i, _i, _i, _vp]),
    "rf_ffab_scratch_bytes": (_i, [_i, _i, _i, _i, _psz]),
    "rf_ffab": (_i, [_vp, _vp, C.POINTER(_vp), _vp, _i, _i, _i, _i, _vp]),
    "rf_affine_clamp_add": (_i, [_vp, _vp, _vp, _sz, _f, _f, _f, _f, _vp]),
    "rf_upcat_scratch_bytes": (_i, [_i, _psz]),
    "rf_upcat": (_i, [_vp] * 8 + [_i, _i, _i, _i, _vp]),
    "rf_mamba_chunk_len": (_i, []),
    "rf_mamba_workspace_bytes": (C.c_longlong, [_i, _i, _i, _i, _i, _i]),
    "rf_mamba_forward": (_i, [_vp, _vp, C.POINTER(_vp), _vp, _sz, _i, _i, _i, _i, _i, _i, _i, _vp]),
    "rf_mamba_backward_workspace_bytes": (C.c_longlong, [_i, _i, _i, _i, _i, _i]),
    "rf_mamba_backward": (_i, [_vp, _vp, _vp, C.POINTER(_vp), C.POINTER(_vp), _vp, _sz, _i, _i, _i, _i, _i, _i, _i, _i, _vp]),
    "rf_wm_workspace_bytes": (C.c_longlong, [_i, _i, _i, _i]),
    "rf_wm_forward": (_i, [_vp, _vp, C.POINTER(_vp), _vp, _sz, _i, _i, _i, _i, _vp]),
    "rf_wm_backward_workspace_bytes": (C.c_longlong, [_i, _i, _i, _i]),
    "rf_wm_backward": (_i, [_vp, _vp, _vp, C.POINTER(_vp), C.POINTER(_vp), _vp, _sz, _i, _i, _i, _i, _i, _vp]),
    "rf_rfft2_polar_backward_scratch_bytes": (C.c_longlong, [_i, _i, _i]),
    "rf_rfft2_polar_backward": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _vp]),
    "rf_polar_irfft2_backward_scratch_bytes": (C.c_longlong, [_i, _i, _i]),
    "rf_polar_irfft2_backward": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _vp]),
    "rf_feb_backward_workspace_bytes": (C.c_longlong, [_i, _i, _i, _i]),
    "rf_feb_backward": (_i, [_vp, _vp, _vp, C.POINTER(_vp), C.POINTER(_vp), _vp, _sz, _i, _i, _i, _i, _i, _vp]),
    "rf_ffab_backward_workspace_bytes": (C.c_longlong, [_i, _i, _i, _i]),
    "rf_ffab_backward": (_i, [_vp, _vp, _vp, C.POINTER(_vp), C.POINTER(_vp), _vp, _sz, _i, _i, _i, _i, _i, _vp]),
    "rf_wmb_front": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp]),
    "rf_wmb_back": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _vp]),
    "rf_wmb_ffn_sum": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp]),
    "rf_wmb_front_backward_nblk": (_i, [_i, _i, _i, _i]),
    "rf_wmb_front_backward_workspace_bytes": (C.c_longlong, [_i, _i, _i, _i]),
    "rf_wmb_front_backward": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _i, _i, _i, _i, _f, _i, _vp]),
    "rf_wmb_back_backward": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _vp]),
    "rf_dwconv5x5_backward_nblk": (_i, [_i, _i]),
    "rf_dwconv5x5_backward_workspace_bytes": (C.c_longlong, [_i, _i, _i, _i]),
    "rf_dwconv5x5_backward": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _i, _i, _i, _i, _i, _vp]),
    "rf_illumination_estimator_backward_workspace_bytes": (C.c_longlong, [_i, _i, _i, _i, _i, _i, _i]),
    "rf_illumination_estimator_backward": (_i, [_vp, _vp, _vp, _vp, C.POINTER(_vp), C.POINTER(_vp), _vp, _sz, _i, _i, _i, _i, _i, _i, _i, _vp]),
    "rf_layernorm2d_backward_workspace_bytes": (C.c_longlong, [_i, _i, _i, _i]),
    "rf_layernorm2d_backward": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _i, _i, _i, _i, _f, _i, _vp]),
    "rf_wmb_backward_workspace_bytes": (C.c_longlong, [_i, _i, _i, _i, _i]),
    "rf_wmb_backward": (_i, [_vp, _vp, _vp, C.POINTER(_vp), C.POINTER(_vp), _vp, _sz, _i, _i, _i, _i, _i, _i, _f, _i, _vp]),
    "rf_tc_spatial":(_i, [_vp] * 9 + [_i, _i, _i, _i, _vp]),
    "rf_tc_nblk": (_i, [_i, _i]),
    "rf_tc_residual": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp]),
    "rf_tc_color_head": (_i, [_vp] * 10 + [_i, _sz, _vp]),
    "rf_tc_pyramid": (_i, [_vp, _vp, _vp, _i, _i, _i, _vp]),
    "rf_ml_modulate": (_i, [_vp, _vp, _vp, _i, _i] + [_vp] * 5 + [_i, _i, _i, _i, _vp]),
    "rf_ml_step_fused": (_i, [_vp, _vp, _vp, _i, _i] + [_vp] * 10 + [_i, _i, _i, _i, _vp]),
    "rf_ml_residual": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _vp]),
    "rf_flca_pyramid_workspace_bytes": (C.c_longlong, [_i] * 7),
    "rf_flca_pyramid_forward": (_i, [_vp, _vp, _vp, C.POINTER(_vp), _vp, _sz] + [_i] * 7 + [_vp]),
    "rf_flca_pyramid_backward_workspace_bytes": (C.c_longlong, [_i] * 7),
    "rf_flca_pyramid_backward": (_i, [_vp, _vp, _vp, _vp, C.POINTER(_vp), C.POINTER(_vp), _vp, _sz] + [_i] * 8 + [_vp]),
    "rf_ml_corrections_backward_workspace_bytes": (C.c_longlong, [_i, _i, _i]),
    "rf_ml_corrections_backward": (_i, [_vp, _vp, _vp, _sz, _i, _i, _i, _vp]),
}

# rf_optim_control and rf_optim_segment (include/rawformer_hip.h) as numpy record types, for reading the guarded step's device state
OPTIM_CONTROL = [("grad_norm", "<f8"), ("grad_sumsq", "<f8"), ("clip_coef", "<f8"), ("nonfinite", "<i8"), ("steps_applied", "<i8"),
                 ("steps_skipped", "<i8"), ("bias_corr1", "<f4"), ("bias_corr2", "<f4"), ("grad_mul", "<f4"), ("skip", "<i4"),
                 ("n", "<i8"), ("nseg", "<i4"), ("nchunks", "<i4")]
OPTIM_CONTROL_BYTES = 80
OPTIM_SEGMENT = [("sumsq", "<f8"), ("nonfinite", "<i8")]

_lib = None


def load() -> C.CDLL:
    """Load the HIP library (once).  Raises if it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"{LIB_PATH} not found: build it with `python -m bayer_low_light_image_enhancement_amd.build` "
                "(hipcc, gfx950).  There is no CPU fallback for the RawFormer HIP path.")
        lib = C.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(lib, name)   # AttributeError here = header and library out of sync
            fn.restype = res
            fn.argtypes = args
        _lib = lib
    return _lib


def check(rc: int, what: str) -> None:
    if rc != 0:
        msg = load().rf_last_error()
        raise RuntimeError(f"{what} failed ({rc}): {msg.decode() if msg else 'unknown error'}")


def call(name: str, *args) -> None:
    """Checked call of an entry point that takes no stream (``rf_create``, ``rf_set_param``, ``rf_set_shard`` ...): the arguments
    go to ctypes as they are, a failing status raises under the entry point's own name."""
    check(getattr(load(), name)(*args), name)


def size(name: str, *geometry) -> int:
    """What a size query answers, whichever of the header's two conventions it follows (told apart by its ``restype`` in
    ``SIGNATURES``): ``rf_*_scratch_bytes(..., size_t*)`` and its kin return a status and write the size,
    ``rf_*_workspace_bytes(...)`` return it as ``long long``, negative for a status.  Either failure raises through ``check``."""
    fn = getattr(load(), name)
    if SIGNATURES[name][0] is C.c_longlong:
        n = fn(*geometry)
        if n < 0:
            check(n, name)
        return n
    sz = C.c_size_t()
    check(fn(*geometry, C.byref(sz)), name)
    return sz.value


def scratch(name: str, like, *geometry):
    """The scratch area the size query ``name`` asks for at ``geometry``: uint8 on ``like``'s device, never under 16 bytes."""
    return torch.empty(max(size(name, *geometry), 16), dtype=torch.uint8, device=like.device)


_PLAIN = frozenset((int, float, type(None)))      # most arguments of a launch: asked for first, the host cost of a call is this loop


def _argument(a):
    if isinstance(a, torch.Tensor):
        return a.data_ptr()
    if isinstance(a, (list, tuple)):
        return (C.c_void_p * len(a))(*[t.data_ptr() for t in a])
    return int(a) if isinstance(a, bool) else a


def launch(name: str, like, *args) -> None:
    """Checked call of a launching entry point on ``like``'s device and that device's current stream, which every one of them
    takes as its last argument.  A tensor goes in as its data pointer, ``None`` as a null pointer, a list or tuple of tensors as
    a ``void*`` array, a ``bool`` as an ``int``; anything else (numbers, ready-made ctypes values, raw addresses) as it is.
    ``args`` holds every tensor, a contiguous copy made by the caller's check included, until the call has returned."""
    conv = [a if type(a) in _PLAIN else _argument(a) for a in args]
    with torch.cuda.device(like.device):
        check(getattr(load(), name)(*conv, torch.cuda.current_stream(like.device).cuda_stream), name)
