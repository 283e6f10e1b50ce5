"""ctypes binding of libvdr.so (include/vdr.h).  No fallback: if the HIP library is missing or a
symbol is absent this module raises — there is no CPU path behind the boundary."""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libvdr.so")

VDR_F32, VDR_BF16, VDR_F64, VDR_I16, VDR_U8 = 0, 1, 2, 3, 4
ACT_GELU, ACT_SWIGLU, ACT_QUICK_GELU, ACT_GELU_TANH = 0, 1, 2, 3
OUT_CLS, OUT_DENSE, OUT_PATCH_EMBED, OUT_TOKENS, OUT_ENCODER, OUT_POOLED = 0, 1, 2, 3, 4, 5
EPI_BIAS, EPI_BIAS_GELU, EPI_BIAS_RESID, EPI_SWIGLU = 0, 1, 2, 3
EPI_BIAS_QUICK_GELU, EPI_BIAS_GELU_TANH = 8, 9  # (4 .. 7 are internal to the library)
K_COUNT = 11


class VdrError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"libvdr error {code}: {msg}")
        self.code = code


class vdr_config(C.Structure):
    _fields_ = [("img", C.c_int32), ("patch", C.c_int32), ("in_chans", C.c_int32), ("dim", C.c_int32),
                ("heads", C.c_int32), ("layers", C.c_int32), ("mlp_hidden", C.c_int32), ("act", C.c_int32),
                ("pre_ln", C.c_int32), ("layerscale", C.c_int32), ("has_cls", C.c_int32), ("has_pos", C.c_int32),
                ("input_ln", C.c_int32), ("ln_eps", C.c_float), ("micro_batch", C.c_int32),
                ("streams", C.c_int32), ("window", C.c_int32),
                ("global_mask", C.c_int32), ("neck_chans", C.c_int32), ("fp8", C.c_int32), ("no_ln_fold", C.c_int32),
                ("full_last_block", C.c_int32), ("fp8_cls_bf16", C.c_int32), ("resid_fp32", C.c_int32),
                ("ln_fin_fused", C.c_int32)]


class vdr_config_ext(C.Structure):
    _fields_ = [("size", C.c_int32), ("n_register", C.c_int32), ("rope", C.c_int32), ("rope_theta", C.c_float)]


class vdr_mask_decoder_config(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("grid", "img", "channels", "heads", "depth", "mlp_dim", "attention_downsample_rate", "mask_tokens",
                                          "upscale_channels_1", "upscale_channels_2", "iou_head_depth")] + \
               [(n, C.c_float) for n in ("ln_eps", "final_ln_eps", "ln2d_eps")]


class vdr_mask_prompts(C.Structure):
    _fields_ = [("boxes", C.c_void_p), ("points", C.c_void_p), ("labels", C.c_void_p), ("points_per_problem", C.c_int32),
                ("mask_input", C.c_void_p), ("mask_per_image", C.c_int32)]


PROMPT_POINTS, PROMPT_MASK = 1, 2
MASK_EMBED_WEIGHTS = 4684


class vdr_layer_out(C.Structure):
    _fields_ = [("layer", C.c_int32), ("out_mode", C.c_int32), ("out_dtype", C.c_int32), ("norm", C.c_int32),
                ("ld", C.c_int64), ("out", C.c_void_p)]


class vdr_attn_map(C.Structure):
    _fields_ = [("layer", C.c_int32), ("q_rows", C.c_int32), ("head_mean", C.c_int32), ("out_dtype", C.c_int32),
                ("out", C.c_void_p)]


FACET_TOKEN, FACET_QUERY, FACET_KEY, FACET_VALUE = 0, 1, 2, 3
FACETS = {"token": FACET_TOKEN, "query": FACET_QUERY, "key": FACET_KEY, "value": FACET_VALUE}


class vdr_facet_out(C.Structure):
    _fields_ = [("layer", C.c_int32), ("facet", C.c_int32), ("hierarchy", C.c_int32), ("all_rows", C.c_int32),
                ("out_dtype", C.c_int32), ("out", C.c_void_p)]


# every symbol include/vdr.h declares: name -> (restype, argtypes)
_P, _I, _L, _F = C.c_void_p, C.c_int, C.c_int64, C.c_float
SYMBOLS = {
    "vdr_abi_version": (_I, []),
    "vdr_tuning_build": (_I, []),
    "vdr_device_count": (_I, []),
    "vdr_create": (_I, [C.POINTER(vdr_config), _I, C.POINTER(_P)]),
    "vdr_create_ext": (_I, [C.POINTER(vdr_config), C.POINTER(vdr_config_ext), _I, C.POINTER(_P)]),
    "vdr_destroy": (None, [_P]),
    "vdr_last_error": (C.c_char_p, [_P]),
    "vdr_set_weight": (_I, [_P, C.c_char_p, _P, C.POINTER(_L), _I]),
    "vdr_finalize": (_I, [_P]),
    "vdr_set_input_size": (_I, [_P, _I, _I]),
    "vdr_get_input_size": (_I, [_P, C.POINTER(_I), C.POINTER(_I)]),
    "vdr_set_patch_stride": (_I, [_P, _I]),
    "vdr_get_patch_stride": (_I, [_P, C.POINTER(_I)]),
    "vdr_num_weights": (_I, [_P]),
    "vdr_weight_name": (C.c_char_p, [_P, _I]),
    "vdr_workspace_bytes": (_I, [_P, _I, _I, C.POINTER(C.c_size_t)]),
    "vdr_batch_plan": (_I, [_P, _I, _I, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "vdr_forward": (_I, [_P, _P, _I, _I, _P, _I, _I, _P, C.c_size_t, _P]),
    "vdr_forward_layers": (_I, [_P, _P, _I, _I, C.POINTER(vdr_layer_out), _I, _P, C.c_size_t, _P]),
    "vdr_forward_attn_maps": (_I, [_P, _P, _I, _I, C.POINTER(vdr_layer_out), _I, C.POINTER(vdr_attn_map), _I, _P, C.c_size_t,
                                   _P]),
    "vdr_forward_facets": (_I, [_P, _P, _I, _I, C.POINTER(vdr_layer_out), _I, C.POINTER(vdr_attn_map), _I,
                                C.POINTER(vdr_facet_out), _I, _P, C.c_size_t, _P]),
    "vdr_forward_tokens": (_I, [_P, _P, _I, _I, _I, _P, _I, _I, _P, C.c_size_t, _P]),
    "vdr_forward_tokens_varlen": (_I, [_P, _P, _I, _I, _I, _P, _P, _I, _I, _P, C.c_size_t, _P]),
    "vdr_op_layernorm": (_I, [_P, _I, _P, _I, _P, _P, _L, _I, _F, _P]),
    "vdr_op_linear": (_I, [_P, _P, _P, _P, _P, _P, _L, _I, _I, _I, _I, _P]),
    "vdr_op_pack_linear_weight": (_I, [_P, _I, _I, _P, _P]),
    "vdr_op_linear_packed": (_I, [_P, _P, _P, _P, _P, _P, _L, _I, _I, _I, _I, _P]),
    "vdr_ln_fold_weights": (_I, [_P, _P, _P, _P, _I, _I, _I, _P, _P, _P]),
    "vdr_op_linear_ln_stats": (_I, [_P, _P, _P, _P, _P, _P, _P, _P, _L, _I, _I, _I, _P, _L, _P, _P, _F, _P]),
    "vdr_op_ln_finalize": (_I, [_P, _L, _L, _I, _F, _P, _P]),
    "vdr_op_linear_ln_fold": (_I, [_P, _P, _P, _P, _P, _P, _L, _P, _L, _I, _I, _L, _F, _I, _I, _P]),
    "vdr_prepare_scratch_bytes": (C.c_size_t, [_I, _I, _I, _I, _I]),
    "vdr_op_prepare_image": (_I, [_P, _I, _I, _I, _I, _I, _L, _L, _L, _L, _I, _I, _P, _I, _P, _P]),
    "vdr_op_window_ct": (_I, [_P, _I, _L, C.c_double, C.c_double, _P, _P]),
    "vdr_op_hu_to_rgb": (_I, [_P, _I, _L, _P, _P]),
    "vdr_op_crop_hwc": (_I, [_P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _P]),
    "vdr_op_voxel_sequence": (_I, [_P, _P, _P, _P, _L, _I, _P, _I, _P]),
    "vdr_affine_cubic_scratch_bytes": (C.c_size_t, [_I, _I, _L]),
    "vdr_op_affine_cubic": (_I, [_P, _I, _I, _I, _L, C.POINTER(C.c_double), C.POINTER(C.c_double), _P, _I, _P, _P]),
    "vdr_mx_scale_bytes": (C.c_size_t, [_L, _I]),
    "vdr_op_mx_quantize": (_I, [_P, _L, _I, _P, _P, _P]),
    "vdr_op_mx_dequantize": (_I, [_P, _P, _L, _I, _P, _P]),
    "vdr_op_layernorm_mx": (_I, [_P, _P, _P, _F, _L, _I, _P, _P, _P]),
    "vdr_op_linear_mx": (_I, [_P, _P, _P, _P, _P, _P, _P, _P, _P, _L, _I, _I, _I, _I, _P]),
    "vdr_op_attention": (_I, [_P, _P, _I, _I, _I, _I, _P]),
    "vdr_op_attention_hd": (_I, [_P, _P, _I, _I, _I, _I, _I, _P]),
    "vdr_op_attention_varlen": (_I, [_P, _P, _I, _I, _I, _I, _P, _I, _I, _P]),
    "vdr_op_attention_probs": (_I, [_P, _P, _I, _I, _I, _I, _I, _I, _I, _P]),
    "vdr_op_attention_pool": (_I, [_P, _P, _L, _P, _I, _I, _I, _I, _P]),
    "vdr_op_cross_attention": (_I, [_P, _L, _P, _P, _L, _P, _P, _L, _P, _L, _I, _I, _I, _I, _I, _P]),
    "vdr_op_token_linear": (_I, [_P, _L, _P, _L, _P, _P, _P, _L, _P, _I, _L, _I, _I, _I, _I, _I, _P]),
    "vdr_op_mask_upscale": (_I, [_P, _P, _P, _P, _P, _I, _I, _I, _P]),
    "vdr_mask_decoder_create": (_I, [C.POINTER(vdr_mask_decoder_config), _I, C.POINTER(_P)]),
    "vdr_mask_decoder_destroy": (None, [_P]),
    "vdr_mask_decoder_num_weights": (_I, [_P]),
    "vdr_mask_decoder_weight_name": (C.c_char_p, [_P, _I]),
    "vdr_mask_decoder_set_weight": (_I, [_P, C.c_char_p, _P, C.POINTER(_L), _I]),
    "vdr_mask_decoder_finalize": (_I, [_P]),
    "vdr_mask_decoder_workspace_bytes": (_I, [_P, _I, C.POINTER(C.c_size_t)]),
    "vdr_mask_decode": (_I, [_P, _P, _I, _P, _I, _I, _P, C.c_size_t, _P, _P, _P]),
    "vdr_mask_decoder_num_prompt_weights": (_I, [_P]),
    "vdr_mask_decoder_prompt_weight_name": (C.c_char_p, [_P, _I]),
    "vdr_mask_decoder_prompt_support": (_I, [_P]),
    "vdr_mask_decoder_workspace_bytes_prompts": (_I, [_P, _I, _I, C.POINTER(C.c_size_t)]),
    "vdr_mask_decode_prompts": (_I, [_P, _P, _I, C.POINTER(vdr_mask_prompts), _I, _I, _P, C.c_size_t, _P, _P, _P]),
    "vdr_op_mask_embed": (_I, [_P, _I, _P, _I, _P, _P, _I, _I, _I, _F, _P]),
    "vdr_op_mask_box": (_I, [_P, _L, _P, _P, _P, _I, _I, _I, _I, _F, _F, _P]),
    "vdr_mask_stats_workspace_bytes": (C.c_size_t, [_I, _I, _I, _I, _I]),
    "vdr_op_mask_stats": (_I, [_P, _L, _I, _L, _I, _I, _I, _I, _I, _F, _F, _P, C.c_size_t, _P, _P, _P]),
    "vdr_nms_workspace_bytes": (C.c_size_t, [_I]),
    "vdr_mask_binarize_workspace_bytes": (C.c_size_t, [_I, _I, _I, _I, _I]),
    "vdr_op_mask_binarize": (_I, [_P, _L, _I, _L, _I, _I, _I, _I, _I, _F, _P, C.c_size_t, _P, _P]),
    "vdr_connected_components_workspace_bytes": (C.c_size_t, [_I, _I, _I]),
    "vdr_op_connected_components": (_I, [_P, _I, _I, _I, _I, _I, _P, C.c_size_t, _P, _P, _P, _P]),
    "vdr_mask_clean_workspace_bytes": (C.c_size_t, [_I, _I, _I]),
    "vdr_op_mask_clean": (_I, [_P, _I, _I, _I, _I, _I, _I, _P, C.c_size_t, _P, _P, _P, _P]),
    "vdr_distance_transform_workspace_bytes": (C.c_size_t, [_I, _I, _I]),
    "vdr_op_distance_transform": (_I, [_P, _I, _I, _I, _I, _I, _I, _P, C.c_size_t, _P, _P, _P, _P, _P]),
    "vdr_distance_transform_3d_workspace_bytes": (C.c_size_t, [_I, _I, _I, _I]),
    "vdr_op_distance_transform_3d": (_I, [_P, _I, _I, _I, _I, _I, _I, _I, _I, _I, C.c_int64, _P, C.c_size_t, _P, _P, _P, _P]),
    "vdr_op_nms": (_I, [_P, _P, _I, _F, _P, C.c_size_t, _P, _P, _P, _P]),
    "vdr_op_attention_relpos": (_I, [_P, _P, _P, _P, _P, _I, _I, _I, _P]),
    "vdr_op_layernorm_window": (_I, [_P, _P, _P, _P, _I, _I, _I, _I, _F, _P]),
    "vdr_op_layernorm_mx_window": (_I, [_P, _P, _P, _F, _I, _I, _I, _I, _P, _P, _P]),
    "vdr_op_linear_window": (_I, [_P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _P, _L, _P]),
    "vdr_op_im2col3": (_I, [_P, _P, _I, _I, _I, _P]),
    "vdr_op_interpolate_pos": (_I, [_P, _I, _I, _I, _P, _I, _I, _P]),
    "vdr_op_interpolate_rel_pos": (_I, [_P, _I, _I, _P, _I, _P]),
    "vdr_op_rope2d_table": (_I, [_I, _I, _I, _F, _P, _P, _P]),
    "vdr_op_rope2d": (_I, [_P, _I, _I, _I, _I, _I, _P, _P, _P]),
    "vdr_op_patch_embed": (_I, [_P, _I, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _P]),
    "vdr_op_patch_embed_strided": (_I, [_P, _I, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _I, _P]),
    "vdr_op_log_bin": (_I, [_P, _I, _L, _L, _I, _I, _I, _I, _I, _P, _P, _I, _P]),
    "vdr_nn_cosine_work_bytes": (C.c_size_t, [_I, _I, _I]),
    "vdr_op_nn_cosine": (_I, [_P, _L, _L, _I, _P, _L, _L, _I, _I, _I, _P, _P, _P, _P, _P, _P]),
    "vdr_knn_work_bytes": (C.c_size_t, [_I, _I, _I, _I]),
    "vdr_op_knn": (_I, [_P, _L, _L, _I, _P, _L, _L, _I, _I, _I, _I, _I, _I, _P, _P, _P, _P]),
    "vdr_local_correlation_work_bytes": (C.c_size_t, [_I, _I, _I, _I]),
    "vdr_op_local_correlation": (_I, [_P, _L, _L, _P, _L, _L, _I, _I, _I, _I, _I, _I, _P, _P, _P, _P, _P]),
    "vdr_op_window_vote": (_I, [_P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _F, _P, _P, _P, _P, _P]),
    "vdr_affinity_work_bytes": (C.c_size_t, [_I, _I]),
    "vdr_op_affinity_bits": (_I, [_P, _L, _L, _I, _I, _I, _F, _I, _P, _P, _I, _P]),
    "vdr_op_bits_matvec": (_I, [_P, _I, _I, _I, _P, _I, _P, _P, _P]),
    "vdr_pca_work_bytes": (C.c_size_t, [_I, _I, _I, _I]),
    "vdr_op_col_mean": (_I, [_P, _I, _L, _L, _I, _I, _I, _I, _P, _P, _P]),
    "vdr_op_covariance": (_I, [_P, _I, _L, _L, _I, _I, _I, _I, _P, _P, _P, _P]),
    "vdr_op_pca_project": (_I, [_P, _I, _L, _L, _I, _I, _I, _I, _P, _P, _I, _I, _P, _P, _P, _P]),
    "vdr_pca_topk_work_bytes": (C.c_size_t, [_I, _I, _I, _I]),
    "vdr_op_col_mean_any": (_I, [_P, _I, _L, _L, _I, _I, _I, _P, _P, _P]),
    "vdr_op_gram": (_I, [_P, _I, _L, _L, _I, _I, _I, _P, _P, _P, _P]),
    "vdr_op_pca_back_project": (_I, [_P, _I, _L, _L, _I, _I, _I, _P, _P, _P, _I, _P, _P, _P]),
    "vdr_op_sym_topk": (_I, [_P, _I, _I, _I, C.c_float, _I, _P, _P, _P, _P, _P, _P]),
    "vdr_kmeans_work_bytes": (C.c_size_t, [_I, _I, _I, _I, _I]),
    "vdr_op_kmeans_assign": (_I, [_P, _L, _L, _L, _I, _I, _I, _I, _I, _P, _P, _P, _P, _P, _P, _P, _P]),
    "vdr_op_kmeans_update": (_I, [_P, _L, _L, _L, _I, _I, _I, _I, _I, _P, _P, _P, _P, _P, _P]),
    "vdr_op_mahalanobis": (_I, [_P, _L, _L, _L, _I, _I, _I, _I, _P, _L, _P, _L, _I, _P, _P]),
    "vdr_upsample_work_bytes": (C.c_size_t, [_I, _I, _I, _I]),
    "vdr_op_guide_lowres": (_I, [_P, _I, _I, _I, _I, _I, _I, _I, _P, _P]),
    "vdr_op_upsample_guided": (_I, [_P, _I, _L, _L, _I, _I, _I, _I, _P, _I, _I, _I, _I, _I, _I, _I, _F, _F, _P, _I, _I, _I, _I,
                                    _P, _P, _I, _P]),
    "vdr_profile_enable": (_I, [_P, _I]),
    "vdr_profile_mask": (_I, [_P, C.c_uint32]),
    "vdr_profile_read": (_I, [_P, C.POINTER(C.c_double), C.POINTER(_L), C.POINTER(C.c_double),
                              C.POINTER(C.c_double), _I]),
    "vdr_kernel_class_name": (C.c_char_p, [_I]),
}

_lib = None


def bind(lib: C.CDLL, skip_missing: bool = False) -> C.CDLL:
    """Set restype / argtypes of every SYMBOLS entry on `lib`.  A symbol the library does not export is an AttributeError, or
    is left out with skip_missing (tools that open a library older than the table)."""
    for name, (res, args) in SYMBOLS.items():
        try:
            fn = getattr(lib, name)
        except AttributeError:
            if skip_missing:
                continue
            raise
        fn.restype = res
        fn.argtypes = args
    return lib


def load() -> C.CDLL:
    """dlopen libvdr.so and bind every declared symbol.  torch is imported first so that the HIP
    runtime already mapped by PyTorch-ROCm (same SONAME libamdhip64.so.7) is the one libvdr uses:
    streams and device pointers are then directly exchangeable."""
    global _lib
    if _lib is not None:
        return _lib
    import torch  # noqa: F401  (maps libamdhip64 before libvdr asks for it)
    if not os.path.exists(LIB_PATH):
        raise ImportError(f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                          "or `make -C vit-deep-radiomics_amd/csrc`. There is no CPU fallback.")
    lib = bind(C.CDLL(LIB_PATH))  # AttributeError if the library does not export a symbol
    if lib.vdr_abi_version() != 8:
        raise ImportError("libvdr ABI version mismatch")
    _lib = lib
    return lib


def check(rc: int, handle=None):
    if rc != 0:
        msg = load().vdr_last_error(handle)
        raise VdrError(rc, msg.decode() if msg else "?")


def source_id() -> str:
    """sha256 (first 16 hex digits) over the kernel sources under csrc/ (*.hip, *.h, Makefile, sorted by name): identifies
    the kernels a committed profile was taken with, independent of when or where libvdr.so was built."""
    import glob
    import hashlib
    h = hashlib.sha256()
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "csrc")
    for f in sorted(glob.glob(os.path.join(csrc, "*.hip")) + glob.glob(os.path.join(csrc, "*.h")) + [os.path.join(csrc, "Makefile")]):
        h.update(os.path.basename(f).encode())
        h.update(open(f, "rb").read())
    return h.hexdigest()[:16]
