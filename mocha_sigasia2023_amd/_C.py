"""ctypes binding of libmocha_hip.so (include/mocha_hip.h).

There is deliberately no fallback: if the HIP library is missing or a call fails, a
RuntimeError is raised.  The product path never imports the CPU oracle.
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libmocha_hip.so")

ABI_VERSION = 6


class mocha_cfg(C.Structure):
    _fields_ = [(n, C.c_int) for n in (
        "T", "V", "C_in", "patch", "dim",
        "enc_depth", "enc_heads", "enc_dim_head", "enc_mlp",
        "dec_depth", "dec_heads", "dec_dim_head", "dec_mlp", "layout")]


class mocha_comm_info_t(C.Structure):
    _fields_ = [("nranks", C.c_int), ("rank", C.c_int), ("rccl_version", C.c_int), ("device", C.c_int),
                ("pci_bus_id", C.c_char * 32), ("library", C.c_char * 512)]


class mocha_ours_cfg(C.Structure):
    _fields_ = [("src_cnt_mean", C.c_void_p), ("src_cnt_std", C.c_void_p), ("cha_encoded_mean", C.c_void_p), ("cha_encoded_std", C.c_void_p),
                ("noise", C.c_int), ("eps", C.c_void_p), ("seed", C.c_uint64)]


class mocha_inert_cfg(C.Structure):
    _fields_ = [("halflife", C.c_double), ("dt", C.c_double)]


class mocha_ingest_cfg(C.Structure):
    _fields_ = [("lookahead", C.c_int), ("rot_format", C.c_int), ("euler_order", C.c_int * 3), ("unit_scale", C.c_double), ("fps", C.c_double),
                ("contact_velocity_threshold", C.c_double), ("spine", C.c_int), ("shoulder_l", C.c_int), ("shoulder_r", C.c_int),
                ("upleg_l", C.c_int), ("upleg_r", C.c_int)]


BVH_MAX_JOINTS, BVH_ALIGN, BVH_MAX_SLOW = 256, 4096, 4096


class mocha_bvh_hdr(C.Structure):
    _fields_ = [("n_joints", C.c_int32), ("channels", C.c_int32), ("order", C.c_int32 * 3), ("reserved", C.c_int32), ("frames", C.c_int64),
                ("frame_time", C.c_double), ("motion_begin", C.c_int64), ("motion_end", C.c_int64), ("error_offset", C.c_int64),
                ("error", C.c_char * 128), ("parents", C.c_int32 * BVH_MAX_JOINTS), ("name_length", C.c_int32 * BVH_MAX_JOINTS),
                ("name_offset", C.c_int64 * BVH_MAX_JOINTS), ("offsets", C.c_double * 3 * BVH_MAX_JOINTS)]


class mocha_bvh_report(C.Structure):
    _fields_ = [("tokens", C.c_int64), ("slow", C.c_int64), ("first_bad", C.c_int64)]


BVHW_MAX_TOKEN = 21


class mocha_bvhw_report(C.Structure):
    _fields_ = [("tokens", C.c_int64), ("bytes", C.c_int64), ("first_bad", C.c_int64)]


_vp, _i, _i64 = C.c_void_p, C.c_int, C.c_int64

# name -> (restype, argtypes); every symbol include/mocha_hip.h declares
SIGNATURES = {
    "mocha_abi_version": (_i, []),
    "mocha_create": (_i, [C.POINTER(mocha_cfg), _i, C.POINTER(_vp)]),
    "mocha_destroy": (None, [_vp]),
    "mocha_last_error": (C.c_char_p, [_vp]),
    "mocha_load_weight": (_i, [_vp, C.c_char_p, _vp, C.POINTER(_i64), _i]),
    "mocha_finalize_weights": (_i, [_vp]),
    "mocha_reserve": (_i, [_vp, _i]),
    "mocha_pos_emb": (_i, [_vp, C.POINTER(_vp)]),
    "mocha_embed": (_i, [_vp, _vp, _i, _vp, _i, _vp]),
    "mocha_encoder": (_i, [_vp, _vp, _i, _vp, _vp]),
    "mocha_mvn": (_i, [_vp, _vp, _i, _vp, _vp, _vp, _vp, _vp]),
    "mocha_encode": (_i, [_vp, _vp, _i, _vp, _vp, _vp, _vp, _vp, _vp]),
    "mocha_decoder": (_i, [_vp, _vp, _vp, _i, _vp, _vp]),
    "mocha_to_mot": (_i, [_vp, _vp, _i, _vp, _vp]),
    "mocha_style_constants": (_i, [_vp, _vp, _i, _vp, _vp]),
    "mocha_forward": (_i, [_vp, _vp, _vp, _i, _vp, _vp]),
    "mocha_forward_features": (_i, [_vp, _vp, _vp, _i, _vp, _vp, _vp, _vp, _vp]),
    "mocha_bank_set": (_i, [_vp, _vp, _vp, _i64, _i, _vp]),
    "mocha_match": (_i, [_vp, _vp, _i, _vp, _vp, _vp]),
    "mocha_bank_gather": (_i, [_vp, _vp, _i, _vp, _vp]),
    "mocha_match_topk": (_i, [_vp, _vp, _i, _i, _vp, _vp, _vp]),
    "mocha_bank_gather_blend": (_i, [_vp, _vp, _vp, C.c_float, _i, _i, _vp, _vp]),
    "mocha_characterize": (_i, [_vp, _vp, _i, _vp, _vp, _vp, _vp, _vp]),
    "mocha_set_pose_norm": (_i, [_vp, _vp, _vp, _vp, _vp]),
    "mocha_encode_raw": (_i, [_vp, _vp, _i, _vp, _vp, _vp, _vp, _vp, _vp]),
    "mocha_characterize_raw": (_i, [_vp, _vp, _i, _vp, _vp, _vp, _vp, _vp]),
    "mocha_characterize_pair": (_i, [_vp, _vp, _i, _vp, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "mocha_characterize_pair_raw": (_i, [_vp, _vp, _i, _vp, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "mocha_match_dist_matrix": (_i, [_vp, _vp, _i, _i64, _i64, _vp, _i64, _vp]),
    "mocha_match_path": (_i, [_vp, _vp, _i, _i, _i64, C.POINTER(C.c_int32), _i, C.POINTER(C.c_int32), _i, C.c_double, _vp, _vp, _vp, _vp]),
    "mocha_characterize_path": (_i, [_vp, _vp, _i, _vp, _vp, C.POINTER(C.c_int32), _i, C.POINTER(C.c_int32), _i, C.c_double, _i, _vp, _vp, _vp,
                                     _i, _vp]),
    "mocha_characterize_pair_path": (_i, [_vp, _vp, _i, _vp, _i, _vp, _vp, C.POINTER(C.c_int32), _i, C.POINTER(C.c_int32), _i, C.c_double, _i,
                                          _vp, _vp, _vp, _vp, _vp, _i, _vp]),
    "mocha_bank_set_starts": (_i, [_vp, C.POINTER(_i64), _i, _vp]),
    "mocha_bank_resident_set_starts": (_i, [_vp, _i, C.POINTER(C.c_int32), _i, _vp]),
    "mocha_path_state_bytes": (_i64, [_vp, _i, _i]),
    "mocha_path_state_reset": (_i, [_vp, _vp, _i, _i, C.POINTER(C.c_int32), _i, _vp]),
    "mocha_match_path_advance": (_i, [_vp, _vp, _i, _i, _vp, _i64, _vp, _vp, _vp, _i64, _vp, _vp, C.c_double, _vp, _vp, _vp, _vp]),
    "mocha_match_path_segmented": (_i, [_vp, _vp, _i, _i, _vp, _vp, _vp, C.c_double, _vp, _vp, _vp, _vp, _i64, _vp]),
    "mocha_characterize_segmented_path": (_i, [_vp, _vp, _i, _vp, _vp, _vp, _vp, _i, C.c_double, _vp, _vp, _vp, _vp, _vp, _i, _vp]),
    "mocha_live_step_path": (_i, [_vp, _vp, _vp, _i] + [_vp] * 19 + [_vp, _i, C.c_double, _vp, _vp, _vp]),
    "mocha_live_step_raw_path": (_i, [_vp, _vp, _vp, _vp, _vp, _i] + [_vp] * 13 + [_vp, _i, C.c_double, _vp, _vp, _vp]),
    "mocha_cvae_load_weight": (_i, [_vp, C.c_char_p, _vp, C.POINTER(_i64), _i]),
    "mocha_cvae_finalize": (_i, [_vp]),
    "mocha_cvae_sample": (_i, [_vp, _vp, _i, _vp, _vp, _vp, _vp, _vp]),
    "mocha_cvae_condition": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _vp, _vp]),
    "mocha_cvae_bank_create": (_i, [_vp, _i]),
    "mocha_cvae_bank_store": (_i, [_vp, _i, _vp, _vp, _vp, _vp, _vp]),
    "mocha_cvae_bank_clear": (_i, [_vp, _i, _vp]),
    "mocha_cvae_bank_info": (_i, [_vp, C.POINTER(_i), _vp]),
    "mocha_cvae_sample_grouped": (_i, [_vp, _vp, _i, _vp, _vp, _vp, _vp, _vp, _vp]),
    "mocha_scale_shift": (_i, [_vp, _vp, _vp, _vp, _i, _vp, _vp]),
    "mocha_featurize": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _vp, _vp]),
    "mocha_post_cfg_default": (None, [_vp]),
    "mocha_pose_heads": (_i, [_vp, _vp, _i, _vp, _vp, _vp]),
    "mocha_postprocess": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp]),
    "mocha_post_state_bytes": (_i64, [_vp]),
    "mocha_postprocess_step": (_i, [_vp] * 9 + [_i] + [_vp] * 6),
    "mocha_live_state_bytes": (_i64, [_vp, _i]),
    "mocha_live_reset": (_i, [_vp, _vp, _i, C.POINTER(C.c_int32), _i, _vp]),
    "mocha_live_step": (_i, [_vp, _vp, _vp, _i] + [_vp] * 19),
    "mocha_live_ours_state_bytes": (_i64, [_vp, _i]),
    "mocha_live_ours_reset": (_i, [_vp, _vp, _vp, _i, C.POINTER(C.c_int32), _i, _vp]),
    "mocha_live_step_ours": (_i, [_vp, _vp, _vp, _i] + [_vp] * 11 + [_vp, _vp] + [_vp] * 8 + [_vp]),
    "mocha_live_step_ours_grouped": (_i, [_vp, _vp, _vp, _i] + [_vp] * 11 + [_vp, _vp, _vp] + [_vp] * 8 + [_vp]),
    "mocha_column_stats": (_i, [_vp, _vp, _i64, _vp, _vp, _vp]),
    "mocha_set_option": (_i, [_vp, C.c_char_p, _i]),
    "mocha_linear": (_i, [_vp, _vp, _vp, _vp, _vp, _i64, _i, _i, _i, _vp]),
    "mocha_linear_grouped": (_i, [_vp] * 7 + [_i] * 7 + [_vp, _i, _vp]),
    "mocha_graph_constants": (_i, [_vp, _vp, _vp, _vp, _vp]),
    "mocha_generation": (_i64, [_vp]),
    "mocha_step_graph": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _i, _vp]),
    "mocha_step_graph_lane": (_i, [_vp, _i, _vp, _vp, _vp, _vp, _vp, _i, _vp]),
    "mocha_bank_set_segments": (_i, [_vp, _vp, _vp, _i64, C.POINTER(_i64), _i, _i, _vp]),
    "mocha_match_segmented": (_i, [_vp, _vp, _i, _vp, _vp, _vp, _vp]),
    "mocha_characterize_segmented": (_i, [_vp, _vp, _i, _vp, _vp, _vp, _vp, _vp, _i, _vp]),
    "mocha_step_graph_segmented": (_i, [_vp, _vp, _i, _vp, _vp, _vp, _vp, _vp, _i, _vp]),
    "mocha_match_topk_segmented": (_i, [_vp, _vp, _i, _vp, _i, _vp, _vp, _vp]),
    "mocha_characterize_soft_segmented": (_i, [_vp, _vp, _i, _vp, _i, C.c_float, _vp, _vp, _vp, _vp, _vp, _i, _vp]),
    "mocha_step_graph_soft_segmented": (_i, [_vp, _vp, _i, _vp, _i, C.c_float, _vp, _vp, _vp, _vp, _vp, _i, _vp]),
    "mocha_live_step_soft": (_i, [_vp, _vp, _vp, _i] + [_vp] * 11 + [_i, C.c_float] + [_vp] * 10),
    "mocha_inert_state_bytes": (_i64, [_vp]),
    "mocha_inertialize_step": (_i, [_vp] * 8 + [_i, _vp]),
    "mocha_live_step_inert": (_i, [_vp, _vp, _vp, _i] + [_vp] * 11 + [_i, C.c_float] + [_vp] * 12),
    "mocha_ingest_cfg_default": (None, [_vp, _i]),
    "mocha_ingest_state_bytes": (_i64, [_vp, _i]),
    "mocha_ingest_reset": (_i, [_vp, _vp, _i, C.POINTER(C.c_int32), _i, _vp]),
    "mocha_live_ingest_step": (_i, [_vp, _vp, _vp, _vp, _i] + [_vp] * 12),
    "mocha_live_step_raw": (_i, [_vp, _vp, _vp, _vp, _vp, _i] + [_vp] * 5 + [_i, C.c_float] + [_vp] * 12),
    "mocha_bank_set_labels": (_i, [_vp, C.POINTER(C.c_int32), _vp]),
    "mocha_match_segmented_allow": (_i, [_vp, _vp, _i, _vp, _vp, _i, _vp, _vp, _vp, _vp]),
    "mocha_characterize_segmented_allow": (_i, [_vp, _vp, _i, _vp, _vp, _i, C.c_float, _vp, _vp, _vp, _vp, _vp, _vp, _i, _vp]),
    "mocha_step_graph_segmented_allow": (_i, [_vp, _vp, _i, _vp, _vp, _i, C.c_float, _vp, _vp, _vp, _vp, _vp, _vp, _i, _vp]),
    "mocha_live_step_allow": (_i, [_vp, _vp, _vp, _i] + [_vp] * 11 + [_i, C.c_float] + [_vp] * 14),
    "mocha_live_step_raw_allow": (_i, [_vp, _vp, _vp, _vp, _vp, _i] + [_vp] * 5 + [_i, C.c_float] + [_vp] * 14),
    "mocha_match_mix_segmented": (_i, [_vp, _vp, _i, _vp, _vp, _i, _vp, _vp, _vp, _vp, _vp]),
    "mocha_characterize_mix_segmented": (_i, [_vp, _vp, _i, _vp, _vp, _i, _vp, _vp, _vp, _vp, _vp, _i, _vp]),
    "mocha_step_graph_mix_segmented": (_i, [_vp, _vp, _i, _vp, _vp, _i, _vp, _vp, _vp, _vp, _vp, _i, _vp]),
    "mocha_live_step_mix": (_i, [_vp, _vp, _vp, _i] + [_vp] * 10 + [_i] + [_vp] * 11),
    "mocha_live_step_raw_mix": (_i, [_vp, _vp, _vp, _vp, _vp, _i] + [_vp] * 4 + [_i] + [_vp] * 11),
    "mocha_bank_resident_create": (_i, [_vp, _i64, _i, _i64, _i, _vp]),
    "mocha_bank_resident_add": (_i, [_vp, _i, _vp, _vp, _i64, _vp, C.POINTER(C.c_int32), _vp]),
    "mocha_bank_resident_retire": (_i, [_vp, _i, _vp]),
    "mocha_bank_resident_info": (_i, [_vp, _i] + [C.POINTER(_i64)] * 4),
    "mocha_ingest_clips": (_i, [_vp, _vp, _vp, _vp, _vp, C.POINTER(C.c_int32), _i, C.POINTER(C.c_int32), C.POINTER(C.c_ubyte)] + [_vp] * 6),
    "mocha_clip_window_count": (_i, [C.POINTER(C.c_int32), _i, _i, _i, C.POINTER(_i64)]),
    "mocha_clip_windows": (_i, [_vp] * 6 + [_i, C.POINTER(C.c_int32), _i, _i, _i] + [_vp] * 6),
    "mocha_mirror_map_default": (_i, [_i, C.POINTER(C.c_int32)]),
    "mocha_resample_frames": (_i64, [_i64, _i, _i]),
    "mocha_resample_clips": (_i, [_vp, _i, C.POINTER(C.c_int), _vp, _vp, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32), _i,
                                  C.POINTER(C.c_int32), _vp, _vp, _vp]),
    "mocha_resample_state_bytes": (_i64, [_vp, _i]),
    "mocha_resample_reset": (_i, [_vp, _vp, _i, C.POINTER(C.c_int32), _i, _vp]),
    "mocha_resample_step": (_i, [_vp, _i, C.POINTER(C.c_int), _vp, _i, _vp, _vp, _i, _i, _i64, _vp, _vp, C.POINTER(C.c_int32), _vp]),
    "mocha_world_bind_bytes": (_i64, [_vp]),
    "mocha_world_bind": (_i, [_vp, _vp, _vp, C.POINTER(C.c_double), _vp, _vp]),
    "mocha_world_pose": (_i, [_vp, _vp, _vp, _i, _i64, _vp, _vp, _vp, _vp, _vp, _vp]),
    "mocha_bvh_header": (_i,[_vp, _i64, C.POINTER(mocha_bvh_hdr)]),
    "mocha_bvh_motion": (_i, [_vp, _vp, _i64, _vp, C.POINTER(_i64), C.POINTER(_i64), C.POINTER(C.c_int32), _i, _i, _i, C.POINTER(C.c_int32), _i,
                              C.POINTER(C.c_float), _vp, _vp, C.POINTER(mocha_bvh_report), _vp]),
    "mocha_bvh_text_bound": (_i64, [_i64, _i, _i]),
    "mocha_bvh_format": (_i, [_vp, _vp, _vp, C.POINTER(C.c_int32), _i, _i, C.POINTER(C.c_int32), C.POINTER(C.c_int32), _i, _vp, _i64,
                              C.POINTER(_i64), C.POINTER(mocha_bvhw_report), _vp]),
    "mocha_set_rccl_library":(_i, [C.c_char_p]),
    "mocha_comm_unique_id": (_i, [_vp, _vp]),
    "mocha_comm_init": (_i, [_vp, _vp, _i, _i]),
    "mocha_comm_destroy": (_i, [_vp]),
    "mocha_comm_info": (_i, [_vp, C.POINTER(mocha_comm_info_t)]),
    "mocha_bank_broadcast": (_i, [_vp, _vp, _i, _i64, _i, _vp]),
    "mocha_bcast_plan": (_i, [_i64, _i, _i, C.POINTER(_i64)]),
    "mocha_build_info": (C.c_char_p, []),
    "mocha_runtime_version": (_i, []),
    "mocha_bank_export": (_i, [_vp, _vp, _vp, _vp]),
    "mocha_scan_byte_state": (_i, [_vp, _i, C.POINTER(C.c_int32), _vp]),
    "mocha_bank_view": (_i, [_vp] + [C.POINTER(_vp)] * 5 + [C.POINTER(_i64)]),
    "mocha_profile_start": (_i, [_vp]),
    "mocha_profile_stop": (_i, [_vp, C.c_char_p, _i64]),
}

_lib = None


def load_library(path: str = LIB_PATH):
    """dlopen the library and bind every declared symbol; raises RuntimeError when absent."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(path):
        raise RuntimeError(
            f"libmocha_hip.so not found at {path}: build it with "
            "`python -c 'import __graft_entry__ as g; g.build()'` or `make -C mocha_sigasia2023_amd/csrc`. "
            "There is no CPU fallback.")
    try:
        lib = C.CDLL(path)
    except OSError as e:  # missing ROCm runtime etc.
        raise RuntimeError(f"cannot load {path}: {e}") from e
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)      # AttributeError if the symbol is not exported
        fn.restype = res
        fn.argtypes = args
    if lib.mocha_abi_version() != ABI_VERSION:
        raise RuntimeError(f"libmocha_hip.so ABI {lib.mocha_abi_version()} != binding ABI {ABI_VERSION}")
    _lib = lib
    return lib


def check(lib, ctx, rc: int, what: str):
    if rc != 0:
        msg = lib.mocha_last_error(ctx)
        raise RuntimeError(f"{what} failed (status {rc}): {msg.decode() if msg else '?'}")
