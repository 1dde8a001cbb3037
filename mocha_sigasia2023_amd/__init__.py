"""mocha_sigasia2023_amd — MI355X-native (gfx950) implementation of the MOCHA ``Generator``
hot path (motion encoder -> context matching -> body-part decoder) behind the reference's
own call surface.  The arithmetic lives in ``libmocha_hip.so`` (``csrc/``, C ABI in
``include/mocha_hip.h``); this package is the thin host-side mirror of the reference interface.
"""
from .generator import CVAE, CVAEBank, CoherentMatch, ContextBank, Generator, OursSession, StreamingCharacterizer, mean_variance_norm  # noqa: F401
from .multi_character import MultiCharacterBank, MultiStreamCharacterizer, OnlinePath, ResidentCharacterBank, action_mask  # noqa: F401
from .bank import BatchPipeline, ShardedContextBank, bank_starts, build_bank, build_database_from_bvh, load_bank, save_bank  # noqa: F401
from .postprocess import Inertializer, PostProcessor, pose_heads, retarget_clip, retarget_clip_ours, retarget_frame_ours, write_bvh  # noqa: F401
from .postprocess import BvhValueRefused, format_bvh_motion, write_bvh_clips  # noqa: F401
from .live import LiveOursSession, LiveSession  # noqa: F401
from .ingest import IngestConfig, Ingestor, StreamResampler, clip_windows, ingest_clips, resample_clips, resample_lengths  # noqa: F401
from .world import SkinBind, world_pose  # noqa: F401
from .bvh import BvhClips, BvhHeader, load_bvh, read_bvh_header  # noqa: F401
from .skeleton import PART_NAMES, skeleton_constants  # noqa: F401
from . import synthetic  # noqa: F401
from .weights import DEFAULT_CFG, param_shapes, synthetic_state_dict  # noqa: F401

__all__ = ["Generator", "CVAE", "CVAEBank", "OursSession", "ContextBank", "StreamingCharacterizer", "mean_variance_norm", "skeleton_constants",
           "synthetic_state_dict", "param_shapes", "DEFAULT_CFG", "build_bank", "save_bank", "load_bank", "ShardedContextBank", "BatchPipeline",
           "PostProcessor", "pose_heads", "MultiCharacterBank", "MultiStreamCharacterizer", "ResidentCharacterBank", "action_mask", "retarget_clip", "retarget_clip_ours", "retarget_frame_ours", "write_bvh", "write_bvh_clips", "format_bvh_motion", "BvhValueRefused",
           "LiveSession", "LiveOursSession", "Inertializer", "Ingestor", "IngestConfig", "ingest_clips", "clip_windows",
           "resample_clips", "resample_lengths", "StreamResampler", "SkinBind", "world_pose",
           "CoherentMatch", "OnlinePath", "bank_starts", "PART_NAMES", "read_bvh_header", "load_bvh", "BvhHeader", "BvhClips", "build_database_from_bvh"]
