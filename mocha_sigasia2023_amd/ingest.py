"""The mocap front end of a live session on the device (``mocha_live_ingest_step``): raw frames in, the live step's inputs out.

A mocap device delivers, per frame, the local rotations and local positions of the skeleton's joints.  The live step takes what the
reference's ``process_data`` makes of a whole clip - a synthetic root bone, velocities, foot contacts - with filters that read frames
after the one they produce.  ``Ingestor`` is that preparation in streaming form: one raw frame per call and stream, and from the 31st
push on every call emits frame ``n-1-lookahead`` of ``process_data`` applied to the frames pushed so far.  ``lookahead=18`` gives the
whole clip's frame 0.3 s late; ``lookahead=0`` the newest frame under the reference's clip-end rules.  ``LiveSession(raw=...)`` runs it
inside the session's captured graph.  Not provided: a flush of the last ``lookahead`` frames at the end of a clip, mirroring, BVH text
parsing.  Inherited from the reference: a character facing exactly -z is singular; contacts flip at a hard speed threshold.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence

import torch

from . import _C
from .generator import Generator, _dev_f32, _ptr, _stream
from .skeleton import LAYOUT_ID

AXES = {"x": 0, "y": 1, "z": 2}


class IngestConfig:
    """``mocha_ingest_cfg``: ``lookahead`` 0..18 frames; ``order``: the Euler channel order as a BVH file holds it ('zyx', ...), degrees,
    or None for quaternion input (w,x,y,z); ``unit_scale`` (0.01: cm -> m), ``fps``, ``contact_velocity_threshold`` (m/s); the role joints
    ``spine``, ``shoulder_l``, ``shoulder_r``, ``upleg_l``, ``upleg_r`` as raw joint indices (default: the layout's)."""

    def __init__(self, lookahead: int = 0, order: Optional[str] = "zyx", unit_scale: float = 0.01, fps: float = 60.0,
                 contact_velocity_threshold: float = 0.5, **roles):
        self.lookahead, self.order = int(lookahead), order
        self.unit_scale, self.fps, self.threshold = float(unit_scale), float(fps), float(contact_velocity_threshold)
        for k in roles:
            if k not in ("spine", "shoulder_l", "shoulder_r", "upleg_l", "upleg_r"):
                raise TypeError(f"unknown ingest option {k!r}")
        self.roles = {k: int(v) for k, v in roles.items()}
        if order is not None and (len(order) != 3 or any(a not in AXES for a in order)):
            raise ValueError("IngestConfig: order is three of 'x', 'y', 'z', or None for quaternions")

    @staticmethod
    def of(raw) -> "IngestConfig":
        return raw if isinstance(raw, IngestConfig) else IngestConfig(lookahead=int(raw))

    def struct(self, model: Generator) -> _C.mocha_ingest_cfg:
        cfg = _C.mocha_ingest_cfg()
        model._ctx.lib.mocha_ingest_cfg_default(C.byref(cfg), LAYOUT_ID[model.layout])
        cfg.lookahead = self.lookahead
        cfg.rot_format = 0 if self.order is None else 1
        for i, a in enumerate(self.order or "zyx"):
            cfg.euler_order[i] = AXES[a]
        cfg.unit_scale, cfg.fps, cfg.contact_velocity_threshold = self.unit_scale, self.fps, self.threshold
        for k, v in self.roles.items():
            setattr(cfg, k, v)
        return cfg


class Ingestor:
    """The standalone stepper (parallel to ``Inertializer`` and ``PostProcessor.step``): ``streams`` independent streams on ``model``'s
    context.  ``post``: the post-processing constants whose ``contact_bones`` are the toes (default: the demo's)."""

    def __init__(self, model: Generator, raw=0, streams: int = 1, post=None):
        from .postprocess import PostProcessor
        if not 1 <= int(streams) <= 16:
            raise ValueError("streams must be 1..16")
        self.model, self.streams = model, int(streams)
        self.post = post or PostProcessor(model)
        self.config = IngestConfig.of(raw)
        self.cfg = self.config.struct(model)
        S, J, dev = self.streams, model.V + 1, model.device
        nbytes = int(model._ctx.lib.mocha_ingest_state_bytes(model._ctx.h, S))
        if nbytes <= 0:
            raise RuntimeError("mocha_ingest_state_bytes failed")
        self.state = torch.zeros((nbytes,), dtype=torch.uint8, device=dev)          # zeroed = no frame seen
        self.width = 3 if self.cfg.rot_format == 1 else 4
        f32 = lambda *shape: torch.zeros(shape, dtype=torch.float32, device=dev)    # noqa: E731
        self.rot, self.pos = f32(S, model.V, self.width), f32(S, model.V, 3)
        self.out = {"Yrot": f32(S, J, 4), "Ypos": f32(S, J, 3), "Yvel": f32(S, J, 3), "Yang": f32(S, J, 3), "src_rvel": f32(S, 3),
                    "src_rang": f32(S, 3), "src_speed": f32(S),
                    "contact": torch.zeros((S, max(int(self.post.cfg.n_contact), 1)), dtype=torch.uint8, device=dev),
                    "have": torch.zeros((S,), dtype=torch.int32, device=dev)}

    def _frame(self, a, buf, name):
        t = _dev_f32(a, buf.device, None, name)
        if t.numel() != buf.numel():
            raise ValueError(f"Ingestor.step: {name} has {t.numel()} values, expected {tuple(buf.shape)}")
        buf.copy_(t.reshape(buf.shape), non_blocking=True)

    def step(self, rot, pos):
        """The new raw frame of every stream: rot (S,V,3) Euler degrees or (S,V,4) quaternions, pos (S,V,3).  Returns the stepper's own
        device tensors - Yrot (S,V+1,4), Ypos / Yvel / Yang (S,V+1,3), src_rvel / src_rang (S,3), src_speed (S,), contact (S,n_contact)
        uint8, have (S,) int32 - overwritten by the next step; rows of a stream with have == 0 are not written.  No host synchronisation."""
        self._frame(rot, self.rot, "rot")
        self._frame(pos, self.pos, "pos")
        return self.replay()

    def replay(self):
        """The step on what the fixed buffers ``rot`` / ``pos`` hold."""
        o = self.out
        self.model._ctx.call("mocha_live_ingest_step", C.byref(self.cfg), C.byref(self.post.cfg), _ptr(self.state), self.streams, _ptr(self.rot),
                             _ptr(self.pos), _ptr(o["Yrot"]), _ptr(o["Ypos"]), _ptr(o["Yvel"]), _ptr(o["Yang"]), _ptr(o["src_rvel"]),
                             _ptr(o["src_rang"]), _ptr(o["src_speed"]), _ptr(o["contact"]), _ptr(o["have"]), _stream())
        return o

    def reset(self, streams: Optional[Sequence[int]] = None):
        """All streams, or the listed ones, have seen no frame."""
        reset_ingest(self.model, self.state, self.streams, streams)
        return self


def reset_ingest(model: Generator, state: torch.Tensor, n_streams: int, streams: Optional[Sequence[int]] = None):
    if streams is None:
        model._ctx.call("mocha_ingest_reset", _ptr(state), n_streams, None, 0, _stream())
    else:
        ids = [int(s) for s in streams]
        arr = (C.c_int32 * max(len(ids), 1))(*ids)
        model._ctx.call("mocha_ingest_reset", _ptr(state), n_streams, arr, len(ids), _stream())
