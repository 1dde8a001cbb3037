"""The mocap front end of a live session on the device (``mocha_live_ingest_step``): raw frames in, the live step's inputs out.

A mocap device delivers, per frame, the local rotations and local positions of the skeleton's joints.  The live step takes what the
reference's ``process_data`` makes of a whole clip - a synthetic root bone, velocities, foot contacts - with filters that read frames
after the one they produce.  ``Ingestor`` is that preparation in streaming form: one raw frame per call and stream, and from the 31st
push on every call emits frame ``n-1-lookahead`` of ``process_data`` applied to the frames pushed so far.  ``lookahead=18`` gives the
whole clip's frame 0.3 s late; ``lookahead=0`` the newest frame under the reference's clip-end rules.  ``LiveSession(raw=...)`` runs it
inside the session's captured graph.  A stream never emits the last ``lookahead`` frames of a clip and does not mirror: whole clips go
through ``ingest_clips`` (``mocha_ingest_clips``: every frame of every clip, plain or mirrored as ``animation_mirror`` does, parallel over
frames) and ``clip_windows`` (``divide_clip``), the first link of raw clip -> ``bank.build_database_from_clips`` -> bank and of raw clip
pair -> windows -> ``featurize`` -> ``characterize_pair``.  BVH files are read by ``bvh.load_bvh``.  Inherited from the reference: a character
facing exactly -z is singular; contacts flip at a hard speed threshold.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence

import numpy as np
import torch

from . import _C
from .generator import Generator, _dev_f32, _ptr, _stream
from .skeleton import LAYOUT_ID

AXES = {"x": 0, "y": 1, "z": 2}


class IngestConfig:
    """``mocha_ingest_cfg``: ``lookahead`` 0..18 frames; ``order``: the Euler channel order as a BVH file holds it ('zyx', ...), degrees,
    or None for quaternion input (w,x,y,z); ``unit_scale`` (0.01: cm -> m), ``fps``, ``contact_velocity_threshold`` (m/s); the role joints
    ``spine``, ``shoulder_l``, ``shoulder_r``, ``upleg_l``, ``upleg_r`` as raw joint indices (default: the layout's).  ``mirror_map``
    (``ingest_clips`` only): the joint exchange of a mirrored clip, V ints with map[map[v]] == v; None = the layout's left / right
    exchange (``mocha_mirror_map_default``)."""

    def __init__(self, lookahead: int = 0, order: Optional[str] = "zyx", unit_scale: float = 0.01, fps: float = 60.0,
                 contact_velocity_threshold: float = 0.5, mirror_map=None, **roles):
        self.lookahead, self.order = int(lookahead), order
        self.mirror_map = None if mirror_map is None else [int(v) for v in mirror_map]
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


class ProcessedClips(dict):
    """``ingest_clips``'s result: the dict of device tensors, plus the model whose context made them (``clip_windows`` runs there)."""
    model: Optional[Generator] = None


def default_mirror_map(layout: str):
    """The left / right joint exchange of a layout (``mocha_mirror_map_default``)."""
    m = (C.c_int32 * 32)()
    if _C.load_library().mocha_mirror_map_default(LAYOUT_ID[layout], m) != 0:
        raise ValueError(f"no mirror map for layout {layout!r}")
    return [int(m[v]) for v in range(22 if LAYOUT_ID[layout] == 1 else 24)]


def _offsets(lengths):
    off = np.concatenate([[0], np.cumsum(np.asarray(lengths, dtype=np.int64))])
    if len(off) < 2 or off[-1] >= 2 ** 31:
        raise ValueError("lengths: at least one clip and fewer than 2^31 frames in all")
    return (C.c_int32 * len(off))(*[int(v) for v in off]), int(off[-1])


def ingest_clips(model: Generator, rot, pos, lengths, raw=IngestConfig(), mirror=None, post=None):
    """Whole clips through the reference's ``process_data`` on the device (``mocha_ingest_clips``).  ``rot`` (F,V,3) Euler degrees in
    ``raw.order`` or (F,V,4) quaternions, ``pos`` (F,V,3): the clips concatenated along the frame axis, ``lengths`` their frame counts
    (each at least 31).  ``mirror``: per clip, truthy = mirrored first (``animation_mirror`` with ``raw.mirror_map``); None = no clip.
    ``post``: the post-processing constants whose ``contact_bones`` are the toes (default: the demo's).  Returns device tensors, root
    bone first: ``pos`` / ``vel`` / ``ang`` (F,V+1,3), ``rot`` (F,V+1,4) fp32, ``contact`` (F,n_contact) uint8.  Every frame of every
    clip is there; nothing crosses a clip boundary.  Waits for the current stream once (the tables' upload); not for graph capture.
    The dict is a ``ProcessedClips``: it remembers ``model`` for ``clip_windows``."""
    from .postprocess import PostProcessor
    post = post or PostProcessor(model)
    cfg = IngestConfig.of(raw)
    st = cfg.struct(model)
    width = 3 if st.rot_format == 1 else 4
    V, J, dev = model.V, model.V + 1, model.device
    off, F = _offsets(lengths)
    r = _dev_f32(rot, dev, (V, width), "rot")
    p = _dev_f32(pos, dev, (V, 3), "pos")
    if r.numel() != F * V * width or p.numel() != F * V * 3:
        raise ValueError(f"ingest_clips: rot / pos do not hold the {F} frames of lengths")
    n = len(lengths)
    flags = None
    if mirror is not None:
        if len(mirror) != n:
            raise ValueError("ingest_clips: one mirror flag per clip")
        flags = (C.c_ubyte * n)(*[1 if m else 0 for m in mirror])
    mp = cfg.mirror_map if cfg.mirror_map is not None else (default_mirror_map(model.layout) if flags is not None else None)
    if mp is not None and len(mp) != V:
        raise ValueError(f"ingest_clips: mirror_map needs {V} entries")
    mp_arr = None if mp is None else (C.c_int32 * V)(*mp)
    nc = max(int(post.cfg.n_contact), 1)
    f32 = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)    # noqa: E731
    out = ProcessedClips({"pos": f32(F, J, 3), "vel": f32(F, J, 3), "rot": f32(F, J, 4), "ang": f32(F, J, 3),
                          "contact": torch.zeros((F, nc), dtype=torch.uint8, device=dev)})
    out.model = model
    model._ctx.call("mocha_ingest_clips", C.byref(st), C.byref(post.cfg), _ptr(r), _ptr(p), off, n, mp_arr, flags, _ptr(out["pos"]),
                    _ptr(out["vel"]), _ptr(out["rot"]), _ptr(out["ang"]), _ptr(out["contact"]), _stream())
    return out


def clip_window_counts(lengths, window: int = 60, step: int = 1):
    """Windows per clip as ``divide_clip(divide=True)`` cuts them (``mocha_clip_window_count``)."""
    off, _ = _offsets(lengths)
    counts = (C.c_int64 * len(lengths))()
    if _C.load_library().mocha_clip_window_count(off, len(lengths), int(window), int(step), counts) != 0:
        raise ValueError("clip_window_counts: window must be at least 4, step at least 1, every length positive")
    return [int(v) for v in counts]


def clip_windows(processed, lengths, window: int = 60, step: int = 1, model: Optional[Generator] = None):
    """``divide_clip(divide=True)`` of processed clips in one launch (``mocha_clip_windows``).  ``processed``: ``ingest_clips``'s dict, or
    any dict of pos / vel / ang (F,V+1,3), rot (F,V+1,4) fp32 and contact (F,n_contact) uint8 together with ``model``.
    Returns ``Yrot`` (B,window,V+1,4), ``Ypos`` / ``Yvel`` / ``Yang`` (B,window,V+1,3) as ``featurize`` takes them and ``contact``
    (B,window,n_contact), clip after clip; short slices padded with their first / last frame, ``Yvel`` / ``Yang`` padding zero."""
    model = model or getattr(processed, "model", None)
    if model is None:
        raise ValueError("clip_windows: processed is not ingest_clips's result; pass model=")
    off, F = _offsets(lengths)
    J, dev = model.V + 1, model.device
    B = sum(clip_window_counts(lengths, window, step))
    src = {k: _dev_f32(processed[k], dev, (J, w), k) for k, w in (("pos", 3), ("vel", 3), ("rot", 4), ("ang", 3))}
    con = processed["contact"]
    if con.dtype != torch.uint8 or any(t.shape[0] != F for t in src.values()) or con.shape[0] != F:
        raise ValueError(f"clip_windows: processed does not hold the {F} frames of lengths (contact uint8)")
    con = con.to(dev).contiguous()
    nc = int(con.shape[1])
    f32 = lambda w: torch.empty((B, window, J, w), dtype=torch.float32, device=dev)    # noqa: E731
    out = {"Yrot": f32(4), "Ypos": f32(3), "Yvel": f32(3), "Yang": f32(3),
           "contact": torch.zeros((B, window, nc), dtype=torch.uint8, device=dev)}
    model._ctx.call("mocha_clip_windows", _ptr(src["pos"]), _ptr(src["vel"]), _ptr(src["rot"]), _ptr(src["ang"]), _ptr(con), nc, off,
                    len(lengths), int(window), int(step), _ptr(out["Yrot"]), _ptr(out["Ypos"]), _ptr(out["Yvel"]), _ptr(out["Yang"]),
                    _ptr(out["contact"]), _stream())
    return out


# ---------------------------------------------------------------------------------------------------------------- resampling
def _fraction(x, what):
    from fractions import Fraction
    if isinstance(x, Fraction):
        f = x
    elif isinstance(x, (int, np.integer)):
        f = Fraction(int(x))
    else:
        f = Fraction(float(x)).limit_denominator(1000)
    if f <= 0:
        raise ValueError(f"{what} must be positive")
    return f


def resample_ratio(source_fps, target_fps=60.0):
    """The step between outputs in source frames, ``source_fps / target_fps`` reduced to (num, den), each 1..4096.  Ints, floats or
    ``Fraction``s; a float goes through ``Fraction(x).limit_denominator(1000)``."""
    r = _fraction(source_fps, "source_fps") / _fraction(target_fps, "target_fps")
    if r.numerator > 4096 or r.denominator > 4096:
        raise ValueError(f"resampling: {source_fps} -> {target_fps} fps reduces to {r.numerator}/{r.denominator}; each term must be at most 4096")
    return r.numerator, r.denominator


def _ratios(n_clips, source_fps, target_fps):
    from fractions import Fraction
    if isinstance(source_fps, (int, float, np.integer, np.floating, Fraction)):
        source_fps = [source_fps] * n_clips
    if len(source_fps) != n_clips:
        raise ValueError("resampling: source_fps is one value, or one per clip")
    return [resample_ratio(s, target_fps) for s in source_fps]


def resample_lengths(lengths, source_fps, target_fps=60.0):
    """Frames per clip after resampling (``mocha_resample_frames``): ``floor((n-1) * den / num) + 1`` with num/den = source/target."""
    lib = _C.load_library()
    out = []
    for n, (num, den) in zip(lengths, _ratios(len(lengths), source_fps, target_fps)):
        m = int(lib.mocha_resample_frames(int(n), num, den))
        if m < 1:
            raise ValueError(f"resample_lengths: a clip of {n} frames cannot be resampled (every clip needs at least one frame)")
        out.append(m)
    return out


def resample_clips(model: Generator, rot, pos, lengths, source_fps, target_fps=60.0, order="zyx"):
    """Whole clips from ``source_fps`` to ``target_fps`` on the device (``mocha_resample_clips``).  ``rot`` (F,V,3) Euler degrees in
    ``order`` or, with ``order=None``, (F,V,4) quaternions; ``pos`` (F,V,3) in the file's units; the clips concatenated along the frame
    axis, ``lengths`` their frame counts (a clip may have one frame).  ``source_fps``: one value, or one per clip.  Returns
    ``(rot_q (F',V,4), pos (F',V,3), new_lengths)``: unit quaternions w,x,y,z sign-unrolled along time and positions, fp32 on the device -
    what ``ingest_clips(..., raw=IngestConfig(order=None, fps=target_fps))`` takes.  Output k of a clip sits k * source / target source
    frames in: on a source frame it is that frame, between two it turns at constant angular velocity (slerp) and moves linearly.  No
    low-pass filter before decimation, no cubic interpolation.  Waits for the current stream once; not for graph capture."""
    if order is not None and (len(order) != 3 or sorted(order) != ["x", "y", "z"]):
        raise ValueError("resample_clips: order is a permutation of 'xyz', or None for quaternions")
    width = 4 if order is None else 3
    V, dev = model.V, model.device
    off, F = _offsets(lengths)
    n = len(lengths)
    ratios = _ratios(n, source_fps, target_fps)
    new_lengths = resample_lengths(lengths, source_fps, target_fps)
    off_out, F_out = _offsets(new_lengths)
    r = _dev_f32(rot, dev, (V, width), "rot")
    p = _dev_f32(pos, dev, (V, 3), "pos")
    if r.numel() != F * V * width or p.numel() != F * V * 3:
        raise ValueError(f"resample_clips: rot / pos do not hold the {F} frames of lengths")
    rot_q = torch.empty((F_out, V, 4), dtype=torch.float32, device=dev)
    pos_o = torch.empty((F_out, V, 3), dtype=torch.float32, device=dev)
    eo = (C.c_int * 3)(*[AXES[a] for a in (order or "zyx")])
    model._ctx.call("mocha_resample_clips", 0 if order is None else 1, eo, _ptr(r), _ptr(p), off, (C.c_int32 * n)(*[a for a, _ in ratios]),
                    (C.c_int32 * n)(*[b for _, b in ratios]), n, off_out, _ptr(rot_q), _ptr(pos_o), _stream())
    return rot_q, pos_o, new_lengths


class StreamResampler:
    """The streaming form (``mocha_resample_step``; parallel to ``Ingestor`` and ``Inertializer``): ``streams`` streams of one source
    rate, advancing in lockstep.  ``push(rot, pos)`` takes the new source frame of every stream - rot (S,V,3) Euler degrees in ``order``
    or, with ``order=None``, (S,V,4) quaternions; pos (S,V,3) - and returns how many output frames it produced (a host int, 0..4, known
    without asking the device); they are ``out["rot"][:, :n]`` (S,4,V,4) and ``out["pos"][:, :n]`` (S,4,V,3), overwritten by the next push.
    The outputs of all pushes, concatenated, are ``resample_clips`` of the pushed frames bit for bit.  One launch per push in front of a
    quaternion-input session: ``for e in range(n): session.push_raw(out["rot"][:, e], out["pos"][:, e])``.  A source more than four times
    slower than the target is refused."""

    def __init__(self, model: Generator, source_fps, target_fps=60.0, order="zyx", streams: int = 1):
        if not 1 <= int(streams) <= 16:
            raise ValueError("streams must be 1..16")
        if order is not None and (len(order) != 3 or sorted(order) != ["x", "y", "z"]):
            raise ValueError("StreamResampler: order is a permutation of 'xyz', or None for quaternions")
        self.model, self.streams, self.order = model, int(streams), order
        self.num, self.den = resample_ratio(source_fps, target_fps)
        if self.den > 4 * self.num:
            raise ValueError(f"StreamResampler: {source_fps} -> {target_fps} fps gives more than 4 outputs per source frame")
        S, V, dev = self.streams, model.V, model.device
        nbytes = int(model._ctx.lib.mocha_resample_state_bytes(model._ctx.h, S))
        if nbytes <= 0:
            raise RuntimeError("mocha_resample_state_bytes failed")
        self.state = torch.zeros((nbytes,), dtype=torch.uint8, device=dev)          # zeroed = no frame seen
        self.width = 4 if order is None else 3
        f32 = lambda *shape: torch.zeros(shape, dtype=torch.float32, device=dev)    # noqa: E731
        self.rot, self.pos = f32(S, V, self.width), f32(S, V, 3)
        self.out = {"rot": f32(S, 4, V, 4), "pos": f32(S, 4, V, 3)}
        self._order = (C.c_int * 3)(*[AXES[a] for a in (order or "zyx")])
        self.pushes = 0

    def _frame(self, a, buf, name):
        t = _dev_f32(a, buf.device, None, name)
        if t.numel() != buf.numel():
            raise ValueError(f"StreamResampler.push: {name} has {t.numel()} values, expected {tuple(buf.shape)}")
        buf.copy_(t.reshape(buf.shape), non_blocking=True)

    def push(self, rot, pos) -> int:
        self._frame(rot, self.rot, "rot")
        self._frame(pos, self.pos, "pos")
        return self.replay()

    def replay(self) -> int:
        """The push on what the fixed buffers ``rot`` / ``pos`` hold."""
        n = C.c_int32(0)
        self.model._ctx.call("mocha_resample_step", 0 if self.order is None else 1, self._order, _ptr(self.state), self.streams,
                             _ptr(self.rot), _ptr(self.pos), self.num, self.den, self.pushes, _ptr(self.out["rot"]), _ptr(self.out["pos"]),
                             C.byref(n), _stream())
        self.pushes += 1
        return int(n.value)

    def restart(self, streams: Optional[Sequence[int]] = None):
        """The listed streams (None = all) forget their previous frame: every output of their next push is the new frame itself.  The
        output schedule goes on in lockstep."""
        ids = None if streams is None else [int(s) for s in streams]
        arr = None if ids is None else (C.c_int32 * max(len(ids), 1))(*ids)
        self.model._ctx.call("mocha_resample_reset", _ptr(self.state), self.streams, arr, 0 if ids is None else len(ids), _stream())
        return self

    def reset(self):
        """All streams have seen no frame, and the next push is push 0."""
        self.restart()
        self.pushes = 0
        return self
