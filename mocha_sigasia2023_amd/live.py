"""Live sessions: one mocap frame in, one characterized, root-integrated, foot-locked pose out (``mocha_live_step``).

A ``LiveSession`` keeps, per stream, the last 60 frames of local bone data in a ring on the device, and the state of the demo's frame
loop (root transform, blended positions, contact records).  ``push`` copies the new frame of every stream into fixed buffers and
replays ONE captured HIP graph: ring push + featurize -> segmented characterize of the streams' windows, every stream against its own
character of a ``MultiCharacterBank`` -> pose heads -> one post-processing frame.  Nothing is computed on the host and nothing
synchronises; a stream that has not seen 60 frames yet is reported as ``valid == 0`` and its output rows are left as they were.

A ``LiveOursSession`` is the same loop with the CVAE ("Ours") branch inside the graph (``mocha_live_step_ours``): the decoder reads a
character feature sampled from the stream's previous one, the autoregressive state and the sampler's noise staying on the device.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence

import numpy as np
import torch

from . import _C
from .generator import DIM, NTOK, CoherentMatch, _dev_f32, _ptr, _stream
from .multi_character import MIX_PARTS, MultiCharacterBank, OnlinePath, _refuse_with_mix, mix_count, mix_tensors, soft_params
from .ingest import IngestConfig, reset_ingest
from .postprocess import PostProcessor
from .world import SkinBind, _launch as _world_launch


class LiveSession:
    """``streams`` live streams (1..16) on ``bank``'s context.  ``post``: the post-processing constants (default: the demo's);
    ``bvh``: also produce the BVH writer's channels.  Needs ``Generator.set_pose_norm``.  ``soft=(k, temperature)``: every stream's decoder
    reads the softmax(-dist / temperature)-weighted blend of its k nearest entries instead of the nearest one (``mocha_live_step_soft``):
    no pop when two entries are nearly equidistant; the outputs gain ``idx_k`` (S,k) and ``weight`` (S,k), ``idx`` is column 0.
    ``inertial=halflife`` (seconds): a stream that names another character does not pop - the jump of its pose heads becomes an offset
    that decays with that half-life (``mocha_live_step_inert``: the reference's inertializers, state and decision on the device, the frame
    time taken from ``post``); a stream that never switches gets the bits of ``inertial=None``.
    ``raw=IngestConfig(...)`` or ``raw=lookahead``: the session also takes RAW mocap frames (``push_raw``: local rotations and positions of
    the V joints) - the mocap front end (``ingest.py``, ``mocha_live_step_raw``) runs inside the same captured graph and produces what
    ``push`` takes; a stream emits its first frame on its 31st raw push, so ``valid`` first becomes 1 on push 90.
    ``constrained=True`` (a bank with action labels): every stream carries a 64-bit allow mask of admissible actions in ``self.allow``
    ((S,) int64 on the device; ``push(..., allow=)``, ``set_allow`` or written in place) and is matched among its character's entries of those actions
    (``mocha_live_step_allow`` / ``mocha_live_step_raw_allow``); the outputs gain ``applied`` (S,): 1 constrained, 0 nothing asked or
    warming, -1 the character has no such entry and the whole character was searched.  With zero masks the session gives the plain
    session's bits.  A change of the allowed actions is not inertialized (``soft=`` softens it).
    ``mix=J`` (1 .. 4): every stream is characterized by up to J (character, six body-part weights) components instead of one character
    (``mocha_live_step_mix`` / ``mocha_live_step_raw_mix``): ``mix_ids`` (S,J) int32 and ``mix_weights`` (S,J,6) float32 are device tensors
    the captured step reads - ``push(..., mix=(ids, weights))``, ``set_mix`` or written in place, e.g. a weight ramp for a cross-fade or a
    0/1 mask per body part for a splice; ``characters`` is not used.  ``idx`` is then (S,J) and the outputs gain ``weight`` (S,J,6), the
    weights normalised per body part.  A stream none of whose components is present (no loaded character with a usable weight) sits the
    step out as a warming one.  Combines with ``raw=``; not with ``soft``, ``inertial`` or ``constrained``.
    ``world=SkinBind(...)`` or ``world=True``: every push also gives the frame in WORLD space - the outputs gain ``gpos`` (S,V+1,3) and
    ``grot`` (S,V+1,4) float64, the reference's ``quat.fk`` of ``pos`` and ``ik_rot``, and with a bind ``palette`` (S,V,12) fp32, the 3x4
    skinning matrices ``pre . world . inverse(bind)`` of bones 1..V in one buffer a renderer can bind (``world.py``).  ONE
    ``mocha_world_pose`` launch BEHIND the captured graph, on the same stream, reads ``out["pos"]``, ``out["ik_rot"]`` and ``out["valid"]``
    - it is not a node of the graph, as the resampler sits in front of the graph and not in it - so the step's capture, its key and every
    existing output are what they are without ``world``.  Fixed tensors, overwritten by the next push; rows of a warming stream are not
    written; no host synchronisation.  The default ``None`` leaves everything as it is.
    ``coherent=jump`` (a number, or a ``CoherentMatch`` without ``relative``): coherent matching, one step of the path per pushed frame
    (``mocha_live_step_path`` / ``mocha_live_step_raw_path``; ``OnlinePath``).  A session pushes one stride-1 window per step against a bank
    of stride-1 windows of smooth clips, so the right answer for consecutive pushes is almost always "the next row": every transition
    that is not "next row of the same clip" pays ``jump``, in the units of the matcher's distances (a live stream has no clip to take a
    median from, so ``relative=True`` raises: run ``query_path(..., relative=True)`` on a recorded clip for a unit).  The clip starts are
    the bank's (``MultiCharacterBank(starts=)`` / ``set_starts``, ``ResidentCharacterBank.add(starts=)``).  The outputs gain ``dist`` (S,)
    fp32 and ``continued`` (S,) uint8; ``self.restart`` (S,) int32 on the device restarts a stream's path where it is non-zero (written
    in place, cleared by the step).  A stream restarts on its own when its character changes or is replaced and after ``reset``.
    ``coherent=0`` gives the plain session's bits on an fp32 bank.  Combines with ``raw=`` and ``world=``; not with ``soft``,
    ``inertial``, ``constrained`` or ``mix``."""

    def __init__(self, bank: MultiCharacterBank, cnt_mean, cnt_std, streams: int = 1, post: Optional[PostProcessor] = None, bvh: bool = True,
                 soft=None, inertial: Optional[float] = None, raw=None, constrained: bool = False, mix=None, world=None, coherent=None):
        if not 1 <= int(streams) <= 16:
            raise ValueError("streams must be 1..16")
        if coherent is not None:
            co = CoherentMatch.of(coherent)
            if co.relative:
                raise ValueError("LiveSession: coherent= takes an absolute jump penalty - a live stream has no clip to take a median from; "
                                 "run query_path(..., relative=True) on a recorded clip for the unit")
            if co.bank_starts is not None or co.src_starts is not None:
                raise ValueError("LiveSession: the clip starts of a live session are the bank's (MultiCharacterBank(starts=), add(starts=))")
            for name, v in (("soft", soft is not None), ("inertial", inertial is not None), ("constrained", constrained), ("mix", mix is not None)):
                if v:
                    raise ValueError(f"LiveSession: coherent= does not combine with {name}")
        self.mix = None
        if mix is not None:
            self.mix = mix_count(mix, "LiveSession")
            _refuse_with_mix("LiveSession", soft=soft is not None, inertial=inertial is not None, constrained=constrained)
        self.bank, self.model = bank, bank.model
        m, dev = self.model, bank.model.device
        if post is not None and post.model is not m:
            raise ValueError("LiveSession: post belongs to another model")
        self.post = post or PostProcessor(m)
        self.streams = S = int(streams)
        self.bvh = bool(bvh)
        self.soft = soft_params(soft, "LiveSession")
        self.mean = _dev_f32(cnt_mean, dev, (NTOK, DIM), "cnt_mean")
        self.std = _dev_f32(cnt_std, dev, (NTOK, DIM), "cnt_std")
        J, V = m.V + 1, m.V
        self.n_contact = max(int(self.post.cfg.n_contact), 1)
        nbytes = int(m._ctx.lib.mocha_live_state_bytes(m._ctx.h, S))
        if nbytes <= 0:
            raise RuntimeError("mocha_live_state_bytes failed")
        self.live = torch.zeros((nbytes,), dtype=torch.uint8, device=dev)          # zeroed = a reset session
        self.inert = self.icfg = None
        if inertial is not None:
            if not (float(inertial) >= 0.0 and float(inertial) != float("inf")):
                raise ValueError("LiveSession: inertial is a half-life in seconds, finite and >= 0")
            ibytes = int(m._ctx.lib.mocha_inert_state_bytes(m._ctx.h))
            if ibytes <= 0:
                raise RuntimeError("mocha_inert_state_bytes failed")
            self.inert = torch.zeros((S, ibytes), dtype=torch.uint8, device=dev)   # zeroed = no stream has seen a frame
            self.icfg = _C.mocha_inert_cfg(float(inertial), float(self.post.cfg.dt))
        self.raw = self.rcfg = self.ingest = None
        if raw is not None:
            self.raw = IngestConfig.of(raw)
            self.rcfg = self.raw.struct(m)
            rbytes = int(m._ctx.lib.mocha_ingest_state_bytes(m._ctx.h, S))
            if rbytes <= 0:
                raise RuntimeError("mocha_ingest_state_bytes failed")
            self.ingest = torch.zeros((rbytes,), dtype=torch.uint8, device=dev)        # zeroed = no raw frame seen
            self.raw_rot = torch.zeros((S, V, 3 if self.rcfg.rot_format == 1 else 4), dtype=torch.float32, device=dev)
            self.raw_pos = torch.zeros((S, V, 3), dtype=torch.float32, device=dev)

        def f32(*shape):
            return torch.zeros(shape, dtype=torch.float32, device=dev)
        # the fixed input buffers the captured step reads ...
        self.rot, self.pos, self.vel, self.ang = f32(S, J, 4), f32(S, J, 3), f32(S, J, 3), f32(S, J, 3)
        self.rvel, self.rang, self.speed = f32(S, 3), f32(S, 3), f32(S)
        self.contact = torch.zeros((S, self.n_contact), dtype=torch.uint8, device=dev)
        self.ids = torch.zeros((S,), dtype=torch.int32, device=dev)
        # ... and the outputs it writes
        f64 = lambda *shape: torch.zeros(shape, dtype=torch.float64, device=dev)   # noqa: E731
        self.out = {"pos": f64(S, J, 3), "rot": f64(S, J, 4), "ik_rot": f64(S, J, 4)}
        if self.bvh:
            self.out["bvh_pos"], self.out["bvh_euler"] = f64(S, V, 3), f64(S, V, 3)
        self.out["idx"] = torch.full((S,), -1, dtype=torch.int32, device=dev)
        self.out["valid"] = torch.zeros((S,), dtype=torch.int32, device=dev)
        if self.soft is not None:
            self.out["idx_k"] = torch.full((S, self.soft[0]), -1, dtype=torch.int32, device=dev)
            self.out["weight"] = torch.zeros((S, self.soft[0]), dtype=torch.float32, device=dev)
        self.constrained = bool(constrained)
        if self.constrained:
            if bank.labels is None:
                raise RuntimeError("LiveSession: constrained=True needs a bank with action labels (MultiCharacterBank(labels=))")
            self.allow = torch.zeros((S,), dtype=torch.int64, device=dev)
            self.out["applied"] = torch.zeros((S,), dtype=torch.int32, device=dev)
        if self.mix is not None:
            self.mix_ids = torch.full((S, self.mix), -1, dtype=torch.int32, device=dev)
            self.mix_weights = torch.zeros((S, self.mix, MIX_PARTS), dtype=torch.float32, device=dev)
            self.out["idx"] = torch.full((S, self.mix), -1, dtype=torch.int32, device=dev)
            self.out["weight"] = torch.zeros((S, self.mix, MIX_PARTS), dtype=torch.float32, device=dev)
        self.world = self.world_bind = None
        if world is not None and world is not False:
            if world is not True and not isinstance(world, SkinBind):
                raise TypeError("LiveSession: world is a SkinBind, True (global poses, no palette) or None")
            if world is not True and world.model is not m:
                raise ValueError("LiveSession: world belongs to another model")
            self.world, self.world_bind = True, (None if world is True else world)
            self.out["gpos"], self.out["grot"] = f64(S, J, 3), f64(S, J, 4)
            if self.world_bind is not None:
                self.out["palette"] = f32(S, V, 12)
        self.path = None
        if coherent is not None:
            self.path = OnlinePath(bank, S, CoherentMatch.of(coherent).jump)
            self.restart = self.path.restart
            self.out["dist"], self.out["continued"] = self.path.dist, self.path.continued
        bank._ensure()

    @property
    def characters(self) -> torch.Tensor:
        """The step's own character ids (streams,) int32 on the device: a producer may write them in place."""
        return self.ids

    def _frame(self, a, buf, name):
        t = _dev_f32(a, buf.device, None, name)
        if t.numel() != buf.numel():
            raise ValueError(f"LiveSession.push: {name} has {t.numel()} values, expected {tuple(buf.shape)}")
        buf.copy_(t.reshape(buf.shape), non_blocking=True)

    def set_allow(self, allow):
        """New allow masks for the next step (constrained sessions), one per stream - an int mask, an iterable of labels or None each, or
        one int for all; checked on the host, copied into ``self.allow``.  ``push(..., allow=)`` calls this; before ``push_raw`` call it
        yourself (or write ``self.allow`` in place)."""
        if not self.constrained:
            raise RuntimeError("LiveSession: allow= needs a session created with constrained=True")
        self.allow.copy_(self.bank._allow(allow, self.streams, "LiveSession"), non_blocking=True)

    def set_mix(self, mix):
        """New (ids, weights) for the next step (mix sessions; see ``mix_tensors``), copied into ``mix_ids`` / ``mix_weights``.
        ``push(..., mix=)`` calls this; before ``push_raw`` call it yourself (or write the two tensors in place)."""
        if self.mix is None:
            raise RuntimeError("LiveSession: mix= needs a session created with mix=J")
        mids, mw = mix_tensors(mix, self.streams, self.model.device, "LiveSession", self.mix)
        self.mix_ids.copy_(mids, non_blocking=True)
        self.mix_weights.copy_(mw, non_blocking=True)

    def _set_characters(self, characters):
        if self.mix is not None:
            raise ValueError("LiveSession: a mix session takes mix=, not characters")
        self.ids.copy_(self.bank._ids(characters, self.streams), non_blocking=True)

    def push(self, Yrot, Ypos, Yvel, Yang, src_rvel, src_rang, src_speed, contact, characters=None, allow=None, mix=None):
        """The new frame of every stream: Yrot (S,V+1,4) (w,x,y,z), Ypos / Yvel / Yang (S,V+1,3), root bone first; src_rvel / src_rang
        (S,3), src_speed (S,), contact (S,n_contact) of that frame [, characters: one id per stream; default: the ids already set].
        Returns the session's own device tensors - pos (S,V+1,3), rot / ik_rot (S,V+1,4), (bvh_pos / bvh_euler (S,V,3)), idx (S,) the
        matched row local to the stream's character (-1 while warming up), valid (S,) - overwritten by the next push.  Rows of a stream
        with valid == 0 are not written.  No host synchronisation.  ``allow`` (constrained sessions): new allow masks, one per stream -
        an int mask, an iterable of labels or None each, or one int for all; default: the masks already set."""
        if allow is not None:
            self.set_allow(allow)
        if mix is not None:
            self.set_mix(mix)
        if characters is not None:
            self._set_characters(characters)
        for a, buf, name in ((Yrot, self.rot, "Yrot"), (Ypos, self.pos, "Ypos"), (Yvel, self.vel, "Yvel"), (Yang, self.ang, "Yang"),
                             (src_rvel, self.rvel, "src_rvel"), (src_rang, self.rang, "src_rang")):
            self._frame(a, buf, name)
        self._frame(torch.as_tensor(src_speed, dtype=torch.float32).reshape(-1), self.speed, "src_speed")
        ct = torch.as_tensor(contact).to(device=self.contact.device, dtype=torch.uint8)
        if ct.numel() != self.contact.numel():
            raise ValueError(f"LiveSession.push: contact has {ct.numel()} values, expected {tuple(self.contact.shape)}")
        self.contact.copy_(ct.reshape(self.contact.shape), non_blocking=True)
        return self.replay()

    def push_raw(self, rot, pos, characters=None):
        """The new RAW frame of every stream (``raw=`` sessions): rot (S,V,3) Euler degrees in the configured order or (S,V,4) quaternions
        (w,x,y,z), pos (S,V,3) in the configured unit, joint 0 the hips [, characters].  Returns what ``push`` returns; the frame behind
        it is frame ``n-1-lookahead`` of the stream.  No host synchronisation."""
        if self.raw is None:
            raise RuntimeError("LiveSession.push_raw: the session was not created with raw=")
        if characters is not None:
            self._set_characters(characters)
        self._frame(rot, self.raw_rot, "rot")
        self._frame(pos, self.raw_pos, "pos")
        return self.replay_raw()

    def replay_raw(self):
        """The raw step on what ``raw_rot`` / ``raw_pos`` hold (a producer on the device may have written them in place)."""
        return self._world_pose(self._step_raw())

    def _step_raw(self):
        if self.raw is None:
            raise RuntimeError("LiveSession.replay_raw: the session was not created with raw=")
        self.bank._ensure()
        o = self.out
        k, t = self.soft if self.soft is not None else (0, 0.0)
        if self.path is not None:
            p = self.path
            self.model._ctx.call("mocha_live_step_raw_path", C.byref(self.post.cfg), C.byref(self.rcfg), _ptr(self.live), _ptr(self.ingest),
                                 self.streams, _ptr(self.raw_rot), _ptr(self.raw_pos), _ptr(self.ids), _ptr(self.mean), _ptr(self.std),
                                 _ptr(o["pos"]), _ptr(o["rot"]), _ptr(o["ik_rot"]), _ptr(o["bvh_pos"]) if self.bvh else None,
                                 _ptr(o["bvh_euler"]) if self.bvh else None, _ptr(o["idx"]), _ptr(o["valid"]), _stream(), _ptr(p.state),
                                 p.state_rows, C.c_double(p.jump), _ptr(p.restart), _ptr(p.dist), _ptr(p.continued))
            return o
        if self.mix is not None:
            self.model._ctx.call("mocha_live_step_raw_mix", C.byref(self.post.cfg), C.byref(self.rcfg), _ptr(self.live), _ptr(self.ingest),
                                 self.streams, _ptr(self.raw_rot), _ptr(self.raw_pos), _ptr(self.mix_ids), _ptr(self.mix_weights), self.mix,
                                 _ptr(self.mean), _ptr(self.std), _ptr(o["pos"]), _ptr(o["rot"]), _ptr(o["ik_rot"]),
                                 _ptr(o["bvh_pos"]) if self.bvh else None, _ptr(o["bvh_euler"]) if self.bvh else None, _ptr(o["idx"]),
                                 _ptr(o["valid"]), _ptr(o["weight"]), _stream())
            return o
        if self.constrained:
            self.model._ctx.call("mocha_live_step_raw_allow", C.byref(self.post.cfg), C.byref(self.rcfg), _ptr(self.live), _ptr(self.ingest),
                                 self.streams, _ptr(self.raw_rot), _ptr(self.raw_pos), _ptr(self.ids), _ptr(self.mean), _ptr(self.std), k, t,
                                 _ptr(o["pos"]), _ptr(o["rot"]), _ptr(o["ik_rot"]), _ptr(o["bvh_pos"]) if self.bvh else None,
                                 _ptr(o["bvh_euler"]) if self.bvh else None, _ptr(o["idx"]), _ptr(o["valid"]), _ptr(o.get("idx_k")),
                                 _ptr(o.get("weight")), _stream(), _ptr(self.inert) if self.inert is not None else None,
                                 C.byref(self.icfg) if self.icfg is not None else None, _ptr(self.allow), _ptr(o["applied"]))
            return o
        self.model._ctx.call("mocha_live_step_raw", C.byref(self.post.cfg), C.byref(self.rcfg), _ptr(self.live), _ptr(self.ingest), self.streams,
                             _ptr(self.raw_rot), _ptr(self.raw_pos), _ptr(self.ids), _ptr(self.mean), _ptr(self.std), k, t, _ptr(o["pos"]),
                             _ptr(o["rot"]), _ptr(o["ik_rot"]), _ptr(o["bvh_pos"]) if self.bvh else None,
                             _ptr(o["bvh_euler"]) if self.bvh else None, _ptr(o["idx"]), _ptr(o["valid"]), _ptr(o.get("idx_k")),
                             _ptr(o.get("weight")), _stream(), _ptr(self.inert) if self.inert is not None else None,
                             C.byref(self.icfg) if self.icfg is not None else None)
        return o

    def replay(self):
        """The step on what the fixed buffers hold (a producer on the device may have written them in place)."""
        return self._world_pose(self._step())

    def _world_pose(self, o):
        """``world=``: one ``mocha_world_pose`` launch behind the captured step, on its stream, from the frame the step just wrote."""
        if self.world is not None:
            _world_launch(self.model, o["ik_rot"], o["pos"], self.streams, o["valid"], self.world_bind, o["gpos"], o["grot"], o.get("palette"))
        return o

    def _step(self):
        self.bank._ensure()
        o = self.out
        if self.path is not None:
            p = self.path
            self.model._ctx.call("mocha_live_step_path", C.byref(self.post.cfg), _ptr(self.live), self.streams, _ptr(self.rot), _ptr(self.pos),
                                 _ptr(self.vel), _ptr(self.ang), _ptr(self.rvel), _ptr(self.rang), _ptr(self.speed), _ptr(self.contact),
                                 _ptr(self.ids), _ptr(self.mean), _ptr(self.std), _ptr(o["pos"]), _ptr(o["rot"]), _ptr(o["ik_rot"]),
                                 _ptr(o["bvh_pos"]) if self.bvh else None, _ptr(o["bvh_euler"]) if self.bvh else None, _ptr(o["idx"]),
                                 _ptr(o["valid"]), _stream(), _ptr(p.state), p.state_rows, C.c_double(p.jump), _ptr(p.restart), _ptr(p.dist),
                                 _ptr(p.continued))
            return o
        if self.mix is not None:
            self.model._ctx.call("mocha_live_step_mix", C.byref(self.post.cfg), _ptr(self.live), self.streams, _ptr(self.rot), _ptr(self.pos),
                                 _ptr(self.vel), _ptr(self.ang), _ptr(self.rvel), _ptr(self.rang), _ptr(self.speed), _ptr(self.contact),
                                 _ptr(self.mix_ids), _ptr(self.mix_weights), self.mix, _ptr(self.mean), _ptr(self.std), _ptr(o["pos"]),
                                 _ptr(o["rot"]), _ptr(o["ik_rot"]), _ptr(o["bvh_pos"]) if self.bvh else None,
                                 _ptr(o["bvh_euler"]) if self.bvh else None, _ptr(o["idx"]), _ptr(o["valid"]), _ptr(o["weight"]), _stream())
            return o
        if self.constrained:
            k, t = self.soft if self.soft is not None else (0, 0.0)
            self.model._ctx.call("mocha_live_step_allow", C.byref(self.post.cfg), _ptr(self.live), self.streams, _ptr(self.rot), _ptr(self.pos),
                                 _ptr(self.vel), _ptr(self.ang), _ptr(self.rvel), _ptr(self.rang), _ptr(self.speed), _ptr(self.contact),
                                 _ptr(self.ids), _ptr(self.mean), _ptr(self.std), k, t, _ptr(o["pos"]), _ptr(o["rot"]),
                                 _ptr(o["ik_rot"]), _ptr(o["bvh_pos"]) if self.bvh else None, _ptr(o["bvh_euler"]) if self.bvh else None,
                                 _ptr(o["idx"]), _ptr(o["valid"]), _ptr(o.get("idx_k")), _ptr(o.get("weight")), _stream(),
                                 _ptr(self.inert) if self.inert is not None else None, C.byref(self.icfg) if self.icfg is not None else None,
                                 _ptr(self.allow), _ptr(o["applied"]))
            return o
        if self.inert is not None:
            k, t = self.soft if self.soft is not None else (0, 0.0)
            self.model._ctx.call("mocha_live_step_inert", C.byref(self.post.cfg), _ptr(self.live), self.streams, _ptr(self.rot), _ptr(self.pos),
                                 _ptr(self.vel), _ptr(self.ang), _ptr(self.rvel), _ptr(self.rang), _ptr(self.speed), _ptr(self.contact),
                                 _ptr(self.ids), _ptr(self.mean), _ptr(self.std), k, t, _ptr(o["pos"]), _ptr(o["rot"]),
                                 _ptr(o["ik_rot"]), _ptr(o["bvh_pos"]) if self.bvh else None, _ptr(o["bvh_euler"]) if self.bvh else None,
                                 _ptr(o["idx"]), _ptr(o["valid"]), _ptr(o.get("idx_k")), _ptr(o.get("weight")), _stream(), _ptr(self.inert),
                                 C.byref(self.icfg))
            return o
        if self.soft is not None:
            self.model._ctx.call("mocha_live_step_soft", C.byref(self.post.cfg), _ptr(self.live), self.streams, _ptr(self.rot), _ptr(self.pos),
                                 _ptr(self.vel), _ptr(self.ang), _ptr(self.rvel), _ptr(self.rang), _ptr(self.speed), _ptr(self.contact),
                                 _ptr(self.ids), _ptr(self.mean), _ptr(self.std), self.soft[0], self.soft[1], _ptr(o["pos"]), _ptr(o["rot"]),
                                 _ptr(o["ik_rot"]), _ptr(o["bvh_pos"]) if self.bvh else None, _ptr(o["bvh_euler"]) if self.bvh else None,
                                 _ptr(o["idx"]), _ptr(o["valid"]), _ptr(o["idx_k"]), _ptr(o["weight"]), _stream())
            return o
        self.model._ctx.call("mocha_live_step", C.byref(self.post.cfg), _ptr(self.live), self.streams, _ptr(self.rot), _ptr(self.pos), _ptr(self.vel),
                             _ptr(self.ang), _ptr(self.rvel), _ptr(self.rang), _ptr(self.speed), _ptr(self.contact), _ptr(self.ids),
                             _ptr(self.mean), _ptr(self.std), _ptr(o["pos"]), _ptr(o["rot"]), _ptr(o["ik_rot"]),
                             _ptr(o["bvh_pos"]) if self.bvh else None, _ptr(o["bvh_euler"]) if self.bvh else None, _ptr(o["idx"]), _ptr(o["valid"]),
                             _stream())
        return o

    def reset(self, streams: Optional[Sequence[int]] = None):
        """All streams, or the listed ones, start over: their rings warm up again and their next valid frame is a first frame."""
        ctx = self.model._ctx
        if streams is None:
            ctx.call("mocha_live_reset", _ptr(self.live), self.streams, None, 0, _stream())
        else:
            ids = [int(s) for s in streams]
            arr = (C.c_int32 * max(len(ids), 1))(*ids)
            ctx.call("mocha_live_reset", _ptr(self.live), self.streams, arr, len(ids), _stream())
        if self.ingest is not None:
            reset_ingest(self.model, self.ingest, self.streams, streams)
        return self

    def run_clip_raw(self, rot, pos, characters=None):
        """Convenience: pushes the F raw frames of every stream's clip - rot (S,F,V,3|4), pos (S,F,V,3) - into a RESET session and returns
        the stacked valid frames: a dict of (S, F - 89, ...) tensors.  The last ``lookahead`` frames of the clip are not produced."""
        dev = self.model.device
        rot = torch.as_tensor(rot).to(device=dev, dtype=torch.float32)
        pos = torch.as_tensor(pos).to(device=dev, dtype=torch.float32)
        F = rot.shape[1]
        if F < 90:
            raise ValueError("run_clip_raw: a clip needs at least 90 frames")
        self.reset()
        keep = [k for k in self.out if k != "valid"]
        frames = {k: [] for k in keep}
        for f in range(F):
            o = self.push_raw(rot[:, f], pos[:, f], characters if f == 0 else None)
            if f >= 89:
                for k in keep:
                    frames[k].append(o[k].clone())
        return {k: torch.stack(v, dim=1) for k, v in frames.items()}

    def run_clip(self, Yrot, Ypos, Yvel, Yang, src_rvel, src_rang, src_speed, contact, characters=None):
        """Convenience: pushes the F frames of every stream's clip - Yrot (S,F,V+1,4), Ypos / Yvel / Yang (S,F,V+1,3); src_rvel /
        src_rang (S,F,3), src_speed (S,F), contact (S,F,n_contact), frame f being the inputs of the push of frame f - into a RESET
        session and returns the stacked valid frames: a dict of (S, F - 59, ...) tensors (idx (S, F - 59))."""
        dev, S = self.model.device, self.streams
        to = lambda a, dt: torch.as_tensor(a).to(device=dev, dtype=dt)             # noqa: E731
        rot, pos, vel, ang, rv, ra = (to(a, torch.float32) for a in (Yrot, Ypos, Yvel, Yang, src_rvel, src_rang))
        sp = to(src_speed, torch.float32).reshape(S, -1)
        F = rot.shape[1]
        ct = to(contact, torch.uint8).reshape(S, F, -1)
        if F < 60:
            raise ValueError("run_clip: a clip needs at least 60 frames")
        self.reset()
        keep = [k for k in self.out if k != "valid"]
        frames = {k: [] for k in keep}
        for f in range(F):
            o = self.push(rot[:, f], pos[:, f], vel[:, f], ang[:, f], rv[:, f], ra[:, f], sp[:, f], ct[:, f], characters if f == 0 else None)
            if f >= 59:
                for k in keep:
                    frames[k].append(o[k].clone())
        return {k: torch.stack(v, dim=1) for k, v in frames.items()}


class LiveOursSession(LiveSession):
    """A ``LiveSession`` whose decoder reads the CVAE ("Ours") branch's character feature (``mocha_live_step_ours``;
    test_fullframework.py:446-457): per stream the feature is seeded with the matched bank row on the first valid frame - that frame is
    ``LiveSession``'s frame - and from then on sampled from the previous one, the autoregressive state staying on the device.  A stream
    that is reset, or whose character changes, seeds again.

    ``cvae_state_dict`` is loaded into the model's own context (``Generator.load_cvae``): ONE CVAE, with its four (90,256) statistics,
    serves every stream of the model, while streams may still name different characters of the bank.  ``cvae_state_dict=None`` keeps
    the CVAE the model already has: loading one synchronises the device and makes every captured graph of the model capture again,
    so further sessions on a model should pass None.  ``noise``: ``"device"`` draws the
    sampler's noise on the device from ``seed`` (Philox4x32-10 counted by stream and frame: the same seed repeats the session),
    ``"given"`` reads ``sess.eps`` (S,256), which the caller writes before a push, ``"none"`` takes z = mu.  ``push`` / ``replay`` /
    ``run_clip`` / ``reset`` as in ``LiveSession``; the outputs gain ``seeded`` (S,) int32: 1 where the frame was a seed frame.

    ``cvaes=CVAEBank(...)``: ONE CVAE PER CHARACTER instead (``mocha_live_step_ours_grouped``).  The session owns ``self.cvae_of``, a
    device int32 tensor with one entry per character of the bank - the character's slot of ``cvaes`` - initialised from ``cvae_of``
    (default: all -1); ``set_cvae(character, slot)`` writes an entry in place, and so may a producer on the device: no new capture.  A
    stream samples with its character's CVAE and statistics; a stream whose character has none (-1, a slot outside the bank, a cleared
    or never stored slot) falls back to plain context matching - every valid frame is a seed frame.  ``cvae_state_dict`` and the four
    statistics must then be None."""

    NOISE = {"none": 0, "given": 1, "device": 2}

    def __init__(self, bank: MultiCharacterBank, cnt_mean, cnt_std, cvae_state_dict, src_cnt_mean, src_cnt_std, cha_encoded_mean,
                 cha_encoded_std, streams: int = 1, post: Optional[PostProcessor] = None, bvh: bool = True, noise: str = "device",
                 seed: int = 0, soft=None, inertial=None, raw=None, constrained: bool = False, cvaes=None, cvae_of=None, mix=None, world=None):
        if cvaes is None and cvae_of is not None:
            raise ValueError("LiveOursSession: cvae_of needs cvaes=CVAEBank(...)")
        if cvaes is not None:
            if cvaes.model is not bank.model:
                raise ValueError("LiveOursSession: cvaes belongs to another model")
            if any(a is not None for a in (cvae_state_dict, src_cnt_mean, src_cnt_std, cha_encoded_mean, cha_encoded_std)):
                raise ValueError("LiveOursSession: with cvaes= the CVAEs and their statistics come from the bank - pass None for "
                                 "cvae_state_dict and the four statistics")
        if constrained:
            raise ValueError("LiveOursSession: constrained=True is not supported - the branch's seed match searches the whole character")
        if raw is not None:
            raise ValueError("LiveOursSession: raw= is not supported - the CVAE branch's step has no mocap front end; run an Ingestor and "
                             "push its emitted frames")
        if inertial is not None:
            raise ValueError("LiveOursSession: inertial does not apply - the branch seeds again on a character switch and keeps its own chain state")
        if soft is not None:
            raise ValueError("LiveOursSession: soft matching does not apply - the decoder already reads a sampled character feature")
        if mix is not None:
            raise ValueError("LiveOursSession: mix= is not supported - the CVAE branch samples one character's feature per stream")
        if noise not in self.NOISE:
            raise ValueError(f"noise must be one of {sorted(self.NOISE)}")
        super().__init__(bank, cnt_mean, cnt_std, streams=streams, post=post, bvh=bvh, world=world)
        m, dev, S = self.model, self.model.device, self.streams
        self.cvaes, self.cvae_of = cvaes, None
        if cvaes is not None:
            of = torch.full((bank.S,), -1, dtype=torch.int32) if cvae_of is None else torch.as_tensor(cvae_of).to(torch.int32).reshape(-1).cpu()
            if of.numel() != bank.S:
                raise ValueError(f"LiveOursSession: cvae_of has {of.numel()} entries, the bank has {bank.S} characters")
            self.cvae_of = of.to(dev)
            self.stats = []
        else:
            if cvae_state_dict is not None:
                m.load_cvae(cvae_state_dict)
            elif not getattr(m, "_cvae_loaded", False):
                raise RuntimeError("LiveOursSession: cvae_state_dict=None needs a CVAE on the model (Generator.load_cvae)")
            self.stats = [_dev_f32(a, dev, (NTOK, DIM), n) for a, n in ((src_cnt_mean, "src_cnt_mean"), (src_cnt_std, "src_cnt_std"),
                                                                       (cha_encoded_mean, "cha_encoded_mean"), (cha_encoded_std, "cha_encoded_std"))]
        nbytes = int(m._ctx.lib.mocha_live_ours_state_bytes(m._ctx.h, S))
        if nbytes <= 0:
            raise RuntimeError("mocha_live_ours_state_bytes failed")
        self.ours = torch.zeros((nbytes,), dtype=torch.uint8, device=dev)          # zeroed = every stream seeds on its first valid frame
        self.eps = torch.zeros((S, DIM), dtype=torch.float32, device=dev)
        self.noise, self.seed = noise, int(seed) & 0xFFFFFFFFFFFFFFFF
        self.ocfg = _C.mocha_ours_cfg(*([t.data_ptr() for t in self.stats] or [None] * 4), self.NOISE[noise], self.eps.data_ptr(), self.seed)
        self.out["seeded"] = torch.zeros((S,), dtype=torch.int32, device=dev)
        at = ((S * 12 + 255) // 256) * 256                                          # `prev` follows the counters (include/mocha_hip.h)
        self._prev = self.ours[at: at + S * NTOK * DIM * 4].view(torch.float32).reshape(S, NTOK, DIM)

    @property
    def cha_encoded(self) -> torch.Tensor:
        """The streams' current character features (S,90,256): a view of the state the next step conditions on."""
        return self._prev

    def set_cvae(self, character: int, slot: int):
        """Character ``character`` samples with slot ``slot`` of the CVAE bank from the next step on (-1: no CVAE - plain context
        matching).  An in-place device write on the current stream: no new capture, and a chaining stream does not seed again."""
        if self.cvae_of is None:
            raise RuntimeError("LiveOursSession.set_cvae: the session was not created with cvaes=")
        if not 0 <= int(character) < self.cvae_of.numel():
            raise ValueError(f"LiveOursSession.set_cvae: character {character} out of range 0 .. {self.cvae_of.numel() - 1}")
        self.cvae_of[int(character)].fill_(int(slot))
        return self

    def _step(self):
        self.bank._ensure()
        o = self.out
        if self.cvae_of is not None:
            self.model._ctx.call("mocha_live_step_ours_grouped", C.byref(self.post.cfg), _ptr(self.live), self.streams, _ptr(self.rot),
                                 _ptr(self.pos), _ptr(self.vel), _ptr(self.ang), _ptr(self.rvel), _ptr(self.rang), _ptr(self.speed),
                                 _ptr(self.contact), _ptr(self.ids), _ptr(self.mean), _ptr(self.std), _ptr(self.ours), C.byref(self.ocfg),
                                 _ptr(self.cvae_of), _ptr(o["pos"]), _ptr(o["rot"]), _ptr(o["ik_rot"]), _ptr(o["bvh_pos"]) if self.bvh else None,
                                 _ptr(o["bvh_euler"]) if self.bvh else None, _ptr(o["idx"]), _ptr(o["valid"]), _ptr(o["seeded"]), _stream())
            return o
        self.model._ctx.call("mocha_live_step_ours", C.byref(self.post.cfg), _ptr(self.live), self.streams, _ptr(self.rot), _ptr(self.pos),
                             _ptr(self.vel), _ptr(self.ang), _ptr(self.rvel), _ptr(self.rang), _ptr(self.speed), _ptr(self.contact),
                             _ptr(self.ids), _ptr(self.mean), _ptr(self.std), _ptr(self.ours), C.byref(self.ocfg), _ptr(o["pos"]),
                             _ptr(o["rot"]), _ptr(o["ik_rot"]), _ptr(o["bvh_pos"]) if self.bvh else None,
                             _ptr(o["bvh_euler"]) if self.bvh else None, _ptr(o["idx"]), _ptr(o["valid"]), _ptr(o["seeded"]), _stream())
        return o

    def reset(self, streams: Optional[Sequence[int]] = None):
        """All streams, or the listed ones, start over: they warm up again and their next valid frame is a seed frame."""
        ctx = self.model._ctx
        if streams is None:
            ctx.call("mocha_live_ours_reset", _ptr(self.live), _ptr(self.ours), self.streams, None, 0, _stream())
        else:
            ids = [int(s) for s in streams]
            arr = (C.c_int32 * max(len(ids), 1))(*ids)
            ctx.call("mocha_live_ours_reset", _ptr(self.live), _ptr(self.ours), self.streams, arr, len(ids), _stream())
        return self
