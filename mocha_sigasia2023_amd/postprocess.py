"""Host mirror of the demo's post-processing: decoded windows -> animated skeleton -> BVH.

``pose_heads``, ``PostProcessor.run`` and ``PostProcessor.step`` call the HIP kernels of csrc/postprocess.hip through the C ABI; nothing here
computes on the host except the hierarchy lines of ``write_bvh`` (the reference's motion/bvh.py:179-224 layout): with ``model=`` the numbers
of the MOTION block are formatted on the device too (``format_bvh_motion``, ``write_bvh_clips``; csrc/bvh_format.hip), without it on the host.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence

import numpy as np
import torch

from . import _C
from .generator import Generator, _dev_f32, _ptr, _stream


class PostCfg(C.Structure):
    """``mocha_post_cfg`` of include/mocha_hip.h; defaults are the demo's constants (test_fullframework.py:104-114)."""
    _fields_ = [("dt", C.c_double), ("ik_max_length_buffer", C.c_double), ("ik_foot_height", C.c_double),
                ("ik_unlock_radius", C.c_double), ("ik_blending_halflife", C.c_double),
                ("ik_enabled", C.c_int), ("n_contact", C.c_int), ("contact_bones", C.c_int * 4), ("blend_enabled", C.c_int)]


def pose_heads(model: Generator, Y):
    """Y (B,60,V,15) de-normalised -> (heads (B,V,13) = [pos | quat wxyz | vel | ang] of the last frame, speed (B,))."""
    Y = _dev_f32(Y, model.device, (model.cfg["nframes"], model.V, model.cfg["mot_in_dim"]), "Y")
    B = Y.shape[0]
    heads = torch.empty((B, model.V, 13), dtype=torch.float32, device=model.device)
    speed = torch.empty((B,), dtype=torch.float32, device=model.device)
    model._ctx.call("mocha_pose_heads", _ptr(Y), B, _ptr(heads), _ptr(speed), _stream())
    return heads, speed


class PostProcessor:
    """Root integration + blending + foot-lock IK on the device, one wave per clip: whole clips (``run``) or one frame per call with
    the loop's state kept in a device tensor (``state`` / ``step``)."""

    def __init__(self, model: Generator, contact_bones: Optional[Sequence[int]] = None, ik_enabled: bool = True, blend: bool = True, **ik):
        self.model = model
        self.cfg = PostCfg()
        model._ctx.lib.mocha_post_cfg_default(C.byref(self.cfg))
        if contact_bones is not None:
            if len(contact_bones) > 4:
                raise ValueError("at most 4 contact bones")
            self.cfg.n_contact = len(contact_bones)
            for i, b in enumerate(contact_bones):
                self.cfg.contact_bones[i] = int(b)
        self.cfg.ik_enabled = int(ik_enabled)
        self.cfg.blend_enabled = int(blend)     # blend=False, ik_enabled=False: the demo's "cm_" stream (test_fullframework.py:512-527, 637-641)
        for k, v in ik.items():
            if k not in ("dt", "ik_max_length_buffer", "ik_foot_height", "ik_unlock_radius", "ik_blending_halflife"):
                raise TypeError(f"unknown post-processing option {k!r}")
            setattr(self.cfg, k, float(v))

    def run(self, heads, speed, src_rvel, src_rang, src_speed, contact, bvh: bool = True):
        """One clip (N, ...) or a batch of clips (C, N, ...).  Returns a dict of float64 device tensors:
        pos (.., N, V+1, 3), rot / ik_rot (.., N, V+1, 4) and, with ``bvh``, bvh_pos / bvh_euler (.., N, V, 3)."""
        m, dev, V = self.model, self.model.device, self.model.V
        heads = torch.as_tensor(heads)
        single = heads.dim() == 3
        lead = () if single else (heads.shape[0],)

        def f32(a, tail, name):
            return _dev_f32(torch.as_tensor(a).reshape((-1,) + tail), dev, None, name)
        N = heads.shape[-3]
        nclip = 1 if single else heads.shape[0]
        h = f32(heads, (V, 13), "heads")
        sp, ssp = f32(speed, (), "speed"), f32(src_speed, (), "src_speed")
        rv, ra = f32(src_rvel, (3,), "src_rvel"), f32(src_rang, (3,), "src_rang")
        nc = self.cfg.n_contact
        ct = torch.as_tensor(contact).to(device=dev, dtype=torch.uint8).reshape(-1, max(nc, 1)).contiguous()
        rows = nclip * N
        for t, name in ((h, "heads"), (sp, "speed"), (ssp, "src_speed"), (rv, "src_rvel"), (ra, "src_rang"), (ct, "contact")):
            if t.shape[0] != rows:
                raise ValueError(f"postprocess: {name} has {t.shape[0]} rows, expected {rows}")
        out = {"pos": torch.empty(lead + (N, V + 1, 3), dtype=torch.float64, device=dev),
               "rot": torch.empty(lead + (N, V + 1, 4), dtype=torch.float64, device=dev),
               "ik_rot": torch.empty(lead + (N, V + 1, 4), dtype=torch.float64, device=dev)}
        if bvh:
            out["bvh_pos"] = torch.empty(lead + (N, V, 3), dtype=torch.float64, device=dev)
            out["bvh_euler"] = torch.empty(lead + (N, V, 3), dtype=torch.float64, device=dev)
        m._ctx.call("mocha_postprocess", C.byref(self.cfg), _ptr(h), _ptr(sp), _ptr(rv), _ptr(ra), _ptr(ssp), _ptr(ct), nclip, N,
                    _ptr(out["pos"]), _ptr(out["rot"]), _ptr(out["ik_rot"]),
                    _ptr(out["bvh_pos"]) if bvh else None, _ptr(out["bvh_euler"]) if bvh else None, _stream())
        return out


    def state(self, n_clips: int = 1) -> torch.Tensor:
        """A zeroed state for ``step``: (n_clips, mocha_post_state_bytes) uint8 on the device.  All-zero bytes mean "no frame seen
        yet", so ``state.zero_()`` (or zeroing one clip's row) is a reset, and ``state.clone()`` / ``state.copy_`` a snapshot / rollback."""
        ctx = self.model._ctx
        nbytes = int(ctx.lib.mocha_post_state_bytes(ctx.h))
        if nbytes <= 0:
            raise RuntimeError("mocha_post_state_bytes failed")
        return torch.zeros((int(n_clips), nbytes), dtype=torch.uint8, device=self.model.device)

    def step(self, state, heads, speed, src_rvel, src_rang, src_speed, contact, bvh: bool = True, out: Optional[dict] = None):
        """ONE frame of every clip of ``state`` (``mocha_postprocess_step``): heads (V,13) or (C,V,13), speed / src_speed () or (C,),
        src_rvel / src_rang (3,) or (C,3), contact (n_contact,) or (C,n_contact) of the current frame.  Advances ``state`` in place and
        returns the same dict as ``run`` for that one frame: pos (.., V+1, 3), rot / ik_rot (.., V+1, 4), bvh_pos / bvh_euler (.., V, 3).
        Stepping a clip frame by frame from a zeroed state gives exactly what ``run`` gives for the whole clip.  ``out``: a dict of
        tensors from an earlier call to write into (fixed buffers, e.g. under graph capture)."""
        m, dev, V = self.model, self.model.device, self.model.V
        if not (isinstance(state, torch.Tensor) and state.dtype == torch.uint8 and state.dim() == 2 and state.is_contiguous()
                and state.device == dev):
            raise ValueError("postprocess step: state must come from PostProcessor.state()")
        nclip = state.shape[0]
        heads = torch.as_tensor(heads)
        single = heads.dim() == 2
        if single and nclip != 1:
            raise ValueError(f"postprocess step: heads of one clip for a state of {nclip}")
        lead = () if single else (nclip,)

        def f32(a, tail, name):
            return _dev_f32(torch.as_tensor(a).reshape((-1,) + tail), dev, None, name)
        h = f32(heads, (V, 13), "heads")
        sp, ssp = f32(speed, (), "speed"), f32(src_speed, (), "src_speed")
        rv, ra = f32(src_rvel, (3,), "src_rvel"), f32(src_rang, (3,), "src_rang")
        nc = self.cfg.n_contact
        ct = torch.as_tensor(contact).to(device=dev, dtype=torch.uint8).reshape(-1, max(nc, 1)).contiguous()
        for t, name in ((h, "heads"), (sp, "speed"), (ssp, "src_speed"), (rv, "src_rvel"), (ra, "src_rang"), (ct, "contact")):
            if t.shape[0] != nclip:
                raise ValueError(f"postprocess step: {name} has {t.shape[0]} rows, expected {nclip}")
        if out is None:
            out = {"pos": torch.empty(lead + (V + 1, 3), dtype=torch.float64, device=dev),
                   "rot": torch.empty(lead + (V + 1, 4), dtype=torch.float64, device=dev),
                   "ik_rot": torch.empty(lead + (V + 1, 4), dtype=torch.float64, device=dev)}
            if bvh:
                out["bvh_pos"] = torch.empty(lead + (V, 3), dtype=torch.float64, device=dev)
                out["bvh_euler"] = torch.empty(lead + (V, 3), dtype=torch.float64, device=dev)
        bvh = "bvh_pos" in out
        m._ctx.call("mocha_postprocess_step", C.byref(self.cfg), _ptr(state), _ptr(h), _ptr(sp), _ptr(rv), _ptr(ra), _ptr(ssp), _ptr(ct), nclip,
                    _ptr(out["pos"]), _ptr(out["rot"]), _ptr(out["ik_rot"]),
                    _ptr(out["bvh_pos"]) if bvh else None, _ptr(out["bvh_euler"]) if bvh else None, _stream())
        return out


class Inertializer:
    """The reference's per-bone inertializers (motion/Inertialization.py:71-91) on the pose heads, on the device
    (``mocha_inertialize_step``): when a stream names another character, or is told so by ``trigger``, the jump between its previous
    heads and the new ones becomes an offset that decays with half-life ``halflife`` (seconds; ``dt`` seconds per frame) instead of
    popping.  The root bone is not part of the heads and is not inertialized: the frame loop integrates it from its own output."""

    def __init__(self, model: Generator, halflife: float = 0.1, dt: float = 1.0 / 60.0):
        self.model = model
        self.cfg = _C.mocha_inert_cfg(float(halflife), float(dt))

    def state(self, n: int = 1) -> torch.Tensor:
        """A zeroed state for ``step``: (n, mocha_inert_state_bytes) uint8 on the device.  All-zero bytes are a reset stream, so
        ``state.zero_()`` (or zeroing one row) is a reset and ``state.clone()`` / ``state.copy_`` a snapshot / rollback."""
        ctx = self.model._ctx
        nbytes = int(ctx.lib.mocha_inert_state_bytes(ctx.h))
        if nbytes <= 0:
            raise RuntimeError("mocha_inert_state_bytes failed")
        return torch.zeros((int(n), nbytes), dtype=torch.uint8, device=self.model.device)

    def step(self, state, heads, ids=None, trigger=None, valid=None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """ONE frame of the n streams of ``state``: heads (n,V,13) fp32 as ``pose_heads`` gives them -> the inertialized heads (n,V,13),
        written to ``out`` (which may be ``heads`` itself).  ids / trigger / valid: (n,) int32, each optional - a stream transitions when
        its id differs from the one of its previous valid frame or its trigger is non-zero; a stream with valid == 0 is left untouched
        and its state cleared.  A stream that never transitions gets its input back bit for bit."""
        m, dev, V = self.model, self.model.device, self.model.V
        if not (isinstance(state, torch.Tensor) and state.dtype == torch.uint8 and state.dim() == 2 and state.is_contiguous()
                and state.device == dev):
            raise ValueError("inertializer step: state must come from Inertializer.state()")
        n = state.shape[0]
        h = _dev_f32(torch.as_tensor(heads), dev, (V, 13), "heads")
        if h.numel() != n * V * 13:
            raise ValueError(f"inertializer step: heads {tuple(h.shape)} for a state of {n} streams")
        if out is None:
            out = torch.empty((n, V, 13), dtype=torch.float32, device=dev)
        elif not (out.dtype == torch.float32 and out.device == dev and out.is_contiguous() and out.numel() == n * V * 13):
            raise ValueError("inertializer step: out must be a contiguous float32 (n,V,13) tensor on the model's device")

        def i32(a, name):
            if a is None:
                return None
            t = torch.as_tensor(a).to(device=dev, dtype=torch.int32).reshape(-1).contiguous()
            if t.numel() != n:
                raise ValueError(f"inertializer step: {name} has {t.numel()} entries, expected {n}")
            return t
        ids, trigger, valid = i32(ids, "ids"), i32(trigger, "trigger"), i32(valid, "valid")
        m._ctx.call("mocha_inertialize_step", C.byref(self.cfg), _ptr(state), _ptr(h), _ptr(out), _ptr(ids), _ptr(trigger), _ptr(valid), n,
                    _stream())
        return out


def retarget_clip(bank, src_X, cnt_mean, cnt_std, src_rvel, src_rang, src_speed, contact, raw: bool = False,
                  post: Optional[PostProcessor] = None, bvh: bool = True, coherent=None):
    """The NN branch of the demo from featurised source windows to the animated skeleton, all on the device:
    characterize (encode, match, decode, to_mot; test_fullframework.py:438-443, 465-467) -> pose heads (:457-462) ->
    root integration / blending / foot-lock IK (:492-632) -> BVH channels (:677-681, 697).  ``src_X`` must lead to
    de-normalised windows: pass ``raw=True`` after ``Generator.set_pose_norm`` or de-normalise the result yourself.
    src_speed (N,) is mean_t |src_Yvel[i, t, 1]| (:493).  ``coherent``: ``ContextBank.characterize``'s (None: the hard match)."""
    Y = bank.characterize(src_X, cnt_mean, cnt_std, raw=raw) if coherent is None else \
        bank.characterize(src_X, cnt_mean, cnt_std, raw=raw, coherent=coherent)
    heads, speed = pose_heads(bank.model, Y)
    return (post or PostProcessor(bank.model)).run(heads, speed, src_rvel, src_rang, src_speed, contact, bvh=bvh)


def retarget_clip_ours(session, src_encoded, src_cnt, src_rvel, src_rang, src_speed, contact, eps=None, deterministic: bool = False,
                       post: Optional[PostProcessor] = None, bvh: bool = True, denorm=None):
    """The demo's CVAE ("Ours") branch for a whole clip (test_fullframework.py:446-457 per frame, then :474-632): the
    autoregressive frame loop through ``OursSession`` (already ``reset`` with the first matched character feature), then the
    pose heads and the post-processing of all frames at once.  src_encoded / src_cnt (N,90,256); ``eps`` (N,256) fixes the
    sampler's noise; ``denorm`` = (Y_mean, Y_std) broadcastable to (60,V,15) de-normalises the decoded windows as :457 does."""
    m = session.model
    N = src_encoded.shape[0]
    Ys = []
    for i in range(N):
        y, _ = session.step(src_encoded[i], src_cnt[i], eps=None if eps is None else eps[i:i + 1], deterministic=deterministic)
        Ys.append(y.clone())                    # the session returns views of buffers that the next step overwrites
    Y = torch.cat(Ys)
    if denorm is not None:
        mean, std = (torch.as_tensor(a, dtype=torch.float32, device=m.device) for a in denorm)
        Y = Y * std + mean
    heads, speed = pose_heads(m, Y)
    return (post or PostProcessor(m)).run(heads, speed, src_rvel, src_rang, src_speed, contact, bvh=bvh)


def retarget_frame_ours(session, post_state, src_encoded, src_cnt, src_rvel, src_rang, src_speed, contact, eps=None,
                        deterministic: bool = False, post: Optional[PostProcessor] = None, bvh: bool = True, denorm=None):
    """``retarget_clip_ours`` one frame at a time: one ``OursSession.step`` (test_fullframework.py:446-457), the pose heads of the
    decoded window and ONE frame of the post-processing (:492-632, 677-681) whose state lives in ``post_state``
    (``PostProcessor.state(B)``, zeroed before the clip's first frame) - a posed frame per call, no decoded window is kept.
    src_encoded / src_cnt (90,256) or (B,90,256); the per-frame inputs as for ``PostProcessor.step``; the result has a leading
    clip dimension B (1 for a single clip).  The same frames through ``retarget_clip_ours`` give the same poses."""
    m = session.model
    Y, _ = session.step(src_encoded, src_cnt, eps=eps, deterministic=deterministic)
    if denorm is not None:
        mean, std = (torch.as_tensor(a, dtype=torch.float32, device=m.device) for a in denorm)
        Y = Y * std + mean
    heads, speed = pose_heads(m, Y)
    return (post or PostProcessor(m)).step(post_state, heads, speed, src_rvel, src_rang, src_speed, contact, bvh=bvh)


_CHANNEL = {"x": "Xrotation", "y": "Yrotation", "z": "Zrotation"}
_AXIS = {"x": 0, "y": 1, "z": 2}


class BvhValueRefused(ValueError):
    """``format_bvh_motion``: a channel value is NaN, infinite or at least 1e12 in magnitude (``first_bad``: its token ordinal,
    frame * columns + column) - the device writes no text for such input; ``write_bvh`` formats it on the host instead."""

    def __init__(self, first_bad: int, message: str):
        super().__init__(message)
        self.first_bad = first_bad


def _dev_f64(model: Generator, a) -> torch.Tensor:
    """A contiguous float64 tensor on the model's device; anything else is cast THERE (fp32 -> float64 is exact)."""
    if isinstance(a, np.ndarray):
        a = torch.from_numpy(a)
    return torch.as_tensor(a).to(model.device).to(torch.float64).contiguous()


def format_bvh_motion(model: Generator, positions, euler_deg, visit: Sequence[int], order: str = "zyx", save_positions: bool = False,
                      clip_offsets: Optional[Sequence[int]] = None):
    """The MOTION block of the reference's writer (motion/bvh.py:210-224) as bytes ON THE DEVICE (``mocha_bvh_format``): positions /
    euler_deg (F,V,3), float64 on the device as ``PostProcessor.run`` leaves ``bvh_pos`` / ``bvh_euler`` (anything else is cast on the
    device), ``visit`` the joint order ``write_bvh`` returns, every number as Python's ``"%f "``, a newline behind every frame.
    ``clip_offsets`` (n_clips + 1 frame offsets increasing from 0 to F; default one clip) cuts the frames into clips whose text blocks lie
    back to back.  Returns (text, offsets): a uint8 device tensor of exactly the text's length and the n_clips + 1 byte offsets of the
    clips' blocks in it (numpy int64).  Raises ``BvhValueRefused`` for NaN, infinities and |x| >= 1e12.  Waits for the current stream once
    (the totals); the text itself is written behind that wait, in stream order.  Not for graph capture."""
    pos, rot = _dev_f64(model, positions), _dev_f64(model, euler_deg)
    if pos.dim() != 3 or pos.shape[2] != 3 or pos.shape != rot.shape:
        raise ValueError(f"format_bvh_motion: positions {tuple(pos.shape)} and euler_deg {tuple(rot.shape)} must both be (F,V,3)")
    F, V = int(pos.shape[0]), int(pos.shape[1])
    offs = [0, F] if clip_offsets is None else [int(v) for v in clip_offsets]
    if offs[-1] != F:
        raise ValueError(f"format_bvh_motion: clip_offsets end at {offs[-1]}, the arrays hold {F} frames")
    n = len(offs) - 1
    ctx = model._ctx
    bound = int(ctx.lib.mocha_bvh_text_bound(F, V, int(save_positions)))
    if bound >= 2 ** 31:
        raise ValueError(f"format_bvh_motion: {F} frames of {V} joints may take 2^31 bytes of text or more: format fewer frames per call")
    text = torch.empty((max(bound, 1),), dtype=torch.uint8, device=model.device)
    begin = (C.c_int64 * (n + 1))()
    rep = _C.mocha_bvhw_report()
    with torch.cuda.device(model.device):
        rc = ctx.lib.mocha_bvh_format(ctx.h, _ptr(pos), _ptr(rot), (C.c_int32 * (n + 1))(*offs), n, V, (C.c_int32 * len(visit))(*[int(j) for j in visit]),
                                      (C.c_int32 * 3)(*[_AXIS[c] for c in order]), int(save_positions), _ptr(text), bound, begin, C.byref(rep),
                                      C.c_void_p(torch.cuda.current_stream(model.device).cuda_stream))
    if rc != 0 and rep.first_bad >= 0:
        raise BvhValueRefused(int(rep.first_bad), (ctx.lib.mocha_last_error(ctx.h) or b"?").decode())
    _C.check(ctx.lib, ctx.h, rc, "mocha_bvh_format")
    return text[: int(rep.bytes)], np.array(list(begin), dtype=np.int64)


def _bvh_header_lines(names, parents, off, order: str, frames: int, frametime: float, save_positions: bool):
    """The lines of a BVH file in front of its MOTION numbers, in the reference writer's layout (motion/bvh.py:145-208), and ``visit``:
    the depth-first joint order, which is the column order of the motion block."""
    chan = " ".join(_CHANNEL[c] for c in order)
    lines, visit = [], [0]

    def joint(i, tabs):
        visit.append(i)
        lines.append(f"{tabs}JOINT {names[i]}"); lines.append(f"{tabs}{{")
        t = tabs + "\t"
        lines.append("%sOFFSET %f %f %f" % (t, off[i, 0], off[i, 1], off[i, 2]))
        if save_positions:
            lines.append(f"{t}CHANNELS 6 Xposition Yposition Zposition {chan} ")      # (the reference's trailing space, bvh.py:152)
        else:
            lines.append(f"{t}CHANNELS 3 {chan}")
        kids = [j for j, p in enumerate(parents) if p == i]
        for j in kids:
            joint(j, t)
        if not kids:
            lines.append(f"{t}End Site"); lines.append(f"{t}{{")
            lines.append("%s\tOFFSET %f %f %f" % (t, 0.0, 0.0, 0.0))
            lines.append(f"{t}}}")
        lines.append(f"{tabs}}}")

    lines += ["HIERARCHY", f"ROOT {names[0]}", "{"]
    lines.append("\tOFFSET %f %f %f" % (off[0, 0], off[0, 1], off[0, 2]))
    lines.append(f"\tCHANNELS 6 Xposition Yposition Zposition {chan} ")
    for j, p in enumerate(parents):
        if p == 0:
            joint(j, "\t")
    lines += ["}", "MOTION", "Frames: %i" % frames, "Frame Time: %f" % frametime]
    return lines, visit


def _host_motion_block(pos, rot, visit, order: str, save_positions: bool) -> Optional[str]:
    """The MOTION block on the host (no trailing newline; None without frames): per frame the root's position, then every visited
    joint's three angles in channel order - with ``save_positions`` every visited joint's position and angles -, each number as
    "%f " - one matrix in that column order and ONE format operation for the whole block (a Python loop over frames and joints
    took 20 ms for a 585-frame clip, several times the GPU's share of the demo)."""
    ax = [_AXIS[c] for c in order]
    n = rot.shape[0]
    if not n:
        return None
    if save_positions:
        cols = [a for j in visit for a in (pos[:, j, :], rot[:, j][:, ax])]
    else:
        cols = [pos[:, 0, :]] + [rot[:, j][:, ax] for j in visit]
    M = np.concatenate(cols, axis=1)                            # (n, 3 + 3 * len(visit)) or (n, 6 * len(visit))
    row_fmt = "%f " * M.shape[1]
    return ("\n".join([row_fmt] * n)) % tuple(M.ravel().tolist())


def _write_with_text(path, lines, text: Optional[np.ndarray]):
    """Header lines, then the motion block as the bytes the device produced (they end with the last frame's newline)."""
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
        if text is not None and len(text):
            f.flush()
            f.buffer.write(text.data)


def write_bvh(path: str, names: Sequence[str], parents: Sequence[int], positions, euler_deg, offsets=None,
              order: str = "zyx", frametime: float = 1.0 / 60.0, save_positions: bool = False, model: Optional[Generator] = None):
    """BVH text in the reference writer's layout (motion/bvh.py:145-224): the hierarchy is walked depth-first in child-index
    order, every joint has three rotation channels named after ``order``, the root also three position channels - with
    ``save_positions`` every joint has six -, leaves get a zero ``End Site``.  positions / euler_deg (N,V,3); offsets default to the
    first frame's positions (test_fullframework.py:699).  Returns the joint order of the motion columns.
    With ``model`` the numbers are formatted on the model's device (``format_bvh_motion``): the arrays stay there (float64 as
    ``PostProcessor.run`` leaves them; anything else is cast there), one copy brings the text bytes back and they go to the file as they
    are.  Input the device refuses (NaN, infinities, |x| >= 1e12) takes the host route below; the file is the same bytes on either route.
    Without ``model`` every number goes through Python's "%f " on the host."""
    parents = [int(p) for p in parents]
    if model is not None and len(euler_deg):
        pos_d, rot_d = _dev_f64(model, positions), _dev_f64(model, euler_deg)
        if not (pos_d.dim() == rot_d.dim() == 3 and len(names) == len(parents) == pos_d.shape[1] == rot_d.shape[1]):
            raise ValueError("write_bvh: names, parents, positions and rotations disagree on the joint count")
        off = pos_d[0].cpu().numpy() if offsets is None else np.asarray(offsets, dtype=np.float64)
        lines, visit = _bvh_header_lines(names, parents, off, order, int(rot_d.shape[0]), frametime, save_positions)
        try:
            text, _ = format_bvh_motion(model, pos_d, rot_d, visit, order, save_positions)
        except BvhValueRefused:
            text = None
        if text is not None:
            _write_with_text(path, lines, text.cpu().numpy())         # the one copy: the text's bytes
            return visit
    pos = np.asarray(positions.cpu() if torch.is_tensor(positions) else positions, dtype=np.float64)
    rot = np.asarray(euler_deg.cpu() if torch.is_tensor(euler_deg) else euler_deg, dtype=np.float64)
    off = pos[0] if offsets is None else np.asarray(offsets, dtype=np.float64)
    if not (len(names) == len(parents) == pos.shape[1] == rot.shape[1]):
        raise ValueError("write_bvh: names, parents, positions and rotations disagree on the joint count")
    lines, visit = _bvh_header_lines(names, parents, off, order, len(rot), frametime, save_positions)
    block = _host_motion_block(pos, rot, visit, order, save_positions)
    if block is not None:
        lines.append(block)
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    return visit


def write_bvh_clips(model: Generator, paths: Sequence[str], names: Sequence[str], parents: Sequence[int], positions, euler_deg,
                    clip_offsets: Sequence[int], offsets=None, order: str = "zyx", frametime: float = 1.0 / 60.0,
                    save_positions: bool = False):
    """Many files of ONE skeleton: positions / euler_deg (F,V,3) hold the clips one after the other, ``clip_offsets`` (len(paths) + 1,
    increasing from 0 to F) cuts them, file i gets clip i.  All numbers are formatted by one ``format_bvh_motion`` call and come back
    in one copy (into pinned host memory where torch offers it); each file gets its own header - ``offsets`` (V,3), or by default the
    first frame of ITS clip - and its slice of the text.  Calls whose text bound reaches 2 GiB are split at clip boundaries.  A clip
    the device refuses (see ``write_bvh``) is written by the host route; every file equals what ``write_bvh`` writes for its clip.
    Returns the joint order of the motion columns."""
    offs = [int(v) for v in clip_offsets]
    if len(offs) != len(paths) + 1 or offs[0] != 0 or any(b <= a for a, b in zip(offs, offs[1:])):
        raise ValueError("write_bvh_clips: clip_offsets must hold len(paths) + 1 frame offsets increasing from 0")
    parents = [int(p) for p in parents]
    pos_d, rot_d = _dev_f64(model, positions), _dev_f64(model, euler_deg)
    if not (pos_d.dim() == rot_d.dim() == 3 and len(names) == len(parents) == pos_d.shape[1] == rot_d.shape[1]) or pos_d.shape[0] != offs[-1]:
        raise ValueError("write_bvh_clips: names, parents, positions, rotations and clip_offsets disagree on the joints or frames")
    V = len(names)
    firsts = None if offsets is not None else pos_d[torch.as_tensor(offs[:-1], device=pos_d.device)].cpu().numpy()      # (n_clips,V,3)
    fixed = None if offsets is None else np.asarray(offsets, dtype=np.float64)
    bound = lambda frames: int(model._ctx.lib.mocha_bvh_text_bound(frames, V, int(save_positions)))
    visit, first = None, 0
    while first < len(paths):
        last = first + 1                                             # clips first .. last-1 share a call
        while last < len(paths) and bound(offs[last + 1] - offs[first]) < 2 ** 31:
            last += 1
        lo, hi = offs[first], offs[last]
        heads = [_bvh_header_lines(names, parents, fixed if fixed is not None else firsts[i], order, offs[i + 1] - offs[i], frametime,
                                   save_positions) for i in range(first, last)]
        visit = heads[0][1]
        try:
            text, begin = format_bvh_motion(model, pos_d[lo:hi], rot_d[lo:hi], visit, order, save_positions, [o - lo for o in offs[first: last + 1]])
        except BvhValueRefused:
            for i in range(first, last):
                write_bvh(paths[i], names, parents, pos_d[offs[i]: offs[i + 1]], rot_d[offs[i]: offs[i + 1]],
                          None if fixed is None else fixed, order, frametime, save_positions, model=model)
            first = last
            continue
        try:
            host = torch.empty(text.shape, dtype=torch.uint8, pin_memory=True)
        except RuntimeError:
            host = torch.empty(text.shape, dtype=torch.uint8)
        host.copy_(text)                                             # the one copy
        data = host.numpy()
        for i in range(first, last):
            _write_with_text(paths[i], heads[i - first][0], data[begin[i - first]: begin[i - first + 1]])
        first = last
    return visit
