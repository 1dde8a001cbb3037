"""World-space poses and skinning palettes on the device (``mocha_world_bind``, ``mocha_world_pose``).

Everything else in the package emits LOCAL poses - ``pos (.., V+1, 3)`` and ``rot / ik_rot (.., V+1, 4)`` (w,x,y,z), parent-relative, the
trajectory root bone in front.  ``world_pose`` runs the reference's ``quat.fk`` (motion/quat.py:166-173) over any number of such frames in
one launch and returns the global positions and rotations in float64 - what the reference's demo computes at its end
(test_fullframework.py:672-690) and hands to ``animation_plot`` (:670) - and, with a ``SkinBind``, the fp32 palette of 3x4 matrices
``pre . world . inverse(bind)`` of the V bones behind the root: one contiguous buffer per call that a renderer can bind.

No mesh is skinned here, no global velocities (``quat.fk_vel``) and no dual quaternions are produced, and a call takes one bind."""
from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np
import torch

from .generator import _ptr, _stream


def _f64_dev(a, device, shape, name):
    t = torch.as_tensor(np.asarray(a, dtype=np.float64) if not isinstance(a, torch.Tensor) else a)
    t = t.to(device=device, dtype=torch.float64).contiguous()
    if tuple(t.shape) != tuple(shape):
        raise ValueError(f"SkinBind: {name} has shape {tuple(t.shape)}, expected {tuple(shape)}")
    return t


class SkinBind:
    """The rest pose a skinned mesh was bound in, as the device-side inverse bind transforms of ``model``'s (V+1)-bone skeleton.

    ``rest_pos`` (V+1,3) and ``rest_rot`` (V+1,4) (w,x,y,z; default identity; normalised once) are LOCAL, the trajectory root bone first;
    ``pre`` (3,4) is an affine map applied in front of every world transform - unit scale, axis swap, handedness - default identity and
    refused when not finite.  The inverses are computed on the device by the forward kinematics ``world_pose`` runs."""

    def __init__(self, model, rest_pos, rest_rot=None, pre=None):
        self.model = model
        dev, J = model.device, model.V + 1
        pos = _f64_dev(rest_pos, dev, (J, 3), "rest_pos")
        rot = None if rest_rot is None else _f64_dev(rest_rot, dev, (J, 4), "rest_rot")
        arr = None
        if pre is not None:
            host = np.ascontiguousarray(np.asarray(pre.cpu() if isinstance(pre, torch.Tensor) else pre, dtype=np.float64)).reshape(-1)
            if host.size != 12:
                raise ValueError(f"SkinBind: pre has {host.size} values, expected a (3,4) affine map")
            arr = (C.c_double * 12)(*host.tolist())
        ctx = model._ctx
        nbytes = int(ctx.lib.mocha_world_bind_bytes(ctx.h))
        if nbytes <= 0:
            raise RuntimeError("mocha_world_bind_bytes failed")
        self.buf = torch.zeros((nbytes // 8,), dtype=torch.float64, device=dev)
        ctx.call("mocha_world_bind", _ptr(rot), _ptr(pos), arr, _ptr(self.buf), _stream())
        self.rest_pos, self.rest_rot = pos, rot

    @classmethod
    def from_bvh_header(cls, model, offsets, rest_rot=None, pre=None):
        """The bind of a BVH file's own rest pose: ``offsets`` (V,3) as ``read_bvh_header(...).offsets`` (or ``BvhClips.offsets``) gives
        them, the trajectory root bone prepended at the origin."""
        off = np.asarray(offsets.cpu() if isinstance(offsets, torch.Tensor) else offsets, dtype=np.float64)
        if off.shape != (model.V, 3):
            raise ValueError(f"SkinBind.from_bvh_header: offsets have shape {off.shape}, expected {(model.V, 3)}")
        return cls(model, np.concatenate([np.zeros((1, 3)), off]), rest_rot, pre)


def _launch(model, rot, pos, n, valid, bind, gpos, grot, palette):
    model._ctx.call("mocha_world_pose", _ptr(rot), _ptr(pos), 1 if rot.dtype == torch.float32 else 0, int(n), _ptr(valid),
                    _ptr(bind.buf) if bind is not None else None, _ptr(gpos), _ptr(grot), _ptr(palette), _stream())


def world_pose(model, rot, pos, bind: Optional[SkinBind] = None, valid=None, out=None):
    """Global poses of local ones: ``rot (.., V+1, 4)`` and ``pos (.., V+1, 3)`` on ``model``'s device with any leading shape - whole clips
    from ``PostProcessor.run`` go through in one call - both float64 (what post-processing and the live steps emit) or both float32 (what
    ``ingest_clips``, ``resample_clips`` and the live mocap front end emit; the kernel widens them on load, no torch op converts).
    Returns ``dict(gpos (.., V+1, 3), grot (.., V+1, 4))`` float64 and, with ``bind``, ``palette (.., V, 12)`` float32: row-major 3x4
    matrices of bones 1..V.  ``valid`` (leading shape) int32: rows whose entry is 0 are left as they are.  ``out``: a dict of tensors of
    those shapes to write into (any subset of the keys; the others are not computed) - without it fresh zero tensors are returned.
    One launch on the current stream, no host synchronisation."""
    J, V, dev = model.V + 1, model.V, model.device
    if not (isinstance(rot, torch.Tensor) and isinstance(pos, torch.Tensor)):
        raise TypeError("world_pose: rot and pos are torch tensors on the model's device")
    if rot.dtype != pos.dtype or rot.dtype not in (torch.float32, torch.float64):
        raise TypeError(f"world_pose: rot and pos must both be float32 or both float64, got {rot.dtype} and {pos.dtype}")
    if rot.device != dev or pos.device != dev:
        raise ValueError("world_pose: rot and pos must be on the model's device")
    lead = tuple(rot.shape[:-2])
    if tuple(rot.shape[-2:]) != (J, 4) or tuple(pos.shape) != lead + (J, 3):
        raise ValueError(f"world_pose: expected rot (.., {J}, 4) and pos (.., {J}, 3), got {tuple(rot.shape)} and {tuple(pos.shape)}")
    if bind is not None and bind.model is not model:
        raise ValueError("world_pose: bind belongs to another model")
    rot, pos = rot.contiguous(), pos.contiguous()
    n = int(np.prod(lead, dtype=np.int64)) if lead else 1
    shapes = {"gpos": (lead + (J, 3), torch.float64), "grot": (lead + (J, 4), torch.float64), "palette": (lead + (V, 12), torch.float32)}
    if out is None:
        out = {k: torch.zeros(s, dtype=dt, device=dev) for k, (s, dt) in shapes.items() if k != "palette" or bind is not None}
    else:
        if not out or any(k not in shapes for k in out):
            raise ValueError(f"world_pose: out holds some of {sorted(shapes)}")
        if "palette" in out and bind is None:
            raise ValueError("world_pose: a palette needs bind=")
        for k, t in out.items():
            s, dt = shapes[k]
            if tuple(t.shape) != s or t.dtype != dt or t.device != dev or not t.is_contiguous():
                raise ValueError(f"world_pose: out[{k!r}] must be a contiguous {dt} tensor of shape {s} on the model's device")
    if valid is not None:
        if valid.dtype != torch.int32 or valid.device != dev or tuple(valid.shape) != lead:
            raise ValueError(f"world_pose: valid must be an int32 tensor of shape {lead} on the model's device")
        valid = valid.contiguous()
    _launch(model, rot, pos, n, valid, bind, out.get("gpos"), out.get("grot"), out.get("palette"))
    return out
