"""What mocha_world_bind / mocha_world_pose MEAN, restated in NumPy and generic over the dtype: forward kinematics as the reference's
quat.fk (motion/quat.py:166-173 with mul :112-120 and mul_vec :128-130) and the skinning palette
pre o [to_xform(G) | g] o [to_xform(B) | c]^-1 (to_xform :27-40, normalize :15-16) of include/mocha_hip.h.  float64 is the evaluation the
fixture tests/golden/world_pose.npz holds (test_world_ref.py: bit for bit for fk, equal after the one rounding for the palette);
numpy.longdouble is the truth the float64 kernel outputs are measured against (test_world_pose_kernel.py).  Nothing here is transcribed
from the kernels: a frame is a Python loop over bones, a matrix product a loop over rows and columns."""
from __future__ import annotations

import numpy as np


def bone_parents(joint_parents):
    """Parents of the (V+1)-bone skeleton, the trajectory root bone in front: [-1] + (joint parents + 1) (test_fullframework.py:101-102)."""
    return [-1] + [int(p) + 1 for p in joint_parents]


def _mul(x, y):
    x0, x1, x2, x3 = (x[..., k] for k in range(4))
    y0, y1, y2, y3 = (y[..., k] for k in range(4))
    return np.stack([y0 * x0 - y1 * x1 - y2 * x2 - y3 * x3,
                     y0 * x1 + y1 * x0 - y2 * x3 + y3 * x2,
                     y0 * x2 + y1 * x3 + y2 * x0 - y3 * x1,
                     y0 * x3 - y1 * x2 + y2 * x1 + y3 * x0], axis=-1)


def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1],
                     a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], axis=-1)


def _mul_vec(q, v):
    two = q.dtype.type(2.0)
    t = two * _cross(q[..., 1:], v)
    return v + q[..., 0:1] * t + _cross(q[..., 1:], t)


def fk(rot, pos, parents, dtype=np.float64):
    """rot (..,J,4), pos (..,J,3) local -> (grot, gpos) global, evaluated in `dtype`; parents[0] = -1, parents[b] < b."""
    rot, pos = np.asarray(rot).astype(dtype), np.asarray(pos).astype(dtype)
    grot, gpos = np.empty_like(rot), np.empty_like(pos)
    grot[..., 0, :], gpos[..., 0, :] = rot[..., 0, :], pos[..., 0, :]
    for b in range(1, len(parents)):
        pa = parents[b]
        assert 0 <= pa < b
        gpos[..., b, :] = _mul_vec(grot[..., pa, :], pos[..., b, :]) + gpos[..., pa, :]
        grot[..., b, :] = _mul(grot[..., pa, :], rot[..., b, :])
    return grot, gpos


def to_xform(q):
    """(..,4) -> (..,3,3)."""
    one = q.dtype.type(1.0)
    qw, qx, qy, qz = (q[..., k] for k in range(4))
    x2, y2, z2 = qx + qx, qy + qy, qz + qz
    xx, yy, wx = qx * x2, qy * y2, qw * x2
    xy, yz, wy = qx * y2, qy * z2, qw * y2
    xz, zz, wz = qx * z2, qz * z2, qw * z2
    rows = [[one - (yy + zz), xy - wz, xz + wy], [xy + wz, one - (xx + zz), yz - wx], [xz - wy, yz + wx, one - (xx + yy)]]
    return np.stack([np.stack(r, axis=-1) for r in rows], axis=-2)


def normalize(q):
    eps = q.dtype.type(1e-8)
    return q / (np.sqrt(np.sum(q * q, axis=-1))[..., None] + eps)


def compose(R1, t1, R2, t2):
    """(R1 | t1) o (R2 | t2) = (R1 R2 | R1 t2 + t1), every sum over k = 0, 1, 2 in that order."""
    shape = np.broadcast_shapes(R1.shape, R2.shape)
    R, t = np.empty(shape, R1.dtype), np.empty(shape[:-1], R1.dtype)
    for i in range(3):
        for j in range(3):
            R[..., i, j] = R1[..., i, 0] * R2[..., 0, j] + R1[..., i, 1] * R2[..., 1, j] + R1[..., i, 2] * R2[..., 2, j]
        t[..., i] = (R1[..., i, 0] * t2[..., 0] + R1[..., i, 1] * t2[..., 1] + R1[..., i, 2] * t2[..., 2]) + t1[..., i]
    return R, t


def inverse_bind(rest_rot, rest_pos, parents, dtype=np.float64):
    """The rigid inverses (R^T, -R^T c) of the rest pose's globals, bones 0..V: (J,3,3), (J,3).  rest_rot None = identity rotations."""
    J = len(parents)
    if rest_rot is None:
        q = np.zeros((J, 4), dtype)
        q[:, 0] = 1
    else:
        q = normalize(np.asarray(rest_rot).astype(dtype))
    B, c = fk(q, np.asarray(rest_pos).astype(dtype), parents, dtype)
    Rt = np.swapaxes(to_xform(B), -1, -2)
    t = np.empty_like(c)
    for i in range(3):
        t[..., i] = -(Rt[..., i, 0] * c[..., 0] + Rt[..., i, 1] * c[..., 1] + Rt[..., i, 2] * c[..., 2])
    return Rt, t


def palette_wide(grot, gpos, rest_rot, rest_pos, pre, parents, dtype=np.float64):
    """(..,V,3,4) in `dtype`, before the rounding: pre o [to_xform(G[b]) | g[b]] o inverse bind[b], b = 1..V.  pre (3,4) or None."""
    pre = np.eye(3, 4) if pre is None else np.asarray(pre).reshape(3, 4)
    pre = pre.astype(dtype)
    grot, gpos = np.asarray(grot).astype(dtype), np.asarray(gpos).astype(dtype)
    Ri, ti = inverse_bind(rest_rot, rest_pos, parents, dtype)
    R, t = compose(pre[:, :3], pre[:, 3], to_xform(grot[..., 1:, :]), gpos[..., 1:, :])
    R, t = compose(R, t, Ri[1:], ti[1:])
    return np.concatenate([R, t[..., None]], axis=-1)


def palette(grot, gpos, rest_rot, rest_pos, pre, parents, dtype=np.float64):
    """(..,V,12) fp32: palette_wide rounded once, row-major."""
    m = palette_wide(grot, gpos, rest_rot, rest_pos, pre, parents, dtype)
    return m.reshape(m.shape[:-2] + (12,)).astype(np.float32)


def frame_error(got, truth):
    """max over frames of (largest |got - truth| of the frame) / (largest |truth| of the frame): got, truth (n,J,k)."""
    truth = np.asarray(truth)
    err = np.abs(np.asarray(got).astype(truth.dtype) - truth).reshape(len(truth), -1).max(axis=1)
    return float((err / np.abs(truth).reshape(len(truth), -1).max(axis=1)).max())
