"""NumPy float64 restatement of the resampler (mocha_resample_clips, mocha_resample_step), whole clips and one source frame at a time.

The step between outputs is num / den source frames.  A clip of n >= 1 frames gives m = floor((n-1) den / num) + 1 outputs; output k sits at
t = k num: source frame i = t div den, a = (t mod den) / den.  q = the clip's quaternions in float64 (clip_ingest_ref.euler_to_quat, or as
given), sign-unrolled along time (clip_ingest_ref.unroll).  a == 0: the output is q[i], p[i] themselves and frame i+1 is not read.  Otherwise

    q_mul(exp_half(a * scaled_angle_axis(q_abs(q_mul(q[i+1], q_inv(q[i]))))), q[i]),     p[i] + a * (p[i+1] - p[i])

with the reference's eps = 1e-5 branches (quat.py:149-164): rotation at the constant angular velocity that the reference's difference formula
assigns to the interval (generate_database.py:148-149), positions linear, in the file's units.  ``StreamRef`` is the same one source frame at
a time: push j (from 0) emits the outputs k with floor((j-1) den / num) < k <= floor(j den / num) from the stored previous frame and the new
one; a stream without a predecessor emits the new frame for every output of that push.

Measured deviation from the definition evaluated with the reference's own quat functions on tests/golden/resample.npz (45 frames, 24 joints,
orders zyx / yzx, seven ratios), as test_resample_ref.py::test_fixture prints and asserts it (run of 2026-10-21: NumPy on x86-64): see E."""
from __future__ import annotations

import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from clip_ingest_ref import euler_to_quat, unroll  # noqa: E402
from ingest_ref import AXIS, q_inv, q_mul  # noqa: E402

# Largest |restatement - reference composition| over the fixture: rot 0, pos 0 - every float is the reference's bit for bit.  The one place
# where the two are written differently, quat.exp's np.sinc(h / pi) against sin(h) / h here, rounds alike on all of the fixture's values.
E = 0.0
MAX_OUT = 4


def count(n, num, den):
    return (n - 1) * den // num + 1


def at(k, num, den):
    t = k * num
    return t // den, float(t % den) / float(den)


def between(q0, q1, p0, p1, a, eps=1e-5):
    """The frame at a in (0, 1) between two frames; quaternions (4, ...) unrolled, positions (3, ...)."""
    d = q_mul(q1, q_inv(q0))
    d = np.where(d[0] > 0.0, d, -d)                                               # quat.abs
    ln = np.sqrt((d[1] * d[1] + d[2] * d[2]) + d[3] * d[3])
    with np.errstate(invalid="ignore", divide="ignore"):
        s = a * (2.0 * (np.where(ln < eps, 1.0, np.arctan2(ln, d[0]) / ln) * d[1:]))   # a * to_scaled_angle_axis
        x = s / 2.0                                                                # from_scaled_angle_axis
        h = np.sqrt((x[0] * x[0] + x[1] * x[1]) + x[2] * x[2])
        c = np.where(h < eps, 1.0, np.cos(h))
        sc = np.where(h < eps, 1.0, np.sin(h) / h)
    return q_mul(np.concatenate([c[None], sc * x]), q0), p0 + a * (p1 - p0)


def quats(rot, order):
    """(n,V,3) degrees in `order` ('zyx', ...) or, with order None, (n,V,4) quaternions; fp32 values -> (4,n,V) float64, unrolled."""
    rot = np.asarray(rot, np.float32).astype(np.float64)
    return unroll(rot.transpose(2, 0, 1).copy() if order is None else euler_to_quat(rot, [AXIS[a] for a in order]))


def resample_clip(rot, pos, order, num, den):
    """One clip -> rot (m,V,4), pos (m,V,3) float64."""
    q = quats(rot, order)
    p = np.asarray(pos, np.float32).astype(np.float64).transpose(2, 0, 1)
    m = count(q.shape[1], num, den)
    oq, op = np.empty((4, m, q.shape[2])), np.empty((3, m, q.shape[2]))
    for k in range(m):
        i, a = at(k, num, den)
        if a == 0.0:
            oq[:, k], op[:, k] = q[:, i], p[:, i]
        else:
            oq[:, k], op[:, k] = between(q[:, i], q[:, i + 1], p[:, i], p[:, i + 1], a)
    return oq.transpose(1, 2, 0), op.transpose(1, 2, 0)


def push_count(j, num, den):
    """Outputs of push j (from 0), and the first one's index: pure integer arithmetic."""
    first = 0 if j == 0 else (j - 1) * den // num + 1
    return j * den // num - first + 1, first


class StreamRef:
    """One stream: the previous unrolled quaternions and positions, and whether there is a predecessor."""

    def __init__(self, order, num, den):
        assert den <= MAX_OUT * num
        self.order, self.num, self.den = order, num, den
        self.j, self.q, self.p = 0, None, None

    def restart(self):
        self.q = self.p = None

    def push(self, rot, pos):
        """rot (V,3|4), pos (V,3) -> [(q (V,4), p (V,3))] of this push."""
        rot = np.asarray(rot, np.float32).astype(np.float64)
        q1 = rot.T.copy() if self.order is None else euler_to_quat(rot[None], [AXIS[a] for a in self.order])[:, 0]
        p1 = np.asarray(pos, np.float32).astype(np.float64).T
        if self.q is not None:
            d = ((q1[0] * self.q[0] + q1[1] * self.q[1]) + q1[2] * self.q[2]) + q1[3] * self.q[3]
            q1 = np.where(d < 0.0, -q1, q1)
        n, first = push_count(self.j, self.num, self.den)
        out = []
        for k in range(first, first + n):
            i, a = at(k, self.num, self.den)
            if a == 0.0 or self.q is None:
                out.append((q1.T.copy(), p1.T.copy()))
            else:
                assert i == self.j - 1
                oq, op = between(self.q, q1, self.p, p1, a)
                out.append((oq.T, op.T))
        self.q, self.p, self.j = q1, p1, self.j + 1
        return out
