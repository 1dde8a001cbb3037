"""NumPy float64 restatement of the streaming mocap front end (mocha_live_ingest; preprocess/generate_database.py:86-177 of the reference,
one frame per call).

A stream has pushed raw frames r_0 .. r_{n-1}: local rotations (Euler degrees in a BVH order, or quaternions w,x,y,z) and local positions
of the V joints, joint 0 the hips.  Once n >= 31 a push emits frame t = n-1-L (L = lookahead, 0..18) of the reference's ``process_data``
applied to that prefix: positions, velocities, rotations, angular velocities of the V+1 bones (synthetic root bone first) and the foot
contacts.  What a push does, in the kernel's order:

  store    from_euler (or the quaternion as given) -> unroll against the previous frame's quaternion of that bone -> forward kinematics
           of the frame -> the spine joint on xz and the projected, normalised across-direction.  The frame goes into a ring of RING
           frames: the emitted frame reads at most the last 38 (contacts at t-3 read the root at t-4, whose 31-tap fit reaches t-19).
  root     for the frames t-4 .. min(t+3, n-1): root position = 15-tap cubic fit of the spine joint, root direction = 31-tap cubic fit
           of the across-direction, renormalised; each with the centre row of the fit, or, for a frame closer than half a window to
           either end of the prefix, that frame's row of the fit over the first / last window (savgol_filter's mode='interp').
           The rows are those of A (A^T A)^-1 A^T for the cubic Vandermonde matrix on centred abscissae (``fit_rows``).
  hips     root rotation = normalize(between(z, direction)); the hips made local to it.
  vel/ang  for the frames t-3 .. min(t+2, n-1): central differences, the last frame of the prefix extrapolated v[-1] = 2 v[-2] - v[-3].
  contact  fk_vel down every toe chain in those frames, speed < threshold, then "at least 3 of the frames t-3 .. t+2 (clamped to the
           prefix)" - what ndimage.median_filter(size=6, mode='nearest') computes on a boolean track.
  derived  src_rvel / src_rang = inv_mul_vec(Yrot[0], Yvel[0] / Yang[0]) of the fp32-rounded emitted frame; src_speed = mean |v| of bone 1
           over the last 60 emitted fp32 frames, v their central difference with the window-edge rule (test_fullframework.py:164-169),
           0 while fewer than 60 frames were emitted.  All in float64.

Measured deviation of this restatement from the reference's own process_data on tests/golden/live_ingest.npz (every prefix 31..100,
L in {0, 2, 7, 18}, pos / vel / rot / ang, 25 bones): see E below and test_ingest_ref.py, which asserts it.
"""
from __future__ import annotations

import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mocha_sigasia2023_amd.synthetic import raw_walk_clip  # noqa: E402

FIRST = 31           # pushes before the first emission: savgol_filter(window_length=31) refuses a shorter clip
RING = 40            # raw frames kept per stream
MAX_LOOKAHEAD = 18
# Largest |restatement - reference| over the whole fixture, as test_ingest_ref.py::test_fixture prints it (run of 2026-10-19: NumPy on
# x86-64, float64, scipy 1.15.3 behind the fixture): pos 6.36e-15, vel 1.87e-13, rot 5.55e-16, ang 4.16e-14.  The velocity leads: it is
# 60 x a difference of root positions, where scipy's polyfit at a prefix end and this file's fit rows differ in the last bits.  E is the
# largest of the four, rounded up in its second digit.
E = 1.9e-13

AXIS = {"x": 0, "y": 1, "z": 2}


def fit_rows(window: int, order: int = 3) -> np.ndarray:
    """(window, window): row r = the weights that evaluate, at sample r, the least-squares polynomial through the window's samples."""
    x = np.arange(window, dtype=np.longdouble) - (window - 1) / 2
    A = np.stack([x ** k for k in range(order + 1)], axis=1)
    return _hat(A)


def _hat(A):
    """A (A^T A)^-1 A^T in long double, the inverse by Gauss-Jordan with partial pivoting (np.linalg has no long double)."""
    n = A.shape[1]
    M = np.concatenate([A.T @ A, np.eye(n, dtype=np.longdouble)], axis=1)
    for c in range(n):
        p = c + int(np.argmax(np.abs(M[c:, c])))
        M[[c, p]] = M[[p, c]]
        M[c] = M[c] / M[c, c]
        for r in range(n):
            if r != c:
                M[r] = M[r] - M[r, c] * M[c]
    return (A @ M[:, n:] @ A.T).astype(np.float64)


# ------------------------------------------------------------------------------------------------------------------ quaternions (w,x,y,z)
def q_mul(x, y):
    x0, x1, x2, x3 = x
    y0, y1, y2, y3 = y
    return np.array([y0 * x0 - y1 * x1 - y2 * x2 - y3 * x3,
                     y0 * x1 + y1 * x0 - y2 * x3 + y3 * x2,
                     y0 * x2 + y1 * x3 + y2 * x0 - y3 * x1,
                     y0 * x3 - y1 * x2 + y2 * x1 + y3 * x0])


def q_inv(q):
    return np.array([q[0], -q[1], -q[2], -q[3]])


def cross(a, b):
    return np.array([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]])


def q_mul_vec(q, x):
    t = 2.0 * cross(q[1:], x)
    return x + q[0] * t + cross(q[1:], t)


def q_abs(q):
    return q if q[0] > 0.0 else -q


def scaled_angle_axis(q, eps=1e-5):
    ln = np.sqrt(q[1] * q[1] + q[2] * q[2] + q[3] * q[3])
    h = 1.0 if ln < eps else np.arctan2(ln, q[0]) / ln
    return 2.0 * (h * q[1:])


def from_euler_deg(e, order):
    """quat.from_euler(np.radians(e), order): e (3,) degrees, order three axis indices."""
    r = np.asarray(e, np.float64) * (np.pi / 180.0)
    qs = []
    for k in range(3):
        q = np.zeros(4)
        q[0] = np.cos(r[k] / 2.0)
        q[1 + order[k]] = np.sin(r[k] / 2.0)
        qs.append(q)
    return q_mul(qs[0], q_mul(qs[1], qs[2]))


class IngestRef:
    """One stream.  ``parents``: the V raw joints' parents (-1 for the hips); ``order``: None for quaternion input, else three axis
    indices or a string like 'zyx'; ``roles`` = (spine, shoulder_l, shoulder_r, upleg_l, upleg_r) raw joint indices; ``toes``: bone
    indices in the (V+1)-bone skeleton (mocha_post_cfg.contact_bones)."""

    def __init__(self, parents, lookahead, order, roles, toes, unit_scale=0.01, fps=60.0, threshold=0.5):
        assert 0 <= lookahead <= MAX_LOOKAHEAD
        self.par = [int(p) for p in parents]
        self.V = len(self.par)
        self.L = int(lookahead)
        self.order = None if order is None else [AXIS[a] if isinstance(a, str) else int(a) for a in order]
        self.roles, self.toes = [int(r) for r in roles], [int(t) for t in toes]
        self.scale, self.fps, self.thr = float(unit_scale), float(fps), float(threshold)
        self.H15, self.H31 = fit_rows(15), fit_rows(31)
        self.reset()

    def reset(self):
        V = self.V
        self.n = 0
        self.ref = np.zeros((V, 4))
        self.q, self.p = np.zeros((RING, V, 4)), np.zeros((RING, V, 3))
        self.sp, self.dir = np.zeros((RING, 2)), np.zeros((RING, 2))
        self.hips = np.zeros((60, 3), np.float32)
        self.emitted = 0

    # -- the fit of one series at frame j of the prefix of n frames; get(i) reads sample i
    @staticmethod
    def _fit(H, j, n, get):
        W = H.shape[0]
        h = W // 2
        if j < h:
            start, row = 0, j
        elif j > n - 1 - h:
            start, row = n - W, j - (n - W)
        else:
            start, row = j - h, h
        acc = 0.0
        for k in range(W):
            acc += H[row, k] * get(start + k)
        return acc

    def _root(self, j, n):
        """Root position (3,), root rotation (4,), hips position (3,) and rotation (4,) local to the root, at frame j."""
        px = self._fit(self.H15, j, n, lambda i: self.sp[i % RING, 0])
        pz = self._fit(self.H15, j, n, lambda i: self.sp[i % RING, 1])
        dx = self._fit(self.H31, j, n, lambda i: self.dir[i % RING, 0])
        dz = self._fit(self.H31, j, n, lambda i: self.dir[i % RING, 1])
        ln = np.sqrt(dx * dx + dz * dz)
        dx, dz = dx / ln, dz / ln
        # between([0,0,1], d) = [sqrt(|z|^2 |d|^2) + d.z, cross(z, d)]; normalize(x) = x / (|x| + 1e-8)
        b = np.array([np.sqrt(1.0 * (dx * dx + dz * dz)) + dz, -0.0, dx, 0.0])
        R = b / (np.sqrt(b[0] * b[0] + b[1] * b[1] + b[2] * b[2] + b[3] * b[3]) + 1e-8)
        rp = np.array([px, 0.0, pz])
        s = j % RING
        Ri = q_inv(R)
        return rp, R, q_mul_vec(Ri, self.p[s, 0] - rp), q_mul(Ri, self.q[s, 0])

    def push(self, rot, pos):
        """rot (V,3) degrees or (V,4), pos (V,3): fp32 values.  Returns None while warming, else the emitted frame as a dict."""
        V, par = self.V, self.par
        rot = np.asarray(rot, np.float32).astype(np.float64)
        pos = np.asarray(pos, np.float32).astype(np.float64)
        s = self.n % RING
        for v in range(V):
            q = from_euler_deg(rot[v], self.order) if self.order is not None else rot[v].copy()
            if self.n > 0 and np.sum(q * self.ref[v]) < 0.0:      # quat.unroll: d0 < d1 with d1 == -d0 exactly
                q = -q
            self.ref[v] = q
            self.q[s, v] = q
            self.p[s, v] = pos[v] * self.scale
        gr, gp = [None] * V, [None] * V
        gr[0], gp[0] = self.q[s, 0], self.p[s, 0]
        for v in range(1, V):
            gp[v] = q_mul_vec(gr[par[v]], self.p[s, v]) + gp[par[v]]
            gr[v] = q_mul(gr[par[v]], self.q[s, v])
        spine, sl, sr, hl, hr = self.roles
        self.sp[s] = gp[spine][[0, 2]]
        a = (gp[sl] - gp[sr]) + (gp[hl] - gp[hr])
        d = np.array([-a[2], a[0]])                               # [1,0,1] * cross(across, [0,1,0])
        self.dir[s] = d / np.sqrt(d[0] * d[0] + d[1] * d[1])
        self.n += 1
        n = self.n
        if n < FIRST:
            return None

        t = n - 1 - self.L
        J = V + 1
        jp = [-1] + [p + 1 for p in par]
        lo, hi = t - 4, min(t + 3, n - 1)
        root = {j: self._root(j, n) for j in range(lo, hi + 1)}

        def P(j, b):
            return root[j][0] if b == 0 else root[j][2] if b == 1 else self.p[j % RING, b - 1]

        def Q(j, b):
            return root[j][1] if b == 0 else root[j][3] if b == 1 else self.q[j % RING, b - 1]

        f = self.fps
        vlo, vhi = t - 3, min(t + 2, n - 1)
        vel, ang = {}, {}
        for j in range(vlo, min(vhi, n - 2) + 1):
            vel[j] = np.stack([0.5 * (P(j + 1, b) - P(j, b)) * f + 0.5 * (P(j, b) - P(j - 1, b)) * f for b in range(J)])
            ang[j] = np.stack([0.5 * scaled_angle_axis(q_abs(q_mul(Q(j + 1, b), q_inv(Q(j, b))))) * f +
                               0.5 * scaled_angle_axis(q_abs(q_mul(Q(j, b), q_inv(Q(j - 1, b))))) * f for b in range(J)])
        if vhi == n - 1:
            vel[n - 1] = vel[n - 2] + (vel[n - 2] - vel[n - 3])
            ang[n - 1] = ang[n - 2] + (ang[n - 2] - ang[n - 3])

        contact = np.zeros(len(self.toes), bool)
        for ci, toe in enumerate(self.toes):
            chain = []
            b = toe
            while b != -1:
                chain.append(b)
                b = jp[b]
            chain.reverse()
            votes = 0
            for jj in range(t - 3, t + 3):
                j = min(jj, n - 1)
                gp_, gr_, gv_, ga_ = P(j, 0), Q(j, 0), vel[j][0], ang[j][0]
                for b in chain[1:]:
                    lp = q_mul_vec(gr_, P(j, b))
                    ngv = q_mul_vec(gr_, vel[j][b]) + cross(ga_, lp) + gv_
                    nga = q_mul_vec(gr_, ang[j][b]) + ga_
                    gp_, gr_, gv_, ga_ = lp + gp_, q_mul(gr_, Q(j, b)), ngv, nga
                speed = np.sqrt(gv_[0] * gv_[0] + gv_[1] * gv_[1] + gv_[2] * gv_[2])
                votes += bool(speed < self.thr)
            contact[ci] = votes >= 3

        out = {"pos": np.stack([P(t, b) for b in range(J)]), "rot": np.stack([Q(t, b) for b in range(J)]),
               "vel": vel[t], "ang": ang[t], "contact": contact}
        r32 = out["rot"][0].astype(np.float32).astype(np.float64)
        out["src_rvel"] = q_mul_vec(q_inv(r32), out["vel"][0].astype(np.float32).astype(np.float64))
        out["src_rang"] = q_mul_vec(q_inv(r32), out["ang"][0].astype(np.float32).astype(np.float64))
        self.hips[self.emitted % 60] = out["pos"][1].astype(np.float32)
        self.emitted += 1
        out["src_speed"] = self._speed()
        return out

    def _speed(self):
        if self.emitted < 60:
            return 0.0
        p = np.stack([self.hips[(self.emitted + k) % 60] for k in range(60)]).astype(np.float64)   # oldest .. newest
        f = self.fps
        v = np.empty((60, 3))
        v[1:-1] = 0.5 * (p[2:] - p[1:-1]) * f + 0.5 * (p[1:-1] - p[:-2]) * f
        v[0] = v[1] - (v[3] - v[2])
        v[-1] = v[-2] + (v[-2] - v[-3])
        acc = 0.0
        for k in range(60):
            acc += np.sqrt(v[k, 0] * v[k, 0] + v[k, 1] * v[k, 1] + v[k, 2] * v[k, 2])
        return acc / 60.0


# the synthetic walk the fixture and the GPU tests push: the package's own generator (Euler degrees 'zyx' + centimetres)
walk_clip = raw_walk_clip


def euler_to_quat(rot, order="zyx"):
    """The clip's rotations as fp32 quaternions (frames, V, 4), NOT unrolled: the quaternion input format of the front end."""
    o = [AXIS[a] for a in order]
    F, V = rot.shape[:2]
    return np.stack([np.stack([from_euler_deg(rot[f, v], o) for v in range(V)]) for f in range(F)]).astype(np.float32)
