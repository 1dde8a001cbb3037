"""NumPy float64 restatement of the whole-clip mocap front end (mocha_ingest_clips, mocha_clip_windows; process_data with mirror = False /
True and divide_clip(divide=True) of the reference's preprocess/generate_database.py:40-177).

One clip at a time, every stage over all its frames at once, in the reference's own order: from_euler (or the quaternion as given) ->
unroll, frame after frame -> [animation_mirror: fk, mirror_pos * gpos[map], from_xform(mirror_rot * to_xform(grot[map])), ik; unroll again]
-> fk -> spine joint on xz, projected across-direction -> the 15 / 31-tap cubic fits with ingest_ref.fit_rows (first window, centre row, last
window) -> root rotation, root-local hips -> central differences with v[0] = v[1] - (v[3] - v[2]), v[-1] = v[-2] + (v[-2] - v[-3]) ->
fk_vel, toe speed < threshold -> "at least 3 of t-3 .. t+2, indices clamped to the clip".  Arrays are component-first inside (4 | 3, frames,
joints) so that ingest_ref's q_mul / q_mul_vec / cross apply to whole clips.

Measured deviation from the reference's own process_data on tests/golden/clip_ingest.npz (lengths 31, 32, 45, 62, 100; pos / vel / rot / ang,
25 bones), as test_clip_ingest_ref.py::test_fixture prints and asserts it (run of 2026-10-20: NumPy on x86-64, scipy 1.15.3 behind the
fixture): see E and E_MIRROR below.
"""
from __future__ import annotations

import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ingest_ref as R  # noqa: E402
from ingest_ref import cross, q_inv, q_mul, q_mul_vec  # noqa: E402

FIRST = R.FIRST
# Largest |restatement - reference| over the fixture's plain cases: pos 6.36e-15, vel 1.87e-13, rot 2.78e-16, ang 3.33e-14 - the velocity
# leads, as in ingest_ref: 60 x a difference of root positions whose fits differ from scipy's polyfit in the last bits.  E is the largest
# of the four, rounded up in its second digit; it equals ingest_ref.E.
E = 1.9e-13
# ... and over the mirrored cases: pos 6.30e-15, vel 1.82e-13, rot 3.33e-16, ang 2.53e-14.  Mirroring adds nothing measurable: the
# to_xform / from_xform / ik chain is the reference's expression for expression.
E_MIRROR = 1.9e-13


def euler_to_quat(rot, order):
    """quat.from_euler(np.radians(rot), order) on (F, V, 3) degrees -> (4, F, V)."""
    r = np.asarray(rot, np.float64) * (np.pi / 180.0)
    qs = []
    for k in range(3):
        q = np.zeros((4,) + r.shape[:2])
        q[0] = np.cos(r[..., k] / 2.0)
        q[1 + order[k]] = np.sin(r[..., k] / 2.0)
        qs.append(q)
    return q_mul(qs[0], q_mul(qs[1], qs[2]))


def unroll(q):
    """quat.unroll on (4, F, V): frame after frame, negate when the dot product with the (already unrolled) previous frame is negative."""
    y = q.copy()
    for i in range(1, y.shape[1]):
        d = ((y[0, i] * y[0, i - 1] + y[1, i] * y[1, i - 1]) + y[2, i] * y[2, i - 1]) + y[3, i] * y[3, i - 1]
        y[:, i, d < 0.0] = -y[:, i, d < 0.0]
    return y


def fk(q, p, par):
    gq, gp = [q[:, :, 0]], [p[:, :, 0]]
    for v in range(1, len(par)):
        gp.append(q_mul_vec(gq[par[v]], p[:, :, v]) + gp[par[v]])
        gq.append(q_mul(gq[par[v]], q[:, :, v]))
    return np.stack(gq, axis=2), np.stack(gp, axis=2)


def to_xform(q):
    """quat.to_xform: rows of the matrix as a 3 x 3 list of arrays."""
    qw, qx, qy, qz = q
    x2, y2, z2 = qx + qx, qy + qy, qz + qz
    xx, yy, wx = qx * x2, qy * y2, qw * x2
    xy, yz, wy = qx * y2, qy * z2, qw * y2
    xz, zz, wz = qx * z2, qz * z2, qw * z2
    return [[1.0 - (yy + zz), xy - wz, xz + wy], [xy + wz, 1.0 - (xx + zz), yz - wx], [xz - wy, yz + wx, 1.0 - (xx + yy)]]


def from_xform(m):
    """quat.from_xform with its four branches and the final normalize (x / (|x| + 1e-8))."""
    a = np.stack([m[2][1] - m[1][2], 1.0 + m[0][0] - m[1][1] - m[2][2], m[1][0] + m[0][1], m[0][2] + m[2][0]])
    b = np.stack([m[0][2] - m[2][0], m[1][0] + m[0][1], 1.0 - m[0][0] + m[1][1] - m[2][2], m[2][1] + m[1][2]])
    c = np.stack([m[1][0] - m[0][1], m[0][2] + m[2][0], m[2][1] + m[1][2], 1.0 - m[0][0] - m[1][1] + m[2][2]])
    d = np.stack([1.0 + m[0][0] + m[1][1] + m[2][2], m[2][1] - m[1][2], m[0][2] - m[2][0], m[1][0] - m[0][1]])
    x = np.where(m[2][2] < 0.0, np.where(m[0][0] > m[1][1], a, b), np.where(m[0][0] < -m[1][1], c, d))
    return x / (np.sqrt(((x[0] * x[0] + x[1] * x[1]) + x[2] * x[2]) + x[3] * x[3]) + 1e-8)


def mirror(q, p, par, mp):
    """animation_mirror (generate_database.py:40-55) with the joint exchange mp."""
    gq, gp = fk(q, p, par)
    gpm = gp[:, :, mp] * np.array([-1.0, 1.0, 1.0])[:, None, None]
    m = to_xform(gq[:, :, mp])
    sign = [[-1.0, -1.0, 1.0], [1.0, 1.0, -1.0], [1.0, 1.0, -1.0]]
    gqm = from_xform([[sign[i][j] * m[i][j] for j in range(3)] for i in range(3)])
    lq, lp = [gqm[:, :, 0]], [gpm[:, :, 0]]
    for v in range(1, len(par)):                                  # quat.ik
        pi = q_inv(gqm[:, :, par[v]])
        lq.append(q_mul(pi, gqm[:, :, v]))
        lp.append(q_mul_vec(pi, gpm[:, :, v] - gpm[:, :, par[v]]))
    return np.stack(lq, axis=2), np.stack(lp, axis=2)


def fit_series(H, x):
    """savgol_filter(x, W, 3, mode='interp') on (n,): the centre row inside, the first / last window's own rows within half a window of an end."""
    W, n = H.shape[0], len(x)
    h = W // 2
    out = np.empty(n)
    for j in range(n):
        if j < h:
            start, row = 0, j
        elif j > n - 1 - h:
            start, row = n - W, j - (n - W)
        else:
            start, row = j - h, h
        acc = 0.0
        for k in range(W):
            acc += H[row, k] * x[start + k]
        out[j] = acc
    return out


def scaled_angle_axis(q, eps=1e-5):
    ln = np.sqrt((q[1] * q[1] + q[2] * q[2]) + q[3] * q[3])
    with np.errstate(invalid="ignore", divide="ignore"):
        h = np.where(ln < eps, 1.0, np.arctan2(ln, q[0]) / ln)
    return 2.0 * (h * q[1:])


def q_abs(q):
    return np.where(q[0] > 0.0, q, -q)


_H = {}


def process_clip(rot, pos, parents, order, roles, toes, unit_scale=0.01, fps=60.0, threshold=0.5, mirror_map=None):
    """One clip: rot (n,V,3) degrees or (n,V,4), pos (n,V,3), fp32 values.  Returns pos / vel / ang (n,V+1,3), rot (n,V+1,4) float64 and
    contact (n, len(toes)) bool.  ``order``: None for quaternion input, else a string like 'zyx'; ``toes``: bones of the (V+1)-bone skeleton."""
    par = [int(x) for x in parents]
    n, V = len(rot), len(par)
    assert n >= FIRST, "savgol_filter(window_length=31) refuses a shorter clip"
    rot = np.asarray(rot, np.float32).astype(np.float64)
    p = (np.asarray(pos, np.float32).astype(np.float64) * unit_scale).transpose(2, 0, 1)
    q = rot.transpose(2, 0, 1) if order is None else euler_to_quat(rot, [R.AXIS[a] for a in order])
    q = unroll(q)
    if mirror_map is not None:
        q, p = mirror(q, p, par, [int(x) for x in mirror_map])
        q = unroll(q)
    gq, gp = fk(q, p, par)
    spine, sl, sr, hl, hr = roles
    a = (gp[:, :, sl] - gp[:, :, sr]) + (gp[:, :, hl] - gp[:, :, hr])
    d = np.stack([-a[2], a[0]])                                   # [1,0,1] * cross(across, [0,1,0])
    d = d / np.sqrt(d[0] * d[0] + d[1] * d[1])
    if not _H:
        _H[15], _H[31] = R.fit_rows(15), R.fit_rows(31)
    px, pz = fit_series(_H[15], gp[0, :, spine]), fit_series(_H[15], gp[2, :, spine])
    dx, dz = fit_series(_H[31], d[0]), fit_series(_H[31], d[1])
    ln = np.sqrt(dx * dx + dz * dz)
    dx, dz = dx / ln, dz / ln
    zero = np.zeros(n)
    b = np.stack([np.sqrt(1.0 * (dx * dx + dz * dz)) + dz, zero, dx, zero])     # between([0,0,1], d)
    Rq = b / (np.sqrt(((b[0] * b[0] + b[1] * b[1]) + b[2] * b[2]) + b[3] * b[3]) + 1e-8)
    rp = np.stack([px, zero, pz])
    Ri = q_inv(Rq)
    P = np.concatenate([rp[:, :, None], q_mul_vec(Ri, p[:, :, 0] - rp)[:, :, None], p[:, :, 1:]], axis=2)      # (3, n, V+1)
    Q = np.concatenate([Rq[:, :, None], q_mul(Ri, q[:, :, 0])[:, :, None], q[:, :, 1:]], axis=2)
    vel, ang = np.empty_like(P), np.empty_like(P)
    vel[:, 1:-1] = 0.5 * (P[:, 2:] - P[:, 1:-1]) * fps + 0.5 * (P[:, 1:-1] - P[:, :-2]) * fps
    ang[:, 1:-1] = (0.5 * scaled_angle_axis(q_abs(q_mul(Q[:, 2:], q_inv(Q[:, 1:-1])))) * fps +
                    0.5 * scaled_angle_axis(q_abs(q_mul(Q[:, 1:-1], q_inv(Q[:, :-2])))) * fps)
    for x in (vel, ang):
        x[:, 0] = x[:, 1] - (x[:, 3] - x[:, 2])
        x[:, -1] = x[:, -2] + (x[:, -2] - x[:, -3])
    jp = [-1] + [x + 1 for x in par]
    gr_, gv_, ga_ = [Q[:, :, 0]], [vel[:, :, 0]], [ang[:, :, 0]]
    for bn in range(1, V + 1):                                    # quat.fk_vel
        pr = jp[bn]
        lp = q_mul_vec(gr_[pr], P[:, :, bn])
        gv_.append(q_mul_vec(gr_[pr], vel[:, :, bn]) + cross(ga_[pr], lp) + gv_[pr])
        ga_.append(q_mul_vec(gr_[pr], ang[:, :, bn]) + ga_[pr])
        gr_.append(q_mul(gr_[pr], Q[:, :, bn]))
    contact = np.zeros((n, len(toes)), bool)
    idx = np.clip(np.arange(n)[:, None] + np.arange(-3, 3)[None], 0, n - 1)
    for ci, toe in enumerate(toes):
        g = gv_[toe]
        below = np.sqrt((g[0] * g[0] + g[1] * g[1]) + g[2] * g[2]) < threshold
        contact[:, ci] = below[idx].sum(axis=1) >= 3
    return {"pos": P.transpose(1, 2, 0), "vel": vel.transpose(1, 2, 0), "rot": Q.transpose(1, 2, 0), "ang": ang.transpose(1, 2, 0),
            "contact": contact}


def window_count(n, window, step):
    return len(range(0, n - window // 4, step))


def divide(x, window, step, zero_pad=False):
    """divide_clip(x, window, step, vel_ang=zero_pad, divide=True) on (n, ...): (windows, window, ...)."""
    out = []
    for j in range(0, len(x) - window // 4, step):
        s = x[j:j + window]
        m = len(s)
        if m < window:
            left = np.repeat(s[:1], (window - m) // 2 + (window - m) % 2, axis=0)
            right = np.repeat(s[-1:], (window - m) // 2, axis=0)
            if zero_pad:
                left, right = np.zeros_like(left), np.zeros_like(right)
            s = np.concatenate([left, s, right], axis=0)
        out.append(s)
    return np.stack(out)


def windows(processed, window=60, step=1):
    """The five window stacks of one processed clip, keyed as clip_windows returns them."""
    return {"Ypos": divide(processed["pos"], window, step), "Yvel": divide(processed["vel"], window, step, True),
            "Yrot": divide(processed["rot"], window, step), "Yang": divide(processed["ang"], window, step, True),
            "contact": divide(processed["contact"], window, step)}
