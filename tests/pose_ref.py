"""ctypes loader of the test-only probe of the motion-side launchers (tests/gemm_probe/pose_probe.cpp, built by
`make -C tests/gemm_probe`) and one restatement per operation of what it MEANS, generic over a NumPy dtype: window featurisation
(test_fullframework.py:141-185), the pose heads of a decoded window (:303-308, 338), the per-frame clip loop (:338-437, 457-632 with
motion/Inertialization.py:300-377 and motion/quat.py:295-343) and the BVH channels (:665-687, quat.py:346-355).  float64 is the truth
for the fp32 kernels and numpy.longdouble for the float64 ones; the next narrower dtype is the evaluation that sizes a bound.  Used by
tests/test_pose_kernels.py only.  Nothing here is transcribed from the kernels: no lanes, no LDS columns, no frame-ahead fetch - a frame
is a Python loop over bones and contacts.

The clip loop also reports, per clip, the margin of every discrete decision it takes (`Decisions`): a kernel that computes the same
quantities to rounding takes the same side of each as long as the margin is far above rounding.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "gemm_probe", "libmocha_pose_probe.so")
BAD_ARGUMENT = -2
INVALID_VALUE = 1          # hipErrorInvalidValue
MAX_BONES, MAX_CONTACT, MAX_CHAIN, FEAT_MAX_BONES = 32, 4, 8, 40
STATE_DOUBLES = 8 + MAX_BONES * 3 + MAX_CONTACT * 19
DT = 1.0 / 60.0
IK = dict(max_length_buffer=0.015, foot_height=0.02, unlock_radius=0.2, halflife=0.1)

_vp, _i = C.c_void_p, C.c_int


class pp_post(C.Structure):
    _fields_ = ([(n, _vp) for n in ("heads", "speed", "src_rvel", "src_rang", "src_speed", "contact", "pos", "rot", "ik_rot", "bvh_pos",
                                    "bvh_euler", "state", "valid")] +
                [(n, _i) for n in ("n_clips", "n_frames", "V", "n_contact", "ik_enabled", "blend_enabled")] +
                [("parents", _i * MAX_BONES), ("contact_bones", _i * MAX_CONTACT)] +
                [(n, C.c_double) for n in ("dt", "max_length_buffer", "foot_height", "unlock_radius", "halflife")])


_SIGNATURES = {
    "pp_featurize_init": [],
    "pp_featurize": [_vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _vp],
    "pp_pose_heads": [_vp, _vp, _vp, _i, _i, _i, _vp],
    "pp_post_clip": [C.POINTER(pp_post), _vp],
    "pp_post_step": [C.POINTER(pp_post), _vp],
    "pp_post_state_doubles": [],
}
_lib = None


def load():
    """The probe library; a missing build is an error (no fallback)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(f"{LIB_PATH} is missing: run __graft_entry__.build() (make -C tests/gemm_probe)")
        lib = C.CDLL(LIB_PATH)
        for name, args in _SIGNATURES.items():
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = _i, args
        _lib = lib
    return _lib


def ptr(t):
    """Device (or host) address of a tensor, 0 for None."""
    return 0 if t is None else t.data_ptr()


def full_parents(parents_no_root):
    """parents = [-1] + (joint parents + 1), test_fullframework.py:101-102."""
    return np.concatenate([[-1], np.asarray(parents_no_root, dtype=np.int64) + 1]).astype(np.int32)


def longdouble_is_wider():
    """numpy.longdouble must carry more than float64 (x87 extended: eps 1.08e-19), or a float64-against-longdouble yardstick is 0 = 0."""
    return float(np.finfo(np.longdouble).eps) < 1e-18


def errors(y, ref):
    """Largest and rms error of y against ref, in ref's (wider) dtype, as Python floats."""
    d = np.asarray(y).astype(ref.dtype) - ref
    return float(np.abs(d).max()) if d.size else 0.0, float(np.sqrt(np.mean(d * d))) if d.size else 0.0


# ------------------------------------------------------------------------------------------------------------------ vectors, quaternions (w, x, y, z)
def cross(a, b):                      # motion/quat.py:3-7
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1)


def q_mul(x, y):                      # :112-120
    x0, x1, x2, x3 = (x[..., i] for i in range(4))
    y0, y1, y2, y3 = (y[..., i] for i in range(4))
    return np.stack([y0 * x0 - y1 * x1 - y2 * x2 - y3 * x3, y0 * x1 + y1 * x0 - y2 * x3 + y3 * x2,
                     y0 * x2 + y1 * x3 + y2 * x0 - y3 * x1, y0 * x3 - y1 * x2 + y2 * x1 + y3 * x0], -1)


def q_inv(q):                         # :109-110
    return np.stack([q[..., 0], -q[..., 1], -q[..., 2], -q[..., 3]], -1)


def q_rot(q, v):                      # :128-130 mul_vec
    t = 2.0 * cross(q[..., 1:], v)
    return v + q[..., :1] * t + cross(q[..., 1:], t)


def length(x):
    return np.sqrt(np.sum(x * x, -1))


def normalize(x, eps=1e-8):           # :15-16
    return x / (length(x)[..., None] + x.dtype.type(eps))


def from_angle_axis(angle, axis):     # :21-25
    return np.concatenate([[np.cos(angle / 2.0)], np.sin(angle / 2.0) * axis])


def to_xform_xy(q):                   # :42-55, the first two columns of the rotation matrix, (..., 3, 2) row-major flattened to 6
    w, x, y, z = (q[..., i] for i in range(4))
    x2, y2, z2 = x + x, y + y, z + z
    xx, yy, wx = x * x2, y * y2, w * x2
    xy, yz, wy = x * y2, y * z2, w * y2
    xz, zz, wz = x * z2, z * z2, w * z2
    return np.stack([1.0 - (yy + zz), xy - wz, xy + wz, 1.0 - (xx + zz), xz - wy, yz + wx], -1)


# ------------------------------------------------------------------------------------------------------------------ featurize
def featurize(Yrot, Ypos, Yvel, Yang, parents, dtype):
    """Local bone features of B windows (B, T, J, 4|3|3|3) -> X (B, T, J, 15) in `dtype`: forward kinematics with velocities, the root
    bone replaced by the window's last-frame root, every bone expressed in that frame, [pos 3 | rot xy 6 | vel 3 | ang 3]."""
    lr, lp, lv, la = (np.asarray(a).astype(dtype) for a in (Yrot, Ypos, Yvel, Yang))
    J = lr.shape[2]
    gr, gp, gv, ga = [lr[:, :, 0]], [lp[:, :, 0]], [lv[:, :, 0]], [la[:, :, 0]]
    for i in range(1, J):
        p = int(parents[i])
        rp = q_rot(gr[p], lp[:, :, i])
        gp.append(rp + gp[p])
        gr.append(q_mul(gr[p], lr[:, :, i]))
        gv.append(q_rot(gr[p], lv[:, :, i]) + cross(ga[p], rp) + gv[p])
        ga.append(q_rot(gr[p], la[:, :, i]) + ga[p])
    gr, gp, gv, ga = (np.stack(g, 2) for g in (gr, gp, gv, ga))
    for g in (gr, gp, gv, ga):
        g[:, :, 0] = g[:, -1:, 0]                                           # the window is rooted on its own last frame
    inv = q_inv(gr[:, :, :1])
    return np.concatenate([q_rot(inv, gp - gp[:, :, :1]), to_xform_xy(q_mul(inv, gr)), q_rot(inv, gv), q_rot(inv, ga)], -1)


# ------------------------------------------------------------------------------------------------------------------ pose heads
def quat_from_xy(c0, x1):
    """6-D rotation (first matrix column c0, second column x1, (..., 3) each) -> quaternion (quat.py:96-107 from_xform_xy, :69-94
    from_xform), the branch taken (0..3) and the smallest margin of the conditions that chose it."""
    one = c0.dtype.type(1.0)
    c2 = cross(c0, x1)
    c2 = c2 / length(c2)[..., None]
    c1 = cross(c2, c0)
    c1 = c1 / length(c1)[..., None]
    t00, t10, t20 = (c0[..., i] for i in range(3))
    t01, t11, t21 = (c1[..., i] for i in range(3))
    t02, t12, t22 = (c2[..., i] for i in range(3))
    a = np.stack([t21 - t12, one + t00 - t11 - t22, t10 + t01, t02 + t20], -1)
    b = np.stack([t02 - t20, t10 + t01, one - t00 + t11 - t22, t21 + t12], -1)
    c = np.stack([t10 - t01, t02 + t20, t21 + t12, one - t00 - t11 + t22], -1)
    d = np.stack([one + t00 + t11 + t22, t21 - t12, t02 - t20, t10 - t01], -1)
    neg = t22 < 0
    branch = np.where(neg, np.where(t00 > t11, 0, 1), np.where(t00 < -t11, 2, 3))
    q = np.where((branch == 0)[..., None], a, np.where((branch == 1)[..., None], b, np.where((branch == 2)[..., None], c, d)))
    margin = np.minimum(np.abs(t22), np.where(neg, np.abs(t00 - t11), np.abs(t00 + t11)))
    return q / (length(q)[..., None] + c0.dtype.type(1e-8)), branch, margin.astype(np.float64)


def pose_heads(Y, dtype):
    """Y (B, T, V, 15) -> heads (B, V, 13) = [pos | quat | vel | ang] of the last frame, speed (B,) = mean_t |Y[t, 0, 9:12]|, and the
    quaternion branch / branch margin per (B, V)."""
    Y = np.asarray(Y).astype(dtype)
    last = Y[:, -1]
    q, branch, margin = quat_from_xy(last[..., [3, 5, 7]], last[..., [4, 6, 8]])
    heads = np.concatenate([last[..., 0:3], q, last[..., 9:12], last[..., 12:15]], -1)
    speed = length(Y[:, :, 0, 9:12]).sum(-1) / dtype(Y.shape[1])
    return heads, speed, branch, margin


# ------------------------------------------------------------------------------------------------------------------ the clip loop
class Decisions:
    """Margins (distance of the tested quantity from its threshold, float) of every discrete decision of one clip, by kind, and how
    often each side was taken."""
    KINDS = ("ratio", "h", "radius", "reach", "foot")

    def __init__(self):
        self.margin = {k: [] for k in self.KINDS}
        self.at = (0, 0)                # (frame, hip bone) of the IK evaluation in progress
        self.r2 = []                    # per IK evaluation: (frame, hip bone, |cross(c_a, t_a)|, what one ulp of noise in t does to the hip's rotation)
        self.count = dict(ratio_reset=0, ratio_kept=0, h_small=0, h_large=0, lock=0, label_unlock=0, radius_unlock=0, reach_clamp=0,
                          reach_free=0, foot_clamp=0, foot_free=0)

    def smallest(self, kind):
        return min(self.margin[kind], default=float("inf"))

    def note(self, kind, value, threshold, taken, name_true, name_false):
        self.margin[kind].append(abs(float(value) - float(threshold)))
        self.count[name_true if taken else name_false] += 1


def _exp_half(v, dec):                # quat.py:154-164: from_scaled_angle_axis(v) = exp(v / 2)
    x = v / 2.0
    h = length(x)
    small = bool(h < 1e-5)
    dec.note("h", h, 1e-5, small, "h_small", "h_large")
    if small:
        return np.concatenate([[v.dtype.type(1.0)], x])
    return np.concatenate([[np.cos(h)], np.sin(h) / h * x])


def _clip(x):
    return np.clip(x, -1.0, 1.0)


def _two_bone(a, b, c, target, fwd, hip_gr, knee_gr, par_gr, max_length_buffer, dec):      # quat.py:295-343
    max_ext = length(a - b) + length(b - c) - max_length_buffer
    reach = length(target - a)
    over = bool(reach > max_ext)
    dec.note("reach", reach, max_ext, over, "reach_clamp", "reach_free")
    t = a + max_ext * normalize(target - a) if over else target
    axis = normalize(cross(normalize(c - a), fwd))
    lab, lcb, lat = length(b - a), length(b - c), length(t - a)
    ac_ab_0 = np.arccos(_clip(np.sum(normalize(c - a) * normalize(b - a))))
    ba_bc_0 = np.arccos(_clip(np.sum(normalize(a - b) * normalize(c - b))))
    ac_ab_1 = np.arccos(_clip((lab * lab + lat * lat - lcb * lcb) / (2.0 * lab * lat)))
    ba_bc_1 = np.arccos(_clip((lab * lab + lcb * lcb - lat * lat) / (2.0 * lab * lcb)))
    r0 = from_angle_axis(ac_ab_1 - ac_ab_0, axis)
    r1 = from_angle_axis(ba_bc_1 - ba_bc_0, axis)
    c_a, t_a = normalize(c - a), normalize(t - a)
    swing = np.arccos(_clip(np.sum(c_a * t_a)))
    r2 = from_angle_axis(swing, normalize(cross(c_a, t_a)))
    # With the target on the heel (a contact that has not locked: t = toe + (heel - toe)) c_a and t_a are the same direction, yet swing is
    # not 0 but acos(1 - 2e-8 / |c - a|) = 2e-4 / sqrt(|c - a|) (normalize's eps), and the axis is cross / (|cross| + 1e-8): a t that
    # misses the heel by a few float64 ulps - which the rounding of toe + (heel - toe) decides - turns the hip by sin(swing / 2) times
    # 4 ulps of the positions over |c - a| over 1e-8, about 1e-12 to 1e-10, where the rest of the loop carries 1e-15
    noise = np.sin(swing / 2.0) * (4.0 * 2.220446049250313e-16 * (length(a) + length(c)) / length(c - a)) / 1e-8
    dec.r2.append((dec.at[0], dec.at[1], float(length(cross(c_a, t_a))), float(noise)))
    return q_mul(q_inv(par_gr), q_mul(r2, q_mul(r0, hip_gr))), q_mul(q_inv(hip_gr), q_mul(r1, knee_gr))


def _chain(parents, bone):
    out = []
    while bone != -1:
        out.append(int(bone))
        bone = parents[bone]
    return out                        # bone, its parent, ..., the root


def run_clip(heads, speed, src_rvel, src_rang, src_speed, contact, parents, contact_bones, dtype, dt=DT, max_length_buffer=0.015,
             foot_height=0.02, unlock_radius=0.2, halflife=0.1, ik_enabled=True, blend=True):
    """All frames of one clip: heads (N, V, 13) fp32, speed / src_speed (N,) fp32, src_rvel / src_rang (N, 3) fp32, contact
    (N, n_contact) -> pos (N, V+1, 3), rot, ik_rot (N, V+1, 4) in `dtype`, and the clip's Decisions.  The speed ratio is fp32 arithmetic
    in every dtype: it is defined on the fp32 network output (test_fullframework.py:492-496)."""
    D = dtype
    N, V = heads.shape[:2]
    J = V + 1
    dt, mlb, fh, radius = D(dt), D(max_length_buffer), D(foot_height), D(unlock_radius)
    y = (D(4.0) * np.log(D(2.0))) / (D(halflife) + D(1e-5)) / D(2.0)          # Inertialization.py:13-14
    ydt = y * dt
    e = D(1.0) / (D(1.0) + ydt + D(0.48) * ydt * ydt + D(0.235) * ydt * ydt * ydt)       # :10-11
    dec = Decisions()
    POS, ROT, IKR = np.zeros((N, J, 3), D), np.zeros((N, J, 4), D), np.zeros((N, J, 4), D)
    root_pos, root_rot = np.zeros(3, D), np.array([1, 0, 0, 0], D)
    prev = None
    cons = []
    up = np.array([0, 1, 0], D)
    for i in range(N):
        h = np.asarray(heads[i]).astype(D)
        ratio = np.float32(speed[i]) / np.float32(src_speed[i])
        reset = bool(ratio > np.float32(3.0) or ratio < np.float32(0.33))
        dec.margin["ratio"].append(min(abs(float(ratio) - 3.0), abs(float(ratio) - float(np.float32(0.33)))))
        dec.count["ratio_reset" if reset else "ratio_kept"] += 1
        if reset:
            ratio = np.float32(1.0)
        rv = (np.asarray(src_rvel[i], np.float32) * ratio).astype(D)
        ra = np.asarray(src_rang[i]).astype(D)
        wv, wa = q_rot(root_rot, rv), q_rot(root_rot, ra)
        root_pos = root_pos + wv * dt
        root_rot = q_mul(root_rot, _exp_half(wa * dt, dec))
        pos = np.concatenate([root_pos[None], h[:, 0:3]])
        rot = np.concatenate([root_rot[None], h[:, 3:7]])
        vel = np.concatenate([wv[None], h[:, 7:10]])
        ang = np.concatenate([wa[None], h[:, 10:13]])
        if prev is None:
            for toe in contact_bones:                                       # fk_vel of the toe, quat.py:207-238
                ch = _chain(parents, toe)[::-1]
                gp, gv, gr, ga = pos[0], vel[0], rot[0], ang[0]
                for b in ch[1:]:
                    rp = q_rot(gr, pos[b])
                    gv = gv + q_rot(gr, vel[b]) + cross(ga, rp)
                    ga = q_rot(gr, ang[b]) + ga
                    gp = rp + gp
                    gr = q_mul(gr, rot[b])
                cons.append(dict(state=False, lock=False, position=gp.copy(), velocity=gv.copy(), point=gp.copy(), target=gp.copy(),
                                 off_x=np.zeros(3, D), off_v=np.zeros(3, D)))
            prev = pos
            POS[i], ROT[i], IKR[i] = pos, rot, rot
            continue
        cur = (prev + vel * dt) * 0.5 + pos * 0.5 if blend else pos
        ik = rot.copy()
        if ik_enabled:
            for ci, toe in enumerate(contact_bones):
                ch = _chain(parents, toe)
                heel, knee, hip, par = ch[1], ch[2], ch[3], ch[4]
                gp, gr = {}, {}
                for b in ch[::-1]:
                    p = parents[b]
                    gp[b], gr[b] = (cur[b], rot[b]) if p == -1 else (q_rot(gr[p], cur[b]) + gp[p], q_mul(gr[p], rot[b]))
                c = cons[ci]
                in_pos, in_state = gp[toe], bool(contact[i][ci])
                in_vel = (in_pos - c["target"]) / (dt + D(1e-8))            # Inertialization.py:300-377
                c["target"] = in_pos
                j1 = c["off_v"] + c["off_x"] * y
                c["off_x"], c["off_v"] = e * (c["off_x"] + j1 * dt), e * (c["off_v"] - j1 * y * dt)
                if c["lock"]:
                    c["position"], c["velocity"] = c["point"] + c["off_x"], c["off_v"].copy()
                else:
                    c["position"], c["velocity"] = in_pos + c["off_x"], in_vel + c["off_v"]
                unlock = False
                if c["lock"]:
                    dist = length(c["point"] - in_pos)
                    unlock = bool(dist > radius)
                    dec.margin["radius"].append(abs(float(dist) - float(radius)))
                if not c["state"] and in_state:
                    dec.count["lock"] += 1
                    c["lock"] = True
                    c["point"] = c["position"].copy()
                    c["point"][1] = fh
                    c["off_x"], c["off_v"] = (in_pos + c["off_x"]) - c["point"], in_vel + c["off_v"]
                elif (c["lock"] and c["state"] and not in_state) or unlock:
                    dec.count["radius_unlock" if unlock else "label_unlock"] += 1
                    c["lock"] = False
                    c["off_x"], c["off_v"] = (c["point"] + c["off_x"]) - in_pos, c["off_v"] - in_vel
                c["state"] = in_state
                below = bool(c["position"][1] < fh)
                dec.note("foot", c["position"][1], fh, below, "foot_clamp", "foot_free")
                if below:
                    c["position"][1] = fh
                dec.at = (i, hip)
                ik[hip], ik[knee] = _two_bone(gp[hip], gp[knee], gp[heel], c["position"] + (gp[heel] - gp[toe]), q_rot(gr[knee], up),
                                              gr[hip], gr[knee], gr[par], mlb, dec)
        prev = cur
        POS[i], ROT[i], IKR[i] = cur, rot, ik
    return POS, ROT, IKR, dec


# ------------------------------------------------------------------------------------------------------------------ BVH channels
def bvh_channels(pos, rot, ik_rot, dtype):
    """pos (N, J, 3), rot / ik_rot (N, J, 4) -> BVH positions (N, V, 3), Euler angles in degrees (N, V, 3) and the asin argument before
    its clamp (N, V): the synthetic root (pos[:, 0], rot[:, 0]) folded into bone 1, quat.py:346-355 on the IK rotations."""
    pos, rot, ik = (np.asarray(a).astype(dtype) for a in (pos, rot, ik_rot))
    p, r = pos[:, 1:].copy(), ik[:, 1:].copy()
    p[:, 0] = q_rot(rot[:, 0], pos[:, 1]) + pos[:, 0]
    r[:, 0] = q_mul(rot[:, 0], ik[:, 1])
    w, x, y, z = (r[..., i] for i in range(4))
    s = 2.0 * (w * y - z * x)
    deg = dtype(180.0) / (dtype(4.0) * np.arctan(dtype(1.0)))
    eu = np.stack([np.arctan2(2.0 * (w * x + y * z), 1.0 - 2.0 * (x * x + y * y)), np.arcsin(_clip(s)),
                   np.arctan2(2.0 * (w * z + x * y), 1.0 - 2.0 * (y * y + z * z))], -1) * deg
    return p, eu, s.astype(np.float64)


def euler_to_quat(eu_deg):
    """Inverse of the channel convention above (R = Rz(e2) Ry(e1) Rx(e0)), float64: (..., 3) degrees -> (..., 4)."""
    e = np.radians(np.asarray(eu_deg, np.float64)) / 2.0
    cx, sx, cy, sy, cz, sz = np.cos(e[..., 0]), np.sin(e[..., 0]), np.cos(e[..., 1]), np.sin(e[..., 1]), np.cos(e[..., 2]), np.sin(e[..., 2])
    return np.stack([cz * cy * cx + sz * sy * sx, cz * cy * sx - sz * sy * cx, cz * sy * cx + sz * cy * sx, sz * cy * cx - cz * sy * sx], -1)
