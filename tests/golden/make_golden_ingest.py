#!/usr/bin/env python3
"""Generate tests/golden/live_ingest.npz by running THE REFERENCE'S OWN process_data (preprocess/generate_database.py, motion/quat.py;
needs scipy) on every prefix of one clip.

    MOCHA_REFERENCE=/path/to/the/reference/checkout python tests/golden/make_golden_ingest.py

The clip is ingest_ref.walk_clip (synthetic.raw_walk_clip) on the 24-joint 'mocha' skeleton: 100 frames of Euler degrees ('zyx') and centimetres, rounded to fp32.
For every prefix length n = 31 .. 100 the script calls process_data(prefix, window=n, window_step=n), which returns the processed prefix
as one window without padding, and keeps frame n-1-L of it for L in LOOKAHEAD.  No reference source or bytecode is written anywhere; the
fixture is data only.

Contents:
  rot (100,24,3) fp32 degrees, pos (100,24,3) fp32 centimetres, order 'zyx', parents (24,), names
  lookahead (4,) = 0, 2, 7, 18
  out_pos / out_vel / out_ang (4,70,25,3), out_rot (4,70,25,4) float64, out_contact (4,70,2) bool: [l, n-31] = frame n-1-L[l] of prefix n
  full_pos / full_vel / full_ang / full_rot / full_contact: the whole 100-frame clip processed at once

The run asserts what the issue asks of the clip - every toe has at least two contact transitions among the stored frames, the heading turns
through at least 90 degrees and stays 30 degrees away from -z, one bone's quaternion is flipped by unroll - and the conditions that keep
the reference single-valued: every toe speed that enters a stored contact is at least 1e-3 away from the threshold, every length that
quat.log (to_scaled_angle_axis) branches on and every length of quat.between's result is exactly 0 or >= 1e-3, and |w| >= 1e-3 wherever
quat.abs branches."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, os.path.dirname(HERE))
import ingest_ref as R  # noqa: E402  (the clip synthesis only; the arithmetic below is the reference's)

REF = os.environ.get("MOCHA_REFERENCE")
if not REF:
    sys.exit("set MOCHA_REFERENCE to the reference checkout")
sys.path.insert(0, os.path.join(REF, "motion"))
sys.path.insert(0, os.path.join(REF, "preprocess"))
import quat  # noqa: E402
import generate_database as G  # noqa: E402

NAMES = ["Hips", "LeftUpLeg", "LeftLeg", "LeftFoot", "LeftToeBase", "Spine", "Spine1", "Spine2", "Spine3", "LeftShoulder", "LeftArm",
         "LeftForeArm", "LeftHand", "Neck", "Neck1", "Head", "RightShoulder", "RightArm", "RightForeArm", "RightHand", "RightUpLeg",
         "RightLeg", "RightFoot", "RightToeBase"]
PARENTS = np.array([-1, 0, 1, 2, 3, 0, 5, 6, 7, 8, 9, 10, 11, 8, 13, 14, 8, 16, 17, 18, 0, 20, 21, 22])
LOOKAHEAD = np.array([0, 2, 7, 18])
F, MARGIN, THRESHOLD = 100, 1e-3, 0.5
TOES = [NAMES.index("LeftToeBase") + 1, NAMES.index("RightToeBase") + 1]


class Watch:
    """quat.log / quat.abs / quat.between / quat.unroll / quat.fk_vel wrapped to record what they branch on; the wrapped functions are
    the reference's."""

    def __init__(self):
        self.len, self.w, self.between, self.flips, self.gvel = [], [], [], 0, None
        log, ab, between, unroll, fk_vel = quat.log, quat.abs, quat.between, quat.unroll, quat.fk_vel

        def w_log(x, eps=1e-5):
            self.len.append(np.sqrt(np.sum(np.square(x[..., 1:]), axis=-1)).ravel())
            return log(x, eps)

        def w_abs(x):
            self.w.append(np.abs(x[..., 0]).ravel())
            return ab(x)

        def w_between(x, y):
            r = between(x, y)
            self.between.append(np.sqrt(np.sum(r * r, axis=-1)).ravel())
            return r

        def w_unroll(x):
            y = unroll(x)
            self.flips = np.any(np.sum(x * y, axis=-1) < 0, axis=0)
            return y

        def w_fk_vel(*a):
            r = fk_vel(*a)
            self.gvel = r[2]
            return r
        quat.log, quat.abs, quat.between, quat.unroll, quat.fk_vel = w_log, w_abs, w_between, w_unroll, w_fk_vel

    def check(self):
        ln, w, b = np.concatenate(self.len), np.concatenate(self.w), np.concatenate(self.between)
        assert np.all((ln == 0.0) | (ln >= MARGIN)), ("a log length between 0 and the margin", ln[(ln > 0) & (ln < MARGIN)])
        assert np.all((b == 0.0) | (b >= MARGIN)), ("a between length between 0 and the margin", b.min())
        assert np.all(w >= MARGIN), ("quat.abs with |w| below the margin", w.min())
        return float(ln[ln > 0].min()), float(w.min()), float(b.min()), int((ln == 0).sum())


def process(rot, pos, watch):
    """The reference on one clip: five (n, ...) arrays.  process_data scales the positions it is given in place, hence the copies."""
    n = len(rot)
    d = {"rotations": rot.astype(np.float64), "positions": pos.astype(np.float64), "order": "zyx", "names": NAMES, "parents": PARENTS}
    w, parents, names = G.process_data(d, window=n, window_step=n)
    assert all(len(x) == 1 and len(x[0]) == n for x in w), "process_data padded or split the prefix"
    assert list(parents) == [-1] + list(PARENTS + 1) and names[0] == "Root"
    return [np.array(x[0]) for x in w], np.sqrt(np.sum(watch.gvel[:, TOES] ** 2, axis=-1))


def main():
    rot, pos = R.walk_clip(PARENTS, F)
    watch = Watch()
    nl, nn = len(LOOKAHEAD), F - R.FIRST + 1
    out = {"pos": np.empty((nl, nn, 25, 3)), "vel": np.empty((nl, nn, 25, 3)), "rot": np.empty((nl, nn, 25, 4)), "ang": np.empty((nl, nn, 25, 3)),
           "contact": np.empty((nl, nn, 2), bool)}
    near = []
    for n in range(R.FIRST, F + 1):
        (p, v, r, a, c), toe = process(rot[:n], pos[:n], watch)
        for li, L in enumerate(LOOKAHEAD):
            t = n - 1 - L
            for k, x in (("pos", p), ("vel", v), ("rot", r), ("ang", a), ("contact", c)):
                out[k][li, n - R.FIRST] = x[t]
            near.append(np.abs(toe[np.clip(np.arange(t - 3, t + 3), 0, n - 1)] - THRESHOLD).min())
    try:
        G.process_data({"rotations": rot[:30].astype(np.float64), "positions": pos[:30].astype(np.float64), "order": "zyx", "names": NAMES,
                        "parents": PARENTS}, window=30, window_step=30)
        raise AssertionError("a 30-frame prefix ran: the first emission is not push 31")
    except ValueError:
        pass
    (fp, fv, fr, fa, fc), _ = process(rot, pos, watch)
    flips = watch.flips
    min_len, min_w, min_between, zeros = watch.check()
    assert min(near) >= MARGIN, ("a toe speed within the margin of the threshold enters a stored contact", min(near))
    assert flips.any(), "no bone crosses a sign flip of unroll"
    for li in range(nl):
        for toe in range(2):
            tr = int(np.sum(out["contact"][li, 1:, toe] != out["contact"][li, :-1, toe]))
            assert tr >= 2, ("a toe with fewer than two contact transitions", int(LOOKAHEAD[li]), toe, tr)
    # the heading: the angle of the root's z axis about y, over the stored frames
    z = quat.mul_vec(fr[12:, 0], np.array([0.0, 0.0, 1.0]))
    head = np.degrees(np.unwrap(np.arctan2(z[:, 0], z[:, 2])))
    assert head.max() - head.min() >= 90.0, ("the heading turns through less than 90 degrees", head.min(), head.max())
    assert np.all(np.abs((head % 360.0) - 180.0) >= 30.0), "the heading comes within 30 degrees of -z"
    np.savez_compressed(os.path.join(HERE, "live_ingest.npz"), rot=rot, pos=pos, order="zyx", parents=PARENTS.astype(np.int32),
                        names=np.array(NAMES), lookahead=LOOKAHEAD.astype(np.int32),
                        out_pos=out["pos"], out_vel=out["vel"], out_rot=out["rot"], out_ang=out["ang"], out_contact=out["contact"],
                        full_pos=fp, full_vel=fv, full_rot=fr, full_ang=fa, full_contact=fc)
    print(f"live_ingest.npz: {nn} prefixes x {nl} lookaheads; bones flipped by unroll {np.flatnonzero(flips).tolist()}; heading "
          f"{head.min():.1f} .. {head.max():.1f} deg; min log length > 0 {min_len:.3g} ({zeros} exactly 0), min |w| {min_w:.3g}, "
          f"min between length {min_between:.3g}, min |toe speed - {THRESHOLD}| {min(near):.3g}")


if __name__ == "__main__":
    main()
