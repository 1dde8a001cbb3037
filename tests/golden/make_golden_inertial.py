#!/usr/bin/env python3
"""Generate tests/golden/inertialize.npz by running THE REFERENCE'S OWN inertializers (motion/Inertialization.py, motion/quat.py).

    MOCHA_REFERENCE=/path/to/the/reference/checkout python tests/golden/make_golden_inertial.py

The eight functions a bone's inertializer consists of - inertialize_transition_pos / _rot, inertialize_update_pos / _rot and, through
them, decay_spring_damper_exact_pos / _rot, fast_negexpf and halflife_to_damping - are driven per stream, per frame and per bone, in the
order pose_transition -> pose_update; this script only decides WHEN a stream transitions (the seen / active / valid rules of
include/mocha_hip.h) and stores arrays.  No reference source or bytecode is written anywhere; the fixture is data only.

Contents (V = 22, 24 frames, 3 streams, inputs rounded to fp32):
  heads (24,3,22,13) fp32, ids (24,3) int32   the main run at half-life 0.1: stream 0 never transitions, stream 1 transitions at frames 5
                                              and 6 (consecutive) and 9 (while still decaying), stream 2 at frames 4 and 16
  out (24,3,22,13), off_pos / off_vel / off_ang (24,3,22,3), off_rot (24,3,22,4)   float64, after every frame of the main run
  hl (4,), hl_trigger (4,24), hl_valid (4,24) int32, hl_out (4,24,22,13) float64   stream 2 alone at half-lives 0.02, 0.1, 1.0 and 0,
                                              transitions given as triggers, frames with hl_valid == 0 are warming (rows NaN)
Planted cases: bone 0 of stream 1 keeps its rotation from frame 4 to 5 (a transition between identical rotations: the len < eps branch
of quat.log); bone 1 of stream 2 meets the antipodal quaternion at frame 4 (offset w < 0 before quat.abs); at frame 16 every bone of
stream 2 keeps rotation and angular velocity (a switch of positions alone), which is what lets the half-life 0 run obey the second
condition below; heads[3, 0, 2, 0] is -0.0.

The run asserts the two conditions that keep the reference single-valued: every offset quaternion has |w| >= 1e-3 before quat.abs, and
every vector-part length (quat.log) and half-angle (quat.exp) is exactly 0 or >= 1e-3."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, os.path.dirname(HERE))
import inertial_ref as R  # noqa: E402  (the input synthesis only; the arithmetic below is the reference's)

REF = os.environ.get("MOCHA_REFERENCE")
if not REF:
    sys.exit("set MOCHA_REFERENCE to the reference checkout")
sys.path.insert(0, os.path.join(REF, "motion"))
import quat  # noqa: E402
import Inertialization as I  # noqa: E402

V, F, DT, MARGIN = 22, 24, 1.0 / 60.0, 1e-3
HL = np.array([0.02, 0.1, 1.0, 0.0])


class Watch:
    """quat.log / quat.exp wrapped to record the lengths they branch on; the wrapped functions are the reference's."""

    def __init__(self):
        self.w, self.len = [], []
        self._log, self._exp = quat.log, quat.exp
        quat.log = lambda x, eps=1e-5: (self.len.append(float(np.sqrt(np.sum(np.square(x[..., 1:]))))), self._log(x, eps))[1]
        quat.exp = lambda x, eps=1e-5: (self.len.append(float(np.sqrt(np.sum(np.square(x))))), self._exp(x, eps))[1]

    def check(self):
        w, ln = np.abs(np.array(self.w)), np.array(self.len)
        assert np.all(w >= MARGIN), ("offset quaternion with |w| below the margin", w.min())
        assert np.all((ln == 0.0) | (ln >= MARGIN)), ("a length between 0 and the margin", ln[(ln > 0) & (ln < MARGIN)])
        return int((np.array(self.w) < 0).sum()), int((ln == 0.0).sum())


def run(heads, transition, valid, halflife, watch):
    """One stream: heads (F,V,13) fp32, transition / valid (F,) -> out (F,V,13) and the offsets after every frame, float64."""
    out = np.full((F, V, 13), np.nan)
    offs = {k: np.full((F, V, n), np.nan) for k, n in (("pos", 3), ("vel", 3), ("ang", 3), ("rot", 4))}
    seen = active = False
    for f in range(F):
        if not valid[f]:
            seen = active = False
            continue
        x = heads[f].astype(np.float64)
        if not seen:
            off_p, off_v, off_a = np.zeros((V, 3)), np.zeros((V, 3)), np.zeros((V, 3))
            off_r = np.tile(np.array([1.0, 0.0, 0.0, 0.0]), (V, 1))
            seen, active = True, False
            out[f] = x
        else:
            if transition[f]:
                for j in range(V):
                    off_p[j], off_v[j] = I.inertialize_transition_pos(off_p[j], off_v[j], prev[j, 0:3], prev[j, 7:10], x[j, 0:3], x[j, 7:10])
                    watch.w.append(float(quat.mul(quat.mul(off_r[j], prev[j, 3:7]), quat.inv(x[j, 3:7]))[0]))
                    off_r[j], off_a[j] = I.inertialize_transition_rot(off_r[j], off_a[j], prev[j, 3:7], prev[j, 10:13], x[j, 3:7], x[j, 10:13])
                active = True
            if not active:
                out[f] = x
            else:
                for j in range(V):
                    out[f, j, 0:3], out[f, j, 7:10], off_p[j], off_v[j] = I.inertialize_update_pos(off_p[j], off_v[j], x[j, 0:3], x[j, 7:10], halflife, DT)
                    out[f, j, 3:7], out[f, j, 10:13], off_r[j], off_a[j] = I.inertialize_update_rot(off_r[j], off_a[j], x[j, 3:7], x[j, 10:13], halflife, DT)
        prev = x
        for k, a in (("pos", off_p), ("vel", off_v), ("ang", off_a), ("rot", off_r)):
            offs[k][f] = a
    return out, offs


def main():
    rng = np.random.Generator(np.random.PCG64(20231213))
    chars = [R.smooth_clip(rng, F, V) for _ in range(5)]
    ids = np.zeros((F, 3), np.int32)
    ids[5:, 1] = 1; ids[6:, 1] = 2; ids[9:, 1] = 0
    ids[4:, 2] = 3; ids[16:, 2] = 4
    heads = np.stack([np.stack([chars[ids[f, s]][f] for s in range(3)]) for f in range(F)])
    # Identical rotations across a transition.  q (x) inv(q) has an exactly zero vector part only when its sums of products are exact,
    # so these quaternions sit on a 2^-12 grid (nothing in the reference needs them to be unit to the last bit).
    grid = lambda q: np.round(q * 4096.0) / 4096.0                              # noqa: E731
    heads[4, 1, 0, 3:7] = grid(heads[4, 1, 0, 3:7])
    heads[5, 1, 0, 3:7] = heads[4, 1, 0, 3:7]
    small = quat.from_scaled_angle_axis(np.array([0.5, -0.7, 0.4]))
    heads[4:16, 2, 1, 3:7] = -quat.mul(small, chars[0][4:16, 1, 3:7])          # near the ANTIPODE of the source: offset w < 0 before abs
    # frame 16 of stream 2 switches positions and velocities alone: from there on its rotations and angular velocities are frozen
    heads[15, 2, :, 3:7] = grid(heads[15, 2, :, 3:7])
    heads[16:, 2, :, 3:7] = heads[15, 2, :, 3:7]
    heads[16:, 2, :, 10:13] = heads[15, 2, :, 10:13]
    heads = heads.astype(np.float32)
    heads[3, 0, 2, 0] = -0.0
    trans = np.zeros((F, 3), bool)
    trans[1:] = ids[1:] != ids[:-1]

    watch = Watch()
    out = np.empty((F, 3, V, 13)); offs = {k: np.empty((F, 3, V, n)) for k, n in (("pos", 3), ("vel", 3), ("ang", 3), ("rot", 4))}
    for s in range(3):
        o, of = run(heads[:, s], trans[:, s], np.ones(F, bool), 0.1, watch)
        out[:, s] = o
        for k in offs:
            offs[k][:, s] = of[k]
    assert np.array_equal(out[:, 0].astype(np.float32).view(np.uint32), heads[:, 0].view(np.uint32))
    # stream 2 alone: half-life 0.02 until its offsets would fall below the margin, half-life 0 on the position-only switch
    hl_trigger = np.zeros((4, F), np.int32); hl_valid = np.ones((4, F), np.int32)
    hl_trigger[:, 4] = 1; hl_trigger[:, 16] = 1
    hl_valid[0, 10:] = 0; hl_trigger[0, 16] = 0
    hl_valid[3, :10] = 0
    hl_out = np.empty((4, F, V, 13))
    for i, h in enumerate(HL):
        hl_out[i], _ = run(heads[:, 2], hl_trigger[i], hl_valid[i], float(h), watch)
    neg, zero = watch.check()
    assert neg >= 1 and zero >= 1, (neg, zero)
    np.savez_compressed(os.path.join(HERE, "inertialize.npz"), heads=heads, ids=ids, out=out, off_pos=offs["pos"], off_vel=offs["vel"],
                        off_ang=offs["ang"], off_rot=offs["rot"], hl=HL, hl_trigger=hl_trigger, hl_valid=hl_valid, hl_out=hl_out)
    print(f"inertialize.npz: {len(watch.w)} transitions ({neg} with w < 0), {len(watch.len)} lengths ({zero} exactly 0), "
          f"min |w| {np.abs(watch.w).min():.3g}, min length > 0 {min(x for x in watch.len if x > 0):.3g}")


if __name__ == "__main__":
    main()
