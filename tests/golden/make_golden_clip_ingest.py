#!/usr/bin/env python3
"""Generate tests/golden/clip_ingest.npz by running THE REFERENCE'S OWN process_data (preprocess/generate_database.py, motion/quat.py;
needs scipy) on whole clips, plain and mirrored, and its divide_clip windows.

    MOCHA_REFERENCE=/path/to/the/reference/checkout python tests/golden/make_golden_clip_ingest.py

The clip is ingest_ref.walk_clip (synthetic.raw_walk_clip) on the 24-joint 'mocha' skeleton, the 100 frames of live_ingest.npz; a case is
its prefix of n frames.  No reference source or bytecode is written anywhere; the fixture is data only.

Contents:
  rot (100,24,3) fp32 degrees, pos (100,24,3) fp32 centimetres, order 'zyx', parents (24,), names, mirror_map (24,), lengths = 31, 32, 45,
  62, 100
  plain_<n>_pos / _vel / _ang (n,25,3), _rot (n,25,4) float64, _contact (n,2) bool: process_data(prefix, window=n, window_step=n), which
      returns the processed prefix as one window without padding; mirror_<n>_*: the same with mirror=True
  w30_pos / _vel / _rot / _ang / _contact: the 3 windows of process_data(clip, 60, 30) (the last one padded 10 / 10)
  w1_index = 0, 40, 41, 84 and w1_*: those windows of the 85 of process_data(clip, 60, 1)

The run asserts the conditions that keep the reference single-valued on every case: every toe speed at least 1e-3 away from the threshold,
|w| >= 1e-3 wherever quat.abs branches, no length that quat.log branches on in [1e-7, 1e-3) (mirrored identity rotations give lengths
near 1e-29, far on the `< eps` side), and every quantity from_xform branches on (m22, m00 - m11, m00 + m11) at least 1e-6 from 0.  Should
one fail, change SEED."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, HERE)
import make_golden_ingest as M  # noqa: E402  (the names, parents, toes and the branch watcher; imports the reference's modules)

R, G, quat = M.R, M.G, M.quat
LENGTHS = [31, 32, 45, 62, 100]
W1 = [0, 40, 41, 84]
SEED = 20231213                     # raw_walk_clip's default: the clip of live_ingest.npz
F, THRESHOLD, MARGIN, XFORM_MARGIN = 100, 0.5, 1e-3, 1e-6
KEYS = ("pos", "vel", "rot", "ang", "contact")


def data(rot, pos):
    # process_data scales the positions it is given in place, hence the copies
    return {"rotations": rot.astype(np.float64), "positions": pos.astype(np.float64), "order": "zyx", "names": M.NAMES, "parents": M.PARENTS}


def main():
    rot, pos = R.walk_clip(M.PARENTS, F, seed=SEED)
    watch = M.Watch()
    xform = []
    from_xform = quat.from_xform

    def w_from_xform(ts):
        xform.append(np.stack([ts[..., 2, 2], ts[..., 0, 0] - ts[..., 1, 1], ts[..., 0, 0] + ts[..., 1, 1]]).ravel())
        return from_xform(ts)
    quat.from_xform = w_from_xform

    out, near = {}, {False: [], True: []}
    for mirror in (False, True):
        for n in LENGTHS:
            w, parents, names = G.process_data(data(rot[:n], pos[:n]), window=n, window_step=n, mirror=mirror)
            assert all(len(x) == 1 and len(x[0]) == n for x in w), "process_data padded or split the clip"
            assert list(parents) == [-1] + list(M.PARENTS + 1) and names[0] == "Root"
            p, v, r, a, c = (np.array(x[0]) for x in w)
            for k, x in zip(KEYS, (p, v, r, a, c)):
                out[f"{'mirror' if mirror else 'plain'}_{n}_{k}"] = x
            speed = np.sqrt(np.sum(watch.gvel[:, M.TOES] ** 2, axis=-1))
            near[mirror].append(np.abs(speed - THRESHOLD).min())
    for tag, step, pick in (("w30", 30, None), ("w1", 1, W1)):
        w, _, _ = G.process_data(data(rot, pos), window=60, window_step=step)
        assert len(w[0]) == (3 if step == 30 else 85), len(w[0])
        for k, x in zip(("pos", "vel", "rot", "ang", "contact"), w):
            x = np.stack([np.asarray(y) for y in x])
            out[f"{tag}_{k}"] = x if pick is None else x[pick]
    assert np.array_equal(out["w30_pos"][2, :10], np.repeat(out["w30_pos"][2, 10:11], 10, 0)) and not out["w30_vel"][2, :10].any()
    assert np.array_equal(out["w30_pos"][2, 50:], np.repeat(out["w30_pos"][2, 49:50], 10, 0)) and not out["w30_ang"][2, 50:].any()

    ln, w = np.concatenate(watch.len), np.concatenate(watch.w)
    xf = np.abs(np.concatenate(xform))
    assert not np.any((ln >= 1e-7) & (ln < MARGIN)), ("a log length inside [1e-7, 1e-3)", ln[(ln >= 1e-7) & (ln < MARGIN)])
    assert w.min() >= MARGIN, ("quat.abs with |w| below the margin", w.min())
    assert xf.min() >= XFORM_MARGIN, ("a from_xform branch quantity within the margin of 0", xf.min())
    assert min(near[False]) >= MARGIN and min(near[True]) >= MARGIN, ("a toe speed within the margin of the threshold", near)
    names = M.NAMES
    mirror_map = np.array([names.index("Left" + x[5:]) if x.startswith("Right") else names.index("Right" + x[4:]) if x.startswith("Left")
                           else i for i, x in enumerate(names)], np.int32)
    path = os.path.join(HERE, "clip_ingest.npz")
    np.savez_compressed(path, rot=rot, pos=pos, order="zyx", parents=M.PARENTS.astype(np.int32), names=np.array(names), mirror_map=mirror_map,
                        lengths=np.array(LENGTHS, np.int32), w1_index=np.array(W1, np.int32), **out)
    print(f"clip_ingest.npz: {os.path.getsize(path)} bytes; lengths {LENGTHS} plain and mirrored; min |toe speed - {THRESHOLD}| plain "
          f"{min(near[False]):.3g} mirrored {min(near[True]):.3g}; min from_xform margin {xf.min():.3g}; min |w| {w.min():.3g}; "
          f"log lengths below 1e-7: {int((ln < 1e-7).sum())}, smallest above {ln[ln >= 1e-7].min():.3g}")


if __name__ == "__main__":
    main()
