"""The motion-side kernels against a wider-precision restatement at the kernel boundary (GPU cases: -m gpu; the CPU pins run everywhere).

mocha_featurize (csrc/featurize.hip, featurize_body.h) and mocha_pose_heads, mocha_post_clip, mocha_post_bvh (csrc/postprocess.hip) are
launched directly through tests/gemm_probe/pose_probe.cpp at the smallest shapes that reach each edge - the Python API only ever runs them at
25 bones, 60 frames, 24 joints and two contacts - and held to tests/pose_ref.py, a restatement generic over the NumPy dtype that the
test_reference_* functions pin without a GPU: at fp32 to the bits of oracle.featurize_oracle, at float64 to 1e-13 of
oracle.postprocess_oracle on the golden clip, and numpy.longdouble is checked to be wider than float64.

  F  mocha_featurize (fp32): per channel group (pos, rot-xy, vel, ang) the error against the float64 restatement is bounded by the error of
     the fp32 restatement against float64 times MARGIN32 = (on the largest, on the rms error), plus one fp32 ulp of the group's largest
     output on the largest error.  To the bit: bone 0's position columns are 0, all-zero velocities give zero vel / ang columns, and a
     window's block is the same alone and at any position of any batch.
  H  mocha_pose_heads (fp32): the same yardstick on the quaternion (with its sign where the restatement's branch margin is >= 1e-3, as a
     rotation otherwise) and on the speed; positions, velocities, angular velocities are bit copies.
  C  mocha_post_clip (float64): the error against the longdouble restatement is bounded by the error of the float64 restatement against
     longdouble times MARGIN64, with a floor of 4 float64 ulps of the output's largest magnitude on the largest error.  Every case first
     asserts on the CPU that each discrete decision of the restatement (speed ratio against 3 and 0.33, h against 1e-5, unlock radius, reach
     against max_ext, foot height) has a margin >= 1e-6 - except the decisions a case authors exactly, with values exact in fp32 - so
     kernel and restatement cannot legitimately branch differently.  Bit identities: IK off -> ik_rot = rot, blend off -> pos[1:] = the
     heads' positions, a clip in a batch = the clip alone, the resumable form frame by frame = the clip launch, a masked clip keeps its
     rows and state.
  B  mocha_post_bvh (float64): on the kernel's own pos / rot / ik_rot, positions to the same yardstick, Euler channels as rotations
     (quaternions rebuilt from both triples, up to sign) and directly wherever |asin argument| < 1 - 1e-6; authored gimbal cases to 1e-9 deg.
  Every output sits between 0x7FC0DEAD guard words, every element asked for is written, every refusal leaves all buffers intact.

RESULTS, measured on an MI355X (139 GPU cases; ratio = kernel error / yardstick error, largest / rms; every case prints its own with -s).
Worst per kernel and output, with the case:
  featurize pos 2.92 / 1.51 (chain2-T2-B32-nonunit)   rot 1.53 (chain8-T1-B60-nonunit) / 1.46 (one-T2-B32-still)
  featurize vel 3.22 (chain2-T2-B32-nonunit) / 1.87 (chain2-T1-B1-far)   ang 1.72 (chain40-T1-B1-unit) / 2.81 (one-T1-B1-unit: 3 numbers)
  pose_heads quat 1.48 (T130-V1-B3) / 1.53 (T65-V1-B3)   speed over all shapes 0.94 / 0.84
  post_clip pos 2.49 / 2.47 (flags-ik1-blend0: 1.3e-16 against 5.1e-17, under the floor)   rot 1.97 (locks) / 1.65 (small-rang)
  post_clip ik_rot 2.56 (skeleton-tree31) / 1.80 (constants); straight-leg 1.00 / 1.32 at a reference sensitivity of 5.2e-13: no margin of its own needed
  post_bvh pos 1.00 / 1.09   euler 1.48 (many-5[3]) / 1.23; as rotations at most 6.1e-16 (restatement 4.4e-16 - 7.8e-16)
Margins: (4, 2) for both precisions, as started.  The rms ratios reach 1.5 - 1.9 in featurize and in ik_rot, so the rms margin is not tightened
to 1.5.  Four things differ from the plain scheme, each for a reason the figures give (hold() and run_case() say the same in place):
  - the speed is ONE number per window: per case only its largest error is held, and the rms on the 108 windows of all shapes together
    (a single window measured 65 x the fp32 restatement's lucky 1.8e-9, at 0.98 ulp of its own value);
  - groups of fewer than 64 numbers, and groups whose yardstick is exactly 0 (the rot columns of a lone root bone are exactly 1 and 0 in
    the restatement at both precisions; the kernel's fused w x - x w leaves 1.1e-8 = 0.09 ulp), are held on the largest error alone;
  - ONE float64 output has its rms held by the 4-ulp floor instead of 2 x the yardstick: pos with blending off, a copy of the heads except
    the root's 24 rows, each within one ulp (kernel 5.8e-18 rms against 2.4e-18: 2.47 x).  Every other float64 rms is at most 1.80 x.
  - hips whose IK target sits on the heel to rounding (a contact that has not locked: target = toe + (heel - toe)) hang on whether that
    sum rounds to the heel, in the kernel as in the restatement: acos(1 - 2e-8 / |c - a|) is 2e-4 / sqrt(|c - a|), not 0, and the axis is
    cross / (|cross| + 1e-8).  Those entries (|cross(c_a, t_a)| < 1e-6 in the restatement; 14 cases have some) get the bound pose_ref derives
    for 4 ulps of noise in the target, 1.5e-11 to 1e-10; measured 2.5e-12 in small-rang (frame 1, bone 21: 0.044 of it; every other entry of
    that clip is within 2.2e-15) and at most 2.1e-15 elsewhere.  exact-geometry and exact-geometry-mixamo, where every position is exact in any
    arithmetic, take no such allowance and hold the same hips to the plain yardstick (measured 1.00 / 1.00 and 1.00 / 0.97).
Defect found and fixed: cross() compiles to fused multiply-adds, which leave the rounding error of one product where the cross product of
two identical vectors is exactly 0; in the two-bone IK's r2 = from_angle_axis(acos(dot(c_a, t_a)), normalize(cross(c_a, t_a))) normalize()
divides that 1e-17 by its eps of 1e-8, and every hip of a contact that has not locked yet was turned by a spurious 1e-13 to 3e-12 (13 of the
then 137 cases failed ik_rot: ratio 9.4e-14 against a yardstick of 7.2e-15, reach 3.1e-13 against 2.4e-15, tree31 2.6e-13 against 2.6e-15,
exact-geometry 3.6e-13 against 6.9e-17).  postprocess.hip's cross_unfused() computes that one product without contraction; after it those cases
are at 1.0 - 2.6 x the yardstick, and the library built without it fails exact-geometry alone (3.6e-13 / 4.6e-14 against 6.9e-17 / 8.4e-18).
The two candidates of the issue are not defects: the contact reset reads the clip's own frame 0 (test_clip_counts_and_clips_alone, contacts
held from frame 1), and a masked clip's parked root and BVH rows stay untouched (test_step_valid_mask).
Mutations, each on a scratch copy (never committed), measured before exact-geometry was added (137 cases); new file / the old GPU tests
that run the mutated kernel (test_featurize.py: 2 tests; test_postprocess.py + test_post_step.py: 10 tests):
  1. featurize_body.h o[7] = xz + wy: 29 fail (every test_featurize case with more than one bone) / 2 of 2
  2. featurize_body.h crossv(pa, lp): 26 fail (test_featurize) / 2 of 2
  3. pose heads, the t00 < -t11 branch's q[0] negated: 66 fail (63 shapes, both branch tests, the pooled speed test's quat) / 4 of 10
  4. ratio < 0.033f: 1 fails (test_clip_authored[ratio]) / 2 of 10 (the two retarget_clip end-to-end tests)
  5. the IK merge in descending contact order: 4 fail (contacts-3, contacts-4, contacts-4-rev, test_clip_later_contacts_win) / 0 of 10
  6. (dt + 1e-8) -> dt: 16 fail (every case with a lock) / 3 of 10
  7. clamp1 removed from the asin: 1 fails (test_bvh_gimbal_and_root_merge: NaN) / 0 of 10
  The old files were not run against the kernels a mutation does not touch (1 - 2 against the postprocess files, 3 - 7 against test_featurize.py).
Run time on the MI355X: 4.4 s for the file's 139 GPU cases, CPU restatements included (siblings: 14 - 21 s); slowest case 0.24 s
(test_featurize[mocha-T60-B3-unit], which carries the first launch's set-up); no case needs longer.  The 25 CPU cases take 6 s.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pose_ref as pr  # noqa: E402
from test_pointwise_kernels import GUARD, SENTINEL, D, Out, dev, rng  # noqa: E402  (the guard pattern and the named generators)

from mocha_sigasia2023_amd.skeleton import LAYOUTS  # noqa: E402

gpu = pytest.mark.gpu
MARGIN32 = (4.0, 2.0)                       # fp32 kernels: on the largest / rms error of the fp32 restatement against float64
MARGIN64 = (4.0, 2.0)                       # float64 kernels: on the largest / rms error of the float64 restatement against longdouble
DECISION_MARGIN = 1e-6
R2_ON_HEEL = 1e-6                           # |cross(c_a, t_a)| below which the IK target counts as sitting on the heel
MOCHA = pr.full_parents(LAYOUTS["mocha"]["parents"])        # 25 bones
MIXAMO = pr.full_parents(LAYOUTS["mixamo"]["parents"])      # 23 bones
LD = np.longdouble


def stream():
    return torch.cuda.current_stream().cuda_stream


def guards_intact(out):
    host = out.buf.cpu()
    return bool((host[:GUARD] == SENTINEL).all()) and bool((host[GUARD + out.words:] == SENTINEL).all())


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


RATIOS = {}


def hold(kernel, case, y, wide, narrow, margins, floor_ulps=0.0, extra_ulp=False, rms_floor=False):
    """y (the kernel's output) against `wide` (the restatement one precision up), bounded by `narrow` (the restatement in the kernel's own
    precision) against `wide`.  extra_ulp: one ulp (of y's dtype) of the largest output is added to the bound on the largest error (the
    fp32 scheme); floor_ulps: the bound on the largest error is at least that many ulps of the largest output (the float64 scheme);
    rms_floor: that floor bounds the rms too - for an output that is a copy but for a few rows (run_case says which and why)."""
    y = np.asarray(y)
    emax, erms = pr.errors(y, wide)
    bmax, brms = pr.errors(narrow, wide)
    big = float(np.abs(wide).max()) if wide.size else 0.0
    ulp = float(np.spacing(y.dtype.type(big)))
    mmax, mrms = margins
    bound = max(mmax * bmax + (ulp if extra_ulp else 0.0), floor_ulps * ulp)
    rmax, rrms = emax / max(bmax, 1e-300), erms / max(brms, 1e-300)
    w = RATIOS.setdefault(kernel, [0.0, 0.0])
    w[0], w[1] = max(w[0], rmax if emax > max(ulp, floor_ulps * ulp) else 0.0), max(w[1], rrms if erms > 0 else 0.0)
    print(f"[pose] {kernel:18s} {case:40s} max {emax:.3e} ({rmax:8.2f} x) rms {erms:.3e} ({rrms:6.2f} x) ulp {ulp:.2e}   worst so far {w[0]:.2f} / {w[1]:.2f}")
    assert np.isfinite(y).all(), (kernel, case, "not finite")
    # Two places where the rms yardstick has nothing to say and the output is held on its largest error alone: fewer than 64 numbers (a workgroup's worth, chosen, not measured; no statistic: J = 1 with B T = 1 is 3 to 6 numbers per group), and
    # a yardstick of exactly 0 - the restatement gives the same exactly representable values in both precisions (the rot columns of a
    # lone root bone: 1 and 0), where the output must stay within the one ulp
    rms_bound = max(mrms * brms, floor_ulps * ulp if rms_floor else 0.0)
    rms_ok = erms <= rms_bound or y.size < 64 or (extra_ulp and brms == 0.0 and emax <= ulp)
    assert emax <= bound and rms_ok, (kernel, case, (emax, erms), (bmax, brms), ulp)


# =================================================================================================== no GPU: the restatement is what it claims
def test_reference_longdouble_is_wider_than_float64():
    """The float64 kernels' yardstick is float64 against numpy.longdouble; where longdouble is float64 it would be 0 = 0."""
    assert pr.longdouble_is_wider(), f"numpy.longdouble has eps {np.finfo(np.longdouble).eps}: no wider than float64 on this machine"
    a = LD(1.0) + LD(2.0) ** -60
    assert a != LD(1.0) and float(np.sqrt(LD(2.0)) ** 2 - LD(2.0)) != float(np.sqrt(2.0) ** 2 - 2.0)


def test_reference_featurize_is_the_oracle_to_the_bit(golden_dir):
    """pose_ref.featurize at fp32 against oracle.featurize_oracle.featurize on the fixture's inputs and on a mixamo tree: the same bits."""
    from mocha_sigasia2023_amd import synthetic
    from oracle import featurize_oracle as FO
    z = np.load(os.path.join(golden_dir, "featurize.npz"))
    seed, B = (int(v) for v in z["seed"])
    got = pr.featurize(*synthetic.bone_windows(seed, B), MOCHA, np.float32)
    assert got.dtype == np.float32 and same_bits(got, z["X"]) and same_bits(got, FO.featurize(*synthetic.bone_windows(seed, B), MOCHA))
    inp = synthetic.bone_windows(seed + 1, 2, J=23)
    assert same_bits(pr.featurize(*inp, MIXAMO, np.float32), FO.featurize(*inp, MIXAMO))
    assert pr.featurize(*inp, MIXAMO, np.float64).dtype == np.float64 and pr.featurize(*inp, MIXAMO, LD).dtype == LD


def _golden_clip(golden_dir):
    from mocha_sigasia2023_amd import synthetic
    z = np.load(os.path.join(golden_dir, "postprocess.npz"))
    N = int(z["seed"][1])
    Y, rvel, rang, hipvel, contact = synthetic.postprocess_inputs(int(z["seed"][0]), N)
    Ycm = synthetic.postprocess_inputs(int(z["cm_seed"][0]), int(z["cm_seed"][1]))[0]
    return Y, Ycm, rvel, rang, np.linalg.norm(hipvel, axis=-1).mean(-1).astype(np.float32), contact


def test_reference_postprocess_is_the_oracle(golden_dir):
    """pose_ref.pose_heads / run_clip / bvh_channels at float64 against oracle.postprocess_oracle to 1e-13 on the golden clip's inputs,
    both streams; the decision margins it reports on that clip; the Euler inverse used by family B."""
    from oracle import postprocess_oracle as P
    Y, Ycm, rvel, rang, sspeed, contact = _golden_clip(golden_dir)
    for Yc, kw, okw in ((Y, {}, {}), (Ycm, dict(ik_enabled=False, blend=False), dict(ik_enabled=False, blend=False))):
        N, V = Yc.shape[0], Yc.shape[2]
        h64, s64, branch, margin = pr.pose_heads(Yc, np.float64)
        last = Yc[:, -1].astype(np.float64)
        assert np.abs(h64[..., 3:7] - P.from_xform_xy(last[..., 3:9].reshape(N, V, 3, 2))).max() < 1e-13
        assert np.abs(s64 - np.linalg.norm(Yc.astype(np.float64)[:, :, 0, 9:12], axis=-1).mean(-1)).max() < 1e-13
        h32, s32, _, _ = pr.pose_heads(Yc, np.float32)
        oh, osp = P.pose_heads(Yc)
        assert same_bits(h32, oh) and same_bits(s32, osp)
        pos, rot, ik, dec = pr.run_clip(oh, osp, rvel, rang, sspeed, contact, MOCHA, (5, 24), np.float64, **kw)
        op, orot, oik = P.run_clip(oh, osp, rvel, rang, sspeed, contact, MOCHA, **okw)
        assert max(np.abs(pos - op).max(), np.abs(rot - orot).max(), np.abs(ik - oik).max()) < 1e-13
        bp, be, s = pr.bvh_channels(op, orot, oik, np.float64)
        obp, obe = P.bvh_channels(op, oik)
        assert np.abs(bp - obp).max() < 1e-13 and np.abs(be - obe).max() < 1e-13 and 0.999 < np.abs(s).max() < 1.0
        if not kw:      # what the clip decides and how closely: the figures the margins of family C were sized with
            assert 2.0e-4 < dec.smallest("reach") < 3.0e-4 and 2.0e-2 < dec.smallest("radius") < 2.5e-2
            assert dec.count["reach_clamp"] == 7 and dec.count["reach_clamp"] + dec.count["reach_free"] == 238 and dec.count["h_small"] == 0
            assert dec.count["ratio_reset"] == 1 and dec.count["radius_unlock"] > 0 and dec.count["label_unlock"] == 0
    q = rng("euler").standard_normal((500, 4))
    q /= np.linalg.norm(q, axis=-1, keepdims=True)
    w, x, y, z = (q[..., i] for i in range(4))
    eu = np.degrees(np.stack([np.arctan2(2 * (w * x + y * z), 1 - 2 * (x * x + y * y)), np.arcsin(np.clip(2 * (w * y - z * x), -1, 1)),
                              np.arctan2(2 * (w * z + x * y), 1 - 2 * (y * y + z * z))], -1))
    back = pr.euler_to_quat(eu)
    assert np.minimum(np.abs(back - q).max(-1), np.abs(back + q).max(-1)).max() < 1e-12


# =================================================================================================== F: mocha_featurize
def chain(J):
    return np.arange(-1, J - 1, dtype=np.int32)


def star(J):
    return np.concatenate([[-1], np.zeros(J - 1, dtype=np.int32)]).astype(np.int32)


TREES = {"mocha": MOCHA, "mixamo": MIXAMO, "chain2": chain(2), "chain8": chain(8), "chain40": chain(40), "star40": star(40), "one": chain(1)}
FEAT_GROUPS = (("pos", slice(0, 3)), ("rot", slice(3, 9)), ("vel", slice(9, 12)), ("ang", slice(12, 15)))
# (tree, T, B, inputs): B * T = 1, 60, 64, 65, 180 and about 200 - a partial last workgroup of 64 frames, windows that straddle one
FEAT_CASES = [
    ("mocha", 60, 3, "unit"), ("mocha", 60, 1, "unit"), ("mocha", 64, 1, "unit"), ("mocha", 65, 1, "unit"), ("mocha", 1, 1, "unit"),
    ("mocha", 2, 100, "unit"), ("mocha", 65, 3, "unit"), ("mocha", 1, 65, "unit"), ("mocha", 60, 3, "nonunit"), ("mocha", 60, 3, "far"),
    ("mocha", 65, 3, "still"),
    ("mixamo", 60, 3, "unit"), ("mixamo", 64, 1, "nonunit"), ("mixamo", 2, 32, "far"), ("mixamo", 65, 1, "still"),
    ("chain2", 65, 1, "unit"), ("chain2", 2, 32, "nonunit"), ("chain2", 1, 1, "far"),
    ("chain8", 60, 3, "unit"), ("chain8", 1, 60, "nonunit"), ("chain8", 64, 3, "far"),
    ("chain40", 60, 3, "unit"), ("chain40", 65, 1, "unit"), ("chain40", 1, 1, "unit"), ("chain40", 2, 100, "still"), ("chain40", 60, 1, "far"),
    ("star40", 64, 1, "unit"), ("star40", 2, 90, "nonunit"), ("star40", 65, 3, "far"),
    ("one", 60, 1, "unit"), ("one", 1, 1, "unit"), ("one", 65, 3, "nonunit"), ("one", 2, 32, "still"),
]


def bone_inputs(name, B, T_, J, kind):
    """Local bone features (B, T, J, 4|3|3|3) fp32.  unit: unit quaternions of both signs of w; nonunit: norms 0.5 .. 2 (nobody
    normalises); far: the root 1e3 away from the origin, bones 0.3 long (gp - Rp cancels); still: all-zero velocities."""
    r = rng(name)
    q = r.standard_normal((B, T_, J, 4))
    q /= np.sqrt((q * q).sum(-1, keepdims=True))
    if kind == "nonunit":
        q *= np.exp(r.uniform(np.log(0.5), np.log(2.0), (B, T_, J, 1)))
    pos = 0.3 * r.standard_normal((B, T_, J, 3))
    if kind == "far":
        pos[:, :, 0] = np.array([1e3, -1e3, 1e3]) + 0.5 * r.standard_normal((B, T_, 3))
    vel, ang = r.standard_normal((B, T_, J, 3)), r.standard_normal((B, T_, J, 3))
    if kind == "still":
        vel[:], ang[:] = 0.0, 0.0
    return tuple(a.astype(np.float32) for a in (q, pos, vel, ang))


_feat_ready = False


def launch_featurize(inp, parents, B, T_, J):
    global _feat_ready
    lib = pr.load()
    if not _feat_ready:
        assert lib.pp_featurize_init() == 0
        _feat_ready = True
    d = [D(a) for a in inp]
    par = D(np.asarray(parents, dtype=np.int32))
    X = Out((B, T_, max(J, 1), 15))
    rc = lib.pp_featurize(*[pr.ptr(a) for a in d], pr.ptr(par), X.ptr, B, T_, J, stream())
    return rc, X, d + [par]


@gpu
@pytest.mark.parametrize("tree,T_,B,kind", FEAT_CASES, ids=[f"{c[0]}-T{c[1]}-B{c[2]}-{c[3]}" for c in FEAT_CASES])
def test_featurize(tree, T_, B, kind):
    parents = TREES[tree]
    J = len(parents)
    case = f"{tree}-T{T_}-B{B}-{kind}"
    inp = bone_inputs("feat-" + case, B, T_, J, kind)
    rc, X, _ = launch_featurize(inp, parents, B, T_, J)
    assert rc == 0
    y = X.check(case)
    ref64, ref32 = pr.featurize(*inp, parents, np.float64), pr.featurize(*inp, parents, np.float32)
    for g, s in FEAT_GROUPS:
        hold("featurize " + g, case, y[..., s], ref64[..., s], ref32[..., s], MARGIN32, extra_ulp=True)
    assert not y[:, :, 0, 0:3].any(), "bone 0 sits at the origin of its own frame, exactly"
    if kind == "still":
        assert not y[..., 9:15].any(), "zero velocities in, zero velocities out"
    q = inp[0]
    assert kind == "nonunit" or ((q[..., 0] > 0).any() and (q[..., 0] < 0).any()) or q[..., 0].size < 4


@gpu
@pytest.mark.parametrize("tree,T_,B", [("mocha", 60, 5), ("mocha", 65, 3), ("chain40", 60, 4), ("mixamo", 2, 70)],
                         ids=["mocha-T60-B5", "mocha-T65-B3", "chain40-T60-B4", "mixamo-T2-B70"])
def test_featurize_window_alone_is_the_window_in_a_batch(tree, T_, B):
    """A window's T x J x 15 block has the same bits alone (B = 1) and as any member of a larger batch, in any position: an LDS column or a
    window index taken from the wrong frame shows here whatever the tolerance."""
    parents = TREES[tree]
    J = len(parents)
    inp = bone_inputs(f"feat-batch-{tree}-{T_}-{B}", B, T_, J, "unit")
    rc, X, _ = launch_featurize(inp, parents, B, T_, J)
    assert rc == 0
    whole = X.check("batch")
    order = rng("perm").permutation(B)
    rc, Xp, _ = launch_featurize(tuple(a[order] for a in inp), parents, B, T_, J)
    assert rc == 0
    moved = Xp.check("permuted batch")
    for k, b in enumerate(order if B <= 8 else order[:8]):
        rc, X1, _ = launch_featurize(tuple(a[b:b + 1] for a in inp), parents, 1, T_, J)
        assert rc == 0
        alone = X1.check("alone")[0]
        assert same_bits(alone, whole[b]) and same_bits(alone, moved[k]), (tree, int(b))
    assert same_bits(moved, whole[order])


@gpu
def test_featurize_refusals():
    """J = 0 and J = 41 are the launcher's to refuse: hipErrorInvalidValue, every buffer intact."""
    for J in (0, 41):
        Ja = max(J, 1)
        inp = bone_inputs(f"feat-refuse-{J}", 2, 60, Ja, "unit")
        rc, X, held = launch_featurize(inp, chain(Ja), 2, 60, J)
        assert rc == pr.INVALID_VALUE and X.intact()
        for a, h in zip(inp, held):
            assert same_bits(h.cpu().numpy(), a)


# =================================================================================================== H: mocha_pose_heads
def rot_columns(q):
    """Unit quaternions (..., 4) float64 -> the first two columns of the rotation matrix, (..., 3) each."""
    m = pr.to_xform_xy(q)
    return m[..., [0, 2, 4]], m[..., [1, 3, 5]]


def dominant(r, n, k):
    """n unit quaternions whose component k is the largest by a clear margin: k = 1, 2, 3, 0 lands in from_xform's branch 0, 1, 2, 3."""
    q = 0.45 * r.uniform(-1, 1, (n, 4))
    q[:, k] = r.choice([-1.0, 1.0], n) * r.uniform(0.8, 1.0, n)
    return q / np.linalg.norm(q, axis=-1, keepdims=True)


def heads_windows(name, B, T_, V, rows=None):
    """Y (B, T, V, 15) fp32, normal everywhere; the 6-D rotation of the last frame is a noisy rotation matrix (or `rows`, (B * V, 2, 3))."""
    r = rng(name)
    Y = r.standard_normal((B, T_, V, 15))
    if rows is None:
        q = r.standard_normal((B * V, 4))
        q /= np.linalg.norm(q, axis=-1, keepdims=True)
        c0, c1 = rot_columns(q)
        rows = np.stack([c0, c1], 1) + 0.05 * r.standard_normal((B * V, 2, 3))
    rows = np.asarray(rows).reshape(B, V, 2, 3)
    Y[:, -1, :, 3:9] = np.stack([rows[:, :, 0], rows[:, :, 1]], -1).reshape(B, V, 6)     # (3, 2) row-major: column 0 = 3, 5, 7
    return Y.astype(np.float32)


def run_heads(case, Y, sign_margin=1e-3, pool=None):
    B, T_, V = Y.shape[:3]
    lib = pr.load()
    dY = D(Y)
    heads, speed = Out((B, V, 13)), Out((B,))
    assert lib.pp_pose_heads(pr.ptr(dY), heads.ptr, speed.ptr, B, T_, V, stream()) == 0
    h, s = heads.check(case), speed.check(case)
    assert same_bits(dY.cpu().numpy(), Y)
    h64, s64, branch, margin = pr.pose_heads(Y, np.float64)
    h32, s32, _, _ = pr.pose_heads(Y, np.float32)
    assert np.isfinite(h64).all()
    last = Y[:, -1]
    assert same_bits(h[..., 0:3], last[..., 0:3]) and same_bits(h[..., 7:13], last[..., 9:15]), "positions and velocities are copies"
    q, q64, q32 = h[..., 3:7].copy(), h64[..., 3:7], h32[..., 3:7].copy()
    loose = margin < sign_margin                                          # next to a branch condition either branch is right: compare as rotations
    for a in (q, q32):
        flip = loose & (np.abs(a + q64).max(-1) < np.abs(a - q64).max(-1))
        a[flip] = -a[flip]
    hold("pose_heads quat", case, q, q64, q32, MARGIN32, extra_ulp=True)
    assert float(np.abs(s - s64).max()) <= MARGIN32[0] * float(np.abs(s32 - s64).max()) + float(np.spacing(np.float32(np.abs(s64).max()))), (case, "speed")
    if pool is not None:
        pool.append((s, s64, s32))
    return branch, margin


HEAD_SHAPES = [(T_, V, B) for T_ in (1, 59, 60, 64, 65, 130) for V in (1, 22, 24, 31, 64, 70) for B in (1, 3)]


@gpu
@pytest.mark.parametrize("T_,V,B", HEAD_SHAPES, ids=[f"T{t}-V{v}-B{b}" for t, v, b in HEAD_SHAPES])
def test_pose_heads_shapes(T_, V, B):
    run_heads(f"T{T_}-V{V}-B{B}", heads_windows(f"heads-{T_}-{V}-{B}", B, T_, V))


@gpu
def test_pose_heads_speed_over_all_shapes():
    """The speed is one number per window: per case only its largest error is held (in run_heads); the rms error is a statistic and is
    held here on the 108 windows of all shapes together, against the same yardstick."""
    pool = []
    for T_, V, B in HEAD_SHAPES:
        run_heads(f"T{T_}-V{V}-B{B}", heads_windows(f"heads-{T_}-{V}-{B}", B, T_, V), pool=pool)
    s, s64, s32 = (np.concatenate([p[k] for p in pool]) for k in range(3))
    hold("pose_heads speed", "all shapes", s, s64, s32, MARGIN32, extra_ulp=True)


@gpu
def test_pose_heads_every_branch_with_its_sign():
    """Fifty and more rotations in each of the four quaternion branches, each at a branch margin >= 1e-3: compared with their sign."""
    r = rng("heads-branches")
    B, V = 3, 70
    q = np.concatenate([dominant(r, 53, k) for k in (1, 2, 3, 0)])[r.permutation(212)][:B * V]
    c0, c1 = rot_columns(q)
    rows = np.stack([c0, c1], 1) + 0.01 * r.standard_normal((B * V, 2, 3))
    branch, margin = run_heads("branches", heads_windows("heads-branches-Y", B, 65, V, rows))
    for k in range(4):
        assert ((branch == k) & (margin >= 1e-3)).sum() >= 50, (k, int(((branch == k) & (margin >= 1e-3)).sum()))


@gpu
def test_pose_heads_branch_boundaries_and_hard_columns():
    """Pairs 1e-6 either side of each of the three branch conditions (t22 against 0, t00 against t11, t00 against -t11; compared as
    rotations: either branch is right there), columns 1e-2 rad from parallel (the two cross products cancel), columns of length 1e-3 and 1e3."""
    r = rng("heads-edges")
    rows = []
    for side in (-1.0, 1.0):
        for _ in range(6):
            # unit quaternions: t22 = 1 - 2 (x^2 + y^2), t00 - t11 = 2 (y^2 - x^2) ... in terms of (w, x, y, z): see the three solves below
            d = side * 0.5e-6
            a, b = r.uniform(0, 2 * np.pi, 2)
            s2 = 0.5 - d                                                  # x^2 + y^2 = 1/2 - d: t22 = 2 d
            rows.append([np.sqrt(1 - s2) * np.cos(b), np.sqrt(s2) * np.cos(a), np.sqrt(s2) * np.sin(a), np.sqrt(1 - s2) * np.sin(b)])
            x2 = 0.35 + d / 2                                             # x^2 - y^2 = d with x^2 + y^2 = 0.7 (t22 < 0): t00 - t11 = 2 d
            rows.append([np.sqrt(0.3) * np.cos(b), np.sqrt(x2), np.sqrt(0.7 - x2) * np.sign(np.cos(a)), np.sqrt(0.3) * np.sin(b)])
            w2 = 0.35 + d / 2                                             # w^2 - z^2 = d with w^2 + z^2 = 0.7 (t22 > 0): t00 + t11 = 2 d
            rows.append([np.sqrt(w2), np.sqrt(0.3) * np.cos(a), np.sqrt(0.3) * np.sin(a), np.sqrt(0.7 - w2) * np.sign(np.cos(b))])
    q = np.asarray(rows)
    assert np.abs(np.linalg.norm(q, axis=-1) - 1).max() < 1e-12
    c0, c1 = rot_columns(q)
    near = np.stack([c0, c1], 1)                                          # 36 rows at the boundaries
    qr = r.standard_normal((60, 4))
    qr /= np.linalg.norm(qr, axis=-1, keepdims=True)
    d0, d1 = rot_columns(qr)
    par = np.stack([d0[:20], (np.cos(1e-2) * d0[:20] + np.sin(1e-2) * d1[:20]) * r.uniform(0.5, 2.0, (20, 1))], 1)
    short, long_ = np.stack([d0[20:40], d1[20:40]], 1) * 1e-3, np.stack([d0[40:], d1[40:]], 1) * 1e3
    rows = np.concatenate([near, par, short, long_])                      # 96 rows
    Y = heads_windows("heads-edges-Y", 1, 64, 96, rows)
    branch, margin = run_heads("edges", Y)
    assert (margin[0, :36] < 1e-5).all() and (margin[0, :36] > 1e-8).all(), "the authored pairs sit 1e-6 either side of a condition"
    t = branch[0, :36].reshape(2, 6, 3)
    assert (t[0] != t[1]).all(), "the two sides of every authored pair take different branches in the restatement"


# =================================================================================================== C, B: mocha_post_clip, mocha_post_bvh
def tree31():
    """32 bones (V + 1 = MOCHA_MAX_BONES): bones 1..7 a chain under the root (bone 7's chain to the root has exactly 8 bones), 8..11 another
    (bone 11's has exactly 5), the rest hang off them."""
    p = [-1, 0, 1, 2, 3, 4, 5, 6, 0, 8, 9, 10]
    p += [3, 12, 13, 3, 15, 16, 9, 18, 19, 9, 21, 22, 0, 24, 25, 26, 27, 28, 29, 30]
    return np.asarray(p, dtype=np.int32)


TREE31 = tree31()
TREE5 = np.asarray([-1, 0, 1, 2, 3, 0], dtype=np.int32)                  # V = 5: one chain of exactly 5 bones (0 .. 4) and a stray bone


class Clip:
    """Inputs of one clip, fp32 / uint8 as the kernel reads them."""

    def __init__(self, name, N, V, n_contact, rvel=(0.1, 0.0, 1.2), rang=(0.0, 0.4, 0.0), lift=0.0, on=5, off=4, sway=0.25):
        r = rng(name)
        offs = 0.25 * r.standard_normal((V, 3))
        offs[:, 1] -= 0.15
        offs[0, 1] += lift
        base, drift = r.standard_normal((V, 4)), sway * r.standard_normal((V, 4))
        t = np.arange(N, dtype=np.float64)[:, None, None]
        q = base[None] + drift[None] * np.sin(0.07 * t + np.arange(V)[None, :, None])
        q /= np.sqrt((q * q).sum(-1, keepdims=True))
        h = np.empty((N, V, 13))
        h[..., 0:3] = offs[None] + 0.01 * r.standard_normal((N, V, 3))
        h[..., 3:7] = q
        h[..., 7:10] = 0.5 * r.standard_normal((N, V, 3))
        h[..., 10:13] = r.standard_normal((N, V, 3))
        self.heads = h.astype(np.float32)
        self.speed = r.uniform(0.8, 1.6, N).astype(np.float32)
        self.sspeed = r.uniform(0.8, 1.2, N).astype(np.float32)
        self.rvel = (np.asarray(rvel) + 0.1 * r.standard_normal((N, 3))).astype(np.float32)
        self.rang = (np.asarray(rang) + 0.05 * r.standard_normal((N, 3))).astype(np.float32)
        f = np.arange(N)[:, None] + 3 * np.arange(n_contact)[None]
        self.contact = ((f % (on + off)) < on).astype(np.uint8).reshape(N, n_contact)
        self.N, self.V = N, V

    def arrays(self):
        return self.heads, self.speed, self.rvel, self.rang, self.sspeed, self.contact


class Case:
    def __init__(self, name, parents, bones, clips, exact=(), ik_enabled=True, blend=True, dt=pr.DT, strict_r2=False, **ik):
        self.strict_r2 = strict_r2          # the case's geometry is exact in any arithmetic: no allowance where the IK target sits on the heel
        self.name, self.parents, self.bones, self.clips, self.exact = name, np.asarray(parents, dtype=np.int32), tuple(bones), clips, set(exact)
        self.ik_enabled, self.blend, self.dt = ik_enabled, blend, dt
        self.ik = dict(pr.IK, **ik)
        self.V, self.N = clips[0].V, clips[0].N
        assert len(self.parents) == self.V + 1 and all(c.V == self.V and c.N == self.N and c.contact.shape[1] == len(bones) for c in clips)

    def kwargs(self):
        return dict(dt=self.dt, ik_enabled=self.ik_enabled, blend=self.blend, **self.ik)


_REF = {}


def reference(case):
    """The restatement of every clip of the case at float64 and at longdouble, computed once per session and left unchanged."""
    if case.name not in _REF:
        out = []
        for c in case.clips:
            out.append(tuple(pr.run_clip(*c.arrays(), case.parents, case.bones, dt_, **case.kwargs()) for dt_ in (np.float64, LD)))
        _REF[case.name] = out
    return _REF[case.name]


def check_decisions(case):
    """The condition under which kernel and restatement cannot legitimately branch differently."""
    decs = [r[0][3] for r in reference(case)]
    for kind in pr.Decisions.KINDS:
        if kind not in case.exact:
            for d, dl in zip(decs, [r[1][3] for r in reference(case)]):
                assert d.smallest(kind) >= DECISION_MARGIN, (case.name, kind, d.smallest(kind))
                assert d.count == dl.count, (case.name, "float64 and longdouble restatements decide differently")
    return decs


def total(decs, key):
    return sum(d.count[key] for d in decs)


def post_struct(case, n_clips, n_frames, dbuf, outs, state=None, valid=None):
    q = pr.pp_post()
    for k, v in zip(("heads", "speed", "src_rvel", "src_rang", "src_speed", "contact"), dbuf):
        setattr(q, k, pr.ptr(v))
    for k in ("pos", "rot", "ik_rot", "bvh_pos", "bvh_euler"):
        setattr(q, k, outs[k].ptr if outs.get(k) is not None else 0)
    q.state, q.valid = (state.ptr if state is not None else 0), pr.ptr(valid)
    q.n_clips, q.n_frames, q.V, q.n_contact = n_clips, n_frames, case.V, len(case.bones)
    q.ik_enabled, q.blend_enabled = int(case.ik_enabled), int(case.blend)
    for i in range(min(len(case.parents), pr.MAX_BONES)):
        q.parents[i] = int(case.parents[i])
    for i, b in enumerate(case.bones[:pr.MAX_CONTACT]):
        q.contact_bones[i] = int(b)
    q.dt, q.max_length_buffer, q.foot_height, q.unlock_radius, q.halflife = (case.dt, case.ik["max_length_buffer"], case.ik["foot_height"],
                                                                               case.ik["unlock_radius"], case.ik["halflife"])
    return q


def device_inputs(clips, frames=None):
    """The six input arrays of `clips` stacked (clips, frames, ...) on the device; an empty contact array still gets an address."""
    arrs = []
    for k in range(6):
        a = np.stack([c.arrays()[k] if frames is None else c.arrays()[k][frames] for c in clips])
        arrs.append(D(a) if a.size else torch.zeros(8, dtype=torch.uint8, device=dev()))
    return arrs


def make_outs(n_clips, n_frames, V, bvh=True, written=None):
    J = V + 1
    shapes = {"pos": (n_clips, n_frames, J, 3), "rot": (n_clips, n_frames, J, 4), "ik_rot": (n_clips, n_frames, J, 4)}
    if bvh:
        shapes["bvh_pos"], shapes["bvh_euler"] = (n_clips, n_frames, V, 3), (n_clips, n_frames, V, 3)
    w = (lambda shape: None if written is None else np.broadcast_to(written.reshape(n_clips, 1, 1, 1), shape).copy())
    return {k: Out(shape, "f64", w(shape)) for k, shape in shapes.items()}


def launch_clip(case, clips=None, bvh=True):
    clips = case.clips if clips is None else clips
    dbuf = device_inputs(clips)
    outs = make_outs(len(clips), case.N, case.V, bvh)
    q = post_struct(case, len(clips), case.N, dbuf, outs)
    assert pr.load().pp_post_clip(q, stream()) == 0, case.name
    return {k: o.check(f"{case.name} {k}") for k, o in outs.items()}


def hold_bvh(case, name, got, gimbal=()):
    """Family B on the kernel's own outputs of one clip: got[k] (N, ...)."""
    bp64, be64, s = pr.bvh_channels(got["pos"], got["rot"], got["ik_rot"], np.float64)
    bpl, bel, _ = pr.bvh_channels(got["pos"], got["rot"], got["ik_rot"], LD)
    hold("post_bvh pos", name, got["bvh_pos"], bpl, bp64, MARGIN64, floor_ulps=4)
    assert np.isfinite(got["bvh_euler"]).all(), (name, "Euler channels not finite")
    # as rotations: the quaternions of both triples, up to sign.  Floor: degrees -> radians -> half angle -> six sines and cosines -> sums
    # of products of three of them is about 16 float64 roundings on components of at most 1
    qk, q64, ql = pr.euler_to_quat(got["bvh_euler"]), pr.euler_to_quat(be64), pr.euler_to_quat(bel.astype(np.float64))
    dist = lambda a, b: float(np.minimum(np.abs(a - b).max(-1), np.abs(a + b).max(-1)).max())      # noqa: E731
    ek, eb = dist(qk, ql), dist(q64, ql)
    print(f"[pose] post_bvh euler     {name:40s} as rotations {ek:.3e} (restatement {eb:.3e}), largest |asin argument| {np.abs(s).max():.9f}")
    assert ek <= max(MARGIN64[0] * eb, 16 * np.finfo(np.float64).eps), (name, ek, eb)
    plain = np.abs(s) < 1 - 1e-6
    if plain.any():
        hold("post_bvh euler", name, got["bvh_euler"][plain], bel[plain], be64[plain], MARGIN64, floor_ulps=4)
    for f, j in gimbal:
        err = np.abs(got["bvh_euler"][f, j - 1] - bel[f, j - 1].astype(np.float64)).max()
        assert err <= 1e-9, (name, "gimbal", f, j, got["bvh_euler"][f, j - 1], bel[f, j - 1])


def run_case(case, gimbal=()):
    """CPU condition, launch, C and B yardsticks; returns the kernel's outputs (clips, N, ...) and the decisions."""
    decs = check_decisions(case)
    got = launch_clip(case)
    refs = reference(case)
    for k, idx in (("pos", 0), ("rot", 1), ("ik_rot", 2)):
        wide = np.stack([r[1][idx] for r in refs])
        narrow = np.stack([r[0][idx] for r in refs])
        if k != "ik_rot" or case.strict_r2:
            # With blending off pos is the heads' positions (asserted to the bit in test_clip_flags) and the root's one row per frame: 24 of
            # 600 rows carry all the error, each within one ulp (1.3e-16 at most on values below 1), and whether a row lands on the nearer
            # or the farther neighbour is the whole of the rms (kernel 5.8e-18 against the restatement's 2.4e-18: 2.47 x).  That output
            # alone has its rms held by the 4-ulp floor; every other float64 output keeps 2 x the yardstick
            hold("post_clip " + k, case.name, got[k], wide, narrow, MARGIN64, floor_ulps=4, rms_floor=(k == "pos" and not case.blend))
            continue
        # Where the IK target sits on the heel to rounding (|cross(c_a, t_a)| < R2_ON_HEEL in the restatement: a contact that has not
        # locked yet) the hip's rotation hangs on whether toe + (heel - toe) rounds to the heel, in the kernel as in the restatement:
        # those entries get the bound pose_ref derives for it (Decisions.r2), every other entry the yardstick
        loose = np.zeros(got[k].shape[:3], dtype=bool)
        allow = np.zeros(got[k].shape[:3])
        for ci, r in enumerate(refs):
            for f, hip, cl, noise in r[0][3].r2:
                if cl < R2_ON_HEEL:
                    loose[ci, f, hip], allow[ci, f, hip] = True, max(allow[ci, f, hip], noise)
        hold("post_clip " + k, case.name, got[k][~loose], wide[~loose], narrow[~loose], MARGIN64, floor_ulps=4)
        if loose.any():
            err = np.abs(got[k].astype(LD) - wide).max(-1).astype(np.float64)
            own = np.abs(narrow.astype(LD) - wide).max(-1).astype(np.float64)
            worst = float((err[loose] / allow[loose]).max())
            print(f"[pose] post_clip ik_rot   {case.name:40s} target on the heel, {int(loose.sum())} hips: largest {err[loose].max():.3e} "
                  f"({worst:.3f} of the derived bound; restatement {own[loose].max():.3e})")
            assert (err[loose] <= np.maximum(allow[loose], MARGIN64[0] * own[loose])).all(), (case.name, "hip with the target on the heel")
    for ci in range(len(case.clips)):
        hold_bvh(case, f"{case.name}[{ci}]", {k: v[ci] for k, v in got.items()}, gimbal)
    return got, decs


def step_through(case, clips, valid=None, bvh=True):
    """The resumable form: one launch per frame from zeroed state.  valid (frames, clips) or None.  Returns the outputs stacked
    (clips, frames, ...), with NaN rows where a clip was not stepped, and the state after every frame (frames, clips, STATE_DOUBLES)."""
    lib = pr.load()
    n = len(clips)
    assert lib.pp_post_state_doubles() == pr.STATE_DOUBLES
    state = Out((n, pr.STATE_DOUBLES), "f64")
    state.body.zero_()
    frames, states = [], []
    for i in range(case.N):
        dbuf = device_inputs(clips, i)
        v = None if valid is None else valid[i].astype(bool)
        outs = make_outs(n, 1, case.V, bvh, v)
        dv = None if valid is None else D(valid[i].astype(np.int32))
        before = state.body.cpu().numpy().copy()
        q = post_struct(case, n, 1, dbuf, outs, state, dv)
        assert lib.pp_post_step(q, stream()) == 0, (case.name, i)
        frames.append({k: o.check(f"{case.name} step {i} {k}") for k, o in outs.items()})
        after = state.body.cpu().numpy().copy()
        assert guards_intact(state)
        if v is not None:
            assert same_bits(after[~v], before[~v]), (case.name, i, "the state of a clip that was not stepped changed")
        states.append(after)
    return {k: np.concatenate([f[k] for f in frames], 1) for k in frames[0]}, np.stack(states)


KEYS = ("pos", "rot", "ik_rot", "bvh_pos", "bvh_euler")


def assert_step_is_clip(case, got):
    stepped, states = step_through(case, case.clips)
    for k in KEYS:
        assert same_bits(stepped[k], got[k]), (case.name, k, "stepping frame by frame differs from the clip launch")
    assert (states[-1][:, 0].view(np.int64) == case.N).all()


# ----------------------------------------------------------------------------------------------- the authored cases
def case_ratio():
    """Speed and source speed exact in fp32: ratio exactly 3.0 and exactly 0.33f keep it, one ulp beyond either resets it, 0.2 resets it."""
    c = Clip("ratio", 30, 24, 2)
    f32 = np.float32
    pattern = [f32(3.0), np.nextafter(f32(3.0), f32(4.0)), f32(0.33), np.nextafter(f32(0.33), f32(0.0)), f32(0.2), f32(1.25)]
    c.sspeed[:] = 1.0
    c.speed[:] = np.asarray([pattern[i % 6] for i in range(30)], dtype=np.float32)
    c.speed[18:24] = 0.2                                                  # a run
    return Case("ratio", MOCHA, (5, 24), [c], exact={"ratio"})


def case_small_rang():
    """src_rang = 0 for some frames, then 1e-4 (h = 8.3e-7 < 1e-5: the first-order branch of from_scaled_angle_axis), then 0.4."""
    c = Clip("small-rang", 30, 24, 2)
    c.rang[:10] = 0.0
    c.rang[10:20] = np.asarray([0.0, 1e-4, 0.0], dtype=np.float32)
    return Case("small-rang", MOCHA, (5, 24), [c])


def case_straight_leg():
    """Identity rotations down contact 0's chain, knee and heel offsets collinear (heel = knee / 2, exact in fp32), no velocities there."""
    c = Clip("straight-leg", 24, 24, 2)
    for b in (1, 2, 3, 4, 5):                                             # bones of the full tree; heads row b - 1
        c.heads[:, b - 1, 3:7] = np.asarray([1, 0, 0, 0], dtype=np.float32)
        c.heads[:, b - 1, 7:13] = 0.0
        c.heads[:, b - 1, 0:3] = c.heads[0, b - 1, 0:3]
    c.heads[:, 2, 0:3] = np.asarray([0.125, -0.375, 0.0625], dtype=np.float32)      # bone 3 (knee)
    c.heads[:, 3, 0:3] = c.heads[:, 2, 0:3] * np.float32(0.5)                       # bone 4 (heel)
    return Case("straight-leg", MOCHA, (5, 24), [c])


def case_reach():
    """Contact 1 locks at frame 1 and the root walks away under a radius that never unlocks: the target is beyond reach for a run of
    frames.  Contact 0 never touches and stays above the foot height: its target is exactly the heel's position (r2's cross product is 0)."""
    c = Clip("reach", 30, 24, 2, rvel=(0.1, 0.0, 6.0), lift=1.0)
    c.contact[:, 0] = 0
    c.contact[:, 1] = 1
    c.contact[0, 1] = 0
    return Case("reach", MOCHA, (5, 24), [c], unlock_radius=50.0)


def toe_height(c, parents, toe, frame=0):
    """Height of bone `toe` over the root in a frame of clip c (float64 forward kinematics of the heads; the root stays nearly upright)."""
    gp, gr = np.zeros(3), np.asarray([1.0, 0.0, 0.0, 0.0])
    for b in pr._chain(parents, toe)[::-1][1:]:
        h = c.heads[frame, b - 1].astype(np.float64)
        gp, gr = pr.q_rot(gr, h[0:3]) + gp, pr.q_mul(gr, h[3:7])
    return float(gp[1])


def case_exact_geometry(which="mocha"):
    """Nothing moves and every number is a small dyadic fraction: identity rotations, offsets in 64ths, no velocities, a root at rest, no
    contact ever.  Every position down the chains is then exact in any arithmetic, the never-locked targets are the heels to the bit in
    the kernel as in the restatement, and r2 has to turn nothing: held to the plain yardstick (strict_r2), which a cross product that
    leaves a rounding residual for two identical vectors misses by a factor of 100."""
    parents, bones, V = {"mocha": (MOCHA, (5, 24), 24), "mixamo": (MIXAMO, (18, 22), 22)}[which]
    c = Clip("exact-" + which, 24, V, 2)
    offs = np.round(c.heads[0, :, 0:3] * 64.0) / 64.0
    offs[0, 1] += 2.0
    c.heads[:, :, 0:3] = offs[None].astype(np.float32)
    c.heads[:, :, 3:7] = np.asarray([1, 0, 0, 0], dtype=np.float32)
    c.heads[:, :, 7:13] = 0.0
    c.rvel[:], c.rang[:], c.contact[:] = 0.0, 0.0, 0
    return Case("exact-geometry" + ("" if which == "mocha" else "-" + which), parents, bones, [c], strict_r2=True)


def case_locks():
    """Contact 0: short touches (label-driven unlocks), held from frame 1; contact 1: long touches that leave the radius (radius unlocks).
    Clip a stands with contact 0's toe 3 cm above the foot height, clip b 3 cm below it (the clamp)."""
    cl = []
    for name, above in (("locks-a", 0.03), ("locks-b", -0.03)):
        c = Clip(name, 48, 24, 2, sway=0.01)
        c.heads[:, 0, 1] += np.float32(pr.IK["foot_height"] + above - toe_height(c, MOCHA, 5))
        f = np.arange(48)
        c.contact[:, 0] = ((f - 1) % 6 < 2) & (f >= 1)
        c.contact[:, 1] = (f % 24 < 20) & (f >= 2)
        cl.append(c)
    return Case("locks", MOCHA, (5, 24), cl, unlock_radius=0.25)


def case_contacts(n, order="fwd"):
    bones = {0: (), 1: (23,), 3: (5, 4, 24), 4: (5, 4, 24, 23)}[n]
    c = Clip("contacts", 30, 24, 4)
    c.contact = np.ascontiguousarray(c.contact[:, :n])
    if order == "rev":
        bones, c.contact = bones[::-1], np.ascontiguousarray(c.contact[:, ::-1])
    return Case(f"contacts-{n}-{order}", MOCHA, bones, [c])


def case_skeleton(which):
    if which == "mixamo":
        return Case("skeleton-mixamo", MIXAMO, (18, 22), [Clip("sk-mixamo", 30, 22, 2)])
    if which == "tree31":
        return Case("skeleton-tree31", TREE31, (7, 11), [Clip("sk-tree31", 30, 31, 2)])
    return Case("skeleton-v5", TREE5, (4,), [Clip("sk-v5", 30, 5, 1)])


def case_flags(ik, blend):
    return Case(f"flags-ik{int(ik)}-blend{int(blend)}", MOCHA, (5, 24), [Clip("flags", 24, 24, 2)], ik_enabled=ik, blend=blend)


def many_clips():
    return [Clip(f"many-{i}", 24, 24, 2, rvel=(0.1 * i, 0.0, 1.0 + 0.1 * i), on=3 + i, off=2 + i) for i in range(5)]


def case_many(n):
    cl = many_clips()[:n]
    for c in cl:
        c.contact[1:4] = 1                                                # held from frame 1: the lock follows the reset of frame 0 at once
    return Case(f"many-{n}", MOCHA, (5, 24), cl)


def case_constants():
    return Case("constants", MOCHA, (5, 24), [Clip("constants", 30, 24, 2)], dt=1.0 / 30.0, halflife=0.25, unlock_radius=0.35,
                foot_height=0.05, max_length_buffer=0.04)


def case_gimbal():
    """Rotations (w, 0, y, 0) whose asin argument 2 w y is just below 1, exactly 1 (w = 1/2, y = 1: nobody normalises), and above 1,
    for both signs of y, on bones no contact rewrites (not 1..5 or 21..24); every product is exact in float64.  The root turns by more
    than 90 degrees (src_rang 2.6 rad/s about y over 1 s), which bone 1's root merge has to follow."""
    c = Clip("gimbal", 60, 24, 2, rang=(0.0, 2.6, 0.0))
    f32 = np.float32
    r = f32(0.70710677)
    up, down = np.nextafter(r, f32(1.0)), np.nextafter(r, f32(0.0))
    vals = [(r, r), (up, up), (down, down), (f32(0.5), f32(1.0)), (r, up), (f32(1.0), f32(0.5)), (up, down)]
    marks = []
    for k, (w, y) in enumerate(vals):
        for s, bone in ((1.0, 7 + k), (-1.0, 14 + k)):                   # bones 7..13 and 14..20
            c.heads[5:, bone - 1, 3:7] = np.asarray([w, 0.0, s * y, 0.0], dtype=np.float32)
            marks += [(5, bone), (59, bone)]
    return Case("gimbal", MOCHA, (5, 24), [c]), marks


CPU_CASES = {
    "ratio": case_ratio, "small-rang": case_small_rang, "exact-geometry": case_exact_geometry, "exact-geometry-mixamo": lambda: case_exact_geometry("mixamo"), "straight-leg": case_straight_leg, "reach": case_reach, "locks": case_locks,
    "contacts-0": lambda: case_contacts(0), "contacts-1": lambda: case_contacts(1), "contacts-3": lambda: case_contacts(3),
    "contacts-4": lambda: case_contacts(4), "contacts-4-rev": lambda: case_contacts(4, "rev"),
    "skeleton-mixamo": lambda: case_skeleton("mixamo"), "skeleton-tree31": lambda: case_skeleton("tree31"), "skeleton-v5": lambda: case_skeleton("v5"),
    "flags-00": lambda: case_flags(False, False), "flags-01": lambda: case_flags(False, True), "flags-10": lambda: case_flags(True, False),
    "flags-11": lambda: case_flags(True, True), "many-5": lambda: case_many(5), "constants": case_constants, "gimbal": lambda: case_gimbal()[0],
}


@pytest.mark.parametrize("name", list(CPU_CASES))
def test_clip_case_decisions_have_room(name):
    """On the CPU: every discrete decision of every family C case keeps DECISION_MARGIN, and each case reaches the edge it is authored for."""
    case = CPU_CASES[name]()
    decs = check_decisions(case)
    n = total
    if name == "ratio":
        m = np.asarray(decs[0].margin["ratio"])
        assert (m == 0).sum() >= 8 and n(decs, "ratio_reset") == 18 and n(decs, "ratio_kept") == 30 - n(decs, "ratio_reset")
    if name == "small-rang":
        assert n(decs, "h_small") == 20 and n(decs, "h_large") == 10
    if name.startswith("exact-geometry"):
        assert len(decs[0].r2) == 46 and all(cl == 0.0 for _, _, cl, _ in decs[0].r2), "every target is its heel, to the bit"
        assert all(1e-13 < noise < 1e-9 for _, _, _, noise in decs[0].r2)
        ref = reference(case)[0]
        assert pr.errors(ref[0][2], ref[1][2])[0] < 1e-14 and np.abs(ref[0][2] - ref[0][1]).max() > 1e-9      # the IK still acts (r0, r1)
    if name == "reach":
        on_heel = [cl for f, hip, cl, _ in decs[0].r2 if hip == 2]
        assert len(on_heel) == 29 and sum(cl == 0.0 for cl in on_heel) >= 25, "contact 0 never locks: its target is the heel, r2 has a zero cross product"
    if name == "reach":
        assert n(decs, "reach_clamp") >= 10 and n(decs, "radius_unlock") == 0 and n(decs, "lock") == 1
        assert n(decs, "foot_free") >= 29                                 # contact 0 is never clamped: its IK target is the heel itself
    if name == "locks":
        for d in decs:
            assert d.count["lock"] >= 4 and d.count["label_unlock"] >= 2 and d.count["radius_unlock"] >= 2, d.count
        assert n(decs, "foot_clamp") >= 10 and n(decs, "foot_free") >= 10
        assert all(c.contact[1, 0] == 1 and c.contact[0, 0] == 0 for c in case.clips)
    if name == "straight-leg":
        a, b = case.clips[0].heads[0, 2, 0:3], case.clips[0].heads[0, 3, 0:3]
        assert not np.cross(a.astype(np.float64), b.astype(np.float64)).any()
    if name == "contacts-4":
        ch = {b: pr._chain(MOCHA, b) for b in case.bones}
        assert ch[5][3] == 2 and ch[4][2] == 2 and ch[4][3] == 1 and ch[23][3] == 1      # bone 2: hip of one chain, knee of another
        a, b = reference(case)[0][0][2], reference(CPU_CASES["contacts-4-rev"]())[0][0][2]
        assert np.abs(a[1:, 2] - b[1:, 2]).max() > 1e-3 and np.abs(a[1:, 1] - b[1:, 1]).max() > 1e-3, "the order of the contacts decides bones 1 and 2"
    if name == "skeleton-tree31":
        assert len(pr._chain(TREE31, 7)) == 8 and len(pr._chain(TREE31, 11)) == 5 and len(TREE31) == pr.MAX_BONES
    if name == "gimbal":
        _, marks = case_gimbal()
        ref = reference(case)[0][0]
        s = pr.bvh_channels(ref[0], ref[1], ref[2], np.float64)[2]
        vals = np.asarray([s[f, j - 1] for f, j in marks])
        assert (np.abs(vals) == 1).any() and (np.abs(vals) > 1).any() and ((np.abs(vals) < 1) & (np.abs(vals) > 1 - 1e-6)).any()
        assert (vals > 0).any() and (vals < 0).any()
        assert ref[1][-1, 0, 0] < np.cos(np.radians(45.0))                # the root has turned by more than 90 degrees


# ----------------------------------------------------------------------------------------------- GPU
@gpu
@pytest.mark.parametrize("name", ["ratio", "small-rang", "straight-leg", "reach", "constants", "exact-geometry", "exact-geometry-mixamo"])
def test_clip_authored(name):
    run_case(CPU_CASES[name]())


@gpu
@pytest.mark.parametrize("name", ["locks", "contacts-0", "contacts-1", "contacts-3", "contacts-4", "contacts-4-rev", "skeleton-mixamo",
                                  "skeleton-tree31", "skeleton-v5"])
def test_clip_and_its_resumable_form(name):
    """Cases 5, 6, 7: the clip launch against the restatement, and the resumable form stepped frame by frame from zeroed state = the clip
    launch, bit for bit."""
    case = CPU_CASES[name]()
    got, _ = run_case(case)
    assert_step_is_clip(case, got)


@gpu
def test_clip_later_contacts_win():
    """Bone 2 is the hip of contact (bone) 5's chain and the knee of contact 4's, bone 1 the hip of 4's and 23's: the list in both
    orders gives each chain's own rotations, and the later entry's where two chains meet."""
    fwd, rev = CPU_CASES["contacts-4"](), CPU_CASES["contacts-4-rev"]()
    a, b = launch_clip(fwd, bvh=False)["ik_rot"][0], launch_clip(rev, bvh=False)["ik_rot"][0]
    for bone in (1, 2, 21):                                               # where two chains meet, the order decides
        assert np.abs(a[1:, bone] - b[1:, bone]).max() > 1e-3, bone
    rest = [j for j in range(25) if j not in (1, 2, 21)]
    assert same_bits(a[:, rest], b[:, rest])                              # bones one chain writes, or none, do not depend on the order
    ra, rb = reference(fwd)[0][0][2], reference(rev)[0][0][2]
    for bone in (1, 2, 21):                                               # and it is the LATER entry that stays (far apart: 1e-3 against rounding)
        assert np.abs(a[1:, bone] - ra[1:, bone]).max() < 1e-6 < np.abs(a[1:, bone] - rb[1:, bone]).max(), bone


@gpu
@pytest.mark.parametrize("ik,blend", [(False, False), (False, True), (True, False), (True, True)])
def test_clip_flags(ik, blend):
    case = case_flags(ik, blend)
    got, _ = run_case(case)
    if not ik:
        assert same_bits(got["ik_rot"], got["rot"])
    if not blend:
        assert same_bits(got["pos"][0][:, 1:], case.clips[0].heads[..., 0:3].astype(np.float64))


@gpu
def test_clip_counts_and_clips_alone():
    """1, 3 and 5 different clips per launch: each clip's rows are bit-equal to the same clip launched alone (the contact reset of frame 0
    reads the clip's own heads: every clip's contact is held from frame 1, so a reset from another clip's heads shows at once)."""
    five = case_many(5)
    got5, _ = run_case(five)
    alone = [launch_clip(five, [c]) for c in five.clips]
    got3 = launch_clip(five, five.clips[1:4])
    for k in KEYS:
        for i in range(5):
            assert same_bits(got5[k][i], alone[i][k][0]), (k, i)
        for i in range(3):
            assert same_bits(got3[k][i], alone[i + 1][k][0]), (k, i)


@gpu
def test_step_valid_mask():
    """The resumable form with a valid mask: a clip whose entry is 0 keeps its output rows (guards) and its state bytes (asserted frame
    by frame in step_through), the other clips are bit-equal to an unmasked run, and a clip skipped for k frames and then stepped goes on
    from its stored state - its outputs are those of the clip launched on the frames it was given."""
    case = case_many(3)
    N = case.N
    valid = np.ones((N, 3), dtype=np.int32)
    valid[6:11, 1] = 0                                                    # skipped for five frames in mid-clip
    valid[0:3, 2] = 0                                                     # starts three frames late: its first frame is frame 3
    valid[20:, 2] = 0
    stepped, states = step_through(case, case.clips, valid)
    full = launch_clip(case)
    for k in KEYS:
        assert same_bits(stepped[k][0], full[k][0]), k
    for ci in (1, 2):
        seen = np.flatnonzero(valid[:, ci])
        c, sub = case.clips[ci], Clip.__new__(Clip)
        sub.heads, sub.speed, sub.rvel, sub.rang, sub.sspeed, sub.contact = (np.ascontiguousarray(a[seen]) for a in c.arrays())
        sub.N, sub.V = len(seen), c.V
        want = launch_clip(Case(f"masked-{ci}", case.parents, case.bones, [sub]))
        for k in KEYS:
            assert same_bits(stepped[k][ci][seen], want[k][0]), (k, ci)
        assert int(states[-1][ci, 0].view(np.int64)) == len(seen)
    assert (states[2][2] == 0).all()                                      # never stepped so far: still the zeroed state


@gpu
def test_bvh_gimbal_and_root_merge():
    case, marks = case_gimbal()
    got, _ = run_case(case, gimbal=marks)
    eu = got["bvh_euler"][0]
    hit = [eu[f, j - 1, 1] for f, j in marks]
    assert any(abs(v - 90.0) < 1e-12 for v in hit) and any(abs(v + 90.0) < 1e-12 for v in hit), "the clamp gives +-90 degrees"


@gpu
def test_clip_without_bvh_changes_nothing_else():
    case = case_flags(True, True)
    with_, without = launch_clip(case), launch_clip(case, bvh=False)
    assert set(without) == {"pos", "rot", "ik_rot"}
    for k in without:
        assert same_bits(with_[k], without[k]), k


@gpu
def test_clip_refusals():
    """What the launchers refuse - V + 1 = 33, n_contact = 5, a step with n_frames != 1 or without a state - returns hipErrorInvalidValue
    and leaves every buffer intact."""
    lib = pr.load()
    case = case_flags(True, True)
    c = case.clips[0]
    dbuf = device_inputs([c])
    before = [b.clone() for b in dbuf]

    def refused(q, outs, call, state=None):
        assert call(q, stream()) == pr.INVALID_VALUE
        assert all(o.intact() for o in outs.values()) and (state is None or state.intact())
        assert all(torch.equal(a, b) for a, b in zip(dbuf, before))

    outs = make_outs(1, case.N, 32)                                       # V = 32: V + 1 = 33 bones
    q = post_struct(case, 1, case.N, dbuf, outs)
    q.V = 32
    refused(q, outs, lib.pp_post_clip)
    outs = make_outs(1, case.N, case.V)
    q = post_struct(case, 1, case.N, dbuf, outs)
    q.n_contact = 5
    refused(q, outs, lib.pp_post_clip)
    state = Out((1, pr.STATE_DOUBLES), "f64")
    q = post_struct(case, 1, 2, dbuf, outs, state)                        # a step of two frames
    refused(q, outs, lib.pp_post_step, state)
    q = post_struct(case, 1, 1, dbuf, outs)                               # a step without a state
    refused(q, outs, lib.pp_post_step)
