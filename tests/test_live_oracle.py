"""Live sessions against an independent restatement of the loop (oracle/live_oracle.py: the oracles' own featurisation, network,
float64 search and frame loop), on the layout the live path runs on: `mixamo`, 23 bones, toes = bones 18 and 22.

CPU part (-m "not gpu"): the featurisation and post-processing oracles against fixtures the reference itself produced for this layout
(tests/golden/featurize_mixamo.npz, postprocess_mixamo.npz; recipe: tests/golden/make_golden.py), LiveOracle against the clip-at-once
composition of the same oracle parts, and the conditions the GPU tests' inputs must meet, checked with the oracle alone.

GPU part (-m gpu): LiveSession / mocha_live_step, stage by stage (X_raw, idx, Y, heads, speed read out of the session buffer; the
post-processing frame in isolation) and end to end, for S = 1 and S = 4 over 60 + 43 frames, and for a stream that is reset, a stream
whose character changes and a stream whose ring wraps more than once; PostProcessor.run / .step on the mixamo model against the
reference's own frame loop.

Bounds.  X_raw: 1e-4 * max(1, max|X|) (test_featurize_hip_matches_reference).  idx: the float64 search of the stream's own segment of
the ORACLE's bank; another row only as a near-tie (relative gap <= 2e-6, tests/test_multi_character.py::_check_idx), and the inputs are
chosen so that no near-tie exists (gaps >= 1e-4), so the count must be 0.  Y: 1e-4 against the oracle's decode on the row the device
matched (tests/test_multi_character.py TOL).  heads / speed against postprocess_oracle.pose_heads of the device's own Y: 2e-5 on the
quaternions up to sign, the copied channels equal, 1e-6 on speed (test_pose_heads_parity).  One float64 PostProcess.step fed the
device's own heads: 1e-9 on pos / rot / ik_rot / bvh_pos, 1e-6 on bvh_euler (test_step_against_the_reference_loop).  End to end (pos,
rot of the fully independent oracle run): E2E_BOUND below."""
import functools
import os

import numpy as np
import pytest
import torch

from mocha_sigasia2023_amd import synthetic, weights
from mocha_sigasia2023_amd.skeleton import LAYOUTS
from oracle import featurize_oracle as FO
from oracle import live_oracle as LO
from oracle import postprocess_oracle as P

GOLD = os.path.join(os.path.dirname(__file__), "golden")
LAYOUT = "mixamo"
V, J = 22, 23
PARENTS = FO.full_parents(LAYOUTS[LAYOUT]["parents"])
TOES = (18, 22)
N = 44                                  # valid frames of the two main runs
F = 60 + N - 1                          # 60 + 43 pushes
LONG = 140                              # pushes of the events run; every clip is generated this long
BANK_SEEDS = (121, 103, 123)            # bank clips of the three characters (99 frames = 40 rows each): seeds, and the streams of the
                                        # events run, chosen on the CPU so that every match used has a float64 gap >= 2e-4
KEYS = ("pos", "rot", "ik_rot", "bvh_pos", "bvh_euler")

# End-to-end bound.  Spread between the oracle chain with the network in fp32 and in float64 (same frames, same decoded rows), measured
# on the CPU over every valid frame of every stream of the three runs below (361 frames): max |pos| difference 2.2e-8, max |rot|
# difference 7.0e-7 -> spread 7.0e-7.  4 x spread = 2.8e-6 is below the floor, so the bound max(1e-4, 4 x spread) is 1e-4.
# test_end_to_end_bound_covers_the_oracle_spread repeats the measurement on one stream.
SPREAD = 7.0e-7
E2E_BOUND = max(1e-4, 4 * SPREAD)


def _plan(clip, pushes, char, reset_at=None, char_at=None):
    """The pushes of one stream: ((clip, clip frame, character, reset before this push), ...).  After a reset the stream sees its clip
    from frame 0 again; from push char_at[0] on its character is char_at[1]."""
    out = []
    for k in range(pushes):
        f = k - reset_at if reset_at is not None and k >= reset_at else k
        c = char if char_at is None or k < char_at[0] else char_at[1]
        out.append((clip, f, c, k == reset_at))
    return tuple(out)


# stream plans of the three sessions: S = 1; S = 4 with mixed characters, character 2 used twice; the events run - stream 0 runs for 140
# pushes (its 60-slot ring wraps more than once), stream 1 is reset before push 65 and warms up again while the others run, stream 2
# changes its character before push 90
RUNS = {
    "S1": (_plan(0, F, 2),),
    "S4": (_plan(0, F, 2), _plan(1, F, 0), _plan(2, F, 1), _plan(3, F, 2)),
    "events": (_plan(0, LONG, 0), _plan(2, LONG, 1, reset_at=65), _plan(1, LONG, 1, char_at=(90, 0))),
}


def _pose_norm():
    rng = np.random.Generator(np.random.PCG64(0))
    X_mean = (0.05 * rng.standard_normal((J, 15))).astype(np.float32); X_std = rng.uniform(0.5, 1.5, (J, 15)).astype(np.float32)
    Y_mean = (0.05 * rng.standard_normal((J, 15))).astype(np.float32); Y_std = rng.uniform(0.2, 0.6, (J, 15)).astype(np.float32)
    return X_mean, X_std, Y_mean, Y_std


@functools.lru_cache(maxsize=None)
def _inputs():
    """What both sides are fed, as NumPy: weights, norms, the characters' bank clips, four source clips and their per-frame signals."""
    sd = weights.synthetic_state_dict(1777, 1.0, LAYOUT)
    mean, std = synthetic.cnt_norm(7)
    bank_clips = [synthetic.smooth_bone_clip(s, 60 + 40 - 1, J) for s in BANK_SEEDS]
    clips = [synthetic.smooth_bone_clip(200 + s, LONG, J, phase=0.3 * s) for s in range(4)]
    per = []
    for s in range(4):
        _, rvel, rang, hipvel, contact = synthetic.postprocess_inputs(50 + s, LONG, V=V)
        per.append((rvel, rang, np.linalg.norm(hipvel, axis=-1).mean(-1).astype(np.float32), contact))
    return dict(sd=sd, pose_norm=_pose_norm(), mean=mean, std=std, bank_clips=bank_clips, clips=clips, per=per)


@functools.lru_cache(maxsize=None)
def _oracle_banks(float64=False):
    w = _inputs()
    return [LO.bank_from_clip(w["sd"], LAYOUT, w["pose_norm"], w["mean"], w["std"], c, float64) for c in w["bank_clips"]]


def _oracle(float64=False):
    w = _inputs()
    return LO.LiveOracle(w["sd"], LAYOUT, w["pose_norm"], w["mean"], w["std"], _oracle_banks(float64), TOES, float64=float64)


def _push_args(clip, f):
    w = _inputs()
    return [a[f] for a in w["clips"][clip]] + [a[f] for a in w["per"][clip]]


def _oracle_run(plan, float64=False, forced=None):
    """LiveOracle over one stream's plan -> the list of push() results.  forced: per push the row to decode on (None: the match)."""
    o = _oracle(float64)
    out = []
    for k, (clip, f, char, reset) in enumerate(plan):
        if reset:
            o.reset()
        out.append(o.push(*_push_args(clip, f), char, forced_row=None if forced is None else forced[k]))
    return out


_oracle_run_cached = functools.lru_cache(maxsize=None)(lambda plan: _oracle_run(plan))


def _all_plans():
    seen = []
    for plans in RUNS.values():
        for p in plans:
            if p not in seen:
                seen.append(p)
    return seen


# ------------------------------------------------------------------------------------------------ CPU: the oracles on this layout
def test_featurize_oracle_matches_reference_on_mixamo():
    z = np.load(os.path.join(GOLD, "featurize_mixamo.npz"))
    seed, B = (int(v) for v in z["seed"])
    X = FO.featurize(*synthetic.bone_windows(seed, B, J=J), PARENTS)
    assert X.shape == (B, 60, J, 15) and np.array_equal(X, z["X"])
    # the fixture tells the two parent tables apart
    Xm = FO.featurize(*synthetic.bone_windows(seed, B, J=J), FO.full_parents(LAYOUTS["mocha"]["parents"])[:J])
    assert np.abs(Xm - z["X"]).max() > 1e-2


def _post_inputs():
    z = np.load(os.path.join(GOLD, "postprocess_mixamo.npz"))
    n = int(z["seed"][1])
    Y, rvel, rang, hipvel, contact = synthetic.postprocess_inputs(int(z["seed"][0]), n, V=V)
    Ycm = synthetic.postprocess_inputs(int(z["cm_seed"][0]), int(z["cm_seed"][1]), V=V)[0]
    return z, Y, Ycm, rvel, rang, np.linalg.norm(hipvel, axis=-1).mean(-1).astype(np.float32), contact


def test_postprocess_oracle_matches_reference_loop_on_mixamo():
    z, Y, Ycm, rvel, rang, src_speed, contact = _post_inputs()
    heads, speed = P.pose_heads(Y)
    assert np.array_equal(heads[..., 3:7], z["heads_rot"])
    assert np.array_equal(speed, z["speed"])
    pos, rot, ik = P.run_clip(heads, speed, rvel, rang, src_speed, contact, PARENTS, contact_bones=TOES)
    assert pos.shape == (len(Y), J, 3)
    assert np.abs(pos - z["pos"]).max() < 1e-12
    assert np.abs(rot - z["rot"]).max() < 1e-12
    assert np.abs(ik - z["ik_rot"]).max() < 1e-9
    assert (np.abs(ik - rot).max(axis=(1, 2)) > 1e-6).sum() > 50          # the IK really acts
    bp, be = P.bvh_channels(pos, ik)
    assert np.abs(bp - z["bvh_pos"]).max() < 1e-12
    assert np.abs(be - z["bvh_euler"]).max() < 1e-6
    # the "cm_" stream of the same executed loop: no blending, no IK
    hc, sc = P.pose_heads(Ycm)
    assert np.array_equal(sc, z["cm_speed"])
    pos, rot, ik = P.run_clip(hc, sc, rvel, rang, src_speed, contact, PARENTS, contact_bones=TOES, ik_enabled=False, blend=False)
    assert np.abs(pos - z["cm_pos"]).max() < 1e-12 and np.abs(rot - z["cm_rot"]).max() < 1e-12
    assert np.array_equal(ik, rot)
    bp, be = P.bvh_channels(pos, rot)
    assert np.abs(bp - z["cm_bvh_pos"]).max() < 1e-12 and np.abs(be - z["cm_bvh_euler"]).max() < 1e-6
    assert np.abs(z["cm_pos"][1:, 1:] - hc[1:, :, 0:3]).max() == 0


def test_oracle_exercises_every_contact_transition_on_mixamo():
    z, Y, _, rvel, rang, src_speed, contact = _post_inputs()
    heads, speed = P.pose_heads(Y)
    pp = P.PostProcess(PARENTS, contact_bones=TOES)
    locks, ratios = [], []
    for i in range(len(Y)):
        pp.step(heads[i], speed[i], rvel[i], rang[i], src_speed[i], contact[i])
        locks.append([c.lock for c in pp.contacts])
        ratios.append(speed[i] / src_speed[i])
    locks = np.asarray(locks)
    assert locks.any() and not locks.all()
    assert (locks[1:] & ~locks[:-1]).any()                                                    # a lock
    assert ((~locks[1:]) & locks[:-1] & (contact[1:] == 0)).any()                             # an unlock by the label
    assert ((~locks[1:]) & locks[:-1] & (contact[1:] == 1) & (contact[:-1] == 1)).any()       # an unlock by the radius
    assert max(ratios) > 3.0                                                                  # the ratio reset branch


# ------------------------------------------------------------------------------------------------ CPU: LiveOracle itself
def _composition(clip, char, frames):
    """The clip at once from the same oracle parts: slide_windows -> featurize -> encode -> search -> decode -> run_clip."""
    w = _inputs()
    sd = LO.torch_state(w["sd"])
    X = FO.featurize(*[synthetic.slide_windows(a[:frames]) for a in w["clips"][clip]], PARENTS)
    enc, cnt = LO.encode_windows(sd, X, w["pose_norm"])
    nm, encoded = _oracle_banks()[char]
    q = LO.O.znorm(cnt.numpy(), w["mean"], w["std"])
    idx = np.array([int(LO.search(q[i], nm)[0][0]) for i in range(len(q))])
    Y = np.stack([LO.decode(sd, enc[i:i + 1], encoded[idx[i]], w["pose_norm"]) for i in range(len(q))])
    heads, speed = P.pose_heads(Y)
    per = [a[59:frames] for a in w["per"][clip]]
    pos, rot, ik = P.run_clip(heads, speed, *per, PARENTS, contact_bones=TOES)
    bp, be = P.bvh_channels(pos, ik)
    return dict(X_raw=X, idx=idx, Y=Y, heads=heads, speed=speed, pos=pos, rot=rot, ik_rot=ik, bvh_pos=bp, bvh_euler=be)


def test_live_oracle_equals_the_clip_at_once_composition():
    frames = 60 + 61                                                       # the frame list turns over more than once
    got = _oracle_run(_plan(1, frames, 1))
    assert [g["valid"] for g in got] == [0] * 59 + [1] * 62
    assert all(set(g) == {"valid"} for g in got[:59])
    ref = _composition(1, 1, frames)
    for k in ("X_raw", "idx", "Y", "heads", "speed") + KEYS:
        a = np.stack([np.asarray(g[k]) for g in got[59:]])
        assert a.shape == ref[k].shape and np.array_equal(a, ref[k]), k
    for g in got[59:]:
        assert g["dist"] == g["dists"][g["idx"]] == g["dists"].min() and g["dist2"] >= g["dist"]


def test_live_oracle_reset_reproduces_a_fresh_oracle():
    plan = _plan(2, 60 + 20 + 63, 0, reset_at=80)
    got = _oracle_run(plan)
    fresh = _oracle_run(_plan(2, 63, 0))
    assert [g["valid"] for g in got[80:]] == [0] * 59 + [1] * 4 and [g["valid"] for g in got[59:80]] == [1] * 21
    for a, b in zip(got[80:], fresh):
        assert a.keys() == b.keys()
        for k in a:
            assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), k
    assert not np.array_equal(got[79]["pos"], got[139]["pos"])
    assert np.array_equal(got[139]["ik_rot"], got[139]["rot"])             # the first valid frame after a reset is a first frame


def test_live_oracle_forced_row_and_float64_mode():
    plan = _plan(0, 61, 2)
    a = _oracle_run(plan)[-1]
    other = (a["idx"] + 20) % 40
    b = _oracle_run(plan, forced=[None] * 60 + [other])[-1]
    assert b["idx"] == a["idx"] and np.array_equal(b["dists"], a["dists"])  # the match is reported as it is ...
    assert np.abs(b["Y"] - a["Y"]).max() > 1e-5                             # ... and the decode took the forced row
    c = _oracle_run(plan, float64=True)[-1]
    assert c["Y"].dtype == np.float64 and a["Y"].dtype == np.float32 and c["idx"] == a["idx"]
    assert 0 < np.abs(c["Y"] - a["Y"]).max() < 1e-4


# ------------------------------------------------------------------------------------------------ CPU: conditions on the GPU tests' inputs
def test_inputs_have_clear_matches_and_varied_rows():
    """Every (stream, valid frame) the GPU tests use: the float64 gap between the best and the second-best row of the stream's own
    character is at least 1e-4 relative (50 x the near-tie rule), so the GPU tests may demand zero accepted near-ties; every stream's
    matches cover at least 3 distinct rows; the root-velocity ratio stays clear of its two reset thresholds, where the frame loop is
    discontinuous in the heads."""
    for plan in _all_plans():
        got = [(p, g) for p, g in zip(plan, _oracle_run_cached(plan)) if g["valid"]]
        gaps = [(g["dist2"] - g["dist"]) / g["dist"] for _, g in got]
        rows = {g["idx"] for _, g in got}
        print(f"clip {plan[0][0]}: {len(got)} valid frames, min relative gap {min(gaps):.3e}, {len(rows)} distinct rows")
        assert min(gaps) >= 1e-4, (plan[0], min(gaps))
        assert len(rows) >= 3, (plan[0], rows)
        for (clip, f, _, _), g in got:
            ratio = float(g["speed"]) / float(_inputs()["per"][clip][2][f])
            assert min(abs(ratio - 3.0), abs(ratio - 0.33)) > 1e-3, (clip, f, ratio)


def test_frame_loop_is_well_conditioned_on_the_inputs_used():
    """The 1e-9 bound of the isolated frame-loop check assumes that the decoded heads keep the oracle's IK away from the clip boundaries
    of arccos and from near-zero cross products, where a last-bit difference of the device's float64 arithmetic would be amplified
    without bound.  Measured with the oracle alone: relative noise of 1e-13 in the heads (about 1000 float64 roundings) moves pos /
    rot / ik_rot by at most 6e-12 over every run used; 1e-10 here leaves the GPU check a factor 10 and more."""
    rng = np.random.default_rng(0)
    worst = 0.0
    for plan in _all_plans():
        a = b = None
        for (clip, f, _, reset), g in zip(plan, _oracle_run_cached(plan)):
            if reset:
                a = b = None
            if not g["valid"]:
                continue
            if a is None:
                a, b = (P.PostProcess(PARENTS, contact_bones=TOES) for _ in range(2))
            per = _push_args(clip, f)[4:]
            noisy = g["heads"].astype(np.float64) * (1 + 1e-13 * rng.standard_normal(g["heads"].shape))
            worst = max(worst, max(np.abs(x - y).max() for x, y in zip(a.step(g["heads"], g["speed"], *per), b.step(noisy, g["speed"], *per))))
    print(f"frame loop: 1e-13 relative noise in the heads moves the outputs by {worst:.2e}")
    assert worst < 1e-10


def test_end_to_end_bound_covers_the_oracle_spread():
    """The measurement behind E2E_BOUND, repeated on one stream: the oracle chain with the network in float64 against fp32."""
    plan = RUNS["S1"][0]
    a = _oracle_run_cached(plan)
    b = _oracle_run(plan, float64=True, forced=[g.get("idx") for g in a])
    spread = max(max(np.abs(x[k] - y[k]).max() for k in ("pos", "rot")) for x, y in zip(a, b) if x["valid"])
    print(f"fp32 / float64 oracle spread on pos, rot: {spread:.3e}")
    assert 4 * spread <= E2E_BOUND and 4 * SPREAD <= E2E_BOUND


# ------------------------------------------------------------------------------------------------ GPU
def dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def world():
    from mocha_sigasia2023_amd import Generator, MultiCharacterBank, PostProcessor, build_bank
    d, w = dev(), _inputs()
    model = Generator(layout=LAYOUT, device=d).load_state_dict(w["sd"]).eval()
    model.set_pose_norm(*w["pose_norm"])
    mean, std = torch.from_numpy(w["mean"]).to(d), torch.from_numpy(w["std"]).to(d)
    banks = []
    for clip in w["bank_clips"]:                                           # the device's own encodings of the same bank clips
        b = build_bank(model, model.featurize(*[torch.from_numpy(synthetic.slide_windows(a)) for a in clip]), raw=True)
        banks.append((((b["cnt"] - mean) / std).reshape(-1, 90 * 256), b["encoded"]))
    mb = MultiCharacterBank(model, banks)
    post = PostProcessor(model, contact_bones=list(TOES))
    return dict(model=model, mean=mean, std=std, mb=mb, post=post)


def _staging(sess):
    """Views of the step's staging inside the session buffer: the layout of mocha_live_step's private buffer (every section on a
    256-byte boundary), checked against mocha_live_state_bytes."""
    m, S = sess.model, sess.streams
    lib, h = m._ctx.lib, m._ctx.h
    sections = [("counters", S * 8), ("post", S * int(lib.mocha_post_state_bytes(h))), ("rot", S * 60 * J * 16), ("pos", S * 60 * J * 12),
                ("vel", S * 60 * J * 12), ("ang", S * 60 * J * 12), ("X_raw", S * 60 * J * 60), ("Y", S * 60 * V * 60),
                ("heads", S * V * 52), ("speed", S * 4), ("eff", S * 4)]
    off, at = {}, 0
    for name, n in sections:
        off[name] = at
        at += (n + 255) // 256 * 256
    assert at == int(lib.mocha_live_state_bytes(h, S)) == sess.live.numel()
    shapes = {"X_raw": (S, 60, J, 15), "Y": (S, 60, V, 15), "heads": (S, V, 13), "speed": (S,)}
    return {k: sess.live[off[k]: off[k] + 4 * int(np.prod(s))].view(torch.float32).reshape(s) for k, s in shapes.items()}


def _run_device(world, plans):
    """The session over the streams' plans -> per push a dict of NumPy arrays (all streams): valid, idx, the staging, the outputs."""
    from mocha_sigasia2023_amd import LiveSession
    S = len(plans)
    sess = LiveSession(world["mb"], world["mean"], world["std"], streams=S, post=world["post"])
    stage = _staging(sess)
    for k in KEYS:
        sess.out[k].fill_(-12345.0)
    rec = []
    for k in range(len(plans[0])):
        resets = [s for s in range(S) if plans[s][k][3]]
        if resets:
            sess.reset(resets)
        args = [np.stack([_push_args(plans[s][k][0], plans[s][k][1])[i] for s in range(S)]) for i in range(8)]
        o = sess.push(*[torch.from_numpy(np.ascontiguousarray(a)) for a in args], characters=[plans[s][k][2] for s in range(S)])
        torch.cuda.synchronize()
        r = {n: o[n].cpu().numpy().copy() for n in KEYS + ("idx", "valid")}
        r.update({n: t.cpu().numpy().copy() for n, t in stage.items()})
        rec.append(r)
    return rec


def _check_stream(rec, s, plan, errs):
    """Stream s of a recorded device run against LiveOracle over the same plan, stage by stage and end to end (module docstring).
    Returns the number of accepted near-ties; the largest errors go into errs."""
    oracle = _oracle()
    iso = None                                                              # the frame loop alone, float64, fed the device's heads
    ties, rows = 0, set()
    prev = {k: np.full_like(rec[0][k][s], -12345.0) for k in KEYS}

    def worst(name, e, bound):
        errs[name] = max(errs.get(name, 0.0), float(e))
        assert e < bound, (name, s, k, float(e), bound)
    for k, (clip, f, char, reset) in enumerate(plan):
        r = rec[k]
        args = _push_args(clip, f)
        if reset:
            oracle.reset(); iso = None
        if len(oracle.frames) < 59:                                         # warming up: no match, no output row written
            o = oracle.push(*args, char)
            assert o["valid"] == 0 and int(r["valid"][s]) == 0 and int(r["idx"][s]) == -1, (s, k)
            for n in KEYS:
                assert np.array_equal(r[n][s], prev[n]), (n, s, k)
            continue
        assert int(r["valid"][s]) == 1, (s, k)
        got = int(r["idx"][s])
        o = oracle.push(*args, char, forced_row=got if 0 <= got < len(oracle.banks[char][0]) else None)
        assert 0 <= got < len(o["dists"]), (s, k, got)
        if got != o["idx"]:
            assert o["dists"][got] - o["dist"] <= 2e-6 * o["dist"], (s, k, got, o["idx"], o["dists"][got], o["dist"])
            ties += 1
        rows.add(got)
        worst("X_raw", np.abs(r["X_raw"][s] - o["X_raw"]).max() / max(1.0, float(np.abs(o["X_raw"]).max())), 1e-4)
        worst("Y", np.abs(r["Y"][s] - o["Y"]).max(), 1e-4)
        h, sp = P.pose_heads(r["Y"][s][None])
        a, b = r["heads"][s][:, 3:7], h[0][:, 3:7]
        worst("heads quat", np.minimum(np.abs(a - b).max(-1), np.abs(a + b).max(-1)).max(), 2e-5)
        assert np.array_equal(np.delete(r["heads"][s], np.s_[3:7], -1), np.delete(h[0], np.s_[3:7], -1)), (s, k)
        worst("speed", abs(float(r["speed"][s]) - float(sp[0])), 1e-6)
        if iso is None:
            iso = P.PostProcess(PARENTS, contact_bones=TOES)
        p, q, ik = iso.step(r["heads"][s], r["speed"][s], *args[4:])
        bp, be = P.bvh_channels(p[None], ik[None])
        for n, ref in (("pos", p), ("rot", q), ("ik_rot", ik), ("bvh_pos", bp[0])):
            worst("step " + n, np.abs(r[n][s] - ref).max(), 1e-9)
        worst("step bvh_euler", np.abs(r["bvh_euler"][s] - be[0]).max(), 1e-6)
        for n in ("pos", "rot"):
            worst("end to end " + n, np.abs(r[n][s] - o[n]).max(), E2E_BOUND)
        prev = {n: r[n][s] for n in KEYS}
    assert len(rows) >= 3, (s, rows)
    return ties


def _report(name, errs):
    for k, v in errs.items():
        print(f"{name}: max error {k}: {v:.3e}")


@pytest.mark.gpu
@pytest.mark.parametrize("run", ["S1", "S4"])
def test_live_session_against_the_oracle(world, run):
    """S = 1 and S = 4 (characters 2, 0, 1, 2), 60 + 43 pushes, every valid frame of every stream: X_raw, idx, Y, heads, speed, the
    post-processing frame in isolation, and pos / rot end to end, at the bounds of the module docstring.  End to end: measured fp32 /
    float64 oracle spread 7.0e-7, bound max(1e-4, 4 x 7.0e-7) = 1e-4."""
    plans = RUNS[run]
    rec = _run_device(world, plans)
    errs, ties = {}, 0
    try:
        for s, plan in enumerate(plans):
            ties += _check_stream(rec, s, plan, errs)
    finally:
        _report(run, errs)
    assert ties == 0, ties
    assert all(int(r["valid"].sum()) == (len(plans) if k >= 59 else 0) for k, r in enumerate(rec))


@pytest.fixture(scope="module")
def events(world):
    return _run_device(world, RUNS["events"])


@pytest.mark.gpu
def test_ring_wraps_more_than_once(events):
    """Stream 0 of the events run: 140 pushes, 81 valid frames, while its neighbours are reset / re-targeted."""
    errs = {}
    try:
        assert _check_stream(events, 0, RUNS["events"][0], errs) == 0
    finally:
        _report("events, stream 0", errs)
    assert [int(r["valid"][0]) for r in events] == [0] * 59 + [1] * (LONG - 59)


@pytest.mark.gpu
def test_stream_reset_mid_run(events):
    """Stream 1 is reset before push 65: it reports valid == 0 / idx == -1 and leaves its output rows as they were for 59 pushes, its
    first valid frame afterwards takes the first-frame branch of the post state (the oracle's, from a fresh PostProcess), and the
    other streams are not disturbed (their checks are the two tests next to this one)."""
    errs = {}
    try:
        assert _check_stream(events, 1, RUNS["events"][1], errs) == 0
    finally:
        _report("events, stream 1", errs)
    valid = [int(r["valid"][1]) for r in events]
    assert valid == [0] * 59 + [1] * 6 + [0] * 59 + [1] * (LONG - 124)
    assert np.array_equal(events[124]["ik_rot"][1], events[124]["rot"][1]) and not np.array_equal(events[125]["ik_rot"][1], events[125]["rot"][1])


@pytest.mark.gpu
def test_character_changed_on_a_running_stream(events):
    """Stream 2 goes from character 1 to character 0 before push 90: the ring and the post state go on, the match moves to the other
    character's rows."""
    errs = {}
    try:
        assert _check_stream(events, 2, RUNS["events"][2], errs) == 0
    finally:
        _report("events, stream 2", errs)
    o = _oracle_run_cached(RUNS["events"][2])
    nm0, nm1 = (_oracle_banks()[c][0] for c in (0, 1))
    assert not np.array_equal(nm1[o[89]["idx"]], nm0[o[90]["idx"]])


@pytest.mark.gpu
def test_postprocess_on_mixamo_against_the_reference_loop(world):
    """PostProcessor.run and .step on the 23-bone model against the frame loop the reference executed for this layout
    (postprocess_mixamo.npz): "Ours" and "cm_" streams, 1e-9 / 1e-6; and a third pair of contact bones with the deepest chain the
    kernel takes (bone 9: 8 bones up to the root = MOCHA_MAX_CHAIN) against the oracle."""
    from mocha_sigasia2023_amd import PostProcessor
    model = world["model"]
    z, Y, Ycm, rvel, rang, src_speed, contact = _post_inputs()
    n = len(Y)

    def both(pp, arrs):
        t = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrs]
        run = pp.run(*t)
        st = pp.state()
        steps = [pp.step(st, *[a[i] for a in t]) for i in range(n)]
        return [{k: v.cpu().numpy() for k, v in run.items()}, {k: torch.stack([o[k] for o in steps]).cpu().numpy() for k in KEYS}]
    heads, speed = P.pose_heads(Y)                                           # identical float32 heads for both sides
    for how, out in zip(("run", "step"), both(PostProcessor(model, contact_bones=list(TOES)), [heads, speed, rvel, rang, src_speed, contact])):
        for k in ("pos", "rot", "ik_rot", "bvh_pos"):
            err = np.abs(out[k] - z[k]).max()
            print(f"mixamo {how} vs reference loop, {k}: {err:.3e}")
            assert err < 1e-9, (how, k)
        err = np.abs(out["bvh_euler"] - z["bvh_euler"]).max()
        print(f"mixamo {how} vs reference loop, bvh_euler: {err:.3e}")
        assert err < 1e-6, how
    hc, sc = P.pose_heads(Ycm)
    for how, cm in zip(("run", "step"), both(PostProcessor(model, contact_bones=list(TOES), ik_enabled=False, blend=False),
                                             [hc, sc, rvel, rang, src_speed, contact])):
        for k in ("pos", "rot", "bvh_pos"):
            assert np.abs(cm[k] - z["cm_" + k]).max() < 1e-9, (how, k)
        assert np.array_equal(cm["ik_rot"], cm["rot"])
        assert np.abs(cm["bvh_euler"] - z["cm_bvh_euler"]).max() < 1e-6, how
    deep = (9, 22)                                                           # a hand (chain of 8) and a toe (chain of 6)
    depth = lambda b: 1 if b == 0 else 1 + depth(int(PARENTS[b]))            # noqa: E731
    assert [depth(b) for b in deep] == [8, 6]
    pos, rot, ik = P.run_clip(heads, speed, rvel, rang, src_speed, contact, PARENTS, contact_bones=deep)
    bp, be = P.bvh_channels(pos, ik)
    assert (np.abs(ik - rot).max(axis=(1, 2)) > 1e-6).sum() > 50
    for how, out in zip(("run", "step"), both(PostProcessor(model, contact_bones=list(deep)), [heads, speed, rvel, rang, src_speed, contact])):
        for k, ref in (("pos", pos), ("rot", rot), ("ik_rot", ik), ("bvh_pos", bp)):
            err = np.abs(out[k] - ref).max()
            print(f"mixamo {how}, contact bones {deep}, {k}: {err:.3e}")
            assert err < 1e-9, (how, k)
        assert np.abs(out["bvh_euler"] - be).max() < 1e-6, how
