"""Inertialized character switches inside the live step on the MI355X (run with -m gpu): LiveSession(inertial=halflife) /
mocha_live_step_inert, hard and soft.

The world is the one of tests/test_live_soft.py (mixamo layout, 3 characters of 40 rows, 2 streams, 70 frames, stream 0 switches at frame
64).  The reference composition is the staged route on the SAME context: Generator.featurize on the materialised windows ->
MultiCharacterBank.characterize(raw=True[, soft]) -> pose_heads -> Inertializer.step(ids=...) -> PostProcessor.step, frame by frame.  Same
kernels, same launch shapes: every comparison is exact (torch.equal)."""
import numpy as np
import pytest
import torch

from mocha_sigasia2023_amd import (Generator, Inertializer, LiveSession, MultiCharacterBank, PostProcessor, build_bank, pose_heads, synthetic,
                                   weights)

pytestmark = pytest.mark.gpu
V, J = 22, 23
F = 70                      # frames per clip: 59 warming, 11 valid
SWITCH = 64
SOFT = (4, 2.0)
HALFLIFE = 0.1
CHARS, AFTER = [2, 0], [1, 0]                                               # stream 0 names character 2, from frame 64 on character 1
KEYS = ("pos", "rot", "ik_rot", "bvh_pos", "bvh_euler")


def dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return torch.device("cuda:0")


def _world(weight_gain=1.0):
    d = dev()
    model = Generator(layout="mixamo", device=d).load_state_dict(weights.synthetic_state_dict(1777, weight_gain, "mixamo")).eval()
    rng = np.random.Generator(np.random.PCG64(0))
    X_mean = (0.05 * rng.standard_normal((J, 15))).astype(np.float32); X_std = rng.uniform(0.5, 1.5, (J, 15)).astype(np.float32)
    Y_mean = (0.05 * rng.standard_normal((J, 15))).astype(np.float32); Y_std = rng.uniform(0.2, 0.6, (J, 15)).astype(np.float32)
    model.set_pose_norm(X_mean, X_std, Y_mean, Y_std)
    mean_, std_ = synthetic.cnt_norm(7)
    mean, std = torch.from_numpy(mean_).to(d), torch.from_numpy(std_).to(d)
    banks = []
    for seed in (101, 102, 103):
        clip = synthetic.smooth_bone_clip(seed, 60 + 40 - 1, J)
        X = model.featurize(*[torch.from_numpy(synthetic.slide_windows(a)) for a in clip])
        b = build_bank(model, X, raw=True)
        banks.append((((b["cnt"] - mean) / std).reshape(-1, 90 * 256), b["encoded"]))
    mb = MultiCharacterBank(model, banks)
    clips = [[torch.from_numpy(a).to(d) for a in synthetic.smooth_bone_clip(200 + s, F, J, phase=0.3 * s)] for s in range(2)]
    per = []
    for s in range(2):
        _, rvel, rang, hipvel, contact = synthetic.postprocess_inputs(50 + s, F)
        per.append([torch.from_numpy(np.ascontiguousarray(a)).to(d) for a in
                    (rvel, rang, np.linalg.norm(hipvel, axis=-1).mean(-1).astype(np.float32), contact)])
    post = PostProcessor(model, contact_bones=[18, 22])                     # the two toes of the mixamo layout, root bone in front
    zeros = torch.zeros((2, 60, J, 15), device=d)
    mb.characterize(zeros, [0, 0], mean, std, raw=True)                     # eager first: everything made on first use exists
    mb.characterize(zeros, [0, 0], mean, std, raw=True, soft=SOFT)
    return dict(model=model, mean=mean, std=std, mb=mb, clips=clips, per=per, post=post)


@pytest.fixture(scope="module")
def world():
    return _world()


def _frame(w, f):
    """push() arguments: both streams get frame f of their clip."""
    return [torch.stack([w["clips"][s][k][f] for s in range(2)]) for k in range(4)] + \
           [torch.stack([w["per"][s][k][f] for s in range(2)]) for k in range(4)]


def _session(w, soft=None, inertial=None):
    return LiveSession(w["mb"], w["mean"], w["std"], streams=2, post=w["post"], soft=soft, inertial=inertial)


def _run(sess, w, switch=False, check_generation=False, chars=CHARS, after=AFTER):
    """All F frames from a fresh session -> every output stacked over frames (S, F, ...)."""
    got = {k: [] for k in sess.out}
    gen = None
    for f in range(F):
        c = chars if f == 0 else (after if switch and f == SWITCH else None)
        o = sess.push(*_frame(w, f), characters=c)
        if check_generation:
            gen = gen or w["model"]._ctx.generation()
            assert w["model"]._ctx.generation() == gen, f                     # captured once: a new id is device data
        for k in got:
            got[k].append(o[k].clone())
    return {k: torch.stack(v, 1) for k, v in got.items()}


def _staged(w, soft, switch):
    """The staged route for the valid frames 59 .. F - 1 of both streams, with the inertializer between the heads and the post frame."""
    model, mb, post = w["model"], w["mb"], w["post"]
    inert = Inertializer(model, halflife=HALFLIFE, dt=post.cfg.dt)
    state, istate = post.state(2), inert.state(2)
    out = []
    for f in range(59, F):
        chars = AFTER if switch and f >= SWITCH else CHARS
        X = model.featurize(*[torch.stack([w["clips"][s][k][f - 59: f + 1] for s in range(2)]) for k in range(4)])
        if soft is None:
            Y, idx = mb.characterize(X, chars, w["mean"], w["std"], return_index=True, raw=True)
        else:
            Y, idx_k, _ = mb.characterize(X, chars, w["mean"], w["std"], return_index=True, raw=True, soft=soft)
            idx = idx_k[:, 0]
        h, sp = pose_heads(model, Y)
        inert.step(istate, h, ids=chars, out=h)
        o = post.step(state, h, sp, *[torch.stack([w["per"][s][k][f] for s in range(2)]) for k in range(4)])
        o = {k: v.clone() for k, v in o.items()}
        o["idx"] = idx.clone()
        out.append(o)
    return out


@pytest.fixture(scope="module")
def runs(world):
    """Every session run the tests below share, computed once: (soft?, inertial?, switch?) -> outputs."""
    w = world
    r = {}
    for soft in (None, SOFT):
        r[soft, False, False] = _run(_session(w, soft), w)
        r[soft, True, False] = _run(_session(w, soft, HALFLIFE), w)
        r[soft, True, True] = _run(_session(w, soft, HALFLIFE), w, switch=True, check_generation=True)
    r[None, False, True] = _run(_session(w), w, switch=True)
    torch.cuda.synchronize()
    return r


@pytest.mark.parametrize("soft", [None, SOFT], ids=["hard", "soft"])
def test_without_a_switch_the_inertial_session_is_the_plain_one(runs, soft):
    a, b = runs[soft, True, False], runs[soft, False, False]
    assert bool((b["valid"][:, 59:] == 1).all()) and bool((b["valid"][:, :59] == 0).all())
    assert set(a) == set(b)
    for k in b:
        assert torch.equal(a[k], b[k]), k


@pytest.mark.parametrize("soft", [None, SOFT], ids=["hard", "soft"])
def test_a_switch_equals_the_staged_route(world, runs, soft):
    got, plain = runs[soft, True, True], runs[soft, True, False]
    ref = _staged(world, soft, switch=True)
    torch.cuda.synchronize()
    for n, f in enumerate(range(59, F)):
        assert got["valid"][:, f].tolist() == [1, 1]
        assert torch.equal(got["idx"][:, f], ref[n]["idx"]), f
        for k in KEYS:
            assert torch.equal(got[k][:, f], ref[n][k]), (k, f, float((got[k][:, f] - ref[n][k]).abs().max()))
    for k in got:                                                             # the stream that does not switch never notices
        assert torch.equal(got[k][1], plain[k][1]), k
        assert torch.equal(got[k][0, :SWITCH], plain[k][0, :SWITCH]), k
    assert not torch.equal(got["pos"][0, SWITCH:], plain["pos"][0, SWITCH:])


POP_GAIN, POP_CHARS, POP_AFTER = 1.5, [0, 0], [2, 0]


@pytest.fixture(scope="module")
def pop_world():
    """The same world with the synthetic weights at gain 1.5.  At gain 1.0 the synthetic network's output barely depends on the character
    it is given: measured on the MI355X, over every pair of the three characters (and over other bank seeds and bank-clip amplitudes), the
    non-root bone positions of the plain session move 1e-4 at the switch frame, below the 1e-3 of the ordinary frames 60-63 (the position
    blend's transient after the first valid frame 59) - no choice of bank or clip seeds makes a pop there.  At gain 1.5 the pose heads
    move 0.036 at a switch against 0.003 from frame to frame (float64 oracle on the CPU)."""
    return _world(POP_GAIN)


def _step(x, f):
    """Largest change of any component of stream 0's NON-ROOT bones from frame f - 1 to frame f: the root is not inertialized - the frame
    loop integrates it from its own output - and its own travel (0.02 per frame) would hide the bones.  For quaternions (last dimension 4)
    per bone the smaller of |q1 - q0| and |q1 + q0|: q and -q are one rotation, and an inertializer whose offset had w < 0 (quat.abs)
    hands back the other sign."""
    a, b = x[0, f, 1:], x[0, f - 1, 1:]
    d = (a - b).abs().amax(-1)
    if x.shape[-1] == 4:
        d = torch.minimum(d, (a + b).abs().amax(-1))
    return float(d.max())


def test_the_switch_frame_does_not_pop(pop_world):
    """Measured on the MI355X (hard route, half-life 0.1 s, weights at gain 1.5, stream 0 from character 0 to character 2):
    pos (non-root bones): plain session 0.0180 at the switch frame, ordinary frames 60-63 at most 0.0020, inertialized 0.0015;
    rot (non-root bones): plain session 0.4175 at the switch frame, ordinary frames 60-63 at most 0.0689, inertialized 0.0089.
    With the root bone included the position figure is the root's own travel, 0.0221 per frame, in both sessions."""
    w = pop_world
    plain = _run(_session(w), w, switch=True, chars=POP_CHARS, after=POP_AFTER)
    inert = _run(_session(w, None, HALFLIFE), w, switch=True, chars=POP_CHARS, after=POP_AFTER)
    torch.cuda.synchronize()
    for k in ("pos", "rot"):
        ordinary = max(_step(plain[k], f) for f in range(60, SWITCH))
        jump, smooth = _step(plain[k], SWITCH), _step(inert[k], SWITCH)
        print(f"{k}: plain session {jump:.4f} at the switch frame, ordinary frames 60-63 at most {ordinary:.4f}; inertialized {smooth:.4f}")
        assert jump > 3 * ordinary, (k, jump, ordinary)                       # there is a pop to remove
        assert smooth < jump, (k, smooth, jump)


def test_reset_after_a_switch_starts_over(world, runs):
    """reset([0]) after the switch, then re-warming: the stream's next first valid frame equals a fresh session's, the offsets are gone."""
    w = world
    fresh = runs[None, True, False]
    sess = _session(w, None, HALFLIFE)
    for f in range(F):
        sess.push(*_frame(w, f), characters=CHARS if f == 0 else (AFTER if f == SWITCH else None))
    sess.reset([0])
    sess.characters.copy_(torch.tensor(CHARS, dtype=torch.int32))
    got = []
    for f in range(60):                                                       # stream 0 starts its clip over; stream 1 just needs frames
        bones = [torch.stack([w["clips"][0][k][f], w["clips"][1][k][f]]) for k in range(4)]
        per = [torch.stack([w["per"][0][k][f], w["per"][1][k][f]]) for k in range(4)]
        o = sess.push(*bones, *per)
        got.append({k: v.clone() for k, v in o.items()})
    torch.cuda.synchronize()
    assert [int(g["valid"][0]) for g in got] == [0] * 59 + [1]
    for k in KEYS + ("idx",):
        assert torch.equal(got[59][k][0], fresh[k][0, 59]), k


def test_profiling_runs_the_step_eagerly_and_names_the_launch(world):
    w = world
    sess = _session(w, None, HALFLIFE)
    sess.push(*_frame(w, 0), characters=CHARS)
    w["model"].profile_start()
    sess.replay()
    prof = w["model"].profile_stop()
    assert prof["kernels"]["mocha_inertialize"]["launches"] == 1
    assert [k for k in prof["sites"] if k.split("|")[0] == "live.inert"] == ["live.inert|mocha_inertialize"], list(prof["sites"])
