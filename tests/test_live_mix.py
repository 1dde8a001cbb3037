"""Character mixing inside the live step on the MI355X (run with -m gpu): LiveSession(mix=J) / mocha_live_step_mix / mocha_live_step_raw_mix.

The world is the one of tests/test_live_soft.py and tests/test_live_raw.py (mixamo layout, 3 characters of 40 rows, 2 streams).  The
reference composition is the staged route on the SAME context with the SAME number of streams: Generator.featurize on the materialised
ring windows -> characterize(raw=True, mix=) -> pose_heads -> PostProcessor.step, frame by frame.  Same kernels, same launch shapes:
every comparison is exact (torch.equal)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ingest_ref as IR  # noqa: E402
from mocha_sigasia2023_amd import (Generator, Ingestor, LiveSession, MultiCharacterBank, PostProcessor, ResidentCharacterBank,  # noqa: E402
                                   build_bank, pose_heads, synthetic, weights)
from mocha_sigasia2023_amd.skeleton import LAYOUTS  # noqa: E402

pytestmark = pytest.mark.gpu
V, J = 22, 23
F = 70                      # frames per clip: 59 warming, 11 valid
RAW_F, L = 100, 2           # raw pushes (valid from push 90 on), lookahead
KEYS = ("pos", "rot", "ik_rot", "bvh_pos", "bvh_euler")
SENTINEL = -12345.0
# stream 0: 70 % character 2, 30 % character 0; stream 1: a splice - spine, neck and arms of character 1 at full weight, the legs blended
MIX = (np.array([[2, 0], [1, 2]], np.int32),
       np.array([[[0.7] * 6, [0.3] * 6], [[1, 1, 1, 1, 0.25, 0.25], [0, 0, 0, 0, 0.75, 0.75]]], np.float32))


def dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def world():
    d = dev()
    model = Generator(layout="mixamo", device=d).load_state_dict(weights.synthetic_state_dict(1777, 1.0, "mixamo")).eval()
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
        banks.append((((b["cnt"] - mean) / std).reshape(-1, 90 * 256).contiguous(), b["encoded"].contiguous()))
    mb = MultiCharacterBank(model, banks)
    clips = [[torch.from_numpy(a).to(d) for a in synthetic.smooth_bone_clip(200 + s, F, J, phase=0.3 * s)] for s in range(2)]
    per = []
    for s in range(2):
        _, rvel, rang, hipvel, contact = synthetic.postprocess_inputs(50 + s, F)
        per.append([torch.from_numpy(np.ascontiguousarray(a)).to(d) for a in
                    (rvel, rang, np.linalg.norm(hipvel, axis=-1).mean(-1).astype(np.float32), contact)])
    par = LAYOUTS["mixamo"]["parents"]
    raw = [IR.walk_clip(par, RAW_F, seed=300 + s, legs=((18, 19, 20, 21), (14, 15, 16, 17)), shoulders=(6, 10), spine=(1, 2, 3), flip_bone=9)
           for s in range(2)]
    rot = torch.from_numpy(np.stack([c[0] for c in raw])).to(d)
    pos = torch.from_numpy(np.stack([c[1] for c in raw])).to(d)
    post = PostProcessor(model, contact_bones=[18, 22])                     # the two toes of the mixamo layout, root bone in front
    zeros = torch.zeros((2, 60, J, 15), device=d)
    mb.characterize(zeros, [0, 0], mean, std, raw=True)                     # eager first: everything made on first use exists
    mb.characterize(zeros, None, mean, std, raw=True, mix=MIX)
    return dict(model=model, mean=mean, std=std, mb=mb, banks=banks, clips=clips, per=per, post=post, rot=rot, pos=pos)


def _frame(w, f):
    bones = [torch.stack([w["clips"][s][k][f] for s in range(2)]) for k in range(4)]
    per = [torch.stack([w["per"][s][k][f] for s in range(2)]) for k in range(4)]
    return bones + per


def _staged_frame(w, bank, state, f, mix, sit=()):
    """One valid frame of the staged route on `bank` as it is now; the streams in `sit` keep the post state they had."""
    model, post = w["model"], w["post"]
    X = model.featurize(*[torch.stack([w["clips"][s][k][f - 59: f + 1] for s in range(2)]) for k in range(4)])
    Y, idx, wn = bank.characterize(X, None, w["mean"], w["std"], return_index=True, raw=True, mix=mix)
    h, sp = pose_heads(model, Y)
    before = state.clone()
    o = {k: v.clone() for k, v in post.step(state, h, sp, *[torch.stack([w["per"][s][k][f] for s in range(2)]) for k in range(4)]).items()}
    for s in sit:
        state[s].copy_(before[s])
    o["idx"], o["weight"] = idx, wn
    return o


def _session(w, bank=None, **kw):
    sess = LiveSession(bank or w["mb"], w["mean"], w["std"], streams=2, post=w["post"], **kw)
    for k in KEYS:
        sess.out[k].fill_(SENTINEL)
    return sess


def test_live_mix_equals_the_staged_route(world):
    w = world
    sess = _session(w, mix=2)
    assert sess.out["idx"].shape == (2, 2) and sess.out["weight"].shape == (2, 2, 6)
    state = w["post"].state(2)
    gen = None
    for f in range(F):
        o = sess.push(*_frame(w, f), mix=MIX if f == 0 else None)
        gen = gen or w["model"]._ctx.generation()
        assert w["model"]._ctx.generation() == gen, f                         # captured once, nothing replaced
        if f < 59:                                                            # warming: nothing present, outputs untouched
            assert o["valid"].tolist() == [0, 0] and bool((o["idx"] == -1).all()) and bool((o["weight"] == 0).all()), f
            for k in KEYS:
                assert bool((o[k] == SENTINEL).all()), (k, f)
            continue
        o = {k: v.clone() for k, v in o.items()}
        ref = _staged_frame(w, w["mb"], state, f, MIX)
        torch.cuda.synchronize()
        assert o["valid"].tolist() == [1, 1] and bool((o["idx"] >= 0).all())
        assert torch.equal(o["idx"], ref["idx"]) and torch.equal(o["weight"], ref["weight"]), f
        for k in KEYS:
            assert torch.equal(o[k], ref[k]), (k, f, float((o[k] - ref[k]).abs().max()))
    wt = o["weight"].cpu().numpy()
    assert np.array_equal(wt[0], np.array([[np.float32(0.7) / (np.float32(0.7) + np.float32(0.3))] * 6,
                                           [np.float32(0.3) / (np.float32(0.7) + np.float32(0.3))] * 6], np.float32))
    assert wt[1].tolist() == [[1, 1, 1, 1, 0.25, 0.25], [0, 0, 0, 0, 0.75, 0.75]]


def test_one_hot_mix_is_the_plain_session(world):
    w = world
    chars = [1, 2]
    plain = _session(w)
    mixed = _session(w, mix=2)
    ids = np.array([[1, 0], [0, 2]], np.int32)                                # the stream's character first, or second
    wts = np.array([[3.0, 0.0], [0.0, 0.5]], np.float32)
    for f in range(F):
        a = mixed.push(*_frame(w, f), mix=(ids, wts) if f == 0 else None)
        b = plain.push(*_frame(w, f), characters=chars if f == 0 else None)
        torch.cuda.synchronize()
        for k in KEYS + ("valid",):
            assert torch.equal(a[k], b[k]), (k, f)
        own = torch.stack([a["idx"][0, 0], a["idx"][1, 1]])
        assert torch.equal(own, b["idx"]), f
        if f >= 59:
            assert a["valid"].tolist() == [1, 1] and int(a["idx"][0, 1]) == -1 and int(a["idx"][1, 0]) == -1
            assert a["weight"][0].tolist() == [[1.0] * 6, [0.0] * 6] and a["weight"][1].tolist() == [[0.0] * 6, [1.0] * 6]
    assert not bool((a["pos"] == SENTINEL).any())


def test_cross_fade_ramp_replays_without_a_new_capture(world):
    """A linear 30-frame ramp from character a to b (stream 1: the other way), written in place into the session's weights: frames 40 ..
    69, so that the valid frames see the ramp's last third and its end, where the faded-out component is no longer present."""
    w = world
    sess = _session(w, mix=2)
    sess.mix_ids.copy_(torch.tensor([[2, 1], [2, 1]], dtype=torch.int32))
    state = w["post"].state(2)
    gen = None
    for f in range(F):
        t = np.float32(min(max((f - 39) / 30.0, 0.0), 1.0))
        wts = np.array([[1 - t, t], [t, 1 - t]], np.float32)
        sess.mix_weights.copy_(torch.from_numpy(np.repeat(wts[:, :, None], 6, 2)))
        o = sess.push(*_frame(w, f))
        gen = gen or w["model"]._ctx.generation()
        assert w["model"]._ctx.generation() == gen, f
        if f < 59:
            continue
        o = {k: v.clone() for k, v in o.items()}
        ref = _staged_frame(w, w["mb"], state, f, (sess.mix_ids, wts))
        torch.cuda.synchronize()
        assert o["valid"].tolist() == [1, 1]
        assert torch.equal(o["idx"], ref["idx"]) and torch.equal(o["weight"], ref["weight"]), f
        for k in KEYS:
            assert torch.equal(o[k], ref[k]), (k, f)
        if f < F - 1:
            assert bool((o["idx"] >= 0).all()) and bool((o["weight"] > 0).all()), f
    assert o["idx"][0, 0] == -1 and o["idx"][1, 1] == -1 and o["weight"][0].tolist() == [[0.0] * 6, [1.0] * 6]      # the ramp's end


def test_raw_mix_equals_an_ingestor_feeding_push(world):
    w = world
    other = (np.array([[0, 1], [2, 2]], np.int32), np.array([[0.2, 0.8], [0.5, 0.1]], np.float32))
    switch = 95
    raw = _session(w, mix=2, raw=L)
    ing = Ingestor(w["model"], L, streams=2, post=w["post"])
    staged = _session(w, mix=2)
    gen = None
    for f in range(RAW_F):
        mix = MIX if f == 0 else (other if f == switch else None)
        if mix is not None:
            raw.set_mix(mix)
            staged.set_mix(mix)
        a = raw.push_raw(w["rot"][:, f], w["pos"][:, f])
        gen = gen or w["model"]._ctx.generation()
        e = ing.step(w["rot"][:, f], w["pos"][:, f])
        if f >= IR.FIRST - 1:
            staged.push(e["Yrot"], e["Ypos"], e["Yvel"], e["Yang"], e["src_rvel"], e["src_rang"], e["src_speed"], e["contact"])
        torch.cuda.synchronize()
        assert a["valid"].tolist() == ([1, 1] if f >= 89 else [0, 0]), f
        for k in a:
            assert torch.equal(a[k], staged.out[k]), (k, f)
    assert w["model"]._ctx.generation() == gen
    assert not bool((a["pos"] == SENTINEL).any()) and bool((a["idx"] >= 0).all())


def test_resident_bank_components_come_and_go(world):
    """Stream 0 mixes slots 0 and 1, stream 1 slots 1 and 2.  Frame 62: slot 1 is retired - both streams renormalise onto their other
    component.  Frame 64: slot 2 is retired too - stream 1 has nothing present and sits out (valid 0, outputs untouched, post state not
    advanced).  Frame 67: slot 2 is filled again - stream 1 resumes; frame 68: slot 1.  One capture throughout."""
    w = world
    rb = ResidentCharacterBank(w["model"], 160, 4, 48)
    for c in range(3):
        assert rb.add(*w["banks"][c]) == c
    mix = (np.array([[0, 1], [1, 2]], np.int32), np.array([[0.6, 0.4], [0.5, 0.5]], np.float32))
    rb.characterize(torch.zeros((2, 60, J, 15), device=dev()), None, w["mean"], w["std"], raw=True, mix=mix)
    sess = _session(w, bank=rb, mix=2)
    state = w["post"].state(2)
    gen, prev = None, None
    for f in range(F):
        if f == 62:
            rb.retire(1)
        if f == 64:
            rb.retire(2)
        if f == 67:
            assert rb.add(*w["banks"][2], slot=2) == 2
        if f == 68:
            assert rb.add(*w["banks"][1], slot=1) == 1
        o = sess.push(*_frame(w, f), mix=mix if f == 0 else None)
        gen = gen or w["model"]._ctx.generation()
        assert w["model"]._ctx.generation() == gen, f                         # retire and add capture nothing again
        if f < 59:
            continue
        o = {k: v.clone() for k, v in o.items()}
        out = 64 <= f < 67                                                    # stream 1 sits out
        ref = _staged_frame(w, rb, state, f, mix, sit=(1,) if out else ())
        torch.cuda.synchronize()
        assert o["valid"].tolist() == ([1, 0] if out else [1, 1]), f
        assert torch.equal(o["idx"], ref["idx"]) and torch.equal(o["weight"], ref["weight"]), f
        keep = [0] if out else [0, 1]
        for k in KEYS:
            assert torch.equal(o[k][keep], ref[k][keep]), (k, f, float((o[k][keep] - ref[k][keep]).abs().max()))
            if out:
                assert torch.equal(o[k][1], prev[k][1]), (k, f)               # untouched: what frame 63 left
        wt, ix = o["weight"], o["idx"]
        if f < 62 or f >= 68:
            assert bool((ix >= 0).all()) and wt[1].tolist() == [[0.5] * 6] * 2
        elif f < 64:                                                          # slot 1 gone: each stream's other component carries it
            assert ix[0, 1] == -1 and ix[1, 0] == -1 and wt[0].tolist() == [[1.0] * 6, [0.0] * 6] and wt[1].tolist() == [[0.0] * 6, [1.0] * 6]
        elif out:
            assert bool((ix[1] == -1).all()) and bool((wt[1] == 0).all()) and wt[0].tolist() == [[1.0] * 6, [0.0] * 6]
        else:                                                                 # frame 67: slot 2 is back, slot 1 still empty
            assert ix[1, 0] == -1 and ix[1, 1] >= 0 and wt[1].tolist() == [[0.0] * 6, [1.0] * 6]
        prev = o
    w["mb"].activate()
