"""The captured steps on a resident bank while characters come and go (run with -m gpu): MultiStreamCharacterizer (hard and
constrained=True), LiveSession and LiveOursSession with 3 streams over 70 frames (tests/resident_world.py).  The bank starts with A, B, C in
slots 0 .. 2, one per stream.  At frame 62 D is added (slot 3) and stream 1 switches to it; at frame 66 stream 2's character C is retired;
at frame 68 it is added back into its slot.

  * mocha_generation is the same before the first step and after the last: nothing was captured twice (the CVAE session: from after
    its first push, which allocates the sampler's workspace);
  * every output of every frame equals, bit for bit, the same session on the second model, whose MultiCharacterBank is REBUILT at frames 62,
    66 and 68 to the same content (and re-captures there: those frames are compared too);
  * stream 2 on frames 66 - 67 names an empty slot: idx -1; in the live session valid 0 and its output rows untouched, as a warming stream's.
    The reference has no such state - its stream 2 names a live character on those frames and its post state advances - so the test puts
    the reference's post state of stream 2 back before frame 68 (a device copy of that stream's mocha_post_state_bytes in the session
    buffer, which follows the 256-byte counter section: live_layout, csrc/mocha_api.cpp - the test pins that private layout at frames
    58 and 59, where the post states go from all-zero to written), and skips its rows of stream 2 on 66 - 67;
  * LiveOursSession steps across the add of D without a new capture and equals its rebuilt reference.

Mutations: see tests/test_resident_bank.py.  A retire that leaves the row count fails both test_multi_stream_characterizer cases and
test_live_session (frame 66: valid stays 1); gran_start off by one fails test_multi_stream_characterizer[True]."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import resident_world as RW  # noqa: E402
from mocha_sigasia2023_amd import LiveOursSession, LiveSession, MultiCharacterBank, MultiStreamCharacterizer, ResidentCharacterBank, weights  # noqa: E402

pytestmark = pytest.mark.gpu
A, B, C, D = range(4)
FRAMES, ADD, RETIRE, BACK = 70, 62, 66, 68
S = 3
KEYS = ("pos", "rot", "ik_rot", "bvh_pos", "bvh_euler")
MASKS = [1 << 1, 1 << 0, (1 << 0) | (1 << 3) | (1 << 5)]           # stream 0: action 1 of A; stream 1: action 0 (B has it, D falls back); stream 2: C's 3


@pytest.fixture(scope="module")
def world():
    return RW.build(FRAMES, S)


def _resident(w):
    rb = ResidentCharacterBank(w["model"], RW.CAPACITY, RW.MAX_CHARACTERS, RW.MAX_ROWS)
    for ch in (A, B, C):
        rb.add(*w["banks"][ch], labels=RW.LABELS[ch])
    return rb


def _ref_bank(w, chars):
    return MultiCharacterBank(w["ref_model"], [w["banks"][c] for c in chars], labels=[RW.LABELS[c] for c in chars])


def _events(w, rb, f):
    """The resident bank's event at frame f -> (the streams' slots, the reference's characters, the reference's ids), or None."""
    if f == ADD:
        assert rb.add(*w["banks"][D], labels=RW.LABELS[D]) == 3
        return [0, 3, 2], (A, B, C, D), [0, 3, 2]
    if f == RETIRE:
        rb.retire(2)
        return [0, 3, 2], (A, B, D), [0, 2, 0]                      # (the reference's stream 2 has to name somebody)
    if f == BACK:
        assert rb.add(*w["banks"][C], labels=RW.LABELS[C], slot=2) == 2 and rb.rows(2) == (80, 100)
        return [0, 3, 2], (A, B, C, D), [0, 3, 2]
    return None


def _gone(f):
    return RETIRE <= f < BACK


@pytest.mark.parametrize("constrained", [False, True])
def test_multi_stream_characterizer(world, constrained):
    w = world
    rb = _resident(w)
    got = MultiStreamCharacterizer(rb, w["mean"], w["std"], S, raw=True, constrained=constrained)
    ref = MultiStreamCharacterizer(_ref_bank(w, (A, B, C)), w["mean"], w["std"], S, raw=True, constrained=constrained)
    kw = dict(allow=MASKS) if constrained else {}
    ids, rids, gen = [0, 1, 2], [0, 1, 2], w["model"]._ctx.generation()          # read BEFORE the first step
    for f in range(59, FRAMES):
        ev = _events(w, rb, f)
        if ev:
            ids, chars, rids = ev
            ref.bank = _ref_bank(w, chars)
        X = RW.windows(w, f)
        a = [t.clone() for t in got.step(X, ids, **kw)]
        b = [t.clone() for t in ref.step(X, rids, **kw)]
        torch.cuda.synchronize()
        keep = [0, 1] if _gone(f) else [0, 1, 2]
        for i, (x, y) in enumerate(zip(a, b)):
            assert torch.equal(x[keep], y[keep]), (f, i)
        if _gone(f):
            assert int(a[1][2]) == -1 and (not constrained or int(a[2][2]) == 0), f
        else:
            assert int(a[1][2]) >= 0
        if constrained and not _gone(f):
            assert a[2].tolist() == [1, -1 if f >= ADD else 1, 1], (f, a[2])
    assert w["model"]._ctx.generation() == gen


def test_live_session(world):
    w = world
    model, rmodel = w["model"], w["ref_model"]
    rb = _resident(w)
    got = LiveSession(rb, w["mean"], w["std"], streams=S, post=w["posts"][id(model)])
    ref = LiveSession(_ref_bank(w, (A, B, C)), w["mean"], w["std"], streams=S, post=w["posts"][id(rmodel)])
    pb = int(rmodel._ctx.lib.mocha_post_state_bytes(rmodel._ctx.h))
    at = 256 + 2 * pb                                               # stream 2's post state in the reference's session buffer (S * 8 <= 256)
    assert pb > 0 and at + pb <= ref.live.numel()
    ids, rids, gen, saved, prev = [0, 1, 2], [0, 1, 2], model._ctx.generation(), None, None          # read BEFORE the first push
    for f in range(FRAMES):
        ev = _events(w, rb, f)
        if ev:
            ids, chars, rids = ev
            ref.bank = _ref_bank(w, chars)
        if f == RETIRE:
            saved = ref.live[at: at + pb].clone()
        if f == BACK:
            assert not torch.equal(ref.live[at: at + pb], saved)    # it is the post state: two frames moved it
            ref.live[at: at + pb].copy_(saved)
        a = {k: v.clone() for k, v in got.push(*RW.frame(w, f), characters=ids).items()}
        b = {k: v.clone() for k, v in ref.push(*RW.frame(w, f), characters=rids).items()}
        torch.cuda.synchronize()
        assert model._ctx.generation() == gen, f
        if f in (58, 59):
            # the offsets above are the session buffer's private layout: pin them, so that a change of live_layout fails HERE and not as
            # a silent miscomparison - a warming stream's post state is all zero, and the first valid frame writes every stream's
            post = ref.live[256: 256 + S * pb].reshape(S, pb)
            assert post.any(dim=1).tolist() == [f == 59] * S and not bool(ref.live[:256].reshape(-1)[S * 8:].any()), f
        if f < 59:
            assert a["valid"].tolist() == [0] * S and a["idx"].tolist() == [-1] * S, f
        elif _gone(f):
            assert a["valid"].tolist() == [1, 1, 0] and int(a["idx"][2]) == -1 and b["valid"].tolist() == [1] * S, f
            for k in KEYS:
                assert torch.equal(a[k][:2], b[k][:2]), (k, f)
                assert torch.equal(a[k][2], prev[k][2]), (k, f)          # untouched: what frame 65 left
            assert torch.equal(a["idx"][:2], b["idx"][:2])
        else:
            assert a["valid"].tolist() == [1] * S, f
            for k in a:
                assert torch.equal(a[k], b[k]), (k, f, float((a[k] - b[k]).abs().max()))
        prev = a
    assert model._ctx.generation() == gen and int(a["idx"][2]) >= 0


def test_live_ours_session_steps_across_an_add(world):
    w = world
    model, rmodel = w["model"], w["ref_model"]
    csd = weights.synthetic_cvae_state_dict(99, 1.0)
    rng = np.random.Generator(np.random.PCG64(3))
    stats = ((0.1 * rng.standard_normal((90, 256))).astype(np.float32), rng.uniform(0.5, 1.5, (90, 256)).astype(np.float32),
             (0.1 * rng.standard_normal((90, 256))).astype(np.float32), rng.uniform(0.5, 1.5, (90, 256)).astype(np.float32))
    rb = _resident(w)
    got = LiveOursSession(rb, w["mean"], w["std"], csd, *stats, streams=S, post=w["posts"][id(model)], noise="none")
    ref = LiveOursSession(_ref_bank(w, (A, B, C)), w["mean"], w["std"], csd, *stats, streams=S, post=w["posts"][id(rmodel)], noise="none")
    # the first push of a CVAE session allocates the sampler's workspace for its streams, which moves the generation on any bank: the
    # generation is read after that push - long before the add
    ids, rids, gen = [0, 1, 2], [0, 1, 2], None
    for f in range(ADD + 3):
        if f == ADD:
            ids, chars, rids = _events(w, rb, f)
            ref.bank = _ref_bank(w, chars)
        a = got.push(*RW.frame(w, f), characters=ids)
        gen = gen or model._ctx.generation()
        b = ref.push(*RW.frame(w, f), characters=rids)
        torch.cuda.synchronize()
        assert model._ctx.generation() == gen, f
        for k in a:
            assert torch.equal(a[k], b[k]), (k, f)
        if f >= 59:
            assert a["valid"].tolist() == [1] * S and a["seeded"].tolist() == [int(f == 59), int(f in (59, ADD)), int(f == 59)], (f, a["seeded"])
