"""The online path on a resident bank while characters come and go (run with -m gpu; the world of tests/resident_world.py).

test_online_path_across_replace_and_retire: OnlinePath.step on a ResidentCharacterBank with A, B, C in slots 0 .. 2, one stream each.
  * step 5: slot 1 is REPLACED by a character of the same row count (30), so it lands on the same extent: only the slot's epoch tells the
    step that the rows are somebody else's - the stream restarts; the new character comes with add(starts=[10]), which is honoured;
  * step 9: slot 2 is retired - the stream sits out (idx -1, dist +inf); step 11: it is added back and the stream restarts;
  * every idx / dist / continued equals tests/path_step_ref.py on the distances mocha_match_dist_matrix gives on a FRESH
    MultiCharacterBank (second model) of the characters alive at that step, and the step's own dist_row has those bits;
  * the generation never moves.
test_live_session_keeps_replaying: LiveSession(coherent=) on the resident bank in lockstep with the staged route on the same bank
(characterize(coherent=OnlinePath)) across an add, a retire and an add-back: the captured step is never captured again, the path outputs
agree on every frame, the retired stream sits out and restarts."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import resident_world as RW  # noqa: E402
from mocha_sigasia2023_amd import LiveSession, MultiCharacterBank, OnlinePath, ResidentCharacterBank, pose_heads  # noqa: E402
from path_step_ref import PathStepRef  # noqa: E402

pytestmark = pytest.mark.gpu
A, B, C, D = range(4)
S = 3
FRAMES, ADD, RETIRE, BACK = 70, 62, 66, 68
KEYS = ("pos", "rot", "ik_rot", "bvh_pos", "bvh_euler")
PATH_KEYS = ("idx", "dist", "continued")


@pytest.fixture(scope="module")
def world():
    return RW.build(FRAMES, S)


def _resident(w):
    rb = ResidentCharacterBank(w["model"], RW.CAPACITY, RW.MAX_CHARACTERS, RW.MAX_ROWS)
    for ch in (A, B, C):
        rb.add(*w["banks"][ch], labels=RW.LABELS[ch])
    return rb


def test_online_path_across_replace_and_retire(world):
    w = world
    model = w["model"]
    rb = _resident(w)
    # B': 30 rows that are not B's - the first 30 of A, reversed
    Bp = (w["banks"][A][0][:30].flip(0).contiguous(), w["banks"][A][1][:30].flip(0).contiguous())
    content = {0: w["banks"][A], 1: w["banks"][B], 2: w["banks"][C]}          # slot -> (cnt_nm, encoded) of the character alive in it
    starts = {0: [], 1: [], 2: []}
    epoch = {0: 0, 1: 0, 2: 0}
    steps = 16
    rng = np.random.default_rng(11)
    unit = float(torch.cdist(content[0][0][:8], content[0][0][8:16]).median())
    jump = 0.25 * unit
    path = OnlinePath(rb, S, jump)
    ref = PathStepRef(S, jump)
    gen = model._ctx.generation()
    extent1 = rb.rows(1)
    seen_restart = False
    for t in range(steps):
        if t == 5:
            assert rb.replace(1, *Bp, starts=[10]) == 1 and rb.rows(1) == extent1      # the same extent: only the epoch moved
            content[1], starts[1], epoch[1] = Bp, [10], epoch[1] + 2          # (retire and add bump it once each)
        if t == 9:
            rb.retire(2)
            content[2] = None
        if t == 11:
            assert rb.add(*w["banks"][C], labels=RW.LABELS[C], slot=2, starts=[3, 12]) == 2
            content[2], starts[2], epoch[2] = w["banks"][C], [3, 12], epoch[2] + 2
        # queries: every stream walks along its character's rows, with noise
        q = torch.zeros((S, 90 * 256), dtype=torch.float32, device=RW.dev())
        for s in range(S):
            src = content[s] if content[s] is not None else content[0]
            n = src[0].shape[0]
            noise = torch.from_numpy((0.05 * unit / 150.0 * rng.standard_normal(90 * 256)).astype(np.float32)).to(RW.dev())
            q[s] = src[0][(4 + t) % n] + noise
        dist, idx, cont, rows = [x.clone() for x in path.step(q, [0, 1, 2], return_distances=True)]
        assert model._ctx.generation() == gen, t
        # a fresh bank of the characters alive now, on the second model
        alive = [s for s in range(S) if content[s] is not None]
        fresh = MultiCharacterBank(w["ref_model"], [content[s] for s in alive], dec_cache=False)
        torch.cuda.synchronize()
        for s in range(S):
            if content[s] is None:
                assert (int(idx[s]), int(cont[s])) == (-1, 0) and bool(torch.isinf(dist[s])), (t, s)
                ref.step_stream(s, None, -1)
                continue
            n = content[s][0].shape[0]
            d = fresh.distances(q[s:s + 1], alive.index(s))[0].cpu().numpy()
            assert np.array_equal(rows[s, :n].cpu().numpy().view(np.uint32), d.view(np.uint32)), (t, s)
            m, dm, c, _ = ref.step_stream(s, d, s, first=rb.rows(s)[0], epoch=epoch[s], starts=starts[s])
            assert (int(idx[s]), int(cont[s])) == (m, c), (t, s, int(idx[s]), m)
            assert float(dist[s]) == float(dm), (t, s)
            if t in (5, 11) and s == (1 if t == 5 else 2):
                assert c == 0                                                  # the replaced / re-added character restarts the path
                seen_restart = True
        if t == 4:
            assert int(cont.sum()) > 0, "the scenario never continues"
    assert seen_restart and model._ctx.generation() == gen


def _staged(w, rb, path, state, f, ids):
    model = w["model"]
    X = RW.windows(w, f)
    Y, idx, dist, cont = rb.characterize(X, ids, w["mean"], w["std"], return_index=True, raw=True, coherent=path)
    h, sp = pose_heads(model, Y)
    o = w["posts"][id(model)].step(state, h, sp, *RW.frame(w, f)[4:])
    o = {k: v.clone() for k, v in o.items()}
    o["idx"], o["dist"], o["continued"] = idx.clone(), dist.clone(), cont.clone()
    return o


def test_live_session_keeps_replaying(world):
    w = world
    model = w["model"]
    rb = _resident(w)
    post = w["posts"][id(model)]
    zeros = torch.zeros((S, 60, RW.J, 15), device=RW.dev())
    rb.characterize(zeros, [0, 1, 2], w["mean"], w["std"], raw=True)           # eager first: everything made on first use exists
    probe = OnlinePath(rb, S, 0.0)
    unit = float(rb.characterize(RW.windows(w, 59), [0, 1, 2], w["mean"], w["std"], return_index=True, raw=True, coherent=probe)[2].median())
    jump = 0.25 * unit
    sess = LiveSession(rb, w["mean"], w["std"], streams=S, post=post, coherent=jump)
    path, state = OnlinePath(rb, S, jump), post.state(S)
    ids, gen = [0, 1, 2], None
    for f in range(FRAMES):
        if f == ADD:
            assert rb.add(*w["banks"][D], labels=RW.LABELS[D], starts=[5]) == 3
            ids = [0, 3, 2]
        if f == RETIRE:
            rb.retire(2)
        if f == BACK:
            assert rb.add(*w["banks"][C], labels=RW.LABELS[C], slot=2) == 2
        a = {k: v.clone() for k, v in sess.push(*RW.frame(w, f), characters=ids).items()}
        gen = gen or model._ctx.generation()
        assert model._ctx.generation() == gen, f                               # add, retire and their start tables re-capture nothing
        if f < 59:
            assert a["valid"].tolist() == [0] * S and a["idx"].tolist() == [-1] * S, f
            continue
        b = _staged(w, rb, path, state, f, ids)
        torch.cuda.synchronize()
        gone = RETIRE <= f < BACK
        assert a["valid"].tolist() == ([1, 1, 0] if gone else [1] * S), f
        for k in PATH_KEYS:
            assert torch.equal(a[k], b[k]), (k, f, a[k].tolist(), b[k].tolist())
        if gone:
            assert int(a["idx"][2]) == -1 and bool(torch.isinf(a["dist"][2])) and int(a["continued"][2]) == 0
        keep = [0, 1] if f >= RETIRE else [0, 1, 2]                            # (the staged route's post state of stream 2 moved while it was gone)
        for k in KEYS:
            assert torch.equal(a[k][keep], b[k][keep]), (k, f)
        if f in (59, ADD):
            assert int(a["continued"][1]) == 0                                 # the first frame, and the switch to D
        if f == BACK:
            assert int(a["continued"][2]) == 0 and int(a["idx"][2]) >= 0       # back: the path restarts
    assert model._ctx.generation() == gen
