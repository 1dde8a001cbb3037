"""Action-constrained live sessions on the MI355X (run with -m gpu): LiveSession(constrained=True) / mocha_live_step_allow /
mocha_live_step_raw_allow.  3 streams, 64 pushes (59 warming, 5 valid), characters of 33, 30 and 20 bank rows (tests/allow_world.py).

  * constrained=True with zero masks is the plain LiveSession, bit for bit, in every output;
  * with masks - stream 0 changes its mask at push 62, stream 2 names a character without any entry of the asked actions and falls back -
    plain, soft=(3, t) and inertial= sessions give the idx and applied of the float64 restatement (tests/allow_ref.py, the data rule
    asserted on the CPU), and poses equal to the staged route on the same context: featurize -> characterize(allow=) of the same windows ->
    pose_heads -> (Inertializer.step) -> PostProcessor.step.  Same kernels, same launch shapes: exact (torch.equal);
  * a raw= session (push_raw, front end inside the graph) emits its first valid frame on push 90, so it runs 94 pushes with the mask
    change at push 92, against the staged route Ingestor.step -> push(allow=) of a constrained session without a front end."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import allow_ref as ar  # noqa: E402
import allow_world as W  # noqa: E402
import ingest_ref as R  # noqa: E402
import scan_ref as sr  # noqa: E402
from mocha_sigasia2023_amd import Inertializer, Ingestor, LiveSession, action_mask, pose_heads  # noqa: E402
from mocha_sigasia2023_amd.skeleton import LAYOUTS  # noqa: E402

pytestmark = pytest.mark.gpu
F, CHANGE = 64, 62
S = 3
CHARS = [0, 1, 2]
HALFLIFE = 0.1
KEYS = ("pos", "rot", "ik_rot", "bvh_pos", "bvh_euler")
KINDS = {"hard": dict(), "soft": dict(soft=W.SOFT), "inertial": dict(inertial=HALFLIFE)}
# stream 0: action 1, from push CHANGE on action 2; stream 1: actions 0 or 1 of a character that has both; stream 2: its character has
# action 3 only - falls back
BEFORE = [action_mask([1]), action_mask([1]), action_mask([0, 1, 2])]
AFTER = [action_mask([2]), action_mask([1]), action_mask([0, 1, 2])]


def masks_at(f):
    return BEFORE if f < CHANGE else AFTER


@pytest.fixture(scope="module")
def world():
    return W.build(F, S)


def _frame(w, f):
    bones = [torch.stack([w["clips"][s][k][f] for s in range(S)]) for k in range(4)]
    per = [torch.stack([w["per"][s][k][f] for s in range(S)]) for k in range(4)]
    return bones + per


def _run(sess, w, masked):
    got = {k: [] for k in sess.out}
    gen = None
    for f in range(F):
        kw = {}
        if masked and f in (0, CHANGE):
            kw["allow"] = masks_at(f)
        o = sess.push(*_frame(w, f), characters=CHARS if f == 0 else None, **kw)
        gen = gen or w["model"]._ctx.generation()
        assert w["model"]._ctx.generation() == gen, f                         # captured once: masks are device data
        for k in got:
            got[k].append(o[k].clone())
    return {k: torch.stack(v, 1) for k, v in got.items()}


@pytest.mark.parametrize("name", list(KINDS))
def test_zero_masks_are_the_plain_session(world, name):
    w = world
    a = _run(LiveSession(w["mb"], w["mean"], w["std"], streams=S, post=w["post"], constrained=True, **KINDS[name]), w, False)
    b = _run(LiveSession(w["mb"], w["mean"], w["std"], streams=S, post=w["post"], **KINDS[name]), w, False)
    torch.cuda.synchronize()
    assert bool((b["valid"][:, 59:] == 1).all()) and set(a) == set(b) | {"applied"}
    for k in b:
        assert torch.equal(a[k], b[k]), k
    assert bool((a["applied"] == 0).all())


def _staged(w, kind):
    """The staged route for the valid frames 59 .. F - 1: per frame a dict of the step's outputs, idx / applied of the restatement checked."""
    model, mb, post = w["model"], w["mb"], w["post"]
    soft = kind.get("soft")
    k = soft[0] if soft else 1
    inert = Inertializer(model, halflife=HALFLIFE, dt=post.cfg.dt) if "inertial" in kind else None
    state = post.state(S)
    istate = inert.state(S) if inert else None
    out = []
    for f in range(59, F):
        X = W.windows(w, f)
        masks = masks_at(f)
        res = mb.characterize(X, CHARS, w["mean"], w["std"], return_index=True, raw=True, soft=soft, allow=masks)
        q = W.queries(w, X)
        seg = np.asarray(CHARS, np.int32)
        gap = ar.gaps_ok(q, w["rows"], seg, w["seg_start"], w["labels"], masks, w["rows"].view(np.uint32), k)
        assert gap is not None and gap >= sr.MIN_GAP, (f, gap)
        ridx, _, _, rap = ar.search(q, w["rows"], seg, w["seg_start"], w["labels"], masks, k)
        h, sp = pose_heads(model, res[0])
        if inert:
            inert.step(istate, h, ids=CHARS, out=h)
        o = post.step(state, h, sp, *[torch.stack([w["per"][s][j][f] for s in range(S)]) for j in range(4)])
        o = {n: v.clone() for n, v in o.items()}
        o["ridx"], o["rapplied"] = ridx, rap
        if soft:
            o["idx_k"], o["weight"] = res[1], res[2]
        else:
            o["idx"] = res[1]
        o["applied"] = res[-1]
        out.append(o)
    return out


@pytest.mark.parametrize("name", list(KINDS))
def test_masked_sessions_equal_the_restatement_and_the_staged_route(world, name):
    w = world
    kind = KINDS[name]
    got = _run(LiveSession(w["mb"], w["mean"], w["std"], streams=S, post=w["post"], constrained=True, **kind), w, True)
    ref = _staged(w, kind)
    torch.cuda.synchronize()
    assert bool((got["valid"][:, :59] == 0).all()) and bool((got["applied"][:, :59] == 0).all()) and bool((got["idx"][:, :59] == -1).all())
    lab0 = W.LABELS[0]
    for n, f in enumerate(range(59, F)):
        r = ref[n]
        assert got["valid"][:, f].tolist() == [1] * S
        assert got["idx"][:, f].tolist() == r["ridx"][:, 0].tolist(), (f, got["idx"][:, f], r["ridx"])
        assert got["applied"][:, f].tolist() == r["rapplied"].tolist() == [1, 1, -1], f
        assert torch.equal(got["applied"][:, f], r["applied"])
        if "soft" in kind:
            assert np.array_equal(got["idx_k"][:, f].cpu().numpy(), r["ridx"]) and torch.equal(got["idx_k"][:, f], r["idx_k"])
            assert torch.equal(got["weight"][:, f], r["weight"]), f
        else:
            assert torch.equal(got["idx"][:, f], r["idx"]), f
        assert lab0[int(got["idx"][0, f])] == (1 if f < CHANGE else 2), f           # stream 0 stays inside its allowed action
        for k in KEYS:
            assert torch.equal(got[k][:, f], r[k]), (k, f, float((got[k][:, f] - r[k]).abs().max()))
    assert not torch.equal(got["idx"][0, CHANGE - 1], got["idx"][0, CHANGE])


def test_raw_session(world):
    """push_raw with masks: the front end inside the graph; against Ingestor.step -> push(allow=) of a constrained session without one."""
    w = world
    L, FR, CH = 2, 94, 92
    par = LAYOUTS["mixamo"]["parents"]
    clips = [R.walk_clip(par, FR + 8, seed=300 + s, legs=((18, 19, 20, 21), (14, 15, 16, 17)), shoulders=(6, 10), spine=(1, 2, 3), flip_bone=9)
             for s in range(S)]
    rot = torch.from_numpy(np.stack([c[0] for c in clips])).to(W.dev())
    pos = torch.from_numpy(np.stack([c[1] for c in clips])).to(W.dev())
    from mocha_sigasia2023_amd import PostProcessor
    post = PostProcessor(w["model"], contact_bones=[22, 18])
    mk = lambda f: BEFORE if f < CH else AFTER                                  # noqa: E731
    sess = LiveSession(w["mb"], w["mean"], w["std"], streams=S, post=post, raw=L, constrained=True)
    ing = Ingestor(w["model"], L, streams=S, post=post)
    staged = LiveSession(w["mb"], w["mean"], w["std"], streams=S, post=post, constrained=True)
    staged.characters.copy_(torch.tensor(CHARS, dtype=torch.int32))
    gen = None
    for f in range(FR):
        if f in (0, CH):
            sess.set_allow(mk(f))                                               # (push_raw keeps its argument list)
        a = sess.push_raw(rot[:, f], pos[:, f], characters=CHARS if f == 0 else None)
        gen = gen or w["model"]._ctx.generation()
        a = {k: v.clone() for k, v in a.items()}
        e = ing.step(rot[:, f], pos[:, f])
        if f >= R.FIRST - 1:
            staged.push(e["Yrot"], e["Ypos"], e["Yvel"], e["Yang"], e["src_rvel"], e["src_rang"], e["src_speed"], e["contact"], allow=mk(f))
        b = staged.out
        torch.cuda.synchronize()
        assert a["valid"].tolist() == ([1] * S if f >= 89 else [0] * S), f
        for k in a:
            assert torch.equal(a[k], b[k]), (k, f)
        if f >= 89:
            assert a["applied"].tolist() == [1, 1, -1] and W.LABELS[0][int(a["idx"][0])] == (1 if f < CH else 2), f
        else:
            assert a["applied"].tolist() == [0] * S and a["idx"].tolist() == [-1] * S
    # (the generation moved only while the two sessions captured their graphs, before the first valid frame)
    assert gen is not None
    # the zero-mask raw session is the plain raw session
    p0 = LiveSession(w["mb"], w["mean"], w["std"], streams=S, post=post, raw=L)
    p1 = LiveSession(w["mb"], w["mean"], w["std"], streams=S, post=post, raw=L, constrained=True)
    for f in range(FR):
        a = p0.push_raw(rot[:, f], pos[:, f], characters=CHARS if f == 0 else None)
        b = p1.push_raw(rot[:, f], pos[:, f], characters=CHARS if f == 0 else None)
    torch.cuda.synchronize()
    for k in a:
        assert torch.equal(a[k], b[k]), k
    assert b["applied"].tolist() == [0] * S and b["valid"].tolist() == [1] * S


def test_refusals(world):
    w = world
    with pytest.raises(RuntimeError, match="constrained"):
        LiveSession(w["mb"], w["mean"], w["std"], streams=S, post=w["post"]).push(*_frame(w, 0), allow=[1, 1, 1])
    sess = LiveSession(w["mb"], w["mean"], w["std"], streams=S, post=w["post"], constrained=True)
    with pytest.raises(ValueError):
        sess.push(*_frame(w, 0), allow=[[64], 0, 0])
    with pytest.raises(ValueError):
        sess.push(*_frame(w, 0), allow=[1, 1])
