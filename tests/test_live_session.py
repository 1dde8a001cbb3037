"""Live sessions on the MI355X (run with -m gpu): LiveSession / mocha_live_step - one frame in, one posed frame out, the window ring
and the frame loop's state on the device.

The reference composition is made of calls that already exist and are tested on their own, on the SAME context and with the SAME
number of streams S: Generator.featurize on the S materialised windows, MultiStreamCharacterizer(raw=True).step
(mocha_step_graph_segmented), pose_heads, and PostProcessor.run over the accumulated heads.  Same kernels, same launch shapes: every
comparison is exact (torch.equal)."""
import ctypes as C

import numpy as np
import pytest
import torch

from mocha_sigasia2023_amd import (Generator, LiveSession, MultiCharacterBank, MultiStreamCharacterizer, PostProcessor, build_bank,
                                   pose_heads, synthetic, weights)

pytestmark = pytest.mark.gpu
V, J = 22, 23
N = 44                      # valid frames per clip
F = 60 + N - 1              # frames per clip
KEYS = ("pos", "rot", "ik_rot", "bvh_pos", "bvh_euler")


def dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return torch.device("cuda:0")


def _pose_norm(model):
    rng = np.random.Generator(np.random.PCG64(0))
    X_mean = (0.05 * rng.standard_normal((J, 15))).astype(np.float32); X_std = rng.uniform(0.5, 1.5, (J, 15)).astype(np.float32)
    Y_mean = (0.05 * rng.standard_normal((J, 15))).astype(np.float32); Y_std = rng.uniform(0.2, 0.6, (J, 15)).astype(np.float32)
    model.set_pose_norm(X_mean, X_std, Y_mean, Y_std)


def _contact_bones(model):
    """The two toes of the mixamo layout as bones of the (V+1)-bone skeleton (joints 17 and 21): chains of six bones up to the root bone."""
    from mocha_sigasia2023_amd.skeleton import LAYOUTS
    par = [-1] + [p + 1 for p in LAYOUTS["mixamo"]["parents"]]
    toes = [18, 22]
    for b in toes:
        d, x = 0, b
        while x != -1:
            d += 1; x = par[x]
        assert 5 <= d <= 8, (b, d)
    return toes


def _make_banks(model, seeds):
    banks = []
    for sd_ in seeds:
        clip = synthetic.smooth_bone_clip(sd_, 60 + 40 - 1, J)
        X = model.featurize(*[torch.from_numpy(synthetic.slide_windows(a)) for a in clip])
        b = build_bank(model, X, raw=True)
        banks.append(b)
    return banks


@pytest.fixture(scope="module")
def world():
    d = dev()
    model = Generator(layout="mixamo", device=d).load_state_dict(weights.synthetic_state_dict(1777, 1.0, "mixamo")).eval()
    _pose_norm(model)
    mean_, std_ = synthetic.cnt_norm(7)
    mean, std = torch.from_numpy(mean_).to(d), torch.from_numpy(std_).to(d)

    def to_bank(raw_banks):
        return MultiCharacterBank(model, [(((b["cnt"] - mean) / std).reshape(-1, 90 * 256), b["encoded"]) for b in raw_banks])
    mb = to_bank(_make_banks(model, (101, 102, 103)))
    clips = [[torch.from_numpy(a).to(d) for a in synthetic.smooth_bone_clip(200 + s, F, J, phase=0.3 * s)] for s in range(4)]
    per = []
    for s in range(4):
        _, rvel, rang, hipvel, contact = synthetic.postprocess_inputs(50 + s, F)
        per.append([torch.from_numpy(np.ascontiguousarray(a)).to(d) for a in
                    (rvel, rang, np.linalg.norm(hipvel, axis=-1).mean(-1).astype(np.float32), contact)])
    post = PostProcessor(model, contact_bones=_contact_bones(model))
    mb.characterize(torch.zeros((4, 60, J, 15), device=d), [0] * 4, mean, std, raw=True)   # eager first: everything made on first use exists
    mb.characterize(torch.zeros((1, 60, J, 15), device=d), [0], mean, std, raw=True)
    return dict(model=model, mean=mean, std=std, mb=mb, clips=clips, per=per, post=post, to_bank=to_bank)


def _frame(w, streams, f):
    """push() arguments of frame f (modulo the clip length) for the listed clips."""
    f = f % F
    bones = [torch.stack([w["clips"][s][k][f] for s in streams]) for k in range(4)]
    per = [torch.stack([w["per"][s][k][f] for s in streams]) for k in range(4)]
    return bones + per


def _reference(w, streams, chars, frames):
    """The composition of existing calls for the valid frames `frames` (window i = clip frames i .. i + 59): (dict of (S, n, ...), idx (S, n))."""
    model, S = w["model"], len(streams)
    ms = MultiStreamCharacterizer(w["mb"], w["mean"], w["std"], streams=S, raw=True)
    heads, speeds, idxs = [], [], []
    for i in frames:
        X = model.featurize(*[torch.stack([w["clips"][s][k][i:i + 60] for s in streams]) for k in range(4)])
        Y, idx = ms.step(X, chars)
        h, sp = pose_heads(model, Y)
        heads.append(h); speeds.append(sp); idxs.append(idx.clone())
    heads, speeds = torch.stack(heads, 1), torch.stack(speeds, 1)                 # (S, n, V, 13), (S, n)
    sel = [i + 59 for i in frames]
    per = [torch.stack([w["per"][s][k][sel] for s in streams]) for k in range(4)]
    out = w["post"].run(heads, speeds, *per)
    return out, torch.stack(idxs, 1)


def _run_live(sess, w, streams, chars, frames, record_from=59):
    got = {k: [] for k in KEYS + ("idx", "valid")}
    for f in frames:
        o = sess.push(*_frame(w, streams, f), characters=chars if f == frames[0] else None)
        for k in got:
            got[k].append(o[k].clone())
    return {k: torch.stack(v, 1) for k, v in got.items()}


@pytest.mark.parametrize("S", [1, 4])
def test_live_equals_the_composition_of_existing_calls(world, S):
    w = world
    streams = list(range(S))
    chars = [2, 0, 1, 2][:S]
    sess = LiveSession(w["mb"], w["mean"], w["std"], streams=S, post=w["post"])
    got = _run_live(sess, w, streams, chars, list(range(F)))
    ref, ref_idx = _reference(w, streams, chars, list(range(N)))
    torch.cuda.synchronize()
    assert bool((got["valid"][:, :59] == 0).all()) and bool((got["valid"][:, 59:] == 1).all())
    assert bool((got["idx"][:, :59] == -1).all())
    assert torch.equal(got["idx"][:, 59:], ref_idx)
    assert bool((ref_idx >= 0).all())
    for k in KEYS:
        assert got[k][:, 59:].shape == ref[k].shape, k
        assert torch.equal(got[k][:, 59:], ref[k]), (k, float((got[k][:, 59:] - ref[k]).abs().max()))
    # run_clip: the same frames through the convenience call
    bones = [torch.stack([w["clips"][s][k] for s in streams]) for k in range(4)]
    per = [torch.stack([w["per"][s][k] for s in streams]) for k in range(4)]
    rc = sess.run_clip(*bones, *per, characters=chars)
    for k in KEYS:
        assert torch.equal(rc[k], ref[k]), k
    assert torch.equal(rc["idx"], ref_idx)


def test_ring_window_equals_featurize_over_a_wrap(world):
    """The staging X_raw of the step (read through the session buffer's layout: ring kernel alone would give the same) equals
    Generator.featurize on the materialised window for every push from the 60th on, over more than one wrap of the ring."""
    w = world
    model = w["model"]
    S = 2
    sess = LiveSession(w["mb"], w["mean"], w["std"], streams=S, post=w["post"])
    # two clips of 60 + 61 frames: frames beyond the fixture's clips come from a longer synthetic clip
    long_ = [[torch.from_numpy(a).to(dev()) for a in synthetic.smooth_bone_clip(300 + s, 60 + 61, J)] for s in range(S)]
    per = _frame(w, [0, 1], 0)[4:]
    lib, h = model._ctx.lib, model._ctx.h
    total = int(lib.mocha_live_state_bytes(h, S))
    assert total == sess.live.numel()

    def al(n):
        return (n + 255) // 256 * 256
    off = al(S * 8) + al(S * int(lib.mocha_post_state_bytes(h))) + al(S * 60 * J * 16) + 3 * al(S * 60 * J * 12)   # counters, post state, ring
    nx = S * 60 * J * 15
    for f in range(60 + 61):
        sess.push(*[torch.stack([long_[s][k][f] for s in range(S)]) for k in range(4)], *per, characters=[0, 1] if f == 0 else None)
        if f >= 59:
            X_live = sess.live[off: off + 4 * nx].view(torch.float32).reshape(S, 60, J, 15)
            X_ref = model.featurize(*[torch.stack([long_[s][k][f - 59: f + 1] for s in range(S)]) for k in range(4)])
            assert torch.equal(X_live, X_ref), f
        elif f in (0, 30):
            X_live = sess.live[off: off + 4 * nx].view(torch.float32)
            assert bool(torch.isfinite(X_live).all())                          # a filling ring feeds finite features


def test_warm_up_leaves_outputs_alone(world):
    w = world
    S = 2
    # stream 0 runs from the start of this test's pushes; stream 1 is reset after 30 frames and warms up while stream 0 runs
    sess = LiveSession(w["mb"], w["mean"], w["std"], streams=S, post=w["post"])
    chars = [1, 2]
    for f in range(30):
        o = sess.push(*_frame(w, [0, 1], f), characters=chars)
        assert o["valid"].tolist() == [0, 0] and o["idx"].tolist() == [-1, -1]
    sess.reset([1])
    sentinel = -12345.0
    for k in KEYS:
        sess.out[k].fill_(sentinel)
    ref1, _ = _reference(w, [1, 1], chars, [0])            # stream 1's first frame, at S = 2 (window 0 of clip 1 in both rows)
    for f in range(30, 30 + 60):
        a = _frame(w, [0, 1], f)
        b = _frame(w, [0, 1], f - 30)
        args = [torch.stack([a[k][0], b[k][1]]) for k in range(8)]          # stream 1 starts its clip over
        o = sess.push(*args)
        t = f - 30                                                           # pushes of stream 1 since its reset, minus one
        torch.cuda.synchronize()
        if t < 59:
            assert int(o["valid"][1]) == 0 and int(o["idx"][1]) == -1
            for k in KEYS:
                assert bool((o[k][1] == sentinel).all()), (k, f)
        else:
            assert int(o["valid"][1]) == 1 and int(o["idx"][1]) >= 0
            for k in KEYS:
                assert torch.equal(o[k][1], ref1[k][1, 0]), k
        if f >= 59:
            assert int(o["valid"][0]) == 1
            for k in KEYS:
                assert bool(torch.isfinite(o[k][0]).all()), (k, f)


def test_streams_are_independent(world):
    w = world
    S, k0, pushes = 4, 64, 130
    streams = [0, 1, 2, 3]
    chars = [0, 1, 2, 1]
    A = _run_live(LiveSession(w["mb"], w["mean"], w["std"], streams=S, post=w["post"]), w, streams, chars, list(range(pushes)))
    # run B: stream 2 (running since push 59) is reset after frame k0 and gets another character; it then sees its clip from frame 0 again
    sb = LiveSession(w["mb"], w["mean"], w["std"], streams=S, post=w["post"])
    sf = LiveSession(w["mb"], w["mean"], w["std"], streams=S, post=w["post"])            # a fresh session fed what B sees after the reset
    names = KEYS + ("idx", "valid")
    got_b, got_f = {k: [] for k in names}, {k: [] for k in names}
    for f in range(pushes):
        args = _frame(w, streams, f)
        if f > k0:
            restart = _frame(w, streams, f - k0 - 1)
            args = [torch.stack([a[0], a[1], r[2], a[3]]) for a, r in zip(args, restart)]
        if f == k0 + 1:
            sb.reset([2])
        o = sb.push(*args, characters=chars if f <= k0 else [0, 1, 0, 1])
        for k in names:
            got_b[k].append(o[k].clone())
        if f > k0:
            o = sf.push(*args, characters=[0, 1, 0, 1])
            for k in names:
                got_f[k].append(o[k].clone())
    B = {k: torch.stack(v, 1) for k, v in got_b.items()}
    Fr = {k: torch.stack(v, 1) for k, v in got_f.items()}
    torch.cuda.synchronize()
    assert bool((A["valid"][:, 59:] == 1).all())
    for k in names:
        for s in (0, 1, 3):
            assert torch.equal(B[k][s, 59:], A[k][s, 59:]), (k, s)
        assert torch.equal(B[k][2, 59:k0 + 1], A[k][2, 59:k0 + 1]), k
    # stream 2 after its re-warm-up: valid again from its 60th push after the reset, equal to the fresh session's stream 2
    n_after = pushes - (k0 + 1)
    v2 = B["valid"][2, k0 + 1:]
    assert v2.tolist() == [0] * 59 + [1] * (n_after - 59) and n_after - 59 >= 5
    assert bool((B["idx"][2, k0 + 1:][v2 == 0] == -1).all())
    for k in names:
        assert torch.equal(B[k][2, k0 + 1:][v2 == 1], Fr[k][2][Fr["valid"][2] == 1]), k
    assert not torch.equal(B["pos"][2, k0 + 60:], A["pos"][2, k0 + 60:])


def test_graph_discipline(world):
    w = world
    model, S = w["model"], 4
    streams = [0, 1, 2, 3]
    sess = LiveSession(w["mb"], w["mean"], w["std"], streams=S, post=w["post"])
    sess.push(*_frame(w, streams, 0), characters=[0, 1, 2, 0])
    gen = model._ctx.generation()
    for f in range(1, 70):                                                     # warm-up -> running transition at f = 59
        chars = [f % 3, 1, 2, (f + 1) % 3] if f % 7 == 0 else None              # changed characters
        if f == 20:
            sess.reset([3])
        sess.push(*_frame(w, streams, f), characters=chars)
        assert model._ctx.generation() == gen, f
    # another bank becomes current in between: the next push makes the session's bank current again, which moves the generation, so
    # the step is captured anew - and is still right (compare with a new session)
    other = w["to_bank"](_make_banks(model, (111,)))
    assert model._ctx.generation() != gen
    sess.reset()
    a = _run_live(sess, w, streams, [0, 1, 2, 0], list(range(62)))
    gen2 = model._ctx.generation()
    assert gen2 != gen
    b = _run_live(LiveSession(w["mb"], w["mean"], w["std"], streams=S, post=w["post"]), w, streams, [0, 1, 2, 0], list(range(62)))
    torch.cuda.synchronize()
    assert torch.equal(a["idx"], b["idx"]) and torch.equal(a["valid"], b["valid"])
    assert bool((a["valid"][:, :59] == 0).all()) and bool((a["valid"][:, 59:] == 1).all()) and bool((a["idx"][:, 59:] >= 0).all())
    for k in KEYS:                                                            # (while warming, a session's output rows keep what they held)
        assert torch.equal(a[k][:, 59:], b[k][:, 59:]), k
    assert model._ctx.generation() == gen2
    del other


def test_errors_launch_nothing(world):
    w = world
    d = dev()
    lib = w["model"]._ctx.lib
    S = 2
    sess = LiveSession(w["mb"], w["mean"], w["std"], streams=S, post=w["post"])
    for k in KEYS:
        sess.out[k].fill_(7.0)
    args = _frame(w, [0, 1], 0)
    sess.push(*args, characters=[0, 1])
    torch.cuda.synchronize()
    live0 = sess.live.clone()
    vp = lambda t: C.c_void_p(t.data_ptr())                                     # noqa: E731
    o = sess.out

    def call(h, streams=S, drop=None):
        a = [C.byref(sess.post.cfg), vp(sess.live), streams, vp(sess.rot), vp(sess.pos), vp(sess.vel), vp(sess.ang), vp(sess.rvel), vp(sess.rang),
             vp(sess.speed), vp(sess.contact), vp(sess.ids), vp(sess.mean), vp(sess.std), vp(o["pos"]), vp(o["rot"]), vp(o["ik_rot"]),
             vp(o["bvh_pos"]), vp(o["bvh_euler"]), vp(o["idx"]), vp(o["valid"]), None]
        if drop is not None:
            a[drop] = None
        return lib.mocha_live_step(h, *a)
    h = w["model"]._ctx.h
    gen = w["model"]._ctx.generation()
    assert call(h, streams=0) == -1 and b"streams" in lib.mocha_last_error(h)
    assert call(h, streams=17) == -1
    assert call(h, drop=3) == -1 and b"null" in lib.mocha_last_error(h)        # a NULL frame pointer
    assert call(h, drop=17) == -1                                              # bvh_pos without bvh_euler
    # a context without a pose norm / without a segment table
    from mocha_sigasia2023_amd import ContextBank
    m2 = Generator(layout="mixamo", device=d).load_state_dict(weights.synthetic_state_dict(1777, 1.0, "mixamo")).eval()
    h2 = m2._ctx.h
    assert call(h2) == -3 and b"mocha_set_pose_norm" in lib.mocha_last_error(h2)
    _pose_norm(m2)
    assert call(h2) == -3 and b"mocha_bank_set_segments" in lib.mocha_last_error(h2)
    ContextBank(m2, w["mb"].cnt_nm[:8], w["mb"].encoded[:8])                    # a plain bank: still no segment table
    g2 = m2._ctx.generation()
    assert call(h2) == -3 and b"mocha_bank_set_segments" in lib.mocha_last_error(h2)
    assert m2._ctx.generation() == g2
    torch.cuda.synchronize()
    assert w["model"]._ctx.generation() == gen
    assert torch.equal(sess.live, live0)                                       # nothing was pushed, no state moved
    for k in KEYS:
        assert bool((o[k] == 7.0).all()), k                                    # warming streams: the outputs were never written
    with pytest.raises(ValueError):
        LiveSession(w["mb"], w["mean"], w["std"], streams=17)
    with pytest.raises(ValueError):
        sess.push(*args, characters=[0, 5])                                    # host ids are checked before anything is launched
