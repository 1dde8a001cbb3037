"""Resumable post-processing on the MI355X (run with -m gpu): PostProcessor.step / mocha_postprocess_step, one frame per call with the
loop's state in device memory.

Against the fixture made by executing the reference's own frame loop (tests/golden/postprocess.npz) the bounds are the ones
tests/test_postprocess.py::test_postprocess_clip_parity applies to the clip kernel: 1e-9 on the float64 state, 1e-6 on the Euler
channels.  Everything else compares runs of the same frame code on the same launch shapes and is exact (torch.equal)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from mocha_sigasia2023_amd import synthetic
from oracle import postprocess_oracle as P

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")
KEYS = ("pos", "rot", "ik_rot", "bvh_pos", "bvh_euler")


def _inputs():
    z = np.load(os.path.join(GOLD, "postprocess.npz"))
    N = int(z["seed"][1])
    Y, rvel, rang, hipvel, contact = synthetic.postprocess_inputs(int(z["seed"][0]), N)
    src_speed = np.linalg.norm(hipvel, axis=-1).mean(-1).astype(np.float32)
    return z, Y, rvel, rang, src_speed, contact


def _three_clips():
    clips = []
    for seed in (11, 12, 13):
        Y, rvel, rang, hipvel, contact = synthetic.postprocess_inputs(seed, 70)
        heads, speed = P.pose_heads(Y)
        clips.append((heads, speed, rvel, rang, np.linalg.norm(hipvel, axis=-1).mean(-1).astype(np.float32), contact))
    return [np.stack([c[k] for c in clips]) for k in range(6)]                     # each (3, 70, ...)


@pytest.fixture(scope="module")
def model():
    from mocha_sigasia2023_amd import Generator, synthetic_state_dict
    return Generator(device="cuda:0").load_state_dict(synthetic_state_dict(3, 1.0)).eval()


def _dev(arrs):
    return [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrs]


def _step_all(pp, state, arrs, frames, batched):
    """Steps `frames` (an iterable of frame indices) and returns the stacked outputs, frame axis after the clip axis."""
    outs = {k: [] for k in KEYS}
    for i in frames:
        o = pp.step(state, *[(a[:, i] if batched else a[i]) for a in arrs])
        for k in KEYS:
            outs[k].append(o[k])
    return {k: torch.stack(v, dim=1 if batched else 0) for k, v in outs.items()}


def test_step_against_the_reference_loop(model):
    from mocha_sigasia2023_amd.postprocess import PostProcessor
    z, Y, rvel, rang, src_speed, contact = _inputs()
    heads, speed = P.pose_heads(Y)                                           # identical float32 heads for both sides
    N = len(Y)
    pp = PostProcessor(model)
    out = _step_all(pp, pp.state(), _dev([heads, speed, rvel, rang, src_speed, contact]), range(N), False)
    for k in ("pos", "rot", "ik_rot", "bvh_pos"):
        err = np.abs(out[k].cpu().numpy() - z[k]).max()
        print(f"step vs reference loop, {k}: {err:.3e}")
        assert err < 1e-9, k
    err = np.abs(out["bvh_euler"].cpu().numpy() - z["bvh_euler"]).max()
    print(f"step vs reference loop, bvh_euler: {err:.3e}")
    assert err < 1e-6
    # the "cm_" stream (no blend, no IK) against the same executed reference loop
    Ycm = synthetic.postprocess_inputs(int(z["cm_seed"][0]), int(z["cm_seed"][1]))[0]
    hc, sc = P.pose_heads(Ycm)
    cmp_ = PostProcessor(model, ik_enabled=False, blend=False)
    cm = _step_all(cmp_, cmp_.state(), _dev([hc, sc, rvel, rang, src_speed, contact]), range(N), False)
    for k in ("pos", "rot", "bvh_pos"):
        assert np.abs(cm[k].cpu().numpy() - z["cm_" + k]).max() < 1e-9, k
    assert torch.equal(cm["ik_rot"], cm["rot"])
    assert np.abs(cm["bvh_euler"].cpu().numpy() - z["cm_bvh_euler"]).max() < 1e-6


def test_step_equals_clip_bit_for_bit(model):
    from mocha_sigasia2023_amd.postprocess import PostProcessor
    z, Y, rvel, rang, src_speed, contact = _inputs()
    heads, speed = P.pose_heads(Y)
    arrs = _dev([heads, speed, rvel, rang, src_speed, contact])
    for kw in (dict(), dict(ik_enabled=False, blend=False)):
        pp = PostProcessor(model, **kw)
        ref = pp.run(*arrs)
        out = _step_all(pp, pp.state(), arrs, range(len(Y)), False)
        for k in KEYS:
            assert torch.equal(out[k], ref[k]), (kw, k, float((out[k] - ref[k]).abs().max()))
    # three clips stepped together
    batch = _dev(_three_clips())
    pp = PostProcessor(model)
    ref = pp.run(*batch)
    out = _step_all(pp, pp.state(3), batch, range(70), True)
    for k in KEYS:
        assert out[k].shape == ref[k].shape and torch.equal(out[k], ref[k]), k
    # without the BVH channels the rest is the same
    st = pp.state(3)
    o = pp.step(st, *[a[:, 0] for a in batch], bvh=False)
    assert "bvh_pos" not in o and torch.equal(o["ik_rot"], ref["ik_rot"][:, 0])


def test_state_snapshot_rollback_and_reset(model):
    from mocha_sigasia2023_amd.postprocess import PostProcessor
    batch = _dev(_three_clips())
    pp = PostProcessor(model)
    k0, N = 23, 70
    state = pp.state(3)
    assert not bool(state.any()) and state.shape[1] == int(model._ctx.lib.mocha_post_state_bytes(model._ctx.h))
    _step_all(pp, state, batch, range(k0), True)
    snap = state.clone()
    a = _step_all(pp, state, batch, range(k0, N), True)
    state.copy_(snap)                                                          # rollback is a device copy
    b = _step_all(pp, state, batch, range(k0, N), True)
    for k in KEYS:
        assert torch.equal(a[k], b[k]), k
    # zero the state of clip 1 mid-way: clips 0 and 2 go on undisturbed, clip 1 restarts with the first-frame branch
    state.copy_(snap)
    state[1].zero_()
    c = _step_all(pp, state, batch, range(k0, N), True)
    fresh = pp.state(1)
    d = _step_all(pp, fresh, [x[1:2] for x in batch], range(k0, N), True)
    for k in KEYS:
        assert torch.equal(c[k][0], a[k][0]) and torch.equal(c[k][2], a[k][2]), k
        assert torch.equal(c[k][1], d[k][0]), k
    assert not torch.equal(c["pos"][1], a["pos"][1])                           # it really restarted
    assert torch.equal(c["ik_rot"][1, 0], c["rot"][1, 0])                      # first frame: ik_rot = rot


def test_step_inside_a_captured_graph(model):
    from mocha_sigasia2023_amd.postprocess import PostProcessor
    z, Y, rvel, rang, src_speed, contact = _inputs()
    heads, speed = P.pose_heads(Y)
    arrs = _dev([heads, speed, rvel, rang, src_speed, contact])
    N = len(Y)
    pp = PostProcessor(model)
    eager = _step_all(pp, pp.state(), arrs, range(N), False)
    # fixed buffers: one frame of inputs, the state, the outputs
    bufs = [a[0].clone() for a in arrs]
    state = pp.state()
    out = pp.step(state, *bufs)                                               # warm-up on the side stream's buffers, then start over
    torch.cuda.synchronize()
    state.zero_()
    gen0 = model._ctx.generation()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        pp.step(state, *bufs, out=out)
    state.zero_()                                                              # capture does not execute; be explicit anyway
    got = {k: [] for k in KEYS}
    for i in range(N):
        for b, a in zip(bufs, arrs):
            b.copy_(a[i])
        g.replay()
        for k in KEYS:
            got[k].append(out[k].clone())
    torch.cuda.synchronize()
    for k in KEYS:
        assert torch.equal(torch.stack(got[k]), eager[k]), k
    assert model._ctx.generation() == gen0


def test_step_argument_errors(model):
    from mocha_sigasia2023_amd.postprocess import PostProcessor
    lib, h = model._ctx.lib, model._ctx.h
    pp = PostProcessor(model)
    st = pp.state(2)
    arrs = _dev([a[:2, 0] for a in _three_clips()])
    vp = lambda t: C.c_void_p(t.data_ptr())                                     # noqa: E731
    o = pp.step(st, *arrs)
    torch.cuda.synchronize()
    before = st.clone()
    args = [C.byref(pp.cfg), vp(st)] + [vp(a) for a in arrs] + [2] + [vp(o[k]) for k in KEYS] + [None]
    for drop in (1, 2, 7, 9, 11):                                              # state, heads, contact, pos, ik_rot
        bad = list(args); bad[drop] = None
        assert lib.mocha_postprocess_step(h, *bad) == -1, drop
    bad = list(args); bad[12] = None                                           # bvh_pos without bvh_euler
    assert lib.mocha_postprocess_step(h, *bad) == -1
    assert b"null" in lib.mocha_last_error(h)
    zero = list(args); zero[8] = 0
    assert lib.mocha_postprocess_step(h, *zero) == 0                           # n_clips == 0: a no-op
    torch.cuda.synchronize()
    assert torch.equal(st, before)
    with pytest.raises(RuntimeError):
        PostProcessor(model, contact_bones=[1]).step(pp.state(2), *arrs[:5], arrs[5][:, 1:])     # no 4-ancestor chain
    with pytest.raises(ValueError):
        pp.step(st, arrs[0], arrs[1][:1], *arrs[2:])
