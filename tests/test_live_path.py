"""Coherent matching inside the live step on the MI355X (run with -m gpu): LiveSession(coherent=jump) / mocha_live_step_path /
mocha_live_step_raw_path.

The world is the one of tests/test_live_soft.py (mixamo layout, 3 characters of 40 rows, 2 streams, F = 75 frames: 59 warming, 16 valid),
the bank with clip starts.  The reference composition is the staged route on the SAME context with the SAME number of streams:
Generator.featurize on the materialised windows -> MultiCharacterBank.characterize(raw=True, coherent=OnlinePath) -> pose_heads ->
PostProcessor.step, frame by frame.  Same kernels, same launch shapes: every comparison is exact (torch.equal).  The jump penalty is 0.25 x
the median distance of the hard match over the valid frames of the staged route (measured in the fixture: a parameter of the scenario,
not a tolerance), and a second, huge one under which no jump is ever cheaper than a run that can go on.
"No re-capture" is checked through the context's generation (the library does not expose the graph handles)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ingest_ref as R  # noqa: E402
from mocha_sigasia2023_amd import (CoherentMatch, Generator, Ingestor, LiveSession, MultiCharacterBank, OnlinePath, PostProcessor,  # noqa: E402
                                   build_bank, pose_heads, synthetic, weights)
from mocha_sigasia2023_amd.skeleton import LAYOUTS  # noqa: E402

pytestmark = pytest.mark.gpu
V, J = 22, 23
F = 75                      # frames per clip: 59 warming, 16 valid
STARTS = [[20], [13, 27], []]
KEYS = ("pos", "rot", "ik_rot", "bvh_pos", "bvh_euler")
PATH_KEYS = ("idx", "dist", "continued")
SWITCH, FLAG = 66, 70       # stream 0 names character 1 from frame 66 on; stream 1's restart word is set before frame 70
HUGE = 1e6


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
        banks.append((((b["cnt"] - mean) / std).reshape(-1, 90 * 256), b["encoded"]))
    mb = MultiCharacterBank(model, banks, starts=STARTS)
    clips = [[torch.from_numpy(a).to(d) for a in synthetic.smooth_bone_clip(200 + s, F, J, phase=0.3 * s)] for s in range(2)]
    per = []
    for s in range(2):
        _, rvel, rang, hipvel, contact = synthetic.postprocess_inputs(50 + s, F)
        per.append([torch.from_numpy(np.ascontiguousarray(a)).to(d) for a in
                    (rvel, rang, np.linalg.norm(hipvel, axis=-1).mean(-1).astype(np.float32), contact)])
    post = PostProcessor(model, contact_bones=[18, 22])                     # the two toes of the mixamo layout, root bone in front
    zeros = torch.zeros((2, 60, J, 15), device=d)
    mb.characterize(zeros, [0, 0], mean, std, raw=True)                     # eager first: everything made on first use exists
    w = dict(model=model, mean=mean, std=std, mb=mb, clips=clips, per=per, post=post)
    hard = _staged(w, 0.0, lambda f: [2, 0])
    torch.cuda.synchronize()
    w["jump"] = 0.25 * float(torch.stack([o["dist"] for o in hard]).median())
    return w


def _frame(w, f, src=(0, 1)):
    """push() arguments: stream s gets frame f[s] of clip src[s]."""
    bones = [torch.stack([w["clips"][c][k][f[s]] for s, c in enumerate(src)]) for k in range(4)]
    per = [torch.stack([w["per"][c][k][f[s]] for s, c in enumerate(src)]) for k in range(4)]
    return bones + per


def _chars(f):
    return [2, 0] if f < SWITCH else [1, 0]


def _run(sess, w, frames=F, scenario=True, check_generation=True):
    got = {k: [] for k in sess.out}
    gen = None
    for f in range(frames):
        c = [2, 0] if f == 0 else ([1, 0] if scenario and f == SWITCH else None)
        if scenario and f == FLAG:
            sess.restart[1] = 1                                               # written in place, on the device
        o = sess.push(*_frame(w, (f, f)), characters=c)
        if check_generation:
            gen = gen or w["model"]._ctx.generation()
            assert w["model"]._ctx.generation() == gen, f                     # captured once: ids, restart words and frames are device data
        for k in got:
            got[k].append(o[k].clone())
    return {k: torch.stack(v, 1) for k, v in got.items()}


def _staged(w, jump, chars_of_frame, flag=None):
    """The staged route for the valid frames 59 .. F - 1 of both streams: per frame a dict of the step's outputs."""
    model, mb, post = w["model"], w["mb"], w["post"]
    path = OnlinePath(mb, 2, jump)
    state = post.state(2)
    out = []
    for f in range(59, F):
        X = model.featurize(*[torch.stack([w["clips"][s][k][f - 59: f + 1] for s in range(2)]) for k in range(4)])
        if flag is not None and f == flag:
            path.restart[1] = 1
        Y, idx, dist, cont = mb.characterize(X, chars_of_frame(f), w["mean"], w["std"], return_index=True, raw=True, coherent=path)
        h, sp = pose_heads(model, Y)
        o = post.step(state, h, sp, *[torch.stack([w["per"][s][k][f] for s in range(2)]) for k in range(4)])
        o = {k: v.clone() for k, v in o.items()}
        o["idx"], o["dist"], o["continued"] = idx.clone(), dist.clone(), cont.clone()
        out.append(o)
    assert not bool(path.restart.any())                                       # the step cleared the word it consumed
    return out


@pytest.mark.parametrize("which", ["measured", "huge"])
def test_live_path_equals_the_staged_route(world, which):
    w = world
    jump = w["jump"] if which == "measured" else HUGE
    sess = LiveSession(w["mb"], w["mean"], w["std"], streams=2, post=w["post"], coherent=jump)
    sentinel = -12345.0
    for k in KEYS:
        sess.out[k].fill_(sentinel)
    got = _run(sess, w)
    ref = _staged(w, jump, _chars, flag=FLAG)
    torch.cuda.synchronize()
    assert not bool(sess.restart.any())
    # warming: the streams sit out, outputs untouched
    assert got["valid"][:, :59].eq(0).all() and got["idx"][:, :59].eq(-1).all() and got["continued"][:, :59].eq(0).all()
    assert torch.isinf(got["dist"][:, :59]).all()
    for k in KEYS:
        assert bool((got[k][:, :59] == sentinel).all()), k
    for n, f in enumerate(range(59, F)):
        assert got["valid"][:, f].tolist() == [1, 1]
        for k in PATH_KEYS + KEYS:
            assert torch.equal(got[k][:, f], ref[n][k]), (k, f, got[k][:, f].tolist() if k in PATH_KEYS else None, ref[n][k].tolist() if k in PATH_KEYS else None)
    cont = got["continued"].cpu().numpy()
    idx = got["idx"].cpu().numpy()
    assert cont[:, 59].tolist() == [0, 0]                                     # the first valid frame starts the path
    assert cont[0, SWITCH] == 0 and cont[1, FLAG] == 0                        # the character switch and the restart word restart it
    assert cont[:, 60:].sum() > 0                                             # ... and elsewhere it continues
    for s in range(2):                                                        # a continuation is the next row, never onto a clip start
        for f in range(60, F):
            if cont[s, f]:
                c = _chars(f)[s]
                assert idx[s, f] == idx[s, f - 1] + 1 and idx[s, f] not in STARTS[c], (s, f)


def test_coherent_zero_is_the_plain_live_session(world):
    """lambda = 0 is the lowest-index arg-min of the fp32 distances: on an fp32 bank every output of the plain session, every frame."""
    w = world
    a = _run(LiveSession(w["mb"], w["mean"], w["std"], streams=2, post=w["post"], coherent=0), w)
    plain = LiveSession(w["mb"], w["mean"], w["std"], streams=2, post=w["post"])
    got = {k: [] for k in plain.out}
    for f in range(F):
        o = plain.push(*_frame(w, (f, f)), characters=[2, 0] if f == 0 else ([1, 0] if f == SWITCH else None))
        for k in got:
            got[k].append(o[k].clone())
    c = {k: torch.stack(v, 1) for k, v in got.items()}
    torch.cuda.synchronize()
    assert bool((c["valid"][:, 59:] == 1).all()) and set(a) == set(c) | {"dist", "continued"}
    for k in c:
        assert torch.equal(a[k], c[k]), k


def test_reset_of_one_stream_warms_up_and_restarts(world):
    """Stream 1 is reset after frame 64 and warms up again while stream 0 runs on unchanged: its path restarts with its first valid frame."""
    w = world
    model = w["model"]
    jump = w["jump"]
    A = _run(LiveSession(w["mb"], w["mean"], w["std"], streams=2, post=w["post"], coherent=jump), w, scenario=False)
    sess = LiveSession(w["mb"], w["mean"], w["std"], streams=2, post=w["post"], coherent=jump)
    got = {k: [] for k in sess.out}
    gen = None
    for f in range(65 + 62):
        if f == 65:
            sess.reset([1])
        f1 = f if f < 65 else f - 65                                          # stream 1 starts its clip over after the reset
        o = sess.push(*_frame(w, (f % F, f1)), characters=[2, 0] if f == 0 else None)
        gen = gen or model._ctx.generation()
        assert model._ctx.generation() == gen, f
        for k in got:
            got[k].append(o[k].clone())
    B = {k: torch.stack(v, 1) for k, v in got.items()}
    torch.cuda.synchronize()
    for k in B:                                                               # until the reset both streams are run A; stream 0 stays so
        assert torch.equal(B[k][:, 59:65], A[k][:, 59:65]), k
        assert torch.equal(B[k][0, 65:F], A[k][0, 65:F]), k
    assert B["valid"][1, 65:].tolist() == [0] * 59 + [1, 1, 1] and int(B["valid"][1, 64]) == 1
    assert bool((B["idx"][1, 65:65 + 59] == -1).all()) and bool(torch.isinf(B["dist"][1, 65:65 + 59]).all())
    for k in B:                                                               # its 60th push after the reset is its clip's first frame again,
        for n in range(3):                                                    # and the path goes on from there as run A's did
            assert torch.equal(B[k][1, 65 + 59 + n], A[k][1, 59 + n]), (k, n)
    assert int(B["continued"][1, 65 + 59]) == 0


def test_raw_frames_equal_the_staged_raw_route(world):
    """LiveSession(raw=, coherent=) against tests/test_live_raw.py's staged route: Ingestor.step -> push of the emitted frame into a
    session without a front end."""
    w, d = world, dev()
    look, frames, switch = 2, 100, 95
    par = LAYOUTS["mixamo"]["parents"]
    clips = [R.walk_clip(par, frames, seed=300 + s, legs=((18, 19, 20, 21), (14, 15, 16, 17)), shoulders=(6, 10), spine=(1, 2, 3), flip_bone=9)
             for s in range(2)]
    rot = torch.from_numpy(np.stack([c[0] for c in clips])).to(d)
    pos = torch.from_numpy(np.stack([c[1] for c in clips])).to(d)
    post = PostProcessor(w["model"], contact_bones=[22, 18])
    jump = w["jump"]

    def chars(f):
        return [2, 0] if f == 0 else ([1, 0] if f == switch else None)
    sess = LiveSession(w["mb"], w["mean"], w["std"], streams=2, post=post, raw=look, coherent=CoherentMatch(jump))
    got = {k: [] for k in sess.out}
    for f in range(frames):
        o = sess.push_raw(rot[:, f], pos[:, f], characters=chars(f))
        for k in got:
            got[k].append(o[k].clone())
    got = {k: torch.stack(v, 1) for k, v in got.items()}
    ing = Ingestor(w["model"], look, streams=2, post=post)
    st = LiveSession(w["mb"], w["mean"], w["std"], streams=2, post=post, coherent=jump)
    ref = {k: [] for k in st.out}
    for f in range(frames):
        e = ing.step(rot[:, f], pos[:, f])
        if chars(f) is not None:
            st.characters.copy_(torch.tensor(chars(f), dtype=torch.int32))
        if f >= R.FIRST - 1:
            st.push(e["Yrot"], e["Ypos"], e["Yvel"], e["Yang"], e["src_rvel"], e["src_rang"], e["src_speed"], e["contact"])
        for k in ref:
            ref[k].append(st.out[k].clone())
    ref = {k: torch.stack(v, 1) for k, v in ref.items()}
    torch.cuda.synchronize()
    assert set(got) == set(ref) and {"dist", "continued"} <= set(got)
    assert got["valid"][:, :89].eq(0).all() and got["valid"][:, 89:].eq(1).all()
    for k in got:
        assert torch.equal(got[k], ref[k]), k
    assert int(got["continued"][0, switch]) == 0


def test_refusals():
    class FakeBank:
        model = None
    for kw in (dict(soft=(2, 1.0)), dict(inertial=0.1), dict(constrained=True), dict(mix=2)):
        with pytest.raises(ValueError, match="coherent"):
            LiveSession(FakeBank(), None, None, coherent=1.0, **kw)
    with pytest.raises(ValueError, match="median"):
        LiveSession(FakeBank(), None, None, coherent=CoherentMatch(0.25, relative=True))
    with pytest.raises(ValueError):
        LiveSession(FakeBank(), None, None, coherent=-1.0)
