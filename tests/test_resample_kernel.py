"""mocha_resample_clips / mocha_resample_step on the MI355X (run with -m gpu) against the NumPy restatement tests/resample_ref.py, which
test_resample_ref.py pins to the definition evaluated with the reference's own quat functions (tests/golden/resample.npz).

Per element |got - ref| <= np.spacing(float32(|ref|)) + 4 E: one rounding to fp32 plus a floor of four times the restatement's own measured
deviation (resample_ref.E, which is 0: the floor vanishes) - the criterion of test_clip_ingest_kernel.py.  The inputs are chosen so that no
output lies within 1e-6 of zero without being exactly zero (test_resample_ref.py asserts it of the fixture): one fp32 spacing then covers
every float64 rounding, and exact zeros (single-axis rotations, zero offsets) come out of products with exact zeros on both sides.

Cases: the seven ratios x lengths 1, 2, 3, 31, 45 in one call each, for Euler 'zyx' and 'yzx' on V = 24 (the fixture's clip: a static joint,
one turning 1e-6 rad per frame through the eps branches, one spinning 50 degrees per frame with wrapped angles) and quaternion input with
planted sign flips on V = 22; a clip of CLIP_SCAN_THREADS x CLIP_SCAN_CHUNK + 3 = 4099 frames, past one pass of the unroll scan.  Bit for
bit: 2/1 against every second frame of 1/1; 1/1 on unrolled quaternions against the input; three clips of three ratios in a call against the
three alone, with the middle clip's input NaN; the streaming form (S = 1, 16) against the whole-clip form.

Measured on the MI355X (2026-10-21): 42 tests pass; the largest error / bound that test_parity prints is 0.500 in every Euler case and in
the interpolating quaternion cases - the half spacing of the one rounding to fp32 - and 0.000 for quaternion input at 2/1 and 1/1, where
every output is a source frame."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import clip_ingest_ref as CR  # noqa: E402
import ingest_ref as R  # noqa: E402
import resample_ref as RR  # noqa: E402
from mocha_sigasia2023_amd import Generator, StreamResampler, resample_clips  # noqa: E402
from mocha_sigasia2023_amd.generator import _ptr, _stream  # noqa: E402
from mocha_sigasia2023_amd.skeleton import LAYOUTS  # noqa: E402
from mocha_sigasia2023_amd.synthetic import raw_walk_clip  # noqa: E402

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "resample.npz")
RATIOS = [(2, 1), (1, 2), (3, 2), (5, 3), (5, 6), (2, 5), (1, 1)]
STREAM_RATIOS = [(2, 1), (1, 2), (3, 2), (2, 5)]
LENGTHS = [1, 2, 3, 31, 45]
LONG = 128 * 32 + 3                      # CLIP_SCAN_THREADS * CLIP_SCAN_CHUNK + 3
GUARD, FILL = 64, 7.5
AX = {"x": 0, "y": 1, "z": 2}


def dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return torch.device("cuda:0")


def _call(model, rot, pos, lengths, ratios, order, offsets_out=None):
    """mocha_resample_clips on guarded output buffers.  Returns (rot (F',V,4), pos (F',V,3)) on the host."""
    d, V = model.device, model.V
    n = len(lengths)
    off = np.concatenate([[0], np.cumsum(lengths)])
    if offsets_out is None:
        offsets_out = np.concatenate([[0], np.cumsum([RR.count(m, a, b) for m, (a, b) in zip(lengths, ratios)])])
    off_out = np.asarray(offsets_out)
    Fo = int(off_out[-1])
    r = torch.from_numpy(np.ascontiguousarray(rot, np.float32)).to(d)
    p = torch.from_numpy(np.ascontiguousarray(pos, np.float32)).to(d)
    bufs = [torch.full((Fo * V * w + 2 * GUARD,), FILL, dtype=torch.float32, device=d) for w in (4, 3)]
    outs = [b[GUARD: GUARD + Fo * V * w].view(Fo, V, w) for b, w in zip(bufs, (4, 3))]
    i32 = lambda xs: (C.c_int32 * len(xs))(*[int(x) for x in xs])      # noqa: E731
    eo = (C.c_int * 3)(*[AX[a] for a in (order or "zyx")])
    try:
        model._ctx.call("mocha_resample_clips", 0 if order is None else 1, eo, _ptr(r), _ptr(p), i32(off), i32([a for a, _ in ratios]),
                        i32([b for _, b in ratios]), n, i32(off_out), _ptr(outs[0]), _ptr(outs[1]), _stream())
    finally:
        torch.cuda.synchronize()
    for b in bufs:
        assert bool((torch.cat([b[:GUARD], b[-GUARD:]]) == FILL).all()), "guard words of an output were written"
    return outs[0].cpu().numpy(), outs[1].cpu().numpy(), bufs


def _within(got, ref, what):
    ref = np.asarray(ref, np.float64)
    err = np.abs(got.astype(np.float64) - ref)
    bound = np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64) + 4.0 * RR.E
    assert got.shape == ref.shape and np.all(err <= bound), (what, float(err.max()), float((err / bound).max()),
                                                              np.argwhere(err > bound)[:4].tolist())
    return float((err / bound).max())


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(GOLD))


@pytest.fixture(scope="module")
def model24():
    return Generator(layout="mocha", device=dev())


@pytest.fixture(scope="module")
def model22():
    return Generator(layout="mixamo", device=dev())


@pytest.fixture(scope="module")
def quat22():
    """A walk of 45 frames on the 22-joint layout as fp32 quaternions in metres, a random third of every joint's frames negated."""
    par = LAYOUTS["mixamo"]["parents"]
    rot, pos = R.walk_clip(par, 45, seed=77, legs=((18, 19, 20, 21), (14, 15, 16, 17)), shoulders=(6, 10), spine=(1, 2, 3), flip_bone=9)
    q = CR.euler_to_quat(rot, [2, 1, 0]).transpose(1, 2, 0)
    flip = np.random.Generator(np.random.PCG64(77)).random((45, len(par))) < 1.0 / 3.0
    return np.where(flip[..., None], -q, q).astype(np.float32), (pos.astype(np.float64) * 0.01).astype(np.float32)


def _source(fmt, gold, quat22):
    return (gold["rot"], gold["pos"], fmt) if fmt != "quat" else (quat22[0], quat22[1], None)


@pytest.fixture(scope="module")
def parity(gold, quat22, model24, model22):
    """Every (format, ratio): the five prefix lengths as five clips of one call, and the restatement's outputs.  Computed once, shared."""
    out = {}
    for fmt in ("zyx", "yzx", "quat"):
        rot, pos, order = _source(fmt, gold, quat22)
        model = model22 if fmt == "quat" else model24
        for num, den in RATIOS:
            got_q, got_p, _ = _call(model, np.concatenate([rot[:n] for n in LENGTHS]), np.concatenate([pos[:n] for n in LENGTHS]), LENGTHS,
                                    [(num, den)] * len(LENGTHS), order)
            ref = [RR.resample_clip(rot[:n], pos[:n], order, num, den) for n in LENGTHS]
            out[fmt, num, den] = (got_q, got_p, ref)
    return out


@pytest.mark.parametrize("num,den", RATIOS)
@pytest.mark.parametrize("fmt", ["zyx", "yzx", "quat"])
def test_parity(parity, fmt, num, den):
    got_q, got_p, ref = parity[fmt, num, den]
    at, worst = 0, 0.0
    for n, (rq, rp) in zip(LENGTHS, ref):
        m = RR.count(n, num, den)
        assert len(rq) == m
        worst = max(worst, _within(got_q[at: at + m], rq, (fmt, num, den, n, "rot")), _within(got_p[at: at + m], rp, (fmt, num, den, n, "pos")))
        at += m
    assert at == len(got_q) == len(got_p)
    print(f"{fmt} {num}/{den}: largest error / bound {worst:.3f}")


@pytest.mark.parametrize("fmt,V", [("zyx", 24), ("quat", 22)])
def test_gold_is_the_zyx_case(parity, gold, fmt, V):
    """V = 24 and V = 22 both ran; the zyx case is the reference composition's own floats within the same bound."""
    got_q, got_p, _ = parity[fmt, 3, 2]
    assert got_q.shape[1:] == (V, 4) and got_p.shape[1:] == (V, 3)
    if fmt == "zyx":
        m = RR.count(45, 3, 2)
        _within(got_q[-m:], gold["q_zyx_3_2"], "gold rot")
        _within(got_p[-m:], gold["p_3_2"], "gold pos")


@pytest.mark.parametrize("num,den", [(3, 2), (2, 5), (2, 1)])
def test_long_clip_past_one_scan_pass(model24, num, den):
    rot, pos = raw_walk_clip(LAYOUTS["mocha"]["parents"], LONG)
    raw = CR.euler_to_quat(rot.astype(np.float64), [2, 1, 0])
    assert (np.sum(raw[:, 1:4096] * raw[:, :4095], axis=0) < 0).any(), "no sign flip in the first pass: the second needs no carry"
    got_q, got_p, _ = _call(model24, rot, pos, [LONG], [(num, den)], "zyx")
    rq, rp = RR.resample_clip(rot, pos, "zyx", num, den)
    assert len(got_q) == RR.count(LONG, num, den)
    _within(got_q, rq, ("long rot", num, den))
    _within(got_p, rp, ("long pos", num, den))
    assert np.all(np.sum(got_q[1:].astype(np.float64) * got_q[:-1], axis=-1) > 0), "a sign flip survived the unroll scan"


def test_two_to_one_is_every_second_frame(parity):
    for fmt in ("zyx", "yzx", "quat"):
        two, one = parity[fmt, 2, 1], parity[fmt, 1, 1]
        a2 = a1 = 0
        for n in LENGTHS:
            m2, m1 = RR.count(n, 2, 1), n
            assert np.array_equal(two[0][a2: a2 + m2].view(np.uint32), one[0][a1: a1 + m1: 2].view(np.uint32)), (fmt, n)
            assert np.array_equal(two[1][a2: a2 + m2].view(np.uint32), one[1][a1: a1 + m1: 2].view(np.uint32)), (fmt, n)
            a2, a1 = a2 + m2, a1 + m1


def test_one_to_one_returns_unrolled_quaternions_bit_for_bit(model22, quat22):
    q = RR.quats(quat22[0], None).transpose(1, 2, 0).astype(np.float32)          # unrolled, fp32: consecutive dots stay positive
    assert np.all(np.sum(q[1:].astype(np.float64) * q[:-1], axis=-1) > 0)
    got_q, got_p, _ = _call(model22, q, quat22[1], [45], [(1, 1)], None)
    assert np.array_equal(got_q.view(np.uint32), q.view(np.uint32)) and np.array_equal(got_p.view(np.uint32), quat22[1].view(np.uint32))


def test_three_ratios_in_one_call_and_isolation(model24, gold):
    lens, ratios = [45, 31, 45], [(2, 1), (3, 2), (1, 2)]
    k_last = RR.count(45, 2, 1) - 1
    assert RR.at(k_last, 2, 1) == (44, 0.0), "the first clip's last output must sit on its last frame"
    rot = np.concatenate([gold["rot"][:45], gold["rot"][:31] + np.float32(2.0), gold["rot"][:45] - np.float32(3.0)])
    pos = np.concatenate([gold["pos"][:45], gold["pos"][:31], gold["pos"][:45]])
    got_q, got_p, _ = _call(model24, rot, pos, lens, ratios, "zyx")
    new = [RR.count(n, a, b) for n, (a, b) in zip(lens, ratios)]
    io, oo = np.concatenate([[0], np.cumsum(lens)]), np.concatenate([[0], np.cumsum(new)])
    for c in range(3):
        sq, sp, _ = _call(model24, rot[io[c]: io[c + 1]], pos[io[c]: io[c + 1]], [lens[c]], [ratios[c]], "zyx")
        assert np.array_equal(got_q[oo[c]: oo[c + 1]].view(np.uint32), sq.view(np.uint32)), ("a clip inside the call differs from the clip alone", c)
        assert np.array_equal(got_p[oo[c]: oo[c + 1]].view(np.uint32), sp.view(np.uint32)), c
        _within(sq, RR.resample_clip(rot[io[c]: io[c + 1]], pos[io[c]: io[c + 1]], "zyx", *ratios[c])[0], ("three clips", c))
    rot2, pos2 = rot.copy(), pos.copy()
    rot2[45:76], pos2[45:76] = np.nan, np.nan
    nan_q, nan_p, _ = _call(model24, rot2, pos2, lens, ratios, "zyx")
    for c in (0, 2):
        assert np.array_equal(nan_q[oo[c]: oo[c + 1]].view(np.uint32), got_q[oo[c]: oo[c + 1]].view(np.uint32)), ("NaN leaked into clip", c)
        assert np.array_equal(nan_p[oo[c]: oo[c + 1]].view(np.uint32), got_p[oo[c]: oo[c + 1]].view(np.uint32)), ("NaN leaked into clip", c)
    assert np.isnan(nan_q[oo[1]: oo[2]]).all() and np.isnan(nan_p[oo[1]: oo[2]]).all()


def test_continuity_on_the_spinning_joint(parity, gold):
    spin = int(gold["spin"])
    for fmt in ("zyx", "yzx"):
        for num, den in RATIOS:
            q = parity[fmt, num, den][0][-RR.count(45, num, den):, spin].astype(np.float64)
            assert len(q) == 1 or np.all(np.sum(q[1:] * q[:-1], axis=-1) > 0), (fmt, num, den)


def test_python_entry_matches_the_guarded_call(model24, gold, parity):
    q, p, new = resample_clips(model24, np.concatenate([gold["rot"][:n] for n in LENGTHS]), np.concatenate([gold["pos"][:n] for n in LENGTHS]),
                               LENGTHS, 90, 60.0, order="yzx")
    assert new == [RR.count(n, 3, 2) for n in LENGTHS] and q.dtype == torch.float32 and q.is_cuda
    assert np.array_equal(q.cpu().numpy(), parity["yzx", 3, 2][0]) and np.array_equal(p.cpu().numpy(), parity["yzx", 3, 2][1])
    q2, _, new2 = resample_clips(model24, np.concatenate([gold["rot"], gold["rot"]]), np.concatenate([gold["pos"], gold["pos"]]), [45, 45],
                                 [120, 30])
    assert new2 == [23, 89] and np.array_equal(q2[:23].cpu().numpy(), parity["zyx", 2, 1][0][-23:])
    assert np.array_equal(q2[23:].cpu().numpy(), parity["zyx", 1, 2][0][-89:])


# ------------------------------------------------------------------------------------------------------------------ streams
def _stream_inputs(gold, S):
    """S streams of 45 frames: the fixture's clip, every stream's angles shifted by its own amount."""
    shift = (np.arange(S, dtype=np.float32) * np.float32(1.5))[None, :, None, None]
    return gold["rot"][:, None] + shift, np.repeat(gold["pos"][:, None], S, axis=1)          # (45,S,V,3)


def _run_stream(rs, rot, pos, restart_at=None, restart=None):
    qs, ps, counts = [], [], []
    for j in range(len(rot)):
        if restart_at == j:
            rs.restart(restart)
        n = rs.push(rot[j], pos[j])
        counts.append(n)
        qs.append(rs.out["rot"][:, :n].clone())
        ps.append(rs.out["pos"][:, :n].clone())
    torch.cuda.synchronize()
    return torch.cat(qs, dim=1).cpu().numpy(), torch.cat(ps, dim=1).cpu().numpy(), counts


@pytest.mark.parametrize("num,den", STREAM_RATIOS)
@pytest.mark.parametrize("S", [1, 16])
def test_streams_are_the_whole_clips_bit_for_bit(model24, gold, S, num, den):
    rot, pos = _stream_inputs(gold, S)
    rs = StreamResampler(model24, num, den, order="zyx", streams=S)
    assert (rs.num, rs.den) == (num, den) and rs.out["rot"].shape == (S, 4, 24, 4) and rs.out["pos"].shape == (S, 4, 24, 3)
    q, p, counts = _run_stream(rs, rot, pos)
    assert counts == [RR.push_count(j, num, den)[0] for j in range(45)] and sum(counts) == RR.count(45, num, den)
    wq, wp, _ = _call(model24, rot.transpose(1, 0, 2, 3).reshape(S * 45, 24, 3), pos.transpose(1, 0, 2, 3).reshape(S * 45, 24, 3), [45] * S,
                      [(num, den)] * S, "zyx")
    m = RR.count(45, num, den)
    assert np.array_equal(q.view(np.uint32), wq.reshape(S, m, 24, 4).view(np.uint32)), "streaming rotations differ from the whole clip's"
    assert np.array_equal(p.view(np.uint32), wp.reshape(S, m, 24, 3).view(np.uint32)), "streaming positions differ from the whole clip's"
    rs.reset()                                                                    # and again from push 0
    q2, _, counts2 = _run_stream(rs, rot[:7], pos[:7])
    assert counts2 == counts[:7] and np.array_equal(q2.view(np.uint32), q[:, :sum(counts[:7])].view(np.uint32))


def test_stream_of_quaternions(model22, quat22):
    rs = StreamResampler(model22, 90, 60, order=None, streams=1)
    q, p, counts = _run_stream(rs, quat22[0][:, None], quat22[1][:, None])
    wq, wp, _ = _call(model22, quat22[0], quat22[1], [45], [(3, 2)], None)
    assert sum(counts) == len(wq) and np.array_equal(q[0].view(np.uint32), wq.view(np.uint32)) and np.array_equal(p[0].view(np.uint32), wp.view(np.uint32))


def test_restart_in_mid_clip(model24, gold):
    rot, pos = _stream_inputs(gold, 3)
    plain = _run_stream(StreamResampler(model24, 30, 60, streams=3), rot[:14], pos[:14])
    again = _run_stream(StreamResampler(model24, 30, 60, streams=3), rot[:14], pos[:14], restart_at=10, restart=[1])
    assert plain[2] == again[2] == [1] + [2] * 13
    for s in (0, 2):
        assert np.array_equal(plain[0][s].view(np.uint32), again[0][s].view(np.uint32)), ("restart([1]) changed stream", s)
        assert np.array_equal(plain[1][s].view(np.uint32), again[1][s].view(np.uint32)), ("restart([1]) changed stream", s)
    fresh_q, fresh_p, _ = _call(model24, rot[10, 1][None], pos[10, 1][None], [1], [(1, 2)], "zyx")      # frame 10 alone: the new frame itself
    first = 1 + 2 * 9                                                             # outputs of the pushes 0 .. 9
    for e in (first, first + 1):                                                  # both outputs of push 10
        assert np.array_equal(again[0][1, e].view(np.uint32), fresh_q[0].view(np.uint32)), e
        assert np.array_equal(again[1][1, e].view(np.uint32), fresh_p[0].view(np.uint32)), e
    assert not np.array_equal(plain[0][1, first], again[0][1, first])             # without the restart that output lies between two frames
    # before the restart nothing differs; after it the stream goes on from the new frame, up to the sign it had lost track of
    assert np.array_equal(plain[0][1, :first], again[0][1, :first])
    same = np.sum(plain[0][1, first + 2:].astype(np.float64) * again[0][1, first + 2:], axis=-1)
    assert np.allclose(np.abs(same), 1.0, atol=1e-6)


# ------------------------------------------------------------------------------------------------------------------ refusals
def test_refusals(model24, gold):
    with pytest.raises(ValueError):
        StreamResampler(model24, 10, 60)                                          # den / num = 6 > 4
    with pytest.raises(ValueError):
        StreamResampler(model24, 120, 60, streams=17)
    StreamResampler(model24, 15, 60)                                              # exactly 4 outputs per frame is allowed
    d = model24.device
    state = torch.zeros((int(model24._ctx.lib.mocha_resample_state_bytes(model24._ctx.h, 16)),), dtype=torch.uint8, device=d)
    assert state.numel() > 0 and int(model24._ctx.lib.mocha_resample_state_bytes(model24._ctx.h, 17)) < 0
    assert int(model24._ctx.lib.mocha_resample_state_bytes(model24._ctx.h, 0)) < 0
    rot, pos = torch.zeros((16, 24, 3), device=d), torch.zeros((16, 24, 3), device=d)
    oq, op = torch.full((16, 4, 24, 4), FILL, device=d), torch.full((16, 4, 24, 3), FILL, device=d)
    eo, n = (C.c_int * 3)(2, 1, 0), C.c_int32(-7)

    def step(fmt=1, order=eo, st=state, S=16, r=rot, p=pos, num=2, den=1, push=0, a=oq, b=op, cnt=n):
        model24._ctx.call("mocha_resample_step", fmt, order, None if st is None else _ptr(st), S, None if r is None else _ptr(r),
                          None if p is None else _ptr(p), num, den, push, None if a is None else _ptr(a), None if b is None else _ptr(b),
                          None if cnt is None else C.byref(cnt), _stream())
    for kw in (dict(den=5, num=1), dict(den=9, num=2), dict(num=0), dict(den=0), dict(num=4097), dict(den=4097, num=4096), dict(S=0), dict(S=17),
               dict(st=None), dict(r=None), dict(p=None), dict(a=None), dict(b=None), dict(cnt=None), dict(order=None), dict(fmt=2),
               dict(order=(C.c_int * 3)(1, 1, 0)), dict(push=-1)):
        with pytest.raises(RuntimeError, match="status"):
            step(**kw)
    for st, S in ((_ptr(state), 0), (_ptr(state), 17), (None, 16)):
        with pytest.raises(RuntimeError, match="status"):
            model24._ctx.call("mocha_resample_reset", st, S, None, 0, _stream())
    with pytest.raises(RuntimeError, match="status"):
        model24._ctx.call("mocha_resample_reset", _ptr(state), 16, (C.c_int32 * 1)(16), 1, _stream())
    torch.cuda.synchronize()
    assert n.value == -7 and bool((oq == FILL).all()) and bool((op == FILL).all()), "a refused step wrote something"
    assert not bool(state.any()), "a refused step touched the state"
    step(fmt=0, order=None, r=torch.zeros((16, 24, 4), device=d), den=4, num=1)    # quaternions need no order; 4 outputs per frame
    assert n.value == 1                                                           # push 0 emits output 0 alone
    # whole clips: offsets_out must be the prefix sums of mocha_resample_frames; ratios in range; pointers non-NULL
    r45, p45 = gold["rot"], gold["pos"]
    for bad in ([0, 22], [0, 24], [1, 24], [0, 0]):
        with pytest.raises(RuntimeError, match="status"):
            _call(model24, r45, p45, [45], [(2, 1)], "zyx", offsets_out=bad)
    for ratio in ((0, 1), (1, 0), (4097, 1), (1, 4097)):
        with pytest.raises(RuntimeError, match="status"):
            _call(model24, r45, p45, [45], [ratio], "zyx", offsets_out=[0, 23])
    with pytest.raises(RuntimeError, match="status"):
        model24._ctx.call("mocha_resample_clips", 1, eo, None, None, (C.c_int32 * 2)(0, 45), (C.c_int32 * 1)(2), (C.c_int32 * 1)(1), 1,
                          (C.c_int32 * 2)(0, 23), None, None, _stream())
    with pytest.raises(ValueError):
        resample_clips(model24, r45, p45, [44], 120)                             # rot / pos do not hold the frames of lengths
