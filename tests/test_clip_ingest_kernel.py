"""mocha_ingest_clips / mocha_clip_windows on the MI355X (run with -m gpu): whole clips against the reference's own process_data
(tests/golden/clip_ingest.npz: V = 24, Euler degrees + centimetres, lengths 31, 32, 45, 62, 100, plain and mirrored, and its divide_clip
windows) and against the NumPy restatement tests/clip_ingest_ref.py (V = 22, quaternion input in metres with planted sign flips).

Per element |got - ref| <= np.spacing(float32(|ref|)) + 4 E: one rounding to fp32 plus a floor of four times the restatement's own measured
deviation from the reference (clip_ingest_ref.E, E_MIRROR for mirrored clips) - the bound of test_ingest_kernel.py.  Contacts are exact,
every output sits between guard words, a clip inside a call of several is bit-identical to the same clip alone.

Unroll scan: a lane takes CLIP_SCAN_CHUNK = 32 frames, a wave 64 x 32 = 2048, a workgroup of two waves 4096 per pass.  SCAN_LENGTHS = 31, 32,
33 (lane chunk), 2047, 2048, 2049 (wave), 4095, 4096, 4097 (workgroup pass) and 9000 (three passes), all in one call; then 45 + 40 frames in
one call, whose boundary lies inside the second lane's chunk of frames counted from the call's first.

Against the streaming route (Ingestor(raw=18), frames 12 .. 81 of the 100-frame clip): within the same bound, contacts exact.  Measured on
the MI355X (2026-10-20): all 70 x 25 x 13 floats came out BIT-IDENTICAL (the test prints the count of differing floats: 0 for pos, vel, rot
and ang); the assertion stays the bound, since nothing obliges two kernels to contract their products alike.

Mutations, each made on a scratch copy of csrc/ingest_clip.hip (arithmetic only, every index in bounds), rebuilt, and this file run on the
MI355X against the mutated library (2026-10-20; 22 tests, all pass on the unmutated code):
  quaternions   x and y axes of from_euler exchanged                        15 fail: every parity case, three clips, streaming, windows
  unroll        the carry across workgroup passes dropped                    1 fails: test_unroll_scan_chunk_edges (4097 and 9000 frames)
  unroll        the ballot's lower-lane mask made inclusive                 10 fail: the scan tests, parity at 62 and 100 frames, streaming
  mirror        the second unroll after the mirror dropped                   3 fail: mirrored parity at 62 and 100 frames, three clips
  mirror        mirror_pos without its sign                                  6 fail: every mirrored parity case, three clips
  series        the across-direction's z with the wrong sign                17 fail
  root          an edge row off by one (last window's row j - (n - W) - 1)  16 fail: every parity case, three clips, scan, streaming, windows
  velocities    v[0] = v[1] + (v[3] - v[2])                                  16 fail
  contacts      the vote window shifted by one (t-2 .. t+3)                  17 fail
  windows       left padding one short ((window - m) / 2)                     3 fail: test_windows[100-1], [31-1], test_windows_two_clips
                                                                               ([100-30] pads 10 / 10 and cannot see it)"""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import clip_ingest_ref as CR  # noqa: E402
import ingest_ref as R  # noqa: E402
from mocha_sigasia2023_amd import Generator, IngestConfig, Ingestor, PostProcessor, clip_windows, ingest_clips  # noqa: E402
from mocha_sigasia2023_amd.ingest import clip_window_counts, default_mirror_map  # noqa: E402
from mocha_sigasia2023_amd.generator import _ptr, _stream  # noqa: E402
from mocha_sigasia2023_amd.skeleton import LAYOUTS  # noqa: E402

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "clip_ingest.npz")
GUARD = 64
FLOATS = ("pos", "vel", "rot", "ang")
WIDTH = {"pos": 3, "vel": 3, "rot": 4, "ang": 3}
FILL = {torch.float32: 7.5, torch.uint8: 0xAB}
SCAN_LENGTHS = [31, 32, 33, 2047, 2048, 2049, 4095, 4096, 4097, 9000]


def dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return torch.device("cuda:0")


def _call(model, rot, pos, offsets, cfg=None, flags=None, mirror_map=None, post=None, n_clips=None):
    """mocha_ingest_clips on guarded output buffers: offsets as given (so that a test can hand over bad ones).  Returns the outputs on the
    host and the guarded buffers; raises what the binding raises."""
    cfg = cfg or IngestConfig()
    post = post or PostProcessor(model)
    st = cfg.struct(model) if isinstance(cfg, IngestConfig) else cfg
    d, J = model.device, model.V + 1
    F = int(max(offsets))
    r = torch.from_numpy(np.ascontiguousarray(rot, np.float32)).to(d)
    p = torch.from_numpy(np.ascontiguousarray(pos, np.float32)).to(d)
    n = len(offsets) - 1 if n_clips is None else n_clips
    off = (C.c_int32 * len(offsets))(*[int(x) for x in offsets])
    fl = None if flags is None else (C.c_ubyte * len(flags))(*[int(x) for x in flags])
    mp = None if mirror_map is None else (C.c_int32 * len(mirror_map))(*[int(x) for x in mirror_map])
    bufs, out = {}, {}
    for k, shape, dt in [(k, (F, J, WIDTH[k]), torch.float32) for k in FLOATS] + [("contact", (F, max(int(post.cfg.n_contact), 1)), torch.uint8)]:
        numel = int(np.prod(shape))
        bufs[k] = torch.full((numel + 2 * GUARD,), FILL[dt], dtype=dt, device=d)
        out[k] = bufs[k][GUARD: GUARD + numel].view(shape)
    try:
        model._ctx.call("mocha_ingest_clips", C.byref(st), C.byref(post.cfg), _ptr(r), _ptr(p), off, n, mp, fl, _ptr(out["pos"]),
                        _ptr(out["vel"]), _ptr(out["rot"]), _ptr(out["ang"]), _ptr(out["contact"]), _stream())
    finally:
        torch.cuda.synchronize()
    for k, b in bufs.items():
        edge = torch.cat([b[:GUARD], b[-GUARD:]])
        assert bool((edge == FILL[b.dtype]).all()), f"guard words of {k} were written"
    return {k: v.cpu().numpy() for k, v in out.items()}, bufs


def _within(got, ref, e, what):
    worst = 0.0
    for k in FLOATS:
        r = np.asarray(ref[k], np.float64)
        err = np.abs(got[k].astype(np.float64) - r)
        bound = np.spacing(np.abs(r).astype(np.float32)).astype(np.float64) + 4.0 * e
        worst = max(worst, float((err / bound).max()))
        assert np.all(err <= bound), (what, k, float(err.max()), float((err / bound).max()), np.argwhere(err > bound)[:4].tolist())
    assert np.array_equal(got["contact"].astype(bool), np.asarray(ref["contact"], bool)), (what, "contact")
    return worst


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(GOLD))


@pytest.fixture(scope="module")
def model24():
    return Generator(layout="mocha", device=dev())


def _gold_case(gold, n, mirrored):
    tag = "mirror" if mirrored else "plain"
    return {k: gold[f"{tag}_{n}_{k}"] for k in FLOATS + ("contact",)}


@pytest.fixture(scope="module")
def singles(gold, model24):
    """Every fixture case as a single clip: computed once, shared and left unchanged."""
    out = {}
    for m in (False, True):
        for n in gold["lengths"]:
            n = int(n)
            out[n, m], _ = _call(model24, gold["rot"][:n], gold["pos"][:n], [0, n], flags=[1] if m else None,
                                 mirror_map=gold["mirror_map"] if m else None)
    return out


@pytest.mark.parametrize("mirrored", [False, True], ids=["plain", "mirror"])
@pytest.mark.parametrize("n", [31, 32, 45, 62, 100])
def test_parity_single_clip(gold, singles, n, mirrored):
    w = _within(singles[n, mirrored], _gold_case(gold, n, mirrored), CR.E_MIRROR if mirrored else CR.E, (n, mirrored))
    print(f"n = {n} {'mirrored' if mirrored else 'plain'}: largest error / bound {w:.3f}")


def test_default_mirror_map_is_the_fixtures(gold):
    assert default_mirror_map("mocha") == gold["mirror_map"].tolist()


def test_three_clips_parity_and_isolation(gold, model24, singles):
    lens, flags = [31, 100, 45], [0, 1, 0]
    rot = np.concatenate([gold["rot"][:n] for n in lens])
    pos = np.concatenate([gold["pos"][:n] for n in lens])
    got, _ = _call(model24, rot, pos, [0, 31, 131, 176], flags=flags, mirror_map=gold["mirror_map"])
    at = 0
    for n, m in zip(lens, flags):
        part = {k: v[at: at + n] for k, v in got.items()}
        _within(part, _gold_case(gold, n, bool(m)), CR.E_MIRROR if m else CR.E, ("three clips", n, m))
        for k in part:
            assert np.array_equal(part[k], singles[n, bool(m)][k]), ("a clip inside the call differs from the clip alone", n, k)
        at += n


def test_python_entry_matches_the_guarded_call(gold, model24, singles):
    out = ingest_clips(model24, np.concatenate([gold["rot"][:45], gold["rot"]]), np.concatenate([gold["pos"][:45], gold["pos"]]), [45, 100],
                       mirror=[True, False])
    for k in FLOATS + ("contact",):
        got = out[k].cpu().numpy()
        assert np.array_equal(got[:45], singles[45, True][k]) and np.array_equal(got[45:], singles[100, False][k]), k


# ------------------------------------------------------------------------------------------------------------------ unroll scan, V = 22
ROLES22, TOES22 = (3, 6, 10, 18, 14), (22, 18)


def _flipped_clip(n, seed):
    """A walk of n frames on the 22-joint layout as fp32 quaternions in metres, a random third of every joint's frames negated."""
    par = LAYOUTS["mixamo"]["parents"]
    rot, pos = R.walk_clip(par, n, seed=seed, legs=((18, 19, 20, 21), (14, 15, 16, 17)), shoulders=(6, 10), spine=(1, 2, 3), flip_bone=9)
    q = CR.euler_to_quat(rot, [2, 1, 0]).transpose(1, 2, 0)
    flip = np.random.Generator(np.random.PCG64(seed)).random((n, len(par))) < 1.0 / 3.0
    assert flip[1:].any(axis=0).all(), "a joint without a planted flip"
    q = np.where(flip[..., None], -q, q).astype(np.float32)
    return q, (pos.astype(np.float64) * 0.01).astype(np.float32)


@pytest.fixture(scope="module")
def model22():
    return Generator(layout="mixamo", device=dev())


def _scan_case(model22, lengths, seed0):
    clips = [_flipped_clip(n, seed0 + i) for i, n in enumerate(lengths)]
    post = PostProcessor(model22, contact_bones=[22, 18])
    got, _ = _call(model22, np.concatenate([c[0] for c in clips]), np.concatenate([c[1] for c in clips]),
                   np.concatenate([[0], np.cumsum(lengths)]), cfg=IngestConfig(order=None, unit_scale=1.0), post=post)
    at = 0
    for n, (q, p) in zip(lengths, clips):
        ref = CR.process_clip(q, p, LAYOUTS["mixamo"]["parents"], None, ROLES22, TOES22, unit_scale=1.0)
        part = {k: v[at: at + n] for k, v in got.items()}
        same = np.sum(part["rot"][:, 2:].astype(np.float64) * ref["rot"][:, 2:], axis=-1)
        assert np.all(same > 0.5), ("a sign differs from the restatement's", n, np.argwhere(same <= 0.5)[:4].tolist())
        flipped = np.sum(ref["rot"][:, 2:] * q[:, 1:].astype(np.float64), axis=-1) < 0
        assert flipped.any(axis=0).all() and not flipped.all(axis=0).any(), "unroll negated no frame, or every frame, of a joint"
        _within(part, ref, CR.E, ("scan", n))
        at += n
    return got, clips, post


def test_unroll_scan_chunk_edges(model22):
    _scan_case(model22, SCAN_LENGTHS, 500)


def test_unroll_scan_boundary_inside_a_chunk(model22):
    got, clips, post = _scan_case(model22, [45, 40], 600)
    alone, _ = _call(model22, clips[1][0], clips[1][1], [0, 40], cfg=IngestConfig(order=None, unit_scale=1.0), post=post)
    for k in alone:
        assert np.array_equal(got[k][45:], alone[k]), k


# ------------------------------------------------------------------------------------------------------------------ the streaming route
def test_against_the_streaming_route(gold, model24, singles):
    """Frames 12 .. 81 of the 100-frame clip: push n of Ingestor(raw=18) emits frame n-19 of the whole clip.  The floats came out
    bit-identical on the MI355X (module docstring); the assertion is the bound, not bit equality."""
    ing = Ingestor(model24, IngestConfig(lookahead=18, order=str(gold["order"])), streams=1)
    frames = {k: [] for k in ("Ypos", "Yvel", "Yrot", "Yang", "contact")}
    for f in range(100):
        o = ing.step(gold["rot"][f][None], gold["pos"][f][None])
        if f >= 30:
            for k in frames:
                frames[k].append(o[k][0].clone())
    torch.cuda.synchronize()
    stream = {k[1:] if k != "contact" else k: torch.stack(v).cpu().numpy() for k, v in frames.items()}
    clip = {k: v[12:82] for k, v in singles[100, False].items()}
    assert len(stream["pos"]) == 70
    _within(clip, {k: stream[k].astype(np.float64) if k != "contact" else stream[k] for k in stream}, CR.E, "streaming")
    differ = {k: int(np.sum(clip[k].view(np.uint32) != stream[k].view(np.uint32))) for k in FLOATS}
    print("floats whose bits differ between the clip route and the streaming route:", differ)


# ------------------------------------------------------------------------------------------------------------------ windows
def _processed(model, single):
    d = model.device
    return {k: torch.from_numpy(v).to(d) for k, v in single.items()}


@pytest.mark.parametrize("n,step", [(100, 1), (100, 30), (31, 1)])
def test_windows(gold, model24, singles, n, step):
    src = singles[n, False]
    w = clip_windows(_processed(model24, src), [n], window=60, step=step, model=model24)
    got = {k: v.cpu().numpy() for k, v in w.items()}
    B = CR.window_count(n, 60, step)
    assert clip_window_counts([n], 60, step) == [B] and len(got["Ypos"]) == B and B == {(100, 1): 85, (100, 30): 3, (31, 1): 16}[n, step]
    own = CR.windows(src, 60, step)                               # the gather itself is exact
    for k in own:
        assert np.array_equal(got[k], own[k]), (k, n, step)
    if n == 100:
        tag, sel = ("w30", slice(None)) if step == 30 else ("w1", gold["w1_index"])
        ref = {k: gold[f"{tag}_{k}"] for k in FLOATS + ("contact",)}
    else:                                                         # every window padded: the reference's clip through the restatement's divide
        ref = CR.windows(_gold_case(gold, 31, False), 60, step)
        ref = {"pos": ref["Ypos"], "vel": ref["Yvel"], "rot": ref["Yrot"], "ang": ref["Yang"], "contact": ref["contact"]}
        sel = slice(None)
    _within({"pos": got["Ypos"][sel], "vel": got["Yvel"][sel], "rot": got["Yrot"][sel], "ang": got["Yang"][sel],
             "contact": got["contact"][sel]}, ref, CR.E, ("windows", n, step))
    for b in range(B):
        m = min(60, n - b * step)
        left = (60 - m) // 2 + (60 - m) % 2
        pad = np.r_[0:left, left + m:60]
        assert not got["Yvel"][b, pad].any() and not got["Yang"][b, pad].any(), ("padding of vel / ang is not zero", b)
        if len(pad):
            assert np.array_equal(got["Ypos"][b, :left], np.repeat(got["Ypos"][b, left:left + 1], left, 0))
            assert np.array_equal(got["Yrot"][b, left + m:], np.repeat(got["Yrot"][b, left + m - 1:left + m], 60 - left - m, 0))


def test_windows_two_clips(model24, singles):
    a, b = singles[45, True], singles[100, False]
    both = {k: np.concatenate([a[k], b[k]]) for k in a}
    w = clip_windows(_processed(model24, both), [45, 100], window=60, step=7, model=model24)
    own = [CR.windows(x, 60, 7) for x in (a, b)]
    assert clip_window_counts([45, 100], 60, 7) == [len(own[0]["Ypos"]), len(own[1]["Ypos"])]
    for k in own[0]:
        assert np.array_equal(w[k].cpu().numpy(), np.concatenate([own[0][k], own[1][k]])), k


# ------------------------------------------------------------------------------------------------------------------ refusals
def _refused(model, gold, **kw):
    args = dict(rot=gold["rot"], pos=gold["pos"], offsets=[0, 100])
    args.update(kw)
    with pytest.raises(RuntimeError, match="status"):
        _call(model, args.pop("rot"), args.pop("pos"), args.pop("offsets"), **args)


def test_refusals(gold, model24):
    mp = gold["mirror_map"].tolist()
    _refused(model24, gold, rot=gold["rot"][:30], pos=gold["pos"][:30], offsets=[0, 30])                  # savgol_filter raises there
    _refused(model24, gold, offsets=[0, 70, 100])                                                         # ... and for a clip inside a call
    _refused(model24, gold, offsets=[0, 100, 100])                                                        # offsets that do not increase
    _refused(model24, gold, offsets=[0, 100, 50])
    _refused(model24, gold, offsets=[5, 100])
    _refused(model24, gold, flags=[1])                                                                    # flag without a map
    bad = list(mp); bad[4] = 5                                                                            # noqa: E702  no involution
    _refused(model24, gold, flags=[1], mirror_map=bad)
    bad = list(range(24)); bad[4], bad[23] = 23, 4                                                        # noqa: E702  toes exchanged, feet not
    _refused(model24, gold, flags=[1], mirror_map=bad)
    _refused(model24, gold, flags=[0], mirror_map=bad)                                                    # a bad map is refused even unused
    for kw in (dict(order="zyx", fps=0.0), dict(order="zyx", unit_scale=float("nan")), dict(order="zyx", spine=24), dict(order="zyx", upleg_r=-1)):
        _refused(model24, gold, cfg=IngestConfig(**kw))
    st = IngestConfig().struct(model24)
    st.rot_format = 2
    _refused(model24, gold, cfg=st)
    st = IngestConfig().struct(model24)
    st.euler_order[0] = st.euler_order[1] = 1
    _refused(model24, gold, cfg=st)
    st = IngestConfig().struct(model24)
    st.lookahead = 99                                                                                     # ignored, not refused
    got, _ = _call(model24, gold["rot"], gold["pos"], [0, 100], cfg=st)
    assert np.isfinite(got["pos"]).all()
    with pytest.raises(RuntimeError, match="status"):                                                    # a NULL required pointer
        model24._ctx.call("mocha_ingest_clips", C.byref(st), None, None, None, (C.c_int32 * 2)(0, 100), 1, None, None, None, None, None, None,
                          None, _stream())
    src = {k: torch.zeros((100, 25, WIDTH[k]), device=model24.device) for k in FLOATS}
    src["contact"] = torch.zeros((100, 2), dtype=torch.uint8, device=model24.device)
    for window, step in ((3, 1), (60, 0)):
        with pytest.raises((RuntimeError, ValueError)):
            clip_windows(src, [100], window=window, step=step, model=model24)
    off = (C.c_int32 * 2)(0, 100)
    for window, step in ((3, 1), (60, 0)):
        with pytest.raises(RuntimeError, match="status"):
            model24._ctx.call("mocha_clip_windows", None, None, None, None, None, 2, off, 1, window, step, None, None, None, None, None, _stream())


def test_refusal_launches_nothing(gold, model24):
    """A refused call leaves its outputs as they were."""
    with pytest.raises(RuntimeError, match="status"):
        _call(model24, gold["rot"], gold["pos"], [0, 70, 100])                                            # the second clip has 30 frames
    d = model24.device
    out = {k: torch.full((100, 25, WIDTH[k]), 7.5, device=d) for k in FLOATS}
    con = torch.full((100, 2), 0xAB, dtype=torch.uint8, device=d)
    r, p = torch.from_numpy(gold["rot"]).to(d), torch.from_numpy(gold["pos"]).to(d)
    st, post = IngestConfig().struct(model24), PostProcessor(model24)
    with pytest.raises(RuntimeError, match="status"):
        model24._ctx.call("mocha_ingest_clips", C.byref(st), C.byref(post.cfg), _ptr(r), _ptr(p), (C.c_int32 * 3)(0, 70, 100), 2, None, None,
                          _ptr(out["pos"]), _ptr(out["vel"]), _ptr(out["rot"]), _ptr(out["ang"]), _ptr(con), _stream())
    torch.cuda.synchronize()
    assert all(bool((v == 7.5).all()) for v in out.values()) and bool((con == 0xAB).all())
