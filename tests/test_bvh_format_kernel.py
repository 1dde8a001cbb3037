"""mocha_bvh_format on the MI355X (run with -m gpu), through the public C ABI and through write_bvh(model=...) / write_bvh_clips:
bvh_pos / bvh_euler float64 on the device -> the MOTION text of the reference's writer.

The expected bytes always come from the HOST: Python's "%f " per number and a newline per frame (tests/bvh_fmt_ref.motion_text), or a
whole file from write_bvh WITHOUT ``model`` - never from the code under test.  Every comparison is byte for byte.  The text buffer of
every call sits at an odd offset inside a larger buffer filled with 0xA5, and the bytes in front of it and from report.bytes on must
still be 0xA5 afterwards.

Shapes: a lane formats one token, a workgroup 256 consecutive tokens; a row of 75 tokens (24 joints) does not divide 256, so workgroups
start in the middle of rows and at every byte alignment.  257 frames x 24 joints = 19 275 tokens in 76 workgroups, frame 255 ends on a
workgroup's last token (75 x 256 tokens); 3 frames x 256 joints: one row spans four workgroups; 2 frames x 1 joint: 12 tokens.

Mutations, each made on a scratch copy of csrc/fmt_f6.h or csrc/bvh_format.hip (a predicate or an arithmetic expression only, every index
in bounds), rebuilt, and this file run on the MI355X against the mutated library (2026-10-20; 13 tests, all pass on the unmutated code):
  half-up instead of half-even      5 fail: both test_hard_values (the ties j / 2^k: 1/128 -> 0.007813 for 0.007812),
                                    test_block_and_row_straddling[257-24], test_visit_order_whole_file, test_refusals - the seeded
                                    values evidently hold ties too (which ones was not looked into)
  digit count before the carry      2 fail: both test_hard_values (10^n - 4e-7: 9.9999996 -> 0.000000 for 10.000000); nothing else holds
                                    a value that rounds up into a new digit
  sign from x < 0, not the sign bit 5 fail: both test_hard_values (-0.0 -> 0.000000) and the three golden files, whose channels hold -0.0
                                    (-1e-9 still prints its sign under this mutation)
  a frame's newline dropped when the frame ends on a workgroup's last token (count and write pass alike)
                                    2 fail: test_block_and_row_straddling[257-24] (frame 255 ends on token 75 x 256 - 1) and the golden
                                    file mocha24_pos (144 columns: frame 15 ends on token 9 x 256 - 1)
"""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bvh_fmt_ref as R  # noqa: E402
from mocha_sigasia2023_amd import Generator, _C, write_bvh, write_bvh_clips  # noqa: E402

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ERR_ARG, ERR_STATE = -1, -3
LEAD, TAIL, FILL = 61, 67, 0xA5


@pytest.fixture(scope="module")
def model():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return Generator(layout="mocha", device=torch.device("cuda:0"))


@pytest.fixture(scope="module")
def seeded():
    """The seeded random values, computed once and left unchanged: enough for 257 x 24 x 3 angles and as many positions."""
    v = R.random_values(20262, 2 * 257 * 24 * 3)
    return v


def run(model, pos, rot, visit, order="zyx", save_positions=False, clips=None, capacity=None, lead=LEAD):
    """One call on a guarded buffer.  Returns (status, report, text bytes [0, report.bytes) or None, clip_text_begin, guards intact, whole
    buffer untouched)."""
    F, V = rot.shape[0], rot.shape[1]
    dev = model.device
    offs = [0, F] if clips is None else [0] + [int(v) for v in np.cumsum(clips)]
    n = len(offs) - 1
    bound = int(model._ctx.lib.mocha_bvh_text_bound(F, V, int(save_positions)))
    cap = bound if capacity is None else capacity
    buf = torch.full((lead + bound + TAIL,), FILL, dtype=torch.uint8, device=dev)
    p, r = torch.from_numpy(np.ascontiguousarray(pos)).to(dev), torch.from_numpy(np.ascontiguousarray(rot)).to(dev)
    assert p.dtype == r.dtype == torch.float64
    begin = (C.c_int64 * (n + 1))(*([-7] * (n + 1)))
    rep = _C.mocha_bvhw_report()
    with torch.cuda.device(dev):
        rc = model._ctx.lib.mocha_bvh_format(
            model._ctx.h, C.c_void_p(p.data_ptr()), C.c_void_p(r.data_ptr()), (C.c_int32 * (n + 1))(*offs), n, V,
            (C.c_int32 * V)(*[int(j) for j in visit]), (C.c_int32 * 3)(*[R.AXIS[c] for c in order]), int(save_positions),
            C.c_void_p(buf.data_ptr() + lead), cap, begin, C.byref(rep), C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
        torch.cuda.synchronize()
    host = buf.cpu().numpy()
    nb = int(rep.bytes) if rc == 0 else 0
    guards = bool((host[:lead] == FILL).all() and (host[lead + nb:] == FILL).all())
    return rc, rep, (host[lead: lead + nb].tobytes() if rc == 0 else None), list(begin), guards, bool((host == FILL).all())


def check(model, pos, rot, visit=None, order="zyx", save_positions=False, **kw):
    visit = list(range(rot.shape[1])) if visit is None else visit
    want = R.motion_text(R.columns(pos, rot, visit, order, save_positions))
    rc, rep, text, begin, guards, _ = run(model, pos, rot, visit, order, save_positions, **kw)
    assert rc == 0 and rep.first_bad == -1, (rc, rep.first_bad)
    assert rep.tokens == rot.shape[0] * (6 * len(visit) if save_positions else 3 + 3 * len(visit))
    assert guards, "bytes outside [text_dev, text_dev + report.bytes) were written"
    assert rep.bytes == len(want) and begin[0] == 0 and begin[-1] == len(want), (rep.bytes, len(want), begin)
    if text != want:
        i = next(i for i in range(len(want)) if text[i: i + 1] != want[i: i + 1])
        raise AssertionError((i, text[max(i - 30, 0): i + 30], want[max(i - 30, 0): i + 30]))
    return text, begin


# ------------------------------------------------------------------------------------------------------------------- hard values
@pytest.mark.parametrize("save_positions", (False, True))
def test_hard_values(model, save_positions):
    hard = np.array(R.hard_values())
    assert len(hard) <= 3 * 24 * 3
    rot = np.resize(hard, (3, 24, 3))
    pos = np.resize(np.roll(hard, 5), (3, 24, 3))               # the root's three columns (all 72 with save_positions) hold hard values too
    text, _ = check(model, pos, rot, save_positions=save_positions)
    words = text.split()
    for w in (b"0.007812", b"-0.007812", b"0.023438", b"-0.000000", b"10.000000", b"1000000000.000000", b"999999999999.999878", b"1.000000"):
        assert w in words, w                                      # the host's expectation itself holds the cases the list is there for
    assert b"0.007813" not in words and max(len(w) for w in words) == 20


# ------------------------------------------------------------------------------------------------- block and row straddling
@pytest.mark.parametrize("frames,V", ((257, 24), (3, 256), (2, 1)))
def test_block_and_row_straddling(model, seeded, frames, V):
    rot = seeded[: frames * V * 3].reshape(frames, V, 3)
    pos = seeded[257 * 24 * 3: 257 * 24 * 3 + frames * V * 3].reshape(frames, V, 3)
    visit = list(range(V))
    if V == 256:
        visit = [0] + list(range(255, 0, -1))
    check(model, pos, rot, visit=visit)
    if frames == 257:
        assert (75 * 256) % 256 == 0                              # frame 255 ends on a workgroup's last token
        check(model, pos, rot, visit=visit, save_positions=True, lead=64)       # ... and an aligned destination


# --------------------------------------------------------------------------------------------------------------------- clips
def test_three_clips(model, seeded):
    clips = [1, 40, 7]
    rot = seeded[1000: 1000 + 48 * 24 * 3].reshape(48, 24, 3)
    pos = seeded[9000: 9000 + 48 * 24 * 3].reshape(48, 24, 3)
    text, begin = check(model, pos, rot, clips=clips)
    at, want_begin = 0, [0]
    for n in clips:
        alone = R.motion_text(R.columns(pos[at: at + n], rot[at: at + n], list(range(24)), "zyx", False))
        want_begin.append(want_begin[-1] + len(alone))
        assert text[want_begin[-2]: want_begin[-1]] == alone
        at += n
    assert begin == want_begin
    assert len({b % 4 for b in begin}) > 1                        # the clips' blocks start at different alignments


# --------------------------------------------------------------------------------------------------------------- visit order
def _read(path):
    with open(path, "rb") as f:
        return f.read()


def test_visit_order_whole_file(model, seeded, tmp_path):
    parents = [-1, 0, 0, 1, 2, 1]
    names = ["root", "a", "b", "a1", "b1", "a2"]
    rot = seeded[500: 500 + 9 * 6 * 3].reshape(9, 6, 3)
    pos = seeded[7000: 7000 + 9 * 6 * 3].reshape(9, 6, 3)
    for sp in (False, True):
        host, dev = str(tmp_path / f"host{sp}.bvh"), str(tmp_path / f"dev{sp}.bvh")
        assert write_bvh(host, names, parents, pos, rot, order="xyz", save_positions=sp) == [0, 1, 3, 5, 2, 4]
        assert write_bvh(dev, names, parents, torch.from_numpy(pos), torch.from_numpy(rot), order="xyz", save_positions=sp,
                         model=model) == [0, 1, 3, 5, 2, 4]
        assert _read(dev) == _read(host)
    # fp32 input is cast on the device; fp32 -> float64 is exact, so the host formats the same numbers
    pos32, rot32 = pos.astype(np.float32), rot.astype(np.float32)
    host, dev = str(tmp_path / "host32.bvh"), str(tmp_path / "dev32.bvh")
    write_bvh(host, names, parents, pos32, rot32, order="xyz")
    write_bvh(dev, names, parents, torch.from_numpy(pos32).to(model.device), torch.from_numpy(rot32).to(model.device), order="xyz", model=model)
    assert _read(dev) == _read(host)


@pytest.mark.parametrize("tag", ("mocha24_rot", "mocha24_pos", "mixamo22"))
def test_golden_files_through_the_device(model, tmp_path, tag):
    gold = dict(np.load(os.path.join(GOLDEN, "bvh_parse.npz")))
    names, parents, pos, rot, offsets, order, frametime = R.golden_arrays(gold, tag)
    path = str(tmp_path / "out.bvh")
    write_bvh(path, names, parents, torch.from_numpy(pos).to(model.device), torch.from_numpy(rot).to(model.device), offsets=offsets,
              order=order, frametime=frametime, save_positions=tag == "mocha24_pos", model=model)
    assert _read(path) == R.golden_file(os.path.join(GOLDEN, "bvh", tag + ".bvh"), tag)


# -------------------------------------------------------------------------------------------------------------------- guards
def test_capacity_one_byte_short(model, seeded):
    rot = seeded[: 5 * 24 * 3].reshape(5, 24, 3)
    pos = seeded[3000: 3000 + 5 * 24 * 3].reshape(5, 24, 3)
    want = R.motion_text(R.columns(pos, rot, list(range(24)), "zyx", False))
    rc, rep, _, begin, _, untouched = run(model, pos, rot, list(range(24)), capacity=len(want) - 1)
    assert rc == ERR_ARG and rep.bytes == len(want) and rep.first_bad == -1 and untouched
    assert begin == [0, len(want)]
    rc, rep, text, _, guards, _ = run(model, pos, rot, list(range(24)), capacity=len(want))
    assert rc == 0 and text == want and guards


# ----------------------------------------------------------------------------------------------------------------- refusals
def test_refusals(model, seeded, tmp_path):
    V, frames = 24, 80                                           # 6000 tokens
    rot = seeded[: frames * V * 3].reshape(frames, V, 3).copy()
    pos = seeded[257 * 24 * 3: 257 * 24 * 3 + frames * V * 3].reshape(frames, V, 3).copy()

    def place(t, value):                                          # token t = frame * 75 + column, save_positions False, identity visit, zyx
        f, c = divmod(t, 75)
        assert c >= 3
        rot[f, (c - 3) // 3, 2 - (c - 3) % 3] = value
    place(100, float("nan"))
    place(5000, float("inf"))
    rc, rep, _, _, _, untouched = run(model, pos, rot, list(range(V)))
    assert rc == ERR_STATE and rep.first_bad == 100 and untouched
    place(100, 1.0)
    rc, rep, _, _, _, untouched = run(model, pos, rot, list(range(V)))
    assert rc == ERR_STATE and rep.first_bad == 5000 and untouched
    place(5000, 1e12)
    rc, rep, _, _, _, untouched = run(model, pos, rot, list(range(V)))
    assert rc == ERR_STATE and rep.first_bad == 5000 and untouched      # 1e12 alone is refused
    place(5000, math.nextafter(1e12, 0.0))
    text, _ = check(model, pos, rot)                              # ... and its neighbour below is written
    assert b" 999999999999.999878 " in text
    # write_bvh(model=...) on the NaN input: the host's bytes
    place(100, float("nan"))
    names = [f"j{i}" for i in range(V)]
    parents = [-1] + list(range(V - 1))
    host, dev = str(tmp_path / "host.bvh"), str(tmp_path / "dev.bvh")
    write_bvh(host, names, parents, pos, rot)
    write_bvh(dev, names, parents, torch.from_numpy(pos).to(model.device), torch.from_numpy(rot).to(model.device), model=model)
    assert _read(dev) == _read(host) and b" nan " in _read(dev)


# ---------------------------------------------------------------------------------------------------------- write_bvh_clips
def test_write_bvh_clips(model, seeded, tmp_path):
    parents = [-1, 0, 0, 1, 2, 1]
    names = ["root", "a", "b", "a1", "b1", "a2"]
    clips = [3, 41, 11]
    offs = [0, 3, 44, 55]
    rot = seeded[2000: 2000 + 55 * 6 * 3].reshape(55, 6, 3)
    pos = seeded[8000: 8000 + 55 * 6 * 3].reshape(55, 6, 3)
    for sp in (False, True):
        paths = [str(tmp_path / f"clip{i}_{sp}.bvh") for i in range(3)]
        visit = write_bvh_clips(model, paths, names, parents, torch.from_numpy(pos).to(model.device), torch.from_numpy(rot).to(model.device),
                                offs, order="yxz", frametime=1 / 30, save_positions=sp)
        assert visit == [0, 1, 3, 5, 2, 4]
        for i, n in enumerate(clips):
            alone = str(tmp_path / f"alone{i}_{sp}.bvh")
            write_bvh(alone, names, parents, pos[offs[i]: offs[i + 1]], rot[offs[i]: offs[i + 1]], order="yxz", frametime=1 / 30, save_positions=sp)
            assert _read(paths[i]) == _read(alone), (i, sp)
            assert _read(alone).count(b"\n") > n
