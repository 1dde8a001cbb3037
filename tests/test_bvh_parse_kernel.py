"""mocha_bvh_motion on the MI355X (run with -m gpu), through the public C ABI: the MOTION text of BVH files -> rot / pos fp32.

Every value is compared BIT FOR BIT with np.float32(float(token)) - Python's correctly rounded decimal -> float64, rounded once to fp32 -
computed by tests/bvh_ref.py (line split, float()).  Where the text is meant to convert on the device the call gets NO host copy and the
report must say slow == 0, so the host's strtod cannot hide a broken fast path.  Every output sits between guard words.

Refusals: the "first bad byte" is the first byte at which the text visibly breaks the layout -
  a line with C - 1 tokens   the first token of the NEXT line (it starts a line and is not a multiple of C into the clip)
  a line with C + 1 tokens   that line's token C (it is a multiple of C into the clip and does not start a line)
  one frame too many         the first token of the extra line;      one frame too few: the clip's end byte
  a malformed / overlong token, a token in a gap: its first byte.

Shapes: a lane reads 16 bytes, a wave 1024, a workgroup one block of 4096; a 10-byte token is put 1..9 bytes in front of each of those
edges; texts of 15, 16, 17, 4095, 4096, 4097 bytes end with a token on their last byte (1 byte cannot hold a frame: refused).

Random tokens: 20 004 = 3334 frames of 6 (20 000 is no multiple of a frame), each with at most 15 significant digits and a net decimal
exponent within +-22 - asserted on the CPU before the call.

Mutations, each made on a scratch copy of csrc/bvh_parse.hip (a predicate / an arithmetic expression only, every index in bounds),
rebuilt, and this file run on the MI355X against the mutated library (2026-10-20; 40 tests, all pass on the unmutated code):
  token starts   the byte before a block taken as whitespace (the previous block's last byte dropped from start_mask)
                 10 fail, 1 errors: test_token_across_lane_wave_and_block_edges[4096] (the lane and wave edges 16 and 1024 pass),
                 test_text_lengths_token_on_the_last_byte[4097], test_three_blocks, test_random_tokens, the three fixture files, both
                 test_joint_map cases, test_slow_list_limit, and the three_clips fixture - every text with a token across a block edge
  division       double(m) * (1.0 / 10^-e) in place of double(m) / 10^-e
                 1 fails: test_division_is_ieee_rounded.  "0.1", "0.3" (test_token_forms) and the 20 004 random tokens PASS under this
                 mutation, measured before that test existed: the outputs are fp32, and a float64 that is one ulp off changes the fp32
                 only when it lies within 2^-52 of the midpoint of two fp32 neighbours.  TIES are tokens that sit exactly on such
                 midpoints, which makes the quotient's last bit visible; with them the mutation gives -14861989 for -14861988.5 (even:
                 -14861988), -7158354.5 for -7158354.25, -1812330.4 for -1812330.3125.
"""
import ctypes as C
import os
import random
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bvh_ref  # noqa: E402
from mocha_sigasia2023_amd import Generator, _C, read_bvh_header  # noqa: E402

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ALIGN, GUARD, FILL = 4096, 64, 7.5
ERR_ARG, ERR_STATE = -1, -3
T10 = b"123.456789"                      # the 10-byte token of the edge cases


@pytest.fixture(scope="module")
def model():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return Generator(layout="mocha", device=torch.device("cuda:0"))


def pack(blocks):
    """The packing rule of mocha_hip.h: every clip at a multiple of 4096, gaps and tail '\\n'."""
    begin, end, at = [], [], 0
    for b in blocks:
        begin.append(at); end.append(at + len(b))
        at += max(-(-len(b) // ALIGN), 1) * ALIGN
    buf = np.full(at, 0x0A, dtype=np.uint8)
    for b, s in zip(blocks, begin):
        buf[s: s + len(b)] = np.frombuffer(b, dtype=np.uint8)
    return buf, begin, end


def run(model, blocks, frames, n_joints, channels, joint_map=None, v_out=None, offsets=None, host=False, buf=None, begin=None, end=None):
    """One call on guarded outputs.  Returns (status, rot, pos, report); rot / pos (F,v_out,3) fp32 on the host."""
    if buf is None:
        buf, begin, end = pack(blocks)
    n = len(frames)
    v_out = n_joints if v_out is None else v_out
    F = int(sum(frames))
    dev = model.device
    text = torch.from_numpy(buf).to(dev)
    bufs = [torch.full((F * v_out * 3 + 2 * GUARD,), FILL, dtype=torch.float32, device=dev) for _ in range(2)]
    rot, pos = (b[GUARD: GUARD + F * v_out * 3].view(F, v_out, 3) for b in bufs)
    off = np.concatenate([[0], np.cumsum(frames)])
    rep = _C.mocha_bvh_report()
    jm = None if joint_map is None else (C.c_int32 * n_joints)(*[int(j) for j in joint_map])
    oo = None if offsets is None else np.ascontiguousarray(offsets, np.float32)
    with torch.cuda.device(dev):
        rc = model._ctx.lib.mocha_bvh_motion(
            model._ctx.h, C.c_void_p(text.data_ptr()), len(buf), buf.ctypes.data_as(C.c_void_p) if host else None,
            (C.c_int64 * n)(*begin), (C.c_int64 * n)(*end), (C.c_int32 * (n + 1))(*[int(v) for v in off]), n, n_joints, channels, jm, v_out,
            None if oo is None else oo.ctypes.data_as(C.POINTER(C.c_float)), C.c_void_p(rot.data_ptr()), C.c_void_p(pos.data_ptr()),
            C.byref(rep), C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
        torch.cuda.synchronize()
    for b in bufs:
        assert bool((torch.cat([b[:GUARD], b[-GUARD:]]) == FILL).all()), "guard words were written"
    return rc, rot.cpu().numpy(), pos.cpu().numpy(), rep


def expect(block, frames, n_joints, channels, joint_map=None, v_out=None, offsets=None):
    """rot, pos (frames,v_out,3) fp32 as the reference's loader arranges the numbers of one numeric block (bvh.py:110-118)."""
    _, vals = bvh_ref.motion_tokens(block)
    v_out = n_joints if v_out is None else v_out
    jm = list(range(n_joints)) if joint_map is None else list(joint_map)
    if channels == 3:
        data = vals.reshape(frames, 3 + 3 * n_joints)
        r_file, p_file = data[:, 3:].reshape(frames, n_joints, 3), None
    else:
        data = vals.reshape(frames, n_joints, 6)
        r_file, p_file = data[..., 3:], data[..., :3]
    rot = np.zeros((frames, v_out, 3), np.float32)
    pos = np.zeros((frames, v_out, 3), np.float32)
    if channels == 3:
        pos[:] = np.asarray(offsets, np.float32)[None]
    for j, o in enumerate(jm):
        if o < 0:
            continue
        rot[:, o] = r_file[:, j].astype(np.float32)
        if channels == 6:
            pos[:, o] = p_file[:, j].astype(np.float32)
        elif j == 0:
            pos[:, o] = data[:, :3].astype(np.float32)
    return rot, pos


def same_bits(got, want):
    return got.shape == want.shape and np.array_equal(got.view(np.uint32), want.view(np.uint32))


def check_clean(model, block, frames, n_joints=1, channels=6, **kw):
    """One clip that must convert on the device alone: status 0, slow == 0, bitwise equal."""
    rc, rot, pos, rep = run(model, [block], [frames], n_joints, channels, host=False, **kw)
    assert rc == 0, (rc, rep.first_bad, block[:80])
    want_rot, want_pos = expect(block, frames, n_joints, channels, **kw)
    assert rep.slow == 0 and rep.first_bad == -1 and rep.tokens == len(block.split())
    assert same_bits(rot, want_rot) and same_bits(pos, want_pos), block[:80]
    return rot, pos


# ---------------------------------------------------------------------------------------------------------------- fixture files
@pytest.mark.parametrize("tag", ("mocha24_rot", "mocha24_pos", "mixamo22"))
def test_fixture_files(model, tag):
    gold = np.load(os.path.join(GOLDEN, "bvh_parse.npz"))
    with open(os.path.join(GOLDEN, "bvh", tag + ".bvh"), "rb") as f:
        text = f.read()
    h = read_bvh_header(text)
    block = text[h.motion_begin: h.motion_end]
    rc, rot, pos, rep = run(model, [block], [h.frames], len(h.names), h.channels, offsets=h.offsets, host=False)
    assert rc == 0 and rep.slow == 0 and rep.first_bad == -1
    assert rep.tokens == h.frames * (6 * len(h.names) if h.channels == 6 else 3 + 3 * len(h.names))
    assert same_bits(rot, gold[f"{tag}_rotations"].astype(np.float32))
    assert same_bits(pos, gold[f"{tag}_positions"].astype(np.float32))


# ---------------------------------------------------------------------------------------------------------------- token forms
FORMS = ["0", "-0", "-0.000000", "+1.5", ".5", "-.5", "5.", "1e-05", "1E+2", "1.e3", "123456789012345", "0.000001", "0.1", "0.3",
         "179.999999"]


def test_token_forms(model):
    toks = FORMS + ["1", "2", "3"]
    block = "\n".join(" ".join(toks[i: i + 6]) for i in range(0, 18, 6)).encode() + b"\n"
    rot, pos = check_clean(model, block, 3)
    got = np.concatenate([pos, rot], axis=-1).reshape(-1)
    for t, g in zip(toks, got):
        assert g.view(np.uint32) == np.float32(float(t)).view(np.uint32), t
    assert np.signbit(got[1]) and np.signbit(got[2]) and not np.signbit(got[0])


# Tokens whose float64 value is EXACTLY the midpoint of two fp32 neighbours (25 significant bits) and is reached by a division by 10^5:
# m / 1e5 is exact, so the cast to fp32 ties to even; m * (1 / 1e5) lands one float64 ulp beside the midpoint and the cast goes the other
# way.  Only at such ties does the fp32 output show the last bit of the float64 quotient ("0.1" and "0.3" alone cannot: their float64
# values are far from any fp32 midpoint).  Found by a seeded search over odd 25-bit integers scaled by 2^e; checked on the CPU below.
TIES = ["14861988.50000", "7158354.25000", "1812330.31250"]


def test_division_is_ieee_rounded(model):
    toks = TIES + ["-" + t for t in TIES]
    for t in TIES:
        m = int(t.replace(".", ""))
        assert _fast(t) and m / 1e5 == float(t) and np.float32(m / 1e5) != np.float32(m * (1.0 / 1e5)), t
    rot, pos = check_clean(model, (" ".join(toks) + "\n").encode(), 1)
    got = np.concatenate([pos, rot], axis=-1).reshape(-1)
    for t, g in zip(toks, got):
        assert g.view(np.uint32) == np.float32(float(t)).view(np.uint32), (t, float(g))


SLOW = ["0.1234567890123456789", "1e23", "1e-30", "1234567890" * 4, "123456789012345678e-3"]


def test_slow_tokens(model):
    block = (" ".join(SLOW) + " 2.5\n").encode()
    rc, rot, pos, rep = run(model, [block], [1], 1, 6, host=True)
    assert rc == 0 and rep.slow == len(SLOW) and rep.tokens == 6 and rep.first_bad == -1
    got = np.concatenate([pos, rot], axis=-1).reshape(-1)
    for t, g in zip(SLOW + ["2.5"], got):
        assert g.view(np.uint32) == np.float32(float(t)).view(np.uint32), t
    rc, _, _, rep = run(model, [block], [1], 1, 6, host=False)
    assert rc == ERR_STATE and rep.slow == len(SLOW) and rep.first_bad == -1
    assert b"text_host" in model._ctx.lib.mocha_last_error(model._ctx.h)


def test_slow_list_limit(model):
    frames = 683                                                     # 4098 tokens
    for n_slow, status in ((4096, 0), (4097, ERR_STATE)):
        toks = ["1e23"] * n_slow + ["1.5"] * (frames * 6 - n_slow)
        block = "\n".join(" ".join(toks[i: i + 6]) for i in range(0, len(toks), 6)).encode() + b"\n"
        rc, rot, pos, rep = run(model, [block], [frames], 1, 6, host=True)
        assert rc == status and rep.slow == n_slow, (n_slow, rc, rep.slow)
        if status == 0:
            want_rot, want_pos = expect(block, frames, 1, 6)
            assert same_bits(rot, want_rot) and same_bits(pos, want_pos)


# ---------------------------------------------------------------------------------------------------------------- geometry
def _token_at(start):
    """A text of whole 12-byte lines, then a line whose first token T10 starts at byte `start` (left-padded with spaces)."""
    n = start // 12
    return b"0 0 0 0 0 0\n" * n + b" " * (start - 12 * n) + T10 + b" 1 2 3 4 5\n", n + 1


@pytest.mark.parametrize("edge", (16, 1024, 4096))
def test_token_across_lane_wave_and_block_edges(model, edge):
    for before in range(1, 10):
        block, frames = _token_at(edge - before)
        assert block.index(T10) == edge - before
        rot, pos = check_clean(model, block, frames)
        assert pos[-1, 0, 0] == np.float32(123.456789) and rot[-1, 0, 2] == 5.0


def _text_of(nbytes):
    """nbytes bytes of 6-token lines whose last token ends on the last byte."""
    n = (nbytes - 15) // 12
    last = nbytes - 12 * n - 10                                      # 5 .. 16 bytes
    tok = ("9." + "1234567890123"[: last - 2]) if last <= 15 else "-9." + "1234567890123"[: last - 3]
    block = b"0 0 0 0 0 0\n" * n + b"1 2 3 4 5 " + tok.encode()
    assert len(block) == nbytes and len(tok) == last
    return block, n + 1


@pytest.mark.parametrize("nbytes", (15, 16, 17, 4095, 4096, 4097))
def test_text_lengths_token_on_the_last_byte(model, nbytes):
    block, frames = _text_of(nbytes)
    check_clean(model, block, frames)


def test_one_byte_text_is_too_short(model):
    rc, _, _, rep = run(model, [b"7"], [1], 1, 6)
    assert rc == ERR_STATE and rep.first_bad == 1 and rep.tokens == 1


def _messy(frames, seed, size=None):
    """Frames as write_bvh emits them ('%f ' per value: a trailing space on every line), with tabs, \\r\\n and blank lines mixed in."""
    rng = random.Random(seed)
    out = b""
    for f in range(frames):
        vals = ["%f" % rng.gauss(0.0, 180.0) for _ in range(6)]
        sep = "\t" if f % 3 == 1 else " "
        line = sep.join(vals) + " " + ("\r\n" if f % 2 else "\n")
        if f % 5 == 4:
            line += "\r\n" if f % 2 else " \t\n"
        out += line.encode()
    if size is not None:
        assert len(out) <= size
        out += b"\n" * (size - len(out))
    return out


def test_one_frame(model):
    check_clean(model, b"1.000000 -2.500000 3.250000 0.000000 -0.000000 179.999999 \n", 1)


def test_exactly_one_block(model):
    block = _messy(50, 1, size=ALIGN)
    assert len(block) == ALIGN and len(pack([block])[0]) == ALIGN
    check_clean(model, block, 50)


def test_three_blocks(model):
    block = _messy(150, 2)
    assert 2 * ALIGN < len(block) <= 3 * ALIGN
    check_clean(model, block, 150)


# ---------------------------------------------------------------------------------------------------------------- random tokens
_NUM = re.compile(r"^[+-]?(\d*)\.?(\d*)(?:[eE]([+-]?\d+))?$")


def _fast(tok):
    """The header's fast-path rule, evaluated on the CPU: at most 15 significant digits, |[eE] exponent - fractional digits| <= 22."""
    m = _NUM.match(tok)
    digits = (m.group(1) + m.group(2)).lstrip("0")
    return len(digits) <= 15 and abs(int(m.group(3) or 0) - len(m.group(2))) <= 22


def _random_token(rng):
    nd = rng.randint(1, 15)
    digits = str(rng.randint(1, 9)) + "".join(rng.choice("0123456789") for _ in range(nd - 1))
    cut = rng.randint(0, nd)
    ip, fp = digits[:cut], digits[cut:]
    if rng.random() < 0.3:
        ip = "0" * rng.randint(0, 2) + ip
    body = ip + ("." + fp if fp or rng.random() < 0.3 else "")
    if body in ("", "."):
        body = "0" + body + ("0" if body == "." else "")
    tok = rng.choice(["", "", "-", "+"]) + body
    if rng.random() < 0.4:
        e = rng.randint(len(fp) - 22, len(fp) + 22)
        tok += rng.choice("eE") + (rng.choice(["", "+"]) if e >= 0 else "") + str(e)
    return tok


def test_random_tokens(model):
    rng = random.Random(20231213)
    toks = [_random_token(rng) for _ in range(20004)]
    assert all(_fast(t) for t in toks)
    assert sum("e" in t.lower() for t in toks) > 5000 and sum(t.startswith(".") or "-." in t or "+." in t for t in toks) > 100
    lines = []
    for i in range(0, len(toks), 6):
        lines.append(rng.choice([" ", "  ", "\t"]).join(toks[i: i + 6]) + rng.choice(["\n", " \n", "\r\n"]))
    block = "".join(lines).encode()
    rot, pos = check_clean(model, block, len(toks) // 6)
    got = np.concatenate([pos, rot], axis=-1).reshape(-1)
    want = np.array([float(t) for t in toks]).astype(np.float32)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


# ---------------------------------------------------------------------------------------------------------------- several clips
def _clip(frames, n_joints, channels, seed):
    rng = random.Random(seed)
    per = 3 + 3 * n_joints if channels == 3 else 6 * n_joints
    return "".join("".join("%f " % rng.gauss(0.0, 90.0) for _ in range(per)) + "\n" for _ in range(frames)).encode()


@pytest.fixture(scope="module")
def three_clips(model):
    """Three clips of the 24-joint skeleton, channels == 3, each parsed alone: computed once, shared, left unchanged."""
    offsets = np.random.Generator(np.random.PCG64(5)).uniform(-9, 9, (24, 3)).astype(np.float32)
    blocks = [_clip(n, 24, 3, 100 + n) for n in (31, 40, 33)]
    alone = []
    for b, n in zip(blocks, (31, 40, 33)):
        rc, rot, pos, rep = run(model, [b], [n], 24, 3, offsets=offsets)
        assert rc == 0 and rep.slow == 0
        w_rot, w_pos = expect(b, n, 24, 3, offsets=offsets)
        assert same_bits(rot, w_rot) and same_bits(pos, w_pos)
        alone.append((rot, pos))
    return blocks, offsets, alone


def test_three_clips_in_one_call(model, three_clips):
    blocks, offsets, alone = three_clips
    assert len(blocks[1]) > 2 * ALIGN                                  # clips span several blocks and start on their own
    rc, rot, pos, rep = run(model, blocks, [31, 40, 33], 24, 3, offsets=offsets)
    assert rc == 0 and rep.slow == 0 and rep.tokens == 104 * 75
    assert same_bits(rot, np.concatenate([a[0] for a in alone])) and same_bits(pos, np.concatenate([a[1] for a in alone]))
    assert np.array_equal(pos[:, 1:], np.broadcast_to(offsets[None, 1:], (104, 23, 3)))      # non-root positions = offsets_out


@pytest.mark.parametrize("channels", (3, 6))
def test_joint_map(model, channels):
    rng = np.random.Generator(np.random.PCG64(9))
    perm = [int(v) for v in rng.permutation(24)]
    drop = list(perm)
    for j in (0 if channels == 6 else 5, 17):                          # two joints dropped (with six channels the root among them)
        drop[j] = -1
    kept = sorted(v for v in drop if v >= 0)
    drop = [kept.index(v) if v >= 0 else -1 for v in drop]
    block = _clip(35, 24, channels, 7)
    for jm, v_out in ((perm, 24), (drop, 22)):
        offsets = rng.uniform(-9, 9, (v_out, 3)).astype(np.float32)
        check_clean(model, block, 35, 24, channels, joint_map=jm, v_out=v_out, offsets=offsets)
    rc, _, _, _ = run(model, [block], [35], 24, channels, joint_map=[0] * 24, v_out=24, offsets=np.zeros((24, 3)))
    assert rc == ERR_ARG


# ---------------------------------------------------------------------------------------------------------------- refusals
LINE = b"1.5 2.5 3.5 4.5 5.5 6.5\n"


def _refused(model, block, frames, at, **kw):
    rc, _, _, rep = run(model, [block], [frames], 1, 6, host=True, **kw)
    assert rc == ERR_STATE and rep.first_bad == at, (rc, rep.first_bad, at)
    assert str(at).encode() in model._ctx.lib.mocha_last_error(model._ctx.h)


def test_line_with_a_token_missing(model):
    _refused(model, LINE + b"1 2 3 4 5\n" + LINE, 3, len(LINE) + 10)


def test_line_with_a_token_too_many(model):
    _refused(model, LINE + b"1 2 3 4 5 6 7\n" + LINE, 3, len(LINE) + 12)


def test_one_frame_too_few(model):
    _refused(model, LINE * 2, 3, 2 * len(LINE))


def test_one_frame_too_many(model):
    _refused(model, LINE * 4, 3, 3 * len(LINE))


@pytest.mark.parametrize("bad", ("1.2.3", "abc", "nan", "1e", "inf", "0x10", "1_0", "-", "."))
def test_malformed_token(model, bad):
    _refused(model, LINE + b"1 2 " + bad.encode() + b" 4 5 6\n", 2, len(LINE) + 4)


def test_token_length_limit(model):
    ok = LINE + b"1 2 " + b"1" * 64 + b" 4 5 6\n"
    rc, rot, pos, rep = run(model, [ok], [2], 1, 6, host=True)
    assert rc == 0 and rep.slow == 1 and pos[1, 0, 2] == np.float32(float("1" * 64))
    _refused(model, LINE + b"1 2 " + b"1" * 65 + b" 4 5 6\n", 2, len(LINE) + 4)
    # ... also where the long token crosses the block's end: the 80 bytes staged behind a block decide
    head = b"0 0 0 0 0 0\n" * 340                                      # 4080 bytes
    _refused(model, head + b"1 2 " + b"1" * 65 + b" 4 5 6\n", 341, len(head) + 4)


def test_clip_begin_off_the_grid(model):
    buf, begin, end = pack([LINE * 2, LINE * 2])
    buf[ALIGN + 16: ALIGN + 16 + 2 * len(LINE)] = buf[ALIGN: ALIGN + 2 * len(LINE)]
    rc, rot, pos, rep = run(model, None, [2, 2], 1, 6, buf=buf, begin=[0, ALIGN + 16], end=[end[0], end[1] + 16])
    assert rc == ERR_ARG and rep.first_bad == -1
    assert (rot == FILL).all() and (pos == FILL).all()                 # nothing was launched
    assert b"4096" in model._ctx.lib.mocha_last_error(model._ctx.h)


def test_bytes_in_a_gap(model):
    buf, begin, end = pack([LINE * 2, LINE * 2])
    buf[end[0] + 3] = ord("7")
    rc, _, _, rep = run(model, None, [2, 2], 1, 6, buf=buf, begin=begin, end=end)
    assert rc == ERR_STATE and rep.first_bad == end[0] + 3
    buf, begin, end = pack([LINE * 2, LINE * 2])
    buf[end[1] + 100] = ord("7")                                       # the tail behind the last clip is a gap too
    rc, _, _, rep = run(model, None, [2, 2], 1, 6, buf=buf, begin=begin, end=end)
    assert rc == ERR_STATE and rep.first_bad == end[1] + 100
