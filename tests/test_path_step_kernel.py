"""The online path step on the MI355X through the C ABI alone (run with -m gpu): mocha_match_path_advance on synthetic distance rows over
40 steps, with guard words around every output and around the state.  Every idx, dist and continued of every step must equal
tests/path_step_ref.py exactly.

The kernel's thread t owns the STRIDED columns t, t + 1024, ...: the boundaries a tie can straddle are columns 64 w - 1 | 64 w (two
waves), 1024 k - 1 | 1024 k (thread 1023 and thread 0 of the next round) and j | j + 1024 (one thread's own columns).  Exact ties in d -
and, with integer distances and an integer penalty, in a == lambda - are planted across 63 | 64, 1023 | 1024, 2047 | 2048, 4095 | 4096
and 7 | 1031, in steps that restart (R = d) and in steps that continue; clip starts sit on the same columns.  Restarts come by id, by the
one-shot flag, by a changed row count, by a sit-out step and by mocha_path_state_reset; the streams have different row counts, one of
them for a while more rows than the state or the leading dimension hold (it sits out)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from mocha_sigasia2023_amd import Generator  # noqa: E402
from path_step_ref import PathStepRef  # noqa: E402

pytestmark = pytest.mark.gpu
G = 64                                   # guard elements on either side of an output, guard BYTES around the state
ERR_ARG = -1
STEPS = 40
BOUNDS = (64, 1024, 2048, 4096)          # a tie sits on columns b - 1 | b
SAME = (7, 1031)                         # ... and on two columns of one thread


def dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ctx():
    return Generator(layout="mixamo", device=dev())._ctx          # the pure form needs a context, no weights and no bank


def guarded(n, dtype, fill):
    whole = torch.full((n + 2 * G,), fill, dtype=dtype, device=dev())
    return whole, whole[G:G + n]


def guards_intact(whole, n, fill):
    w = whole.cpu()
    if w.dtype.is_floating_point and np.isnan(fill):
        return bool(torch.isnan(w[:G]).all()) and bool(torch.isnan(w[G + n:]).all())
    return bool((w[:G] == fill).all()) and bool((w[G + n:] == fill).all())


def stream():
    return C.c_void_p(torch.cuda.current_stream(dev()).cuda_stream)


def ptr(t):
    return C.c_void_p(0 if t is None else t.data_ptr())


def distances(N, S, ld, ties, seed):
    """(STEPS, S, ld) fp32 host rows whose first N columns count (the rest NaN)."""
    rng = np.random.default_rng(seed)
    d = np.full((STEPS, S, ld), np.nan, dtype=np.float32)
    if ties:
        d[:, :, :N] = rng.integers(1, 5, (STEPS, S, N)).astype(np.float32)
        # a row minimum that occurs twice across an ownership boundary: in steps that restart (0, and the restarts planned below) and in
        # steps that continue
        plan = ((0, 64), (1, 1024), (2, 2048), (3, 4096), (13, 64), (14, 1024), (20, 2048), (21, 64), (34, 1024))
        for t, b in plan:
            if b < N:
                d[t, :, b - 1] = d[t, :, b] = 0
        for t in (5, 27, 28):
            if SAME[1] < N:
                d[t, :, SAME[0]] = d[t, :, SAME[1]] = 0
    else:
        d[:, :, :N] = rng.uniform(1.0, 2.0, (STEPS, S, N)).astype(np.float32)
    return d


def scenario(N, S, ld):
    """ids, rows (STEPS, S), restart flags (STEPS, S), steps at which stream 0 is reset, per-stream start lists."""
    ids = np.tile(np.arange(S, dtype=np.int32), (STEPS, 1))
    rows = np.tile(np.array([max(1, N - 37 * s) for s in range(S)], dtype=np.int32), (STEPS, 1))
    flags = np.zeros((STEPS, S), dtype=np.int32)
    ids[13:, 0] = 7                                  # a change of id restarts
    flags[20, S - 1] = 1                             # the one-shot flag
    flags[21, S - 1] = 0
    ids[27, 0] = -1                                  # a sit-out step: the next one restarts
    flags[27, 0] = 1                                 # ... and the flag set during it is not consumed by it
    rows[33:, S - 1] = max(1, rows[0, S - 1] - 1)    # a changed extent restarts
    if S > 1:
        rows[36, 1] = ld + 1                         # more rows than the leading dimension (and the state): sits out
        rows[37, 1] = 0
    resets = (30,)
    starts = [sorted(set(b for b in BOUNDS + (SAME[1], 1, N - 1) if 0 < b < N)) if s % 2 == 0 else [] for s in range(S)]
    return ids, rows, flags, resets, starts


def pack_bits(S, N, starts):
    """One bit table for all streams, stream s at the unaligned bit offset 5 + s (N + 3) -> (int32 words, offsets, bool array)."""
    off = np.array([5 + s * (N + 3) for s in range(S)], dtype=np.int32)
    n_bits = int(off[-1]) + N + 3
    bits = np.zeros(n_bits, dtype=bool)
    for s in range(S):
        for b in starts[s]:
            bits[off[s] + b] = True
    words = np.zeros((n_bits + 31) // 32, dtype=np.uint32)
    for i in np.nonzero(bits)[0]:
        words[i >> 5] |= np.uint32(1) << np.uint32(i & 31)
    return words.view(np.int32), off, bits, n_bits


def run(ctx, N, S, ties, lam, seed):
    lib, h = ctx.lib, ctx.h
    ld = N + (5 if N % 2 else 0)
    state_rows = N
    d = distances(N, S, ld, ties, seed)
    ids, rows, flags, resets, starts = scenario(N, S, ld)
    words, off, bits, n_bits = pack_bits(S, N, starts)
    d_dev = torch.from_numpy(d).to(dev())
    ids_dev, rows_dev = torch.from_numpy(ids).to(dev()), torch.from_numpy(rows).to(dev())
    flags_dev = torch.from_numpy(flags).to(dev())
    words_dev, off_dev = torch.from_numpy(words).to(dev()), torch.from_numpy(off).to(dev())
    nbytes = int(lib.mocha_path_state_bytes(h, S, state_rows))
    assert nbytes == S * 64 + S * 2 * state_rows * 8
    sw, sv = guarded(nbytes, torch.uint8, 0xAB)
    sv.zero_()                                       # a zeroed buffer is a reset state
    iw, iv = guarded(STEPS * S, torch.int32, -7)
    dw, dv = guarded(STEPS * S, torch.float32, float("nan"))
    cw, cv = guarded(STEPS * S, torch.uint8, 9)
    rw, rv = guarded(S, torch.int32, -7)
    rv.zero_()
    ref = PathStepRef(S, lam)
    ref_flags = np.zeros(S, dtype=np.int32)
    exp_i, exp_d, exp_c = [], [], []
    for t in range(STEPS):
        if t in resets:
            one = (C.c_int32 * 1)(0)
            assert lib.mocha_path_state_reset(h, ptr(sv), S, state_rows, one, 1, stream()) == 0
            ref.reset([0])
        if flags[t].any():
            rv.copy_(torch.maximum(rv, flags_dev[t]))
            ref_flags = np.maximum(ref_flags, flags[t])
        rc = lib.mocha_match_path_advance(h, ptr(sv), S, state_rows, ptr(d_dev[t]), ld, ptr(ids_dev[t]), ptr(rows_dev[t]), ptr(words_dev), n_bits,
                                          ptr(off_dev), ptr(rv), float(lam), ptr(iv[t * S:]), ptr(dv[t * S:]), ptr(cv[t * S:]), stream())
        assert rc == 0, ctx.lib.mocha_last_error(h)
        i, dd, c = ref.advance(d[t], ids[t], rows[t], start_bits=bits, bit_off=off, restart=ref_flags, limit=state_rows)
        exp_i.append(i); exp_d.append(dd); exp_c.append(c)
    torch.cuda.synchronize()
    where = (N, S, ties, lam)
    assert guards_intact(sw, nbytes, 0xAB), where
    assert guards_intact(iw, STEPS * S, -7) and guards_intact(dw, STEPS * S, float("nan")) and guards_intact(cw, STEPS * S, 9), where
    assert guards_intact(rw, S, -7), where
    got_i = iv.cpu().numpy().reshape(STEPS, S)
    got_d = dv.cpu().numpy().reshape(STEPS, S)
    got_c = cv.cpu().numpy().reshape(STEPS, S)
    exp_i, exp_d, exp_c = np.stack(exp_i), np.stack(exp_d), np.stack(exp_c)
    bad = np.argwhere(got_i != exp_i)
    assert bad.size == 0, (where, bad[:5].tolist(), got_i[tuple(bad[0])], exp_i[tuple(bad[0])])
    assert np.array_equal(got_d.view(np.uint32), exp_d.view(np.uint32)), where
    assert np.array_equal(got_c, exp_c), where
    assert np.array_equal(rv.cpu().numpy(), ref_flags), where                     # the consumed words are cleared, no other
    return exp_i, exp_c


@pytest.mark.parametrize("N", [1, 2, 1023, 1024, 1025, 5000, 16384])
def test_every_step_equals_the_restatement(ctx, N):
    for S in (1, 3, 16):
        for ties, lam in ((True, 1.0), (True, 0.0), (False, 0.37), (True, 2.0)):
            exp_i, exp_c = run(ctx, N, S, ties, lam, seed=1000 * N + 10 * S + int(lam * 4))
            if N >= 64 and lam > 0:
                assert exp_c.sum() > 0                                        # the case exercises continuations at all
            assert (exp_i[27, 0] == -1) and (exp_i[28, 0] >= 0)


def test_refusals_leave_state_and_outputs_untouched(ctx):
    lib, h = ctx.lib, ctx.h
    S, N = 2, 8
    nbytes = int(lib.mocha_path_state_bytes(h, S, N))
    sw, sv = guarded(nbytes, torch.uint8, 0xAB)
    iw, iv = guarded(S, torch.int32, -7)
    dw, dv = guarded(S, torch.float32, float("nan"))
    cw, cv = guarded(S, torch.uint8, 9)
    d = torch.ones((S, N), dtype=torch.float32, device=dev())
    ids = torch.zeros((S,), dtype=torch.int32, device=dev())
    rows = torch.full((S,), N, dtype=torch.int32, device=dev())
    good = dict(state=sv, streams=S, state_rows=N, dist=d, ld=N, ids=ids, rows=rows, lam=1.0, idx=iv)
    bad = [dict(streams=0), dict(streams=17), dict(lam=-1.0), dict(lam=float("nan")), dict(lam=float("inf")), dict(state_rows=0),
           dict(state_rows=16385), dict(state=None), dict(dist=None), dict(ids=None), dict(rows=None), dict(idx=None), dict(ld=0)]
    for kw in bad:
        a = dict(good)
        a.update(kw)
        rc = lib.mocha_match_path_advance(h, ptr(a["state"]), a["streams"], a["state_rows"], ptr(a["dist"]), a["ld"], ptr(a["ids"]), ptr(a["rows"]),
                                          None, 0, None, None, a["lam"], ptr(a["idx"]), ptr(dv), ptr(cv), stream())
        torch.cuda.synchronize()
        assert rc == ERR_ARG, kw
        assert bool((sw == 0xAB).all()) and bool((iw == -7).all()) and bool(torch.isnan(dw).all()) and bool((cw == 9).all()), kw
    assert lib.mocha_path_state_bytes(h, 0, 8) < 0 and lib.mocha_path_state_bytes(h, 17, 8) < 0
    assert lib.mocha_path_state_bytes(h, 1, 0) < 0 and lib.mocha_path_state_bytes(h, 1, 16385) < 0
    assert lib.mocha_path_state_reset(h, None, S, N, None, 0, stream()) == ERR_ARG
    two = (C.c_int32 * 1)(2)
    assert lib.mocha_path_state_reset(h, ptr(sv), S, N, two, 1, stream()) == ERR_ARG
    # dist_out, continued, the start bits and the restart words are optional
    sv.zero_()
    rc = lib.mocha_match_path_advance(h, ptr(sv), S, N, ptr(d), N, ptr(ids), ptr(rows), None, 0, None, None, 1.0, ptr(iv), None, None, stream())
    torch.cuda.synchronize()
    assert rc == 0 and iv.cpu().tolist() == [0, 0]
    assert guards_intact(sw, nbytes, 0xAB) and bool(torch.isnan(dw).all()) and bool((cw == 9).all())
