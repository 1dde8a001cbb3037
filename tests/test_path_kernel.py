"""Coherent context matching on the MI355X through the C ABI alone (run with -m gpu): mocha_match_dist_matrix and mocha_match_path, with
guard words around every output.

Matrix: every entry must be, bit for bit, the distance mocha_match_topk reports for that (query, row) - checked against banks made of
slices of at most 64 rows (k = the slice's rows: the existing library's own answer for every entry, with its row order).
Path: the device path, dist and continued must equal tests/path_ref.py on the same fp32 matrix, every entry; thread t of the forward
kernel owns the c = ceil(N / 1024) columns [t c, (t + 1) c), so the planted ties sit across columns 63 | 64, c 5 - 1 | c 5 and 64 c - 1 | 64 c.
Planted path at the real width D = 23 040: the matrix kernel followed by the path kernel returns the planted rows."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from mocha_sigasia2023_amd import ContextBank, Generator, weights  # noqa: E402
from path_ref import path_ref  # noqa: E402

pytestmark = pytest.mark.gpu
D = 90 * 256
G = 64                                   # guard words on either side of an output
ERR_ARG = -1
SIZES = [3, 16, 17, 200, 64]
RANGES = [(0, 300), (3, 16), (19, 17), (35, 1), (5, 231)]
QS = (1, 8, 9, 16, 17, 33)
DUP = (148, 149)                         # an exact duplicate pair of bank rows; query 32 sits on it


def dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def model():
    sd = weights.synthetic_state_dict(1777, 1.0, "mixamo")
    return Generator(layout="mixamo", device=dev()).load_state_dict(sd).eval()


def guarded(n, dtype, fill):
    """A device buffer of n elements with G guard elements on either side -> (whole, view of the n)."""
    whole = torch.full((n + 2 * G,), fill, dtype=dtype, device=dev())
    return whole, whole[G:G + n]


def guards_intact(whole, n, fill):
    w = whole.cpu()
    f = torch.tensor(fill, dtype=w.dtype)
    same = (lambda a: torch.isnan(a).all()) if (w.dtype.is_floating_point and np.isnan(fill)) else (lambda a: (a == f).all())
    return bool(same(w[:G])) and bool(same(w[G + n:]))


def i32(values):
    return (C.c_int32 * max(len(values), 1))(*[int(v) for v in values])


def stream():
    return C.c_void_p(torch.cuda.current_stream(dev()).cuda_stream)


def ptr(t):
    return C.c_void_p(t.data_ptr())


# ------------------------------------------------------------------------------------------------------------ the matrix
@pytest.fixture(scope="module")
def matrix_data(model):
    rng = np.random.default_rng(35)
    N = sum(SIZES)
    bank = rng.standard_normal((N, D), dtype=np.float32)
    bank[DUP[1]] = bank[DUP[0]]
    q = rng.standard_normal((33, D), dtype=np.float32)
    q[32] = bank[DUP[0]] + 0.02 * rng.standard_normal(D, dtype=np.float32)
    bank_t, q_t = torch.from_numpy(bank).to(dev()), torch.from_numpy(q).to(dev())
    enc = torch.zeros((N, 90, 256), dtype=torch.float32, device=dev())
    # the existing library's answer for every entry the ranges cover: mocha_match_topk on banks of <= 64 rows, all 33 queries at once
    ref = {}
    for r0, n in RANGES:
        for s0 in range(r0, r0 + n, 64):
            s1 = min(s0 + 64, r0 + n)
            if (s0, s1) in ref:
                continue
            e1 = max(s1, s0 + 2)                                          # (a one-row range: a two-row bank, its first row's entries kept)
            ContextBank(model, bank_t[s0:e1].contiguous(), enc[s0:e1], dec_cache=False)
            k = e1 - s0
            idx = torch.empty((33, k), dtype=torch.int32, device=dev())
            dist = torch.empty((33, k), dtype=torch.float32, device=dev())
            model._ctx.call("mocha_match_topk", ptr(q_t), 33, k, ptr(idx), ptr(dist), stream())
            dist, idx = dist.cpu().numpy(), idx.cpu().numpy()
            if e1 != s1:
                keep = idx == 0
                dist, idx = dist[keep].reshape(33, 1), idx[keep].reshape(33, 1)
            ref[(s0, s1)] = (dist, idx)
    full = ContextBank(model, bank_t, enc, dec_cache=False)
    hard = full.query(q_t, k=1)[1][:, 0].cpu().numpy()
    return full, bank_t, q_t, ref, hard


def dist_matrix(model, q_t, Q, r0, n, ld):
    whole, view = guarded(Q * ld, torch.float32, float("nan"))
    model._ctx.call("mocha_match_dist_matrix", ptr(q_t), Q, C.c_int64(r0), C.c_int64(n), ptr(view), C.c_int64(ld), stream())
    torch.cuda.synchronize()
    assert guards_intact(whole, Q * ld, float("nan"))
    m = view.cpu().numpy().reshape(Q, ld)
    assert np.isnan(m[:, n:]).all(), "columns past `rows` were written"
    return m[:, :n]


@pytest.mark.parametrize("rng_", RANGES, ids=[f"rows{a}+{b}" for a, b in RANGES])
def test_matrix_entries_are_topk_distances_bit_for_bit(model, matrix_data, rng_):
    full, bank_t, q_t, ref, _ = matrix_data
    full.activate()
    r0, n = rng_
    for Q in QS:
        for ld in (n, n + 3):
            m = dist_matrix(model, q_t, Q, r0, n, ld)
            for s0 in range(r0, r0 + n, 64):
                s1 = min(s0 + 64, r0 + n)
                rd, ri = ref[(s0, s1)]
                sub = m[:, s0 - r0:s1 - r0]
                for i in range(Q):
                    assert sorted(ri[i].tolist()) == list(range(s1 - s0))
                    got = sub[i][ri[i]]                                    # the matrix entries in the library's row order
                    assert np.array_equal(got.view(np.uint32), rd[i].view(np.uint32)), (Q, ld, s0, i)
                    # ... which is the order of (distance, row): sorting the matrix's own entries gives the same rows
                    order = np.lexsort((np.arange(s1 - s0), sub[i]))
                    assert np.array_equal(order, ri[i]), (Q, ld, s0, i)


def test_matrix_argmin_is_the_hard_match(model, matrix_data):
    full, bank_t, q_t, ref, hard = matrix_data
    full.activate()
    m = dist_matrix(model, q_t, 33, 0, 300, 300)
    assert np.array_equal(m.argmin(1), hard)
    assert hard[32] == DUP[0] and m[32, DUP[0]] == m[32, DUP[1]]           # the duplicate pair: the lower row


def test_matrix_refusals(model, matrix_data):
    full, bank_t, q_t, _, _ = matrix_data
    full.activate()
    lib, h = model._ctx.lib, model._ctx.h
    whole, view = guarded(64, torch.float32, float("nan"))
    for (Q, r0, n, ld, qp, dp) in ((2, 0, 0, 4, q_t, view), (2, 299, 2, 4, q_t, view), (2, -1, 2, 4, q_t, view), (2, 0, 4, 3, q_t, view),
                                   (-1, 0, 4, 4, q_t, view), (2, 0, 4, 4, None, view), (2, 0, 4, 4, q_t, None)):
        rc = lib.mocha_match_dist_matrix(h, ptr(qp) if qp is not None else None, Q, r0, n, ptr(dp) if dp is not None else None, ld, stream())
        assert rc == ERR_ARG, (Q, r0, n, ld)
    assert lib.mocha_match_dist_matrix(h, ptr(q_t), 0, 0, 4, ptr(view), 4, stream()) == 0
    torch.cuda.synchronize()
    assert torch.isnan(whole).all()


# ------------------------------------------------------------------------------------------------------------ the path
def run_path(model, d_dev, Q, N, ld, seq, bstarts, lam):
    """mocha_match_path -> (rc, path, dist, continued) with the guards checked."""
    pw, pv = guarded(Q, torch.int32, -7)
    dw, dv = guarded(Q, torch.float32, float("nan"))
    cw, cv = guarded(Q, torch.uint8, 9)
    lib, h = model._ctx.lib, model._ctx.h
    rc = lib.mocha_match_path(h, ptr(d_dev), Q, N, ld, i32(seq), len(seq) - 1, i32(bstarts) if bstarts else None, len(bstarts), float(lam),
                              ptr(pv), ptr(dv), ptr(cv), stream())
    torch.cuda.synchronize()
    assert guards_intact(pw, Q, -7) and guards_intact(dw, Q, float("nan")) and guards_intact(cw, Q, 9)
    return rc, pv.cpu().numpy(), dv.cpu().numpy(), cv.cpu().numpy()


def crafted(N, kind):
    """(96, ld) fp32 host matrix whose first N columns count."""
    rng = np.random.default_rng(7 * N + kind)
    ld = N + 5 if kind == 2 else N
    d = np.full((96, ld), np.nan, dtype=np.float32)
    if kind == 1:
        m = rng.integers(1, 5, (96, N)).astype(np.float32)
        c = (N + 1023) // 1024
        # a row minimum that occurs twice: across the wave boundary 63 | 64, across two threads' columns, and across a wave's last thread
        # and the next wave's first - in the windows that start a sequence (R = d there), and once more in the middle
        for row, b in ((0, 64), (1, 5 * c), (3, 64 * c), (40, 64), (41, 5 * c)):
            if b < N:
                m[row, b - 1] = m[row, b] = 0
        d[:, :N] = m
    else:
        d[:, :N] = rng.uniform(1.0, 2.0, (96, N)).astype(np.float32)
    return d, ld


@pytest.mark.parametrize("N", [1, 2, 63, 64, 65, 1023, 1024, 1025, 2049, 16384])
def test_path_equals_the_restatement(model, N):
    bstarts = sorted(set(b for b in (64, 1024, N - 1) if 0 <= b < N))
    for kind in (0, 1, 2):
        d, ld = crafted(N, kind)
        d_dev = torch.from_numpy(d).to(dev())
        for Q, seq in ((1, [0, 1]), (2, [0, 2]), (96, [0, 96]), (96, [0, 1, 3, 96])):
            for lam in (0.0, 0.05, 1.0, 1e6):
                for bs in ([], bstarts):
                    if kind == 2 and (lam in (0.05, 1e6) or not bs):
                        continue                                           # the leading dimension does not interact with these
                    rc, path, dist, cont = run_path(model, d_dev, Q, N, ld, seq, bs, lam)
                    assert rc == 0
                    rp, rd, rcont = path_ref(d[:Q, :N], lam, seq_starts=seq, bank_starts=bs)
                    where = (N, kind, Q, len(seq), lam, bs)
                    assert np.array_equal(path, rp), where
                    assert np.array_equal(dist.view(np.uint32), rd.view(np.uint32)), where
                    assert np.array_equal(cont, rcont), where


def test_path_refusals_leave_outputs_untouched(model):
    lib, h = model._ctx.lib, model._ctx.h
    d_dev = torch.ones((2, 16385), dtype=torch.float32, device=dev())
    rc, path, dist, cont = run_path(model, d_dev, 2, 16385, 16385, [0, 2], [], 1.0)
    assert rc == ERR_ARG
    assert (path == -7).all() and np.isnan(dist).all() and (cont == 9).all()
    d_dev = torch.ones((4, 8), dtype=torch.float32, device=dev())
    bad = [dict(lam=-1.0), dict(lam=float("nan")), dict(lam=float("inf")), dict(seq=[1, 4]), dict(seq=[0, 3]), dict(seq=[0, 2, 2, 4]),
           dict(seq=[0, 3, 2, 4]), dict(bs=[8]), dict(bs=[-1]), dict(bs=[3, 2]), dict(ld=7), dict(Q=-1)]
    for kw in bad:
        a = dict(Q=4, N=8, ld=8, seq=[0, 4], bs=[], lam=1.0)
        a.update(kw)
        pw, pv = guarded(4, torch.int32, -7)
        rc = lib.mocha_match_path(h, ptr(d_dev), a["Q"], a["N"], a["ld"], i32(a["seq"]), len(a["seq"]) - 1, i32(a["bs"]) if a["bs"] else None,
                                  len(a["bs"]), a["lam"], ptr(pv), None, None, stream())
        torch.cuda.synchronize()
        assert rc == ERR_ARG and bool((pw == -7).all()), kw
    assert lib.mocha_match_path(h, None, 4, 8, 8, i32([0, 4]), 1, None, 0, 1.0, ptr(pv), None, None, stream()) == ERR_ARG
    assert lib.mocha_match_path(h, ptr(d_dev), 4, 8, 8, i32([0, 4]), 1, None, 0, 1.0, None, None, None, stream()) == ERR_ARG
    assert lib.mocha_match_path(h, ptr(d_dev), 0, 8, 8, None, 0, None, 0, 1.0, None, None, None, stream()) == 0
    # dist_out and continued are optional
    rc = lib.mocha_match_path(h, ptr(d_dev), 4, 8, 8, i32([0, 4]), 1, None, 0, 1.0, ptr(pv), None, None, stream())
    torch.cuda.synchronize()
    assert rc == 0 and pv.cpu().tolist() == [0, 1, 2, 3]


# ------------------------------------------------------------------------------------------------------------ planted path, real width
PLANTED = np.r_[100:140, 20:60]


@pytest.fixture(scope="module")
def planted():
    rng = np.random.default_rng(35)
    bank = np.cumsum(0.1 * rng.standard_normal((300, D)), 0).astype(np.float32)
    q = (bank[PLANTED] + 6.66 * rng.standard_normal((80, D))).astype(np.float32)
    b, qq = bank.astype(np.float64), q.astype(np.float64)
    d = np.sqrt((qq * qq).sum(1)[:, None] + (b * b).sum(1)[None] - 2.0 * qq @ b.T)
    # the fixture's own precondition, in float64 on the host: the restatement returns the planted rows, and again under three sign
    # patterns of a 1e-5 relative perturbation of every distance (the margin tests/test_soft_match.py relies on for fp32 not reordering
    # distances); the independent arg-min does not
    assert int((d.argmin(1) == PLANTED).sum()) < 80
    for lam in (0.5, 1.0, 2.0):
        assert np.array_equal(path_ref(d, lam)[0], PLANTED)
        for s in range(3):
            sign = np.random.default_rng(100 + s).choice([-1.0, 1.0], d.shape)
            assert np.array_equal(path_ref(d * (1.0 + 1e-5 * sign), lam)[0], PLANTED)
    return bank, q


def test_planted_path_at_the_real_width(model, planted):
    bank, q = planted
    bank_t, q_t = torch.from_numpy(bank).to(dev()), torch.from_numpy(q).to(dev())
    ContextBank(model, bank_t, torch.zeros((300, 90, 256), dtype=torch.float32, device=dev()), dec_cache=False)
    d_dev = torch.empty((80, 300), dtype=torch.float32, device=dev())
    model._ctx.call("mocha_match_dist_matrix", ptr(q_t), 80, C.c_int64(0), C.c_int64(300), ptr(d_dev), C.c_int64(300), stream())
    for lam in (0.5, 1.0, 2.0):
        rc, path, dist, cont = run_path(model, d_dev, 80, 300, 300, [0, 80], [], lam)
        assert rc == 0
        assert np.array_equal(path, PLANTED), lam
        assert int(cont.sum()) == 78 and cont[0] == 0 and cont[40] == 0        # one non-continuation after the first window
        assert np.array_equal(dist, d_dev.cpu().numpy()[np.arange(80), PLANTED])
