"""ctypes loader of the test-only probe of the context matcher's launchers (tests/gemm_probe/match_probe.cpp, built by
`make -C tests/gemm_probe`), the float64 restatement of every stage of the matcher and the case generators of
tests/test_match_kernels.py.  float64 is the truth, float32 on the CPU the evaluation that sizes a bound.

What a stage MEANS is taken from csrc/kernels.h and the headers of the match_*.hip files; nothing is transcribed from the kernels' text:
no lanes, no rings, no swizzles.
  bf16            round to nearest even on the uint32 bits of an fp32 value (bf16_rne); the centred copy is bf16(x (-) c), (-) in fp32
  rownorm2        sum of squares of the bf16 values
  rho (rowresid)  >= ||(x - c) - b16||: the kernel states sqrt(r2) * 1.000001 + 1e-6 sqrt(n2)
  byte image      s = max|x (-) c| / 127 (1 for the zero row), u8 = 128 + rint((x - c) / s), rho8 >= ||(x - c) - s (u8 - 128)||
  coarse score    S[z][q][n] = sum over the k of slice z of (a0 + a1)[q][k] b[n][k]; slice z = 64-k steps [z per, (z + 1) per), per = ceil(steps / ksplit)
  selection       v_n = ||b_n - c||^2 - 2 S_n; the answer is the float64 argmin of the direct-form distance, ties to the lowest row
"""
from __future__ import annotations

import ctypes as C
import os
import zlib

import numpy as np
import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "gemm_probe", "libmocha_match_probe.so")
UNSUPPORTED, BAD_ARGUMENT = -1, -2
INVALID_VALUE = 1          # hipErrorInvalidValue
QSTAT_PARTS = 4
MARGIN_BF16, MARGIN_F32 = 5e-5, 4e-6          # what do_match hands the selection (csrc/mocha_api.cpp)

_vp, _i, _ll, _f = C.c_void_p, C.c_int, C.c_longlong, C.c_float
_SIGNATURES = {
    "mp_bf16_ksplit": ([_i, _ll], _i), "mp_pass256_ksplit": ([_i, _ll], _i),
    "mp_tiled_elems": ([_ll, _i], _ll), "mp_tile32_elems": ([_ll, _i], _ll), "mp_qstat_parts": ([], _i),
    "mp_to_bf16": ([_vp, _vp, _i, _vp, _ll, _vp], _i),
    "mp_center_bf16": ([_vp, _vp, _vp, _ll, _i, _vp], _i),
    "mp_rownorm2_bf16": ([_vp, _vp, _ll, _i, _vp], _i),
    "mp_rowresid": ([_vp, _vp, _vp, _vp, _ll, _i, _vp], _i),
    "mp_to_i8": ([_vp, _vp, _vp, _vp, _vp, _ll, _i, _vp], _i),
    "mp_tile_bf16": ([_vp, _vp, _ll, _ll, _i, _vp], _i), "mp_tile32_bf16": ([_vp, _vp, _ll, _ll, _i, _vp], _i),
    "mp_match_gemm_bf16": ([_vp, _ll, _ll, _vp, _vp, _i, _ll, _i, _i, _i, _vp, _ll, _i, _vp, _vp], _i),
    "mp_match_pass256": ([_vp, _ll, _ll, _vp, _vp, _i, _ll, _i, _i, _i, _i, _vp, _ll, _vp], _i),
    "mp_match_select": ([_vp, _i, _ll, _i, _vp, _vp, _vp, _vp, _vp, _f, _i, _ll, _i, _vp, _vp, _vp], _i),
    "mp_match_select2": ([_vp, _i, _ll, _i, _vp, _vp, _vp, _vp, _vp, _vp, _f, _i, _ll, _i, _vp, _vp, _vp], _i),
}
_lib = None


def load():
    """The probe library; a missing build is an error (no fallback)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(f"{LIB_PATH} is missing: run __graft_entry__.build() (make -C tests/gemm_probe)")
        lib = C.CDLL(LIB_PATH)
        for name, (args, res) in _SIGNATURES.items():
            fn = getattr(lib, name)
            fn.argtypes, fn.restype = args, res
        _lib = lib
    return _lib


def ptr(t):
    """Device (or host) address of a tensor, 0 for None."""
    return 0 if t is None else t.data_ptr()


def rng(name):
    return np.random.Generator(np.random.PCG64(zlib.crc32(name.encode())))


# ------------------------------------------------------------------------------------------------------------------ bf16
def bf16_rne(x):
    """fp32 array -> bf16 bit patterns (uint16): round to nearest, ties to even, on the uint32 bits.  Finite inputs (no NaN handling)."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    keep, drop = u >> np.uint32(16), u & np.uint32(0xFFFF)
    up = (drop > 0x8000) | ((drop == 0x8000) & ((keep & np.uint32(1)) == 1))
    return (keep + up.astype(np.uint32)).astype(np.uint16)


def bf16_value(bits):
    """bf16 bit patterns -> the fp32 values they stand for."""
    return (np.asarray(bits).astype(np.uint32) << np.uint32(16)).view(np.float32)


def centred_bf16(x, c):
    """bf16(x (-) c): the subtraction in fp32 (correctly rounded), then RNE - both steps are correctly rounded, so bits are the condition."""
    t = np.asarray(x, np.float32) - (0 if c is None else np.asarray(c, np.float32)[None, :])
    return bf16_rne(t.astype(np.float32))


def planes2(t):
    """The two stacked bf16 query planes of an fp32 array: p0 = bf16(t), p1 = bf16(t (-) p0)."""
    p0 = bf16_rne(t)
    return p0, bf16_rne(np.asarray(t, np.float32) - bf16_value(p0))


# ------------------------------------------------------------------------------------------------------------------ family 1
CONTENTS = ("normal", "far", "centre-row", "outlier", "ties", "tiny", "small")


def contents(kind, rows, cols, r):
    """(x, centre) fp32 of one content class.
    far: rows 1e3 from the origin that cancel against the centre (x - c about 1); centre-row: row 0 IS the centre; outlier: one 1e4 value
    in every row; ties: centre 0 and every value exactly half-way between two bf16 neighbours (truncation, or ties away, shows), both
    parities of the kept bit and both signs; tiny: rows of size 1e-30 (squares leave the fp32 range); small: rows
    of size 1e-17 (the squares of x - c stay in range, those of its bf16 residual, 1e-39, are denormal)."""
    x = r.standard_normal((rows, cols), dtype=np.float32)
    c = (0.1 * r.standard_normal(cols, dtype=np.float32)).astype(np.float32)
    if kind == "far":
        c = (1e3 * np.sign(r.standard_normal(cols, dtype=np.float32)) * (1 + 0.1 * r.random(cols, dtype=np.float32))).astype(np.float32)
        x = (c[None, :] + x).astype(np.float32)
    elif kind == "centre-row":
        x[0] = c
    elif kind == "outlier":
        x[np.arange(rows), r.integers(0, cols, rows)] = 1e4
    elif kind == "ties":
        c = np.zeros(cols, np.float32)
        u = x.view(np.uint32)
        x = ((u & np.uint32(0xFFFF0000)) | np.uint32(0x8000)).view(np.float32)
    elif kind in ("tiny", "small"):
        size = np.float32(1e-30 if kind == "tiny" else 1e-17)
        x = (x * size).astype(np.float32)
        c = (c * size).astype(np.float32)
    else:
        assert kind == "normal", kind
    return np.ascontiguousarray(x, np.float32), np.ascontiguousarray(c, np.float32)


def rownorm2(bits, dtype=np.float64):
    v = bf16_value(bits).astype(dtype)
    return (v * v).sum(1, dtype=dtype)


def resid_norms(x, c, approx):
    """float64: (||(x - c) - approx||, ||x - c||) per row; approx = the values the copy stands for (float64 [rows, cols])."""
    t = x.astype(np.float64) - c.astype(np.float64)[None, :]
    return np.sqrt(((t - approx) ** 2).sum(1)), np.sqrt((t * t).sum(1))


def rho_ceiling(r64, n64):
    """The tightness bound of rowresid / to_i8: the kernels' own formula in float64, with about 100 fp32 roundings per sum."""
    return (1 + 2e-5) * (1.000001 * r64 + 1e-6 * n64)


def i8_scale(x, c):
    """fp32(max|x (-) c|) / 127 in fp32; the zero row gives scale 1."""
    t = np.abs(np.asarray(x, np.float32) - np.asarray(c, np.float32)[None, :]).astype(np.float32)
    m = t.max(1)
    return np.where(m > 0, (m / np.float32(127)).astype(np.float32), np.float32(1)).astype(np.float32)


def i8_ideal(x, c, s):
    """128 + (x - c) / s in float64, unrounded, with the scale s the kernel wrote."""
    return 128 + (x.astype(np.float64) - c.astype(np.float64)[None, :]) / s.astype(np.float64)[:, None]


# ------------------------------------------------------------------------------------------------------------------ family 2
def slices(steps, ksplit):
    """K slice z of a D = 64 steps pass, in 64-k steps [begin, end): per = ceil(steps / ksplit); slices past the end are empty."""
    per = -(-steps // ksplit)
    return [(min(z * per, steps), min((z + 1) * per, steps)) for z in range(ksplit)]


CHUNK = 16
REGIMES1 = ("normal", "index")
REGIMES2 = ("normal", "p0-zero", "p1-neg", "index")


def pass_operands(regime, Q, N, Dk, planes, r):
    """(planes [planes, Q, Dk] uint16, bank [N, Dk] uint16, kq or None).
    normal: plane 0 = bf16 of N(0, 1), plane 1 = bf16 of what plane 0 leaves; p0-zero: plane 0 all zero, plane 1 random; p1-neg: plane 1 =
    -plane 0 (every S exactly 0 only if both planes' products enter); index: each query row a single 1.0 at k(q) - in plane 1 for odd q
    when there are two - and a bank of small integers, so every sum is exact in fp32 and S[q][n] = bank[n][k(q)] in the slab that owns k(q)."""
    bank = bf16_rne(r.standard_normal((N, Dk), dtype=np.float32))
    kq = None
    if regime == "index":
        bank = bf16_rne(r.integers(-8, 9, (N, Dk)).astype(np.float32))
        kq = (np.arange(Q) * 37 + 11) % Dk if Dk % 37 else (np.arange(Q) * 41 + 11) % Dk
        pl = np.zeros((planes, Q, Dk), np.float32)
        which = (np.arange(Q) & 1) if planes == 2 else np.zeros(Q, np.int64)
        pl[which, np.arange(Q), kq] = 1.0
        P = bf16_rne(pl)
    else:
        a = r.standard_normal((Q, Dk), dtype=np.float32)
        if planes == 1:
            assert regime == "normal", regime
            P = bf16_rne(a)[None]
        elif regime == "normal":
            P = np.stack(planes2(a))
        elif regime == "p0-zero":
            P = np.stack([np.zeros((Q, Dk), np.uint16), bf16_rne(a)])
        else:
            assert regime == "p1-neg", regime
            p0 = bf16_rne(a)
            P = np.stack([p0, p0 ^ np.uint16(0x8000)])
    return np.ascontiguousarray(P), np.ascontiguousarray(bank), kq


def coarse_ref(P, bank, steps, ksplit):
    """(S64 [ksplit, Q, N] float64, S32 the same evaluated in fp32 by torch on the CPU) from the bf16 operands.
    The fp32 evaluation states its order: a slab is ONE running fp32 sum over its K range that takes CHUNK = 16 k at a time - the depth of one
    matrix instruction (32x32x16, headers of csrc/match_mfma.hip and match_pass.hip) - the low plane's 16 products, then the high plane's,
    each as one fp32 matrix product.  (torch's own product over the whole K range sums in blocks of its BLAS's choosing - pairwise at
    K = 23040, a fifth of a running sum's error, and different from one CPU to the next.)"""
    b = torch.from_numpy(bf16_value(bank))
    pl = [torch.from_numpy(bf16_value(p)) for p in P]
    a64 = sum(p.double() for p in pl)
    Q, N = pl[0].shape[0], b.shape[0]
    S64, S32 = torch.zeros((ksplit, Q, N), dtype=torch.float64), torch.zeros((ksplit, Q, N), dtype=torch.float32)
    for z, (s0, s1) in enumerate(slices(steps, ksplit)):
        if s1 > s0:
            k0, k1 = 64 * s0, 64 * s1
            S64[z] = a64[:, k0:k1] @ b[:, k0:k1].double().T
            acc = torch.zeros((Q, N), dtype=torch.float32)
            bt = b.T.contiguous()
            for k in range(k0, k1, CHUNK):
                for p in pl[::-1]:                                         # the low plane's products are the small ones
                    acc += p[:, k:k + CHUNK] @ bt[k:k + CHUNK]
            S32[z] = acc
    return S64, S32


def fold_f32(slabs):
    """The slabs added in slab order from zero in fp32 (what the selections and the ticket fold do): numpy fp32 [Q, N]."""
    acc = np.zeros(slabs.shape[1:], np.float32)
    for z in range(slabs.shape[0]):
        acc = (acc + slabs[z].astype(np.float32)).astype(np.float32)
    return acc


# ------------------------------------------------------------------------------------------------------------------ family 3
MIN_GAP = 1e-4            # relative gap in squared distance between the winner and the best other row (or exactly zero)
NEAR = 0.0025             # the winner's squared distance, in units of ||q - c||^2: the bound of the fp32 route is 1.6e-5 of that norm, so
                          # a row 1e-4 of the winner's distance behind it can only be hidden when the winner is this close


class SelectCase:
    """One authored selection problem (see build_select)."""


def _special_rows(N):
    """Rows at which a candidate or the winner sits on an edge: both ends, both sides of the register chunks (4 096, 16 384) and of the
    multiples of 64 and 128 that bound a list window."""
    s = [0, N - 1]
    for e in (64, 128, 4096, 8192, 16384, 64 * 70, 128 * 33):
        s += [e - 1, e]
    out = []
    for v in s:
        if 0 <= v < N and v not in out:
            out.append(v)
    return out


def build_select(name, *, N, D, Q, ksplit, mode, inside, dup=0, planes=1):
    """An authored selection problem.
    mode "f32": raw fp32 bank rows, raw query, margin_rel 4e-6, no query rounding (dq = 0); mode "b16": centred bf16 rows, raw query and
    the centre, margin_rel 5e-5, dq = (q (-) c) - its `planes` bf16 planes.
    Per query: a winner row at distance^2 = NEAR ||q - c||^2, `inside` (one number, or one per query) decoys a little farther (inside what the authored errors can
    hide), `dup` exact copies of the winner at HIGHER rows, and every other row of the bank far away.  inside = "all": every row of the
    bank is one and the same row.  The score slabs are written from the float64 score v_n plus an authored error e_n of 0.9 of the bound
       |e_n| <= 2 ||dq|| ||b_n - c|| + margin_rel (||q - c||^2 + ||b_n - c||^2)
    (header of csrc/match_select2.hip), sign + for the winner and its copies' lowest, - for everything else, split over `ksplit` slabs;
    `seen` is the score the kernel forms from them (slabs added in fp32 in slab order, bnorm - 2 S in fp32).  Checked here, on the CPU:
    the realised error stays inside the bound; every decoy LOOKS better than the winner; the float64 gap in squared distance between
    the winner and the best other row is exactly zero (copies) or at least MIN_GAP relative."""
    r = rng("select-" + name)
    k = SelectCase()
    k.name, k.N, k.D, k.Q, k.ksplit, k.mode = name, N, D, Q, ksplit, mode
    k.margin = MARGIN_F32 if mode == "f32" else MARGIN_BF16
    c = (0.1 * r.standard_normal(D, dtype=np.float32)).astype(np.float32)
    q = (r.standard_normal((Q, D), dtype=np.float32) + c[None, :]).astype(np.float32)
    qc32 = (q - c[None, :]).astype(np.float32)                                  # q (-) c, the subtraction every producer makes
    qc = q.astype(np.float64) - c.astype(np.float64)[None, :]
    if mode == "b16":
        left = qc32.copy()
        for _ in range(planes):
            left = (left - bf16_value(bf16_rne(left))).astype(np.float32)
        dq = np.sqrt((left.astype(np.float64) ** 2).sum(1))
    else:
        dq = np.zeros(Q)
    qn = (qc * qc).sum(1)

    # ---- the rows: far ones everywhere, then per query its winner, copies and decoys
    rows = (r.standard_normal((N, D), dtype=np.float32) + c[None, :]).astype(np.float32)
    allsame = inside == "all"
    k.winner, groups = [], []
    rel = k.margin * 2 + 2 * dq / np.sqrt(qn)                                   # about (bound of one row) / ||q - c||^2
    special = _special_rows(N)
    start = zlib.crc32(name.encode()) % len(special)
    special = special[start:] + special[:start]
    wins = []
    if not allsame:
        free = [int(v) for v in r.permutation(N) if v not in special]
        pool = special + free                                                   # winners (and their copies) first: the edge rows, from a start the name picks
        for i in range(Q):
            grp, pool = pool[:1 + dup], pool[1 + dup:]
            wins.append(grp)
        left = [v for v in pool if v in special]
        pool = [v for v in pool if v not in special]
    for i in range(Q):
        if allsame:
            break
        m = min(int(inside[i] if isinstance(inside, (list, tuple)) else inside), N - 1 - dup)
        assert m >= 0, (N, dup)
        edge, left = left[:min(2, m)], left[min(2, m):]                         # up to two decoys on edge rows, the rest anywhere
        assert len(pool) >= m - len(edge), ("the bank is too small for the queries' clusters", N, Q, m, dup)
        dec, pool = edge + pool[:m - len(edge)], pool[m - len(edge):]
        w = min(wins[i])                                                        # the winner is the LOWEST of its copies
        cp = sorted(v for v in wins[i] if v != w)
        d2 = NEAR * qn[i]
        u = r.standard_normal(D)
        rows[w] = (q[i].astype(np.float64) + u * np.sqrt(d2 / (u * u).sum())).astype(np.float32)
        for v in cp:
            rows[v] = rows[w]
        lo, hi = (2e-4 if mode == "f32" else 0.015), min(1.0, 0.6 * 1.8 * rel[i] / NEAR)
        assert hi > 1.5 * lo, (name, lo, hi)
        for v in dec:
            g = lo + (hi - lo) * r.random()
            u = r.standard_normal(D)
            rows[v] = (q[i].astype(np.float64) + u * np.sqrt(d2 * (1 + g) / (u * u).sum())).astype(np.float32)
        k.winner.append(w)
        groups.append((w, cp, dec))
    if allsame:
        u = r.standard_normal(D)
        rows[:] = (q[0].astype(np.float64) + u * np.sqrt(NEAR * qn[0] / (u * u).sum())).astype(np.float32)[None, :]
        k.winner = [0] * Q
        groups = [(0, list(range(1, N)), [])] * Q

    if mode == "b16":
        k.bank16 = centred_bf16(rows, c)
        bc = bf16_value(k.bank16).astype(np.float64)                           # the rows the kernel searches
        k.bank = None
        diff32 = lambda i: (qc32[i][None, :] - bf16_value(k.bank16)).astype(np.float32)
        diff64 = lambda i: qc32[i].astype(np.float64)[None, :] - bc
    else:
        k.bank, k.bank16 = rows, None
        bc = rows.astype(np.float64) - c.astype(np.float64)[None, :]
        diff32 = lambda i: (q[i][None, :] - rows).astype(np.float32)
        diff64 = lambda i: q[i].astype(np.float64)[None, :] - rows.astype(np.float64)
    bn = (bc * bc).sum(1)
    k.bnorm = bn.astype(np.float32)
    k.query, k.centre = q, c

    # ---- exact distances, the answer, the gap condition
    k.d2_64 = np.stack([(diff64(i) ** 2).sum(1) for i in range(Q)])
    k.d2_32 = np.stack([(diff32(i) ** 2).sum(1, dtype=np.float32) for i in range(Q)])
    k.answer = k.d2_64.argmin(1)                                                # numpy: the first of equal minima
    k.gap = []
    for i in range(Q):
        assert k.answer[i] == k.winner[i], (name, i, int(k.answer[i]), k.winner[i])
        best = k.d2_64[i, k.answer[i]]
        others = np.delete(k.d2_64[i], k.answer[i])
        g = (others.min() - best) / best if N > 1 else np.inf
        assert g == 0.0 or g >= MIN_GAP, (name, i, g)
        if g == 0.0:
            assert dup or allsame, (name, i)
        k.gap.append(g)

    # ---- the authored scores.  b16: the coarse pass's operand is the query's planes, so the exact score is taken on q (-) c as well
    qv = qc32.astype(np.float64) if mode == "b16" else qc
    qn_k = (qv * qv).sum(1)
    v64 = bn[None, :] - 2 * (qv @ bc.T)                                         # [Q, N]
    bound = 2 * dq[:, None] * np.sqrt(bn)[None, :] + k.margin * (qn_k[:, None] + bn[None, :])
    sign = -np.ones((Q, N))
    for i, (w, cp, dec) in enumerate(groups):
        sign[i, w] = 1.0
    target = v64 + 0.9 * sign * bound
    Stot = (k.bnorm.astype(np.float64)[None, :] - target) / 2
    wz = r.random((ksplit, Q, 1)) + 0.25
    wz /= wz.sum(0, keepdims=True)
    k.S = (Stot[None] * wz).astype(np.float32)                                  # [ksplit, Q, N]
    k.seen = (k.bnorm[None, :] - np.float32(2) * fold_f32(k.S)).astype(np.float32)
    k.v64, k.bound = v64, bound
    err = np.abs(k.seen.astype(np.float64) - v64)
    assert (err <= bound).all(), (name, float((err / bound).max()))
    assert (err >= 0.8 * bound).all(), (name, float((err / bound).min()))       # and really sits at its edge
    for i, (w, cp, dec) in enumerate(groups):
        if len(dec) + len(cp):
            assert (k.seen[i, np.array(list(dec) + list(cp))] < k.seen[i, w]).all(), (name, i, "a decoy does not look better than the winner")

    # ---- qstat: {||q - c||^2, ||dq||^2} spread over the four parts, which the consumer adds in part order
    parts = r.random((Q, QSTAT_PARTS, 1)) + 0.1
    parts /= parts.sum(1, keepdims=True)
    k.qstat = (np.stack([qn_k, dq * dq], 1)[:, None, :] * parts).astype(np.float32)      # [Q, parts, 2]
    k.inside = [len(g[2]) + len(g[1]) for g in groups]
    k.groups = groups
    return k


def candidates(k, i, rel=1.0):
    """Rows of query i the candidate rule keeps, in float64 on the scores the kernel sees (threshold scaled by `rel`)."""
    qs = k.qstat.astype(np.float64).sum(1)
    qn, dq = qs[i, 0], np.sqrt(qs[i, 1]) if k.mode == "b16" else 0.0
    s = k.seen[i].astype(np.float64)
    m = int(np.argmin(s))
    bn = k.bnorm.astype(np.float64)
    thr = s[m] + rel * (2 * dq * (np.sqrt(bn) + np.sqrt(bn[m])) + k.margin * (2 * qn + bn + bn[m]))
    return np.flatnonzero(s <= thr)
