"""ctypes loader of the test-only probe of the few-query scans and the segmented matchers (tests/gemm_probe/scan_probe.cpp, built by
`make -C tests/gemm_probe`) and the float64 restatement of what they compute, for tests/test_scan_kernels.py.  Every restatement is generic
over the NumPy dtype: float64 is the truth, the same code in float32 the CPU evaluation that sizes a bound.

What an operation MEANS is taken from csrc/kernels.h and the headers of match_stream.hip, match_scan8.hip, match_segmented.hip and
match_seg_topk.hip; nothing is transcribed from the kernels' text: no lanes, no chunks, no slices.
  distance        d2[q][n] = sum_d (q_d - b_d)^2, the DIRECT form; what is reported is sqrt(d2)
  key             order-preserving bits of the fp32 d2 in the high word, the row in the low word: smaller key = nearer, ties to the lower row
  1-NN / k-NN     the k smallest keys, ascending; a bank (segment) of fewer than k rows: -1 / +inf for the missing ones
  refine rule     coarse d_n = sqrt(max(key value, 0)), m = the row of the smallest key; row n is re-evaluated exactly iff n == m or
                  d_n - rho_n - 2e-5 d_n <= d_m + rho_m + 2e-5 d_m; a NaN key never qualifies; no finite key at all: nothing is excluded
  plan            blocks in segment order, the queries of a segment in input order, 8 per block, an id outside [0, S) in no block
  soft weights    softmax_j(-dist_j / temperature) over the neighbours present, 0 for the others; mocha_gather_blend scales, then subtracts
                  the largest; the soft matcher subtracts the smallest distance, then scales
  blend           sum_j w_j enc[row_j], j ascending
"""
from __future__ import annotations

import ctypes as C
import os
import zlib

import numpy as np

from match_ref import bf16_rne, bf16_value, ptr, rng  # noqa: F401  (one bf16, one seeding rule for both files)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "gemm_probe", "libmocha_scan_probe.so")
UNSUPPORTED, BAD_ARGUMENT = -1, -2
INVALID_VALUE = 1          # hipErrorInvalidValue
CHUNK_F32, CHUNK_BF16, CHUNK_I8 = 1280, 1536, 2560      # csrc/match_stream_body.h, match_scan8.hip: D must be a multiple
ROWS_PER_WG = 16                                         # rows a scan workgroup owns: one per-workgroup minimum each
RF_SPLIT, RF_CAP, RF_KPT_ROWS = 64, 4096, 2048           # the refine: slices per query, rows of an index window, rows a slice holds in registers
S8_DEGENERATE = 12
NOKEY = np.uint64(0xFFFFFFFFFFFFFFFF)

_vp, _i, _ll, _f = C.c_void_p, C.c_int, C.c_longlong, C.c_float
_SIGNATURES = {
    "sp_stream_scratch": ([_i, _ll], _ll), "sp_scan16_scratch_words": ([_ll], _ll), "sp_scan16_head_words": ([], _ll),
    "sp_scan8_mode_word": ([], _ll), "sp_seg_scratch_words": ([_i, _ll], _ll), "sp_seg_plan_ints": ([_i, _i], _ll),
    "sp_seg_keys_words": ([_ll], _ll), "sp_seg_max_q": ([], _i), "sp_seg_topk_q": ([], _i), "sp_seg_topk_max_k": ([], _i),
    "sp_match_stream": ([_vp, _i, _vp, _i, _ll, _i, _vp, _ll, _vp, _vp, _vp], _i),
    "sp_match_topk": ([_vp, _i, _vp, _i, _ll, _i, _i, _vp, _ll, _vp, _vp, _vp], _i),
    "sp_gather_blend": ([_vp, _vp, _vp, _f, _vp, _i, _i, _i, _ll, _vp], _i),
    "sp_gather_rows": ([_vp, _vp, _vp, _i, _i, _ll, _vp], _i),
    "sp_match_scan16": ([_vp, _vp, _vp, _vp, _vp, _i, _ll, _i, _vp, _ll, _vp, _vp, _vp], _i),
    "sp_match_refine": ([_vp, _vp, _i, _vp, _vp, _vp, _vp, _vp, _i, _ll, _i, _vp, _vp, _vp, _ll, _vp], _i),
    "sp_match_scan8": ([_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _ll, _i, _vp, _ll, _vp, _vp, _vp], _i),
    "sp_seg_plan": ([_vp, _i, _i, _vp, _ll, _vp], _i),
    "sp_match_segmented": ([_vp, _i, _ll, _vp, _vp, _i, _vp, _i, _ll, _i, _vp, _ll, _vp, _ll, _vp, _vp, _vp, _vp], _i),
    "sp_match_seg_topk": ([_vp, _i, _ll, _vp, _vp, _i, _vp, _i, _ll, _i, _vp, _ll, _vp, _ll, _vp, _i, _f, _vp, _vp, _vp, _vp, _vp, _vp], _i),
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


# ------------------------------------------------------------------------------------------------------------------ distances and keys
def dist2(q, bank, dtype=np.float64):
    """[Q, N] squared distances in the direct form, every operation in `dtype` (the operands are fp32 values: the conversion is exact)."""
    q, bank = np.asarray(q).astype(dtype), np.asarray(bank).astype(dtype)
    out = np.empty((q.shape[0], bank.shape[0]), dtype)
    for i in range(q.shape[0]):
        d = bank - q[i][None, :]
        out[i] = (d * d).sum(1, dtype=dtype)
    return out


def pack_key(v, row):
    """uint64 keys of fp32 values v and rows: the value's bits with the sign bit set (v >= 0 or +NaN) or all bits flipped (negative), << 32 | row."""
    u = np.ascontiguousarray(v, dtype=np.float32).view(np.uint32)
    hi = np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint64)
    return (hi << np.uint64(32)) | np.asarray(row).astype(np.uint64)


def unpack_key(k):
    """(fp32 value, row) of uint64 keys: pack_key's inverse."""
    k = np.asarray(k, dtype=np.uint64)
    hi = (k >> np.uint64(32)).astype(np.uint32)
    u = np.where(hi & np.uint32(0x80000000), hi & np.uint32(0x7FFFFFFF), ~hi).astype(np.uint32)
    return u.view(np.float32), (k & np.uint64(0xFFFFFFFF)).astype(np.int64)


def knn(d2, k):
    """(idx [Q, k] int64, d2 of them [Q, k]) of the k smallest per row, ascending, ties to the lower row; -1 / +inf where there are fewer."""
    d2 = np.asarray(d2)
    Q, N = d2.shape
    idx = np.full((Q, k), -1, np.int64)
    val = np.full((Q, k), np.inf, d2.dtype)
    for i in range(Q):
        best = sorted(range(N), key=lambda n: (d2[i, n], n))[:k]
        idx[i, :len(best)] = best
        val[i, :len(best)] = d2[i, best]
    return idx, val


def nn(d2):
    idx, val = knn(d2, 1)
    return idx[:, 0], val[:, 0]


# ------------------------------------------------------------------------------------------------------------------ the refine's rule
def refine_candidates(keys, rho, dtype=np.float64):
    """Rows of ONE query the rule keeps, ascending, from its uint64 keys [N] and the residual bounds rho [N]."""
    v, _ = unpack_key(keys)
    v = v.astype(dtype)
    finite = np.isfinite(v)
    rho = np.asarray(rho).astype(dtype)
    N = len(v)
    if not finite.any():
        return np.arange(N)
    m = int(np.argmin(np.asarray(keys, dtype=np.uint64)))
    d = np.sqrt(np.maximum(np.where(np.isnan(v), 0, v), 0))
    eps = dtype(2e-5)
    hi = d[m] + rho[m] + eps * d[m]
    keep = (d - rho - eps * d <= hi) & ~np.isnan(v)
    keep[m] = True
    return np.flatnonzero(keep)


def wg_minima(keys):
    """What the scan leaves beside the keys [Q, N]: the smallest key of every 16 rows, [Q, ceil(N / 16)]."""
    keys = np.asarray(keys, dtype=np.uint64)
    Q, N = keys.shape
    n = -(-N // ROWS_PER_WG)
    pad = np.full((Q, n * ROWS_PER_WG), NOKEY, np.uint64)
    pad[:, :N] = keys
    return pad.reshape(Q, n, ROWS_PER_WG).min(2)


# ------------------------------------------------------------------------------------------------------------------ the plan
def blocks_bound(Q, S):
    """An upper bound of the block count known on the host: sum_s ceil(c_s / 8) <= (Q + 7 min(S, Q)) / 8, and <= Q."""
    return min((Q + 7 * min(S, Q)) // 8, Q)


def plan(seg, S):
    """[(segment, [query, ...]), ...]: segments ascending, the queries of a segment in input order, at most 8 per block."""
    members = {}
    for q, v in enumerate(seg):
        if 0 <= int(v) < S:
            members.setdefault(int(v), []).append(q)
    out = []
    for s in sorted(members):
        out += [(s, members[s][i:i + 8]) for i in range(0, len(members[s]), 8)]
    return out


# ------------------------------------------------------------------------------------------------------------------ weights and blends
def _softmax(x, present, exp):
    w = np.where(present, exp(np.where(present, x, 0)), 0).astype(x.dtype)
    s = w.sum(-1, keepdims=True, dtype=x.dtype)
    return np.where(s > 0, w / np.where(s > 0, s, 1), 0).astype(x.dtype)


def weights_scaled(dist, temperature, present, dtype=np.float64, exp=np.exp):
    """mocha_gather_blend's form: x_j = -dist_j * (1 / temperature), the largest x subtracted, exponentials, normalised over the present."""
    d = np.asarray(dist).astype(dtype)
    x = -d * (dtype(1) / dtype(np.float32(temperature)))
    x = np.where(present, x, -np.inf)
    mx = x.max(-1, keepdims=True)
    return _softmax(np.where(present, x - np.where(np.isfinite(mx), mx, 0), 0).astype(dtype), present, exp)


def weights_diff(dist, temperature, present, dtype=np.float64, exp=np.exp):
    """The soft matcher's form: x_j = (dmin - dist_j) * (1 / temperature), the difference BEFORE the scaling."""
    d = np.asarray(dist).astype(dtype)
    dmin = np.where(present, d, np.inf).min(-1, keepdims=True)
    x = (np.where(np.isfinite(dmin), dmin, 0) - np.where(present, d, 0)) * (dtype(1) / dtype(np.float32(temperature)))
    return _softmax(x.astype(dtype), present, exp)


def exp_2ulp(x):
    """An exponential that is wrong by 2 ulp of its fp32 result, alternately up and down: the yardstick of a FAST exponential."""
    y = np.exp(x)
    sign = np.where((np.arange(y.size).reshape(y.shape) & 1) == 0, 1.0, -1.0)
    return (y + sign * 2 * np.spacing(y.astype(np.float32)).astype(y.dtype)).astype(y.dtype)


def blend(w, rows, enc, dtype=np.float64):
    """[Q, cols]: sum_j w[q][j] enc[rows[q][j]] over the rows >= 0, j ascending, every product and sum in `dtype`."""
    w, enc = np.asarray(w).astype(dtype), np.asarray(enc).astype(dtype)
    out = np.zeros((w.shape[0], enc.shape[1]), dtype)
    for q in range(w.shape[0]):
        for j in range(w.shape[1]):
            if rows[q][j] >= 0:
                out[q] = out[q] + (w[q, j] * enc[int(rows[q][j])]).astype(dtype)
    return out


# ------------------------------------------------------------------------------------------------------------------ the segmented search
def seg_search(q, bank, seg, seg_start, k, dtype=np.float64):
    """Per query the k nearest rows of its OWN segment: (local idx [Q, k], global row [Q, k], d2 [Q, k]); an id outside [0, S), or a
    missing neighbour: -1 / -1 / +inf."""
    Q, S = len(seg), len(seg_start) - 1
    idx, g, val = np.full((Q, k), -1, np.int64), np.full((Q, k), -1, np.int64), np.full((Q, k), np.inf, dtype)
    for i in range(Q):
        s = int(seg[i])
        if not 0 <= s < S:
            continue
        lo, hi = int(seg_start[s]), int(seg_start[s + 1])
        li, lv = knn(dist2(q[i:i + 1], bank[lo:hi], dtype), k)
        idx[i], val[i] = li[0], lv[0]
        g[i] = np.where(li[0] >= 0, li[0] + lo, -1)
    return idx, g, val


# ------------------------------------------------------------------------------------------------------------------ authored banks
MIN_GAP = 1e-4            # relative gap in d2 between two rows a result must order (or exactly zero: bit-identical copies); family 3's figure
KMAX = 8


class Case:
    """One authored problem (build_bank, build_segments, build_refine)."""


def _shells(r, anchor, n, D, spacing, s0):
    """n fp32 rows around `anchor` at squared distances s0 * D * (1 + spacing)^rank, rank 0 .. n - 1: the stated factor between decoys."""
    u = r.standard_normal((n, D))
    u /= np.sqrt((u * u).sum(1, keepdims=True))
    s = np.sqrt(s0 * D * (1 + spacing) ** np.arange(n))
    return (anchor.astype(np.float64)[None, :] + u * s[:, None]).astype(np.float32)


def special_rows(N):
    """Rows where a winner sits on an edge: both ends, both sides of the first 16-row workgroup bound, the first and the last row of the
    last (ragged) workgroup."""
    last = (N - 1) // ROWS_PER_WG * ROWS_PER_WG
    out = []
    for v in (0, N - 1, ROWS_PER_WG - 1, ROWS_PER_WG, ROWS_PER_WG + 1, last, last - 1):
        if 0 <= v < N and v not in out:
            out.append(v)
    return out


def gaps_ok(d2, rows_bits, depth):
    """The gap condition on float64 distances d2 [Q, N]: any two of the `depth` + 1 nearest rows of a query (and the winner against
    everything) differ by at least MIN_GAP relative, or are bit-identical rows.  Returns the smallest nonzero relative gap, or None when
    the condition fails."""
    worst = np.inf
    for i in range(d2.shape[0]):
        order = sorted(range(d2.shape[1]), key=lambda n: (d2[i, n], n))[:depth + 1]
        for a, b in zip(order[:-1], order[1:]):
            g = (d2[i, b] - d2[i, a]) / max(d2[i, b], 1e-300)
            if g == 0.0 and np.array_equal(rows_bits[a], rows_bits[b]):
                continue
            if not g >= MIN_GAP:
                return None
            worst = min(worst, g)
    return worst


def build_bank(name, N, D, Q, bf16, spacing=0.1, copies=False):
    """A bank of N rows and Q queries for the scans.  G = clamp(N // 9, 1, Q) anchors far apart (N(0, 1) vectors, squared distance about
    2 D); the rows are dealt to the anchors in turn and sit on shells around their anchor at squared distances 0.01 D (1 + spacing)^rank;
    query i is its anchor (i mod G) plus noise of 1e-3 of the first shell's radius: the winner is the anchor's rank-0 row (query = that row +
    noise of the shell's radius), its decoys the factor (1 + spacing) farther each, everything else about 200 times farther.  Anchor 0's
    rank-0 row sits on an edge row the name picks (special_rows); copies: its rank-1 row is a bit-identical copy of the rank-0 row, at a
    HIGHER row, in the same wave, the next wave or the next workgroup as the bank allows.
    bf16: the bank is the centred bf16 copy (bank16 bits; `values` what they stand for), the scan's operand the centred queries qc; the fp32
    rows, the centre and rho (an upper bound of the copy's residual norm, from float64) are kept for the exact re-rank.
    d2_64 / d2_32: the direct form on the operands the scan sees, in float64 and in fp32; x_ for the fp32 rows and raw queries."""
    r = rng("scan-bank-" + name)
    k = Case()
    k.name, k.N, k.D, k.Q, k.bf16 = name, N, D, Q, bf16
    G = max(1, min(N // (KMAX + 1), Q))
    c = (0.1 * r.standard_normal(D, dtype=np.float32)).astype(np.float32)
    anchors = r.standard_normal((G, D), dtype=np.float32) + c[None, :]
    sp = special_rows(N)
    first = sp[zlib.crc32(name.encode()) % len(sp)]
    if copies and N > 1:
        first = min(first, N - 2)
    slots = [first] + [int(v) for v in r.permutation(N) if v != first]
    twin = None
    if copies and N > 1:
        step = (ROWS_PER_WG, 4, 1)[zlib.crc32(name.encode()) % 3]              # next workgroup, next wave, same wave
        twin = first + step if first + step < N else first + 1
        slots.remove(twin)
        slots.insert(G, twin)                                                   # anchor 0's rank-1 slot
    rows = np.empty((N, D), np.float32)
    k.group = [slots[g::G] for g in range(G)]                                   # rows of anchor g, by rank
    for g in range(G):
        rows[k.group[g]] = _shells(r, anchors[g], len(k.group[g]), D, spacing, 0.01)
    if twin is not None:
        rows[twin] = rows[first]
    k.twin = twin
    s0 = np.sqrt(0.01 * D)
    q = (anchors[np.arange(Q) % G].astype(np.float64) + 1e-3 * s0 / np.sqrt(D) * r.standard_normal((Q, D))).astype(np.float32)
    k.rows, k.centre, k.query = rows, c, q
    k.x_d2_64, k.x_d2_32 = dist2(q, rows), dist2(q, rows, np.float32)
    if bf16:
        k.bank16 = bf16_rne((rows - c[None, :]).astype(np.float32))
        k.values = bf16_value(k.bank16)
        k.qc = (q - c[None, :]).astype(np.float32)
        t = rows.astype(np.float64) - c.astype(np.float64)[None, :]
        r64, n64 = np.sqrt(((t - k.values) ** 2).sum(1)), np.sqrt((t * t).sum(1))
        k.rho = np.nextafter((1.000001 * r64 + 1e-6 * n64).astype(np.float32), np.float32(np.inf))
        assert (k.rho.astype(np.float64) >= r64).all()
        k.d2_64, k.d2_32 = dist2(k.qc, k.values), dist2(k.qc, k.values, np.float32)
        k.scan_query, k.bits = k.qc, k.bank16
    else:
        k.values, k.scan_query, k.bits = rows, q, rows.view(np.uint32)
        k.d2_64, k.d2_32 = k.x_d2_64, k.x_d2_32
    k.gap = gaps_ok(k.d2_64, k.bits, KMAX)
    k.x_gap = gaps_ok(k.x_d2_64, rows.view(np.uint32), 1)
    return k


def build_segments(name, sizes, D, seg, bf16, spacing=0.1):
    """A multi-character bank: segment s has sizes[s] rows on shells around its own anchor (rank order shuffled inside the segment); query
    i is the anchor of segment seg[i] plus noise (an id outside [0, S): a random vector).  The operands as in build_bank (bf16: the centred
    copy's values and centred queries).  enc: random rows of D floats, one per bank row."""
    r = rng("scan-seg-" + name)
    k = Case()
    S, Q = len(sizes), len(seg)
    k.name, k.D, k.Q, k.S, k.sizes, k.seg, k.bf16 = name, D, Q, S, list(sizes), np.asarray(seg, np.int32), bf16
    k.seg_start = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    k.N = N = int(k.seg_start[-1])
    c = (0.1 * r.standard_normal(D, dtype=np.float32)).astype(np.float32)
    anchors = r.standard_normal((S, D), dtype=np.float32) + c[None, :]
    rows = np.empty((N, D), np.float32)
    for s in range(S):
        lo, n = int(k.seg_start[s]), sizes[s]
        rows[lo + r.permutation(n)] = _shells(r, anchors[s], n, D, spacing, 0.01)
    q = r.standard_normal((Q, D), dtype=np.float32) + c[None, :]
    s0 = np.sqrt(0.01 * D)
    for i, s in enumerate(seg):
        if 0 <= s < S:
            q[i] = (anchors[s].astype(np.float64) + 1e-3 * s0 / np.sqrt(D) * r.standard_normal(D)).astype(np.float32)
    if bf16:
        k.bank16 = bf16_rne((rows - c[None, :]).astype(np.float32))
        k.values, k.scan_query, k.bits = bf16_value(k.bank16), (q - c[None, :]).astype(np.float32), k.bank16
    else:
        k.values, k.scan_query, k.bits = rows, q, rows.view(np.uint32)
    k.enc = r.standard_normal((N, D), dtype=np.float32)
    k.idx, k.gidx, k.d2_64 = seg_search(k.scan_query, k.values, seg, k.seg_start, KMAX)
    _, _, k.d2_32 = seg_search(k.scan_query, k.values, seg, k.seg_start, KMAX, np.float32)
    k.gap = np.inf
    for i, s in enumerate(seg):
        if 0 <= s < S:
            lo, hi = int(k.seg_start[s]), int(k.seg_start[s + 1])
            g = gaps_ok(dist2(k.scan_query[i:i + 1], k.values[lo:hi]), k.bits[lo:hi], KMAX)
            k.gap = None if (g is None or k.gap is None) else min(k.gap, g)
    return k


# ------------------------------------------------------------------------------------------------------------------ authored keys for the refine
def slice_rows(N):
    """The refine's arithmetic: per_slice = ceil(N / 64) rows a slice; a slice of more than 2 048 rows re-reads its keys instead of holding
    them in registers; index windows of 4 096 rows inside a slice.  Rows on both sides of every such bound that exists in a bank of N rows."""
    per = -(-N // RF_SPLIT)
    last_lo = (N - 1) // per * per
    rows = [0, N - 1, per - 1, per, last_lo]
    if per > RF_CAP:
        rows += [RF_CAP - 1, RF_CAP, per + RF_CAP - 1, per + RF_CAP, min(last_lo + RF_CAP - 1, N - 1)]
    rows += [2 * per - 1, last_lo - 1, 1023, 1024, per + 1024]                  # (1 024: the stride of the keys a thread holds)
    out = []
    for v in rows:
        if 0 <= v < N and v not in out:
            out.append(int(v))
    return per, out


def build_refine(name, N, D, nq, ncand, *, rho_scale=0.3, allsame=False, nan_rows=0, all_nan_query=False, copy=False, cand_rows=None):
    """Authored coarse keys for mocha_match_refine alone, as family 3 authors scores.  Every bank row is the TRAP - query 0 itself, nearer
    to every query than anything else - except the candidate rows of each query: a winner at squared distance 0.01 D and ncand - 1 decoys a
    factor (1 + 3e-4 j) farther (ncand = "all": every row is one, 1.5e-4 j; then there is no trap).  rho is authored: rho_scale * d_winner * U[0.8, 1].
    Keys: the float64 distance plus 0.9 of the stated bound B_n = rho_n + 2e-5 d_n for the winner, minus 0.9 B_n for the decoys (every decoy
    looks better; the scan's minimum names a decoy); every other row 1.1 bounds OUT: d16 - 1.1 (rho + 2e-5 d16) = d16_m + rho_m + 2e-5 d16_m.
    A pruned row is the trap, so pruning shows: were it evaluated it would win.  nan_rows: that many further trap rows carry a NaN key.
    all_nan_query: the LAST query's keys are all NaN - nothing is excluded, the answer is the float64 argmin over every row (small N).
    copy: the first decoy is a bit-identical copy of the winner at a higher row with rho = 0 for both: the 2e-5 d terms alone keep the winner.
    allsame: every row identical, every row a candidate, the answer row 0.
    The rows that differ from the trap are `special` (row -> fp32 row); the bank itself is filled by the caller (on the device)."""
    r = rng("scan-refine-" + name)
    k = Case()
    k.name, k.N, k.D, k.nq = name, N, D, nq
    per, edge = slice_rows(N)
    k.per_slice = per
    q0 = r.standard_normal(D, dtype=np.float32)
    q = (q0.astype(np.float64)[None, :] + 1e-3 * r.standard_normal((nq, D))).astype(np.float32)
    q[0] = q0
    k.query, k.trap = q, q0
    k.special = {}
    every = ncand == "all"
    m_all = N if every else ncand
    assert every or nq * ncand + nan_rows <= N
    # rows of the candidates: edge rows first, rotated by query so that winners and decoys both meet every bound
    pool = edge + [int(v) for v in r.permutation(min(N, 1 << 16)) if v not in edge] if cand_rows is None else list(cand_rows)
    keys = np.empty((nq, N), np.uint64)
    rho = np.zeros(N, np.float32)
    k.winner, k.cands, k.d_win64, k.d_win32 = [], [], [], []
    d_w = np.sqrt(0.01 * D)
    rho[:] = (rho_scale * d_w * (0.8 + 0.2 * r.random(N))).astype(np.float32)
    taken = 0
    per_query = []
    for i in range(nq):
        if allsame:
            mine = list(range(N))
        elif every:
            assert nq == 1 or (all_nan_query and i == nq - 1) or i == 0
            mine = list(range(N)) if i == 0 else per_query[0]
            if i == 0:
                rot = edge[zlib_crc(name) % len(edge)]
                mine = [rot] + [v for v in r.permutation(N).tolist() if v != rot]
        else:
            mine = pool[taken:taken + ncand]
            taken += ncand
            rotate = (i + zlib_crc(name)) % len(mine)
            mine = mine[rotate:] + mine[:rotate]
        per_query.append(mine)
    if allsame:
        u = r.standard_normal(D)
        row = (q0.astype(np.float64) + u * d_w / np.sqrt((u * u).sum())).astype(np.float32)
        k.trap = row
        rho[:] = np.float32(rho_scale * d_w)
    elif every:
        rr = _shells_lin(r, q0, N, D, 1.5e-4, 0.01)
        for j, v in enumerate(per_query[0]):
            k.special[v] = rr[j]
    else:
        for i in range(nq):
            if all_nan_query and i == nq - 1:
                continue
            rr = _shells_lin(r, q[i], len(per_query[i]), D, 3e-4, 0.01)
            for j, v in enumerate(per_query[i]):
                k.special[v] = rr[j]
            if copy and len(per_query[i]) > 1:
                w, tw = sorted(per_query[i][:2])
                per_query[i][:2] = [w, tw]
                k.special[w] = rr[0]
                k.special[tw] = rr[0]
                rho[[w, tw]] = 0
    k.per_query = per_query
    srows = np.array(sorted(k.special), np.int64)
    smat = np.stack([k.special[v] for v in srows]) if len(srows) else np.zeros((0, D), np.float32)
    k.srows, k.smat = srows, smat
    nanset = []
    if nan_rows:
        nanset = [v for v in pool[::-1] if v not in k.special][:nan_rows]
    k.nan_rows = nanset
    k.answer = np.zeros(nq, np.int64)
    k.d64, k.d32 = np.zeros(nq), np.zeros(nq, np.float32)
    k.expect_cands = []
    for i in range(nq):
        if allsame:
            d64 = np.full(N, np.sqrt(dist2(q[i:i + 1], k.trap[None])[0, 0]))
            d32 = np.full(N, np.sqrt(dist2(q[i:i + 1], k.trap[None], np.float32)[0, 0]), np.float32)
            sign = -np.ones(N); sign[0] = 1
            rows_i = np.arange(N)
            win = 0
        elif all_nan_query and i == nq - 1:
            keys[i] = pack_key(np.full(N, np.nan, np.float32), np.arange(N))
            dtrap = dist2(q[i:i + 1], k.trap[None])[0, 0]
            dsp = dist2(q[i:i + 1], smat)[0] if len(srows) else np.zeros(0)
            full = np.full(N, dtrap); full[srows] = dsp
            k.answer[i] = int(np.argmin(full))
            k.d64[i] = np.sqrt(full[k.answer[i]])
            full32 = np.full(N, dist2(q[i:i + 1], k.trap[None], np.float32)[0, 0], np.float32)
            if len(srows):
                full32[srows] = dist2(q[i:i + 1], smat, np.float32)[0]
            k.d32[i] = np.sqrt(full32[k.answer[i]])
            k.expect_cands.append(N)
            k.winner.append(int(k.answer[i]))
            continue
        else:
            rows_i = np.array(per_query[i], np.int64)
            mat = np.stack([k.special[v] for v in rows_i])
            d64 = np.sqrt(dist2(q[i:i + 1], mat)[0])
            d32 = np.sqrt(dist2(q[i:i + 1], mat, np.float32)[0])
            order = sorted(range(len(rows_i)), key=lambda j: (d64[j], rows_i[j]))
            win = order[0]
            sign = -np.ones(len(rows_i)); sign[win] = 1
            # the gap condition among the candidates: exactly 0 (copies) or >= MIN_GAP in d2
            for a, b in zip(order[:1], order[1:2]):
                g = (d64[b] ** 2 - d64[a] ** 2) / d64[b] ** 2
                assert (g == 0.0 and np.array_equal(mat[a], mat[b])) or g >= MIN_GAP, (name, i, g)
        B = rho[rows_i].astype(np.float64) + 2e-5 * d64
        d16 = d64 + 0.9 * sign * B
        assert (d16 > 0).all(), name
        v32 = (d16 * d16).astype(np.float32)
        if not allsame:
            # everything else: 1.1 bounds out of the bound the kernel forms from the fp32 keys it is given
            kk = pack_key(v32, rows_i)
            m = int(np.argmin(kk))
            dm = np.sqrt(np.float64(v32[m]))
            hi = dm + float(rho[rows_i[m]]) + 2e-5 * dm
            d_out = (hi + 1.1 * rho.astype(np.float64)) / (1 - 2.2e-5)
            keys[i] = pack_key((d_out * d_out).astype(np.float32), np.arange(N))
        keys[i, rows_i] = pack_key(v32, rows_i)
        if nanset:
            keys[i, nanset] = pack_key(np.full(len(nanset), np.nan, np.float32), np.array(nanset))
        k.answer[i] = rows_i[win] if not allsame else 0
        k.winner.append(int(k.answer[i]))
        k.d64[i], k.d32[i] = d64[win], d32[win]
        k.expect_cands.append(len(rows_i))
    k.keys, k.rho = keys, rho
    k.wgmin = wg_minima(keys)
    return k


def zlib_crc(name):
    return zlib.crc32(name.encode())


def _shells_lin(r, anchor, n, D, step, s0):
    """n fp32 rows around `anchor` at squared distances s0 * D * (1 + step * rank)."""
    u = r.standard_normal((n, D))
    u /= np.sqrt((u * u).sum(1, keepdims=True))
    s = np.sqrt(s0 * D * (1 + step * np.arange(n)))
    return (anchor.astype(np.float64)[None, :] + u * s[:, None]).astype(np.float32)
