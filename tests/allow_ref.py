"""The float64 restatement of action-constrained context matching (include/mocha_hip.h, mocha_bank_set_labels), for the test_allow_*.py
files.  What the operation MEANS is taken from the header; nothing is transcribed from the kernels.
  labels      one label 0 .. 63 per bank row
  any[s]      OR of 1 << label over the rows of segment s
  granules    gran[gran_start[s] + x] = OR of the label bits of the segment's rows [16 x, 16 x + 16)
  constrained a query of segment s with mask m is constrained iff (m & any[s]) != 0; its candidates are the rows of s whose bit is in m
  otherwise   m == 0 (nothing asked: applied 0) or no row of s has an asked label (fell back: applied -1): the whole segment
  answer      the k nearest candidates by the direct-form squared distance, ties to the lower row, the index LOCAL to the segment and
              counting all its rows; fewer than k candidates: -1 / +inf; an id outside [0, S): -1 / +inf / applied 0
Distances and the k-NN rule are scan_ref's (dist2, knn): generic over the NumPy dtype, float64 the truth, float32 the CPU evaluation."""
from __future__ import annotations

import numpy as np

import scan_ref as sr

GRANULE = 16
ALL = (1 << 64) - 1


def action_mask(actions) -> int:
    m = 0
    for a in actions:
        assert 0 <= int(a) <= 63
        m |= 1 << int(a)
    return m


def as_int64(masks):
    """Python int masks (0 .. 2**64 - 1) as the int64 bit patterns the device tensors hold."""
    return np.array([m - (1 << 64) if m >= 1 << 63 else m for m in masks], dtype=np.int64)


def any_table(labels, seg_start):
    return [action_mask(set(int(v) for v in labels[int(seg_start[s]):int(seg_start[s + 1])])) for s in range(len(seg_start) - 1)]


def granule_table(labels, seg_start):
    """(gran_start [S + 1], gran [gran_start[S]]) as Python ints."""
    start, gran = [0], []
    for s in range(len(seg_start) - 1):
        lab = labels[int(seg_start[s]):int(seg_start[s + 1])]
        for x in range(0, len(lab), GRANULE):
            gran.append(action_mask(set(int(v) for v in lab[x:x + GRANULE])))
        start.append(len(gran))
    return start, gran


def applied_of(mask: int, any_s: int) -> int:
    return 0 if mask == 0 else (1 if mask & any_s else -1)


def candidates(labels_seg, mask: int):
    """Local rows of a segment a query with `mask` may be answered with (every row for an unconstrained query)."""
    lab = np.asarray(labels_seg).astype(np.int64)
    any_s = action_mask(set(lab.tolist()))
    if applied_of(mask, any_s) != 1:
        return np.arange(len(lab))
    return np.flatnonzero(np.array([(mask >> int(v)) & 1 for v in lab], dtype=bool))


def search(q, bank, seg, seg_start, labels, masks, k, dtype=np.float64):
    """(idx [Q, k] local rows, gidx [Q, k] global rows, d2 [Q, k], applied [Q]) of the constrained search; masks: Python ints."""
    Q, S = len(seg), len(seg_start) - 1
    idx, g = np.full((Q, k), -1, np.int64), np.full((Q, k), -1, np.int64)
    val, applied = np.full((Q, k), np.inf, dtype), np.zeros(Q, np.int32)
    anys = any_table(labels, seg_start)
    for i in range(Q):
        s = int(seg[i])
        if not 0 <= s < S:
            continue
        lo, hi = int(seg_start[s]), int(seg_start[s + 1])
        applied[i] = applied_of(int(masks[i]), anys[s])
        cand = candidates(labels[lo:hi], int(masks[i]))
        li, lv = sr.knn(sr.dist2(q[i:i + 1], bank[lo:hi][cand], dtype), k)
        have = li[0] >= 0
        idx[i] = np.where(have, cand[np.where(have, li[0], 0)], -1)
        val[i] = lv[0]
        g[i] = np.where(have, idx[i] + lo, -1)
    return idx, g, val, applied


def brute(q, bank, seg, seg_start, labels, masks, k):
    """The same answers by brute force: every row of the segment visited, inadmissible ones skipped, a stable sort by (d2, row)."""
    Q = len(seg)
    idx = np.full((Q, k), -1, np.int64)
    for i in range(Q):
        s = int(seg[i])
        if not 0 <= s < len(seg_start) - 1:
            continue
        lo, hi = int(seg_start[s]), int(seg_start[s + 1])
        lab = [int(v) for v in labels[lo:hi]]
        m = int(masks[i])
        constrained = m != 0 and any((m >> v) & 1 for v in lab)
        rows = [r for r in range(hi - lo) if not constrained or (m >> lab[r]) & 1]
        d = {r: float(((bank[lo + r].astype(np.float64) - q[i].astype(np.float64)) ** 2).sum()) for r in rows}
        best = sorted(rows, key=lambda r: (d[r], r))[:k]
        idx[i, :len(best)] = best
    return idx


def gaps_ok(q, bank, seg, seg_start, labels, masks, bits, depth):
    """The data rule of test_scan_kernels.py on every query's CANDIDATES: any two of the depth + 1 nearest differ in float64 d2 by exactly
    0 (bit-identical rows) or by at least scan_ref.MIN_GAP relative.  Returns the smallest nonzero gap, or None when the rule fails."""
    worst = np.inf
    for i in range(len(seg)):
        s = int(seg[i])
        if not 0 <= s < len(seg_start) - 1:
            continue
        lo, hi = int(seg_start[s]), int(seg_start[s + 1])
        cand = candidates(labels[lo:hi], int(masks[i]))
        g = sr.gaps_ok(sr.dist2(q[i:i + 1], bank[lo:hi][cand]), bits[lo:hi][cand], depth)
        if g is None:
            return None
        worst = min(worst, g)
    return worst
