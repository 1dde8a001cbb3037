"""NumPy restatement of coherent context matching (include/mocha_hip.h, "coherent context matching"): float64, sequential.

d (Q, N): distances (any float dtype; the fp32 values are used as they are, widened to float64).  seq_starts: 0 = s_0 < s_1 < ... (the end Q
may be given or left out).  bank_starts: rows without a predecessor besides row 0.  lam: the jump penalty, finite and >= 0.

    first window of a sequence:  R[i][j] = d[i][j]
    otherwise:                   a = R[i-1][j-1] - M[i-1] if row j has a predecessor else +inf;  cont(i, j) = a < lam (a tie jumps);
                                 R[i][j] = d[i][j] + (a if cont else lam)
    M[i] = min_j R[i][j], m[i] the lowest j attaining it
    backtrack per sequence:      path[last] = m[last];  path[i] = path[i+1] - 1 if cont(i+1, path[i+1]) else m[i]
"""
import numpy as np


def has_pred(N, bank_starts=None):
    p = np.ones(N, dtype=bool)
    p[0] = False
    if bank_starts is not None and len(bank_starts):
        p[np.asarray(bank_starts, dtype=np.int64)] = False
    return p


def seq_bounds(Q, seq_starts=None):
    s = [0] if seq_starts is None else [int(x) for x in seq_starts]
    if not s or s[0] != 0:
        raise ValueError("sequence starts begin at 0")
    if s[-1] != Q:
        s.append(Q)
    if any(b <= a for a, b in zip(s, s[1:])):
        raise ValueError("sequence starts increase strictly and stay below Q")
    return s


def path_ref(d, lam, seq_starts=None, bank_starts=None):
    """-> path (Q,) int32, dist (Q,) of d's dtype, continued (Q,) uint8."""
    d = np.asarray(d)
    Q, N = d.shape
    lam = float(lam)
    if not (np.isfinite(lam) and lam >= 0):
        raise ValueError("the jump penalty is finite and >= 0")
    pred = has_pred(N, bank_starts)
    path = np.zeros(Q, dtype=np.int32)
    cont = np.zeros((Q, N), dtype=bool)
    m = np.zeros(Q, dtype=np.int64)
    s = seq_bounds(Q, seq_starts)
    for i0, i1 in zip(s, s[1:]):
        R = d[i0].astype(np.float64)
        m[i0] = int(np.argmin(R))                  # (numpy's argmin is the first of equal values)
        for i in range(i0 + 1, i1):
            a = np.full(N, np.inf)
            a[1:] = R[:-1] - R[m[i - 1]]
            a[~pred] = np.inf
            c = a < lam
            R = d[i].astype(np.float64) + np.where(c, a, lam)
            cont[i] = c
            m[i] = int(np.argmin(R))
        path[i1 - 1] = m[i1 - 1]
        for i in range(i1 - 2, i0 - 1, -1):
            j = int(path[i + 1])
            path[i] = j - 1 if cont[i + 1, j] else m[i]
    dist = d[np.arange(Q), path]
    continued = np.zeros(Q, dtype=np.uint8)
    for i in range(1, Q):
        if i not in s and path[i] == path[i - 1] + 1 and pred[path[i]]:
            continued[i] = 1
    return path, dist, continued


def path_cost(d, rows, lam, seq_starts=None, bank_starts=None):
    """sum d[i][rows[i]] + lam * (transitions inside a sequence that are not 'next row of the same clip'), in float64."""
    d = np.asarray(d)
    Q, N = d.shape
    pred = has_pred(N, bank_starts)
    s = set(seq_bounds(Q, seq_starts))
    cost = 0.0
    for i in range(Q):
        cost += float(d[i, rows[i]])
        if i and i not in s and not (rows[i] == rows[i - 1] + 1 and pred[rows[i]]):
            cost += float(lam)
    return cost
