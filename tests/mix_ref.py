"""NumPy restatement of character mixing's host-checkable rules (include/mocha_hip.h, "Character mixing"): which components are PRESENT,
the per-body-part normalisation with its fallback, and the part-wise blend of the matched entries' features.  Generic over dtype: in
float32 every operation is the one IEEE operation the kernel performs (a sum with j ascending, one division, a product and a sum rounded
separately), so the float32 results are comparable bit for bit; in float64 it is the reference the tolerance tests hold the kernel to.
It knows nothing of matching: the rows come from the caller."""
import numpy as np

PARTS = 6
MIX_MAX = 4
FLT_MAX = float(np.finfo(np.float32).max)


def usable(w):
    """0 < w <= FLT_MAX; NaN, negatives, zero and infinities are not."""
    w = np.asarray(w)
    with np.errstate(invalid="ignore"):
        return (w > 0) & (w <= FLT_MAX)


def present(ids, weights, loaded):
    """ids (Q,J) ints, weights (Q,J,6), loaded: the set (or boolean array over ids) of ids that name a loaded character -> (Q,J) bool."""
    ids = np.asarray(ids)
    if isinstance(loaded, (set, frozenset, list, tuple, range)):
        ok = np.isin(ids, list(loaded))
    else:
        loaded = np.asarray(loaded, dtype=bool)
        inside = (ids >= 0) & (ids < loaded.shape[0])
        ok = inside & loaded[np.where(inside, ids, 0)]
    return ok & usable(weights).any(axis=2)


def normalise(weights, pres, dtype=np.float32):
    """weights (Q,J,6), pres (Q,J) bool -> the normalised weights (Q,J,6) in `dtype`: per part the usable weights of present components
    divided by their sum (summed with j ascending); a part with no such weight goes to the lowest present component; all 0 where no
    component is present."""
    w = np.asarray(weights).astype(dtype)
    Q, J, P = w.shape
    assert P == PARTS and 1 <= J <= MIX_MAX
    out = np.zeros((Q, J, P), dtype)
    use = usable(np.asarray(weights)) & np.asarray(pres, dtype=bool)[:, :, None]
    for q in range(Q):
        js = np.flatnonzero(pres[q])
        if js.size == 0:
            continue
        for v in range(P):
            s = dtype(0)
            for j in range(J):
                if use[q, j, v]:
                    s = dtype(s + w[q, j, v])
            if s > 0:
                for j in range(J):
                    if use[q, j, v]:
                        with np.errstate(over="ignore"):
                            out[q, j, v] = dtype(w[q, j, v] / s)
            else:
                out[q, js[0], v] = dtype(1)
    return out


def blend(wnorm, feats, dtype=np.float32):
    """wnorm (Q,J,6), feats (Q,J,90,256) the matched entries' encoded features (anything where wnorm is 0: not read) -> F (Q,90,256):
    token t * 6 + v takes sum_j wnorm[j][v] * feats[j], from 0, j ascending, product and sum rounded separately, terms of weight 0
    skipped."""
    wn = np.asarray(wnorm).astype(dtype)
    Q, J, _ = wn.shape
    F = np.zeros((Q, 90, 256), dtype)
    part = np.arange(90) % PARTS
    for q in range(Q):
        for j in range(J):
            wt = wn[q, j][part]                                   # (90,) weight of every token
            on = wt != 0
            if not on.any():
                continue
            p = (wt[on, None] * np.asarray(feats[q][j])[on].astype(dtype)).astype(dtype)
            F[q, on] = (F[q, on] + p).astype(dtype)
    return F
