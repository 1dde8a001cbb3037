"""Generates tests/golden/action_match.npz: the reference's action-constrained nearest-neighbour search on seeded synthetic banks.

The reference picks an action, keeps the character's windows of that action, builds scikit-learn's ``BallTree`` over that subset and
queries it with k = 1 (train_CVAE.py:198-211).  This script does exactly that for 2 characters whose entries carry 3 actions in runs and
16 queries with a picked action each, and stores - a few KB - the seeds, the labels, the queries' characters and actions, the index INSIDE
the subset, that index mapped back to the character's rows, and the distance.  The first queries are near-copies of a row of ANOTHER
action of their character, so that the unconstrained answer differs from the constrained one (asserted here).

    python tests/golden/make_golden_action_match.py        (needs scikit-learn; the tests only read the .npz)
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from mocha_sigasia2023_amd import synthetic  # noqa: E402

CNT_NORM_SEED = 90
CHARACTERS = ((300, (14, 13, 13)), (301, (11, 12, 10)))          # (seed, entries of action 0 / 1 / 2, in runs)
QUERY_SEED, Q, TRAPS = 302, 16, 4
MIN_GAP = 1e-4


def banks():
    """[(z-scored cnt rows (N_c, 23040) float32, labels (N_c,) int32), ...] - what the tests rebuild from the stored seeds."""
    mean, std = synthetic.cnt_norm(CNT_NORM_SEED)
    out = []
    for seed, runs in CHARACTERS:
        cnt = synthetic.token_features(seed, sum(runs))
        nm = ((cnt - mean[np.newaxis]) / std[np.newaxis]).reshape(cnt.shape[0], -1).astype(np.float32)
        out.append((nm, np.repeat(np.arange(len(runs)), runs).astype(np.int32)))
    return out


def queries(bk):
    """(z-scored queries (Q, 23040) float32, character (Q,), picked action (Q,))."""
    mean, std = synthetic.cnt_norm(CNT_NORM_SEED)
    r = np.random.default_rng(QUERY_SEED)
    cnt = synthetic.token_features(QUERY_SEED, Q)
    q = ((cnt - mean[np.newaxis]) / std[np.newaxis]).reshape(Q, -1).astype(np.float32)
    cha = (np.arange(Q) % len(bk)).astype(np.int32)
    act = r.integers(0, 3, Q).astype(np.int32)
    for i in range(TRAPS):                    # a near-copy of a row of ANOTHER action of the query's character
        nm, lab = bk[cha[i]]
        other = np.flatnonzero(lab != act[i])
        q[i] = nm[other[r.integers(0, len(other))]] + np.float32(0.05) * q[i]
    return q, cha, act


def main():
    import sklearn
    from sklearn.neighbors import BallTree
    bk = banks()
    q, cha, act = queries(bk)
    sub_idx, idx, dist, plain = (np.zeros(Q, np.int64) for _ in range(4))
    dist = np.zeros(Q, np.float64)
    for i in range(Q):
        nm, lab = bk[cha[i]]
        picked = np.where(lab == act[i])[0]                                     # the character's entries of the picked action
        tree = BallTree(nm[picked])
        d, n = tree.query(q[i:i + 1], k=2, return_distance=True)
        assert (d[0, 1] ** 2 - d[0, 0] ** 2) / d[0, 1] ** 2 >= MIN_GAP, (i, d)  # no near-tie an fp32 search could resolve the other way
        sub_idx[i], idx[i], dist[i] = n[0, 0], picked[n[0, 0]], d[0, 0]
        plain[i] = BallTree(nm).query(q[i:i + 1], k=1, return_distance=False)[0, 0]
    assert (plain[:TRAPS] != idx[:TRAPS]).all() and (lab_of(bk, cha, plain)[:TRAPS] != act[:TRAPS]).all()
    out = dict(cnt_norm_seed=np.array(CNT_NORM_SEED), char_seeds=np.array([c[0] for c in CHARACTERS]),
               char_runs=np.array([c[1] for c in CHARACTERS]), query_seed=np.array([QUERY_SEED, Q, TRAPS]),
               labels0=bk[0][1], labels1=bk[1][1], character=cha, action=act, subset_idx=sub_idx, idx=idx, dist=dist, plain_idx=plain,
               meta=np.array(repr(dict(sklearn=sklearn.__version__))))
    np.savez(os.path.join(HERE, "action_match.npz"), **out)
    print("action_match", dict(idx=idx.tolist(), plain=plain.tolist()))


def lab_of(bk, cha, rows):
    return np.array([bk[c][1][r] for c, r in zip(cha, rows)])


if __name__ == "__main__":
    main()
