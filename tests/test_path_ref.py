"""The NumPy restatement of coherent context matching (tests/path_ref.py) against a brute force over all row sequences, and the
properties the definition promises: lambda = 0 is the row-wise lowest-index arg-min, a == lambda jumps, sequences are independent."""
import itertools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from path_ref import path_cost, path_ref  # noqa: E402

LAMBDAS = (0.0, 0.5, 1.0, 3.0)


def _matrices(Q, N):
    rng = np.random.default_rng(1000 * Q + N)
    out = [rng.uniform(1.0, 2.0, (Q, N)).astype(np.float32) for _ in range(3)]
    out += [rng.integers(0, 4, (Q, N)).astype(np.float32) for _ in range(3)]      # integer-valued: ties everywhere
    return out


@pytest.mark.parametrize("Q", range(1, 6))
@pytest.mark.parametrize("N", range(1, 5))
def test_restatement_attains_the_brute_force_minimum(Q, N):
    for d in _matrices(Q, N):
        for lam in LAMBDAS:
            for bs in (None, [N - 1]) if N > 1 else (None,):
                path, dist, cont = path_ref(d, lam, bank_starts=bs)
                best = min(path_cost(d, rows, lam, bank_starts=bs) for rows in itertools.product(range(N), repeat=Q))
                got = path_cost(d, path, lam, bank_starts=bs)
                assert abs(got - best) <= 1e-12 * max(1.0, abs(best)), (Q, N, lam, bs, path.tolist())
                assert np.array_equal(dist, d[np.arange(Q), path])
                # continued marks exactly the transitions the cost does not charge
                assert got == pytest.approx(float(d[np.arange(Q), path].astype(np.float64).sum()) + lam * (Q - 1 - int(cont.sum())), rel=1e-12)


def test_lambda_zero_is_the_lowest_index_argmin():
    rng = np.random.default_rng(5)
    d = rng.uniform(1, 2, (12, 9)).astype(np.float32)
    d[:, 6] = d[:, 2]                                  # a duplicated column: the lower one wins
    d[3, 2] = d[3, 6] = d[3].min() - 0.5
    path, dist, cont = path_ref(d, 0.0, bank_starts=[4])
    assert np.array_equal(path, d.argmin(1)) and path[3] == 2
    assert np.array_equal(dist, d.min(1))
    want = [int(i > 0 and path[i] == path[i - 1] + 1 and path[i] not in (0, 4)) for i in range(12)]
    assert cont.tolist() == want                       # 'continued' describes the path, whatever produced it


def test_a_equal_lambda_jumps():
    # window 0: R = [1, 3], M = 1.  Row 1's predecessor is row 0 with a = 0; row ... use three rows so that a == lambda exactly at row 2:
    # R[0] = [1, 3, 9]: a(row 2) = 3 - 1 = 2 == lambda -> a jump, R[1][2] = d + 2 either way, but cont must be False
    d = np.array([[1, 3, 9], [9, 9, 1]], dtype=np.float32)
    path, _, cont = path_ref(d, 2.0)
    assert path.tolist() == [0, 2] and cont.tolist() == [0, 0]
    path, _, cont = path_ref(d, np.nextafter(2.0, 3.0))      # one ulp more: it continues from row 1
    assert path.tolist() == [1, 2] and cont.tolist() == [0, 1]


def test_sequences_are_independent():
    rng = np.random.default_rng(9)
    d = rng.uniform(1, 2, (20, 7)).astype(np.float32)
    starts = [0, 1, 3, 11]
    for lam in (0.05, 0.3, 1.0):
        whole = path_ref(d, lam, seq_starts=starts, bank_starts=[3])
        parts = [path_ref(d[a:b], lam, bank_starts=[3]) for a, b in zip(starts, starts[1:] + [20])]
        for k in range(3):
            assert np.array_equal(whole[k], np.concatenate([p[k] for p in parts]))


def test_bad_arguments():
    d = np.ones((3, 2), dtype=np.float32)
    for lam in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            path_ref(d, lam)
    with pytest.raises(ValueError):
        path_ref(d, 1.0, seq_starts=[1])
    with pytest.raises(ValueError):
        path_ref(d, 1.0, seq_starts=[0, 2, 2])
