"""tests/mix_ref.py pinned on hand-written cases (no GPU): presence, normalisation, the fallback and the blend of character mixing."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mix_ref as R  # noqa: E402

NAN, INF = float("nan"), float("inf")


def _w(*rows):
    """Components' weights, each row either one number (broadcast over the parts) or six."""
    return np.array([[r] * 6 if np.isscalar(r) else list(r) for r in rows], dtype=np.float32)[None]


def test_usable():
    w = np.array([0.0, -0.0, -1.0, NAN, INF, -INF, 1e-45, R.FLT_MAX, 0.5], dtype=np.float32)
    assert R.usable(w).tolist() == [False, False, False, False, False, False, True, True, True]


def test_all_zero_part_weights_fall_back_to_the_lowest_present_component():
    # part 2 is weighed by nobody: it goes to the lowest PRESENT component - component 1, since component 0 names no loaded character
    w = _w([1, 1, 0, 1, 1, 1], [3, 1, 0, 1, 1, 1], [0, 2, 0, 0, 0, 0])
    ids = np.array([[7, 0, 1]])
    pres = R.present(ids, w, {0, 1})
    assert pres.tolist() == [[False, True, True]]
    wn = R.normalise(w, pres)
    assert wn[0, 0].tolist() == [0] * 6
    assert wn[0, 1].tolist() == [1, np.float32(1) / np.float32(3), 1, 1, 1, 1]
    assert wn[0, 2].tolist() == [0, np.float32(2) / np.float32(3), 0, 0, 0, 0]
    # a component whose six weights are all zero is not present at all
    w0 = _w(0, 2)
    p0 = R.present(np.array([[0, 1]]), w0, {0, 1})
    assert p0.tolist() == [[False, True]] and (R.normalise(w0, p0)[0, 1] == 1).all()


def test_nan_negative_and_infinite_weights_count_as_zero():
    w = _w([NAN, -1, INF, -INF, 2, 0.5], [1, 1, 1, 1, 6, NAN])
    pres = R.present(np.array([[0, 1]]), w, {0, 1})
    assert pres.tolist() == [[True, True]]
    wn = R.normalise(w, pres)
    assert wn[0, 0].tolist() == [0, 0, 0, 0, 0.25, 1]
    assert wn[0, 1].tolist() == [1, 1, 1, 1, 0.75, 0]
    assert np.isfinite(wn).all()
    # only unusable weights: not present, whatever the id
    bad = _w([NAN, -1, INF, -INF, 0, -0.0])
    assert R.present(np.array([[0]]), bad, {0}).tolist() == [[False]]
    assert (R.normalise(bad, np.array([[False]])) == 0).all()


def test_repeated_id_adds_through_the_sum():
    w = _w(1, 1, 2)
    ids = np.array([[3, 3, 5]])
    pres = R.present(ids, w, np.array([0, 0, 0, 1, 0, 1], dtype=bool))
    assert pres.all()
    wn = R.normalise(w, pres)
    assert (wn[0, 0] == 0.25).all() and (wn[0, 1] == 0.25).all() and (wn[0, 2] == 0.5).all()
    e = np.random.default_rng(0).standard_normal((2, 90, 256)).astype(np.float32)
    F = R.blend(wn, e[[0, 0, 1]][None])
    # both components of character 3 matched the same row: 0.25 x + 0.25 x + 0.5 y, in that order
    want = (np.float32(0.25) * e[0] + np.float32(0.25) * e[0]) + np.float32(0.5) * e[1]
    assert np.array_equal(F[0], want)


def test_one_hot_splice_copies_bits_part_by_part():
    mask = np.array([1, 0, 1, 1, 0, 0], dtype=np.float32)
    w = np.stack([mask, 1 - mask])[None]
    pres = R.present(np.array([[0, 1]]), w, {0, 1})
    wn = R.normalise(w, pres)
    assert np.array_equal(wn[0, 0], mask) and np.array_equal(wn[0, 1], 1 - mask)
    e = np.random.default_rng(1).standard_normal((2, 90, 256)).astype(np.float32)
    e[0, 0, 0] = -0.0
    F = R.blend(wn, e[None])
    tok = np.arange(90) % 6
    for v in range(6):
        src = e[0] if mask[v] else e[1]
        assert np.array_equal(F[0, tok == v], src[tok == v]), v
    # one effective component: the entry itself, and the other component's row is never read (NaN there changes nothing)
    poisoned = e.copy(); poisoned[1] = NAN
    one = R.normalise(_w(0.3, 0), R.present(np.array([[0, 1]]), _w(0.3, 0), {0, 1}))
    assert np.array_equal(R.blend(one, poisoned[None])[0], e[0])


def test_no_component_present():
    w = _w(1, [0, 0, 0, 0, 0, 0], NAN)
    ids = np.array([[-1, 0, 1]])                    # an id outside the table, a weightless one, one whose weights are unusable
    pres = R.present(ids, w, {0, 1})
    assert not pres.any()
    wn = R.normalise(w, pres)
    assert (wn == 0).all()
    assert (R.blend(wn, np.full((1, 3, 90, 256), NAN, np.float32)) == 0).all()
    # an id past the end of a boolean table, and an empty slot
    assert R.present(np.array([[2, 1]]), _w(1, 1), np.array([True, False])).tolist() == [[False, False]]


def test_generic_over_dtype():
    rng = np.random.default_rng(2)
    w = rng.random((3, 4, 6)).astype(np.float32)
    w[0, 1] = 0; w[1, :, 3] = 0; w[2, 2, 1] = NAN
    ids = np.array([[0, 1, 2, 0], [1, 1, 5, 0], [2, 0, 1, 1]])
    pres = R.present(ids, w, {0, 1, 2})
    w32, w64 = R.normalise(w, pres), R.normalise(w, pres, np.float64)
    assert w32.dtype == np.float32 and w64.dtype == np.float64
    assert np.abs(w32 - w64).max() <= 2.0 ** -23
    assert np.abs(w64.sum(1) - pres.any(1)[:, None]).max() <= 1e-15          # every part of a window with a component sums to 1
    feats = rng.standard_normal((3, 4, 90, 256)).astype(np.float32)
    F32, F64 = R.blend(w32, feats), R.blend(w32, feats, np.float64)
    bound = 5 * 2.0 ** -23 * np.abs(w32[:, :, np.arange(90) % 6, None].astype(np.float64) * feats).sum(1)
    assert (np.abs(F32 - F64) <= bound).all()
