"""The NumPy restatement of the streaming mocap front end (tests/ingest_ref.py) against the reference's own process_data, as recorded in
tests/golden/live_ingest.npz (tests/golden/make_golden_ingest.py): every prefix 31..100 of the clip, every stored lookahead, every bone."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ingest_ref as R  # noqa: E402

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "live_ingest.npz")
ROLES = (7, 9, 16, 1, 20)       # Spine2, LeftShoulder, RightShoulder, LeftUpLeg, RightUpLeg of the 'mocha' joint list
TOES = (5, 24)


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(GOLD))


@pytest.fixture(scope="module")
def runs(gold):
    """Per stored lookahead: the list of what each of the 100 pushes returned."""
    out = {}
    for L in gold["lookahead"]:
        st = R.IngestRef(gold["parents"], int(L), str(gold["order"]), ROLES, TOES)
        out[int(L)] = [st.push(gold["rot"][f], gold["pos"][f]) for f in range(len(gold["rot"]))]
    return out


def test_fixture(gold, runs):
    worst = {}
    for li, L in enumerate(gold["lookahead"]):
        frames = runs[int(L)]
        for n in range(R.FIRST, 101):
            o = frames[n - 1]
            assert o is not None
            for k in ("pos", "vel", "rot", "ang"):
                d = float(np.abs(o[k] - gold["out_" + k][li, n - R.FIRST]).max())
                worst[k] = max(worst.get(k, 0.0), d)
            assert np.array_equal(o["contact"], gold["out_contact"][li, n - R.FIRST]), (int(L), n)
    print("largest |restatement - reference|:", {k: f"{v:.3g}" for k, v in worst.items()})
    assert max(worst.values()) <= R.E, worst


def test_emission_starts_at_push_31(runs):
    for L, frames in runs.items():
        assert all(o is None for o in frames[:R.FIRST - 1]), L
        assert all(o is not None for o in frames[R.FIRST - 1:]), L


def test_lookahead_18_is_the_whole_clip(gold, runs):
    """With 18 frames of lookahead the emitted frame no longer depends on where the prefix ends: it is the whole clip's frame."""
    for n in range(R.FIRST, 101):
        o, t = runs[18][n - 1], n - 1 - 18
        for k in ("pos", "vel", "rot", "ang"):
            assert np.abs(o[k] - gold["full_" + k][t]).max() <= R.E, (k, n)
        assert np.array_equal(o["contact"], gold["full_contact"][t]), n


def test_fixture_reference_lookahead_18_is_exact(gold):
    """The fixture's own claim: at L = 18 the reference's prefix frames ARE the whole clip's, difference exactly 0."""
    li = int(np.flatnonzero(gold["lookahead"] == 18)[0])
    t = np.arange(R.FIRST, 101) - 1 - 18
    for k in ("pos", "vel", "rot", "ang", "contact"):
        assert np.array_equal(gold["out_" + k][li], gold["full_" + k][t]), k


def test_derived_inputs(runs):
    """src_rvel / src_rang are the root's velocities in the root's frame; src_speed is 0 until 60 frames were emitted, then positive."""
    frames = runs[2]
    for n in range(R.FIRST, 101):
        o = frames[n - 1]
        back = R.q_mul_vec(o["rot"][0].astype(np.float32).astype(np.float64), o["src_rvel"])
        assert np.abs(back - o["vel"][0].astype(np.float32)).max() < 1e-6
        assert (o["src_speed"] > 0.0) == (n - R.FIRST + 1 >= 60)


def test_fit_rows():
    for W in (15, 31):
        H = R.fit_rows(W)
        x = np.arange(W) - W // 2
        for poly in (np.ones(W), x, x ** 2, x ** 3):          # a cubic is reproduced at every sample
            assert np.abs(H @ poly - poly).max() < 1e-9 * max(1.0, np.abs(poly).max())
        assert np.abs(H - H.T).max() < 1e-15
