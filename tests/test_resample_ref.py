"""tests/resample_ref.py against the resampler's definition evaluated with the reference's own quat functions (tests/golden/resample.npz,
written by tests/golden/make_golden_resample.py): no GPU.  The floats lie within resample_ref.E, the measured largest deviation, which the
test prints; the streaming restatement equals the whole-clip one exactly on every prefix; outputs that fall on a source frame are that
frame; the output counts are the Fraction-based ones."""
import os
import sys
from fractions import Fraction

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import resample_ref as RR  # noqa: E402

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "resample.npz")
RATIOS = [(2, 1), (1, 2), (3, 2), (5, 3), (5, 6), (2, 5), (1, 1)]


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(GOLD))


def test_fixture_describes_itself(gold):
    assert [tuple(r) for r in gold["ratios"].tolist()] == RATIOS and gold["lengths"].tolist() == [1, 2, 3, 7, 45]
    assert gold["orders"].tolist() == ["zyx", "yzx"] and gold["rot"].shape == (45, 24, 3) and gold["rot"].dtype == np.float32
    assert os.path.getsize(GOLD) <= os.path.getsize(os.path.join(os.path.dirname(GOLD), "clip_ingest.npz"))
    q = RR.quats(gold["rot"], "zyx")
    raw = RR.euler_to_quat(gold["rot"].astype(np.float64), [2, 1, 0])
    flips = (np.sum(raw[:, 1:] * raw[:, :-1], axis=0) < 0).sum(axis=0)
    assert flips[12] >= 1 and flips[int(gold["spin"])] >= 3, flips
    assert np.all(np.sum(q[:, 1:] * q[:, :-1], axis=0) > 0), "unrolled quaternions with a negative consecutive dot"
    assert np.array_equal(q[:, :, int(gold["static"])], np.repeat(q[:, :1, int(gold["static"])], 45, axis=1))


def test_fixture(gold):
    worst = {"rot": 0.0, "pos": 0.0}
    for order in gold["orders"].tolist():
        for num, den in RATIOS:
            for n in gold["lengths"].tolist():
                q, p = RR.resample_clip(gold["rot"][:n], gold["pos"][:n], order, num, den)
                m = RR.count(n, num, den)
                assert q.shape == (m, 24, 4) and p.shape == (m, 24, 3)
                worst["rot"] = max(worst["rot"], float(np.abs(q - gold[f"q_{order}_{num}_{den}"][:m]).max()))
                worst["pos"] = max(worst["pos"], float(np.abs(p - gold[f"p_{num}_{den}"][:m]).max()))
    print("largest |restatement - reference composition|:", {k: f"{v:.3g}" for k, v in worst.items()})
    assert max(worst.values()) <= RR.E, worst
    assert max(worst.values()) >= RR.E / 10.0, ("the recorded deviation is more than ten times what is measured now", worst)
    small = [float(np.abs(v)[(v != 0) & (np.abs(v) < 1e-6)].size) for k, v in gold.items() if k[:2] in ("q_", "p_")]
    assert not any(small), "an output within 1e-6 of zero: there one fp32 spacing no longer covers a float64 rounding"


@pytest.mark.parametrize("order", ["zyx", "yzx"])
def test_outputs_on_a_source_frame_are_that_frame(gold, order):
    q = RR.quats(gold["rot"], order).transpose(1, 2, 0)
    p = gold["pos"].astype(np.float64)
    for num, den in RATIOS:
        oq, op = RR.resample_clip(gold["rot"], gold["pos"], order, num, den)
        hit = 0
        for k in range(len(oq)):
            i, a = RR.at(k, num, den)
            if a == 0.0:
                hit += 1
                assert np.array_equal(oq[k], q[i]) and np.array_equal(op[k], p[i]), (num, den, k)
        assert hit == sum(1 for i in range(45) if (i * den) % num == 0), (num, den)      # source frame i is output i den / num
    one_q, one_p = RR.resample_clip(gold["rot"], gold["pos"], order, 1, 1)
    assert np.array_equal(one_q, q) and np.array_equal(one_p, p)
    two_q, _ = RR.resample_clip(gold["rot"], gold["pos"], order, 2, 1)
    assert np.array_equal(two_q, q[::2])


@pytest.mark.parametrize("num,den", [r for r in RATIOS if r[1] <= 4 * r[0]])
@pytest.mark.parametrize("order", ["zyx", "yzx", None])
def test_streaming_equals_whole_clip_on_every_prefix(gold, order, num, den):
    rot = gold["rot"] if order is not None else RR.quats(gold["rot"], "zyx").transpose(1, 2, 0).astype(np.float32) * \
        np.where(np.arange(45) % 3 == 1, -1.0, 1.0).astype(np.float32)[:, None, None]
    s = RR.StreamRef(order, num, den)
    qs, ps = [], []
    for j in range(45):
        out = s.push(rot[j], gold["pos"][j])
        assert len(out) == RR.push_count(j, num, den)[0] <= RR.MAX_OUT
        qs += [o[0] for o in out]
        ps += [o[1] for o in out]
        wq, wp = RR.resample_clip(rot[:j + 1], gold["pos"][:j + 1], order, num, den)
        assert len(qs) == len(wq) == RR.count(j + 1, num, den)
        assert np.array_equal(np.stack(qs), wq) and np.array_equal(np.stack(ps), wp), ("prefix", j + 1)


def test_restart_emits_the_new_frame(gold):
    s = RR.StreamRef("zyx", 1, 2)
    for j in range(10):
        s.push(gold["rot"][j], gold["pos"][j])
    s.restart()
    out = s.push(gold["rot"][10], gold["pos"][10])
    fresh = RR.quats(gold["rot"][10:11], "zyx")[:, 0].T
    assert len(out) == 2 and all(np.array_equal(o[0], fresh) and np.array_equal(o[1], gold["pos"][10].astype(np.float64)) for o in out)


def test_counts_are_the_fraction_ones():
    for num, den in RATIOS:
        step = Fraction(num, den)
        for n in range(1, 201):
            m = RR.count(n, num, den)
            assert m == sum(1 for k in range(2 * n * den + 2) if k * step <= n - 1), (n, num, den)
            assert (m - 1) * step <= n - 1 < m * step
            if den <= 4 * num:
                assert sum(RR.push_count(j, num, den)[0] for j in range(n)) == m
                assert all(RR.push_count(j, num, den)[0] <= -(-den // num) for j in range(n))
