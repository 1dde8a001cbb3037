"""tests/bvh_fmt_ref.py, the integer restatement of the BVH writer's number format, against Python's own "%f" - the reference writer's
format operator (motion/bvh.py:215-222) - on the hard list and 200 000 seeded float64 values, and against the MOTION blocks of the golden
files, which the reference's writer wrote itself: formatting the arrays of tests/golden/bvh_parse.npz reproduces them byte for byte.
No GPU."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bvh_fmt_ref as R  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TAGS = ("mocha24_rot", "mocha24_pos", "mixamo22")


def test_hard_list_equals_percent_f():
    hard = R.hard_values()
    assert len(hard) == 2 * (6 + 14 * 5 + 5 + 9 + 12 + 1)
    for x in hard:
        assert R.token(x) == "%f" % x, (x.hex(), R.token(x), "%f" % x)
    # what the list is there for: ties go to even, a carry makes a new digit, the sign is the sign bit
    assert R.token(1 / 128) == "0.007812" and R.token(3 / 128) == "0.023438"
    assert R.token(0.9999995) == "1.000000" and R.token(0.9999994999) == "0.999999" and R.token(9.9999996) == "10.000000"
    assert R.token(-0.0) == "-0.000000" and R.token(-1e-9) == "-0.000000" and R.token(5e-324) == "0.000000"
    assert sorted({len(R.token(x).split(".")[0]) for x in hard if x > 0}) == list(range(1, 13))
    assert len(R.token(-math.nextafter(1e12, 0.0))) == 20


def test_refused_values():
    for x in (float("nan"), float("inf"), -float("inf"), 1e12, -1e12, 1e300):
        assert R.token(x) is None
    assert R.token(math.nextafter(1e12, 0.0)) == "999999999999.999878"


def test_seeded_values_equal_percent_f():
    vals = R.random_values(20261, 200000)
    assert float(np.abs(vals).max()) < 1e12 and float(np.abs(vals).min()) >= 2.0 ** -41 and (vals < 0).sum() > 90000
    ex = np.frexp(vals)[1]
    assert ex.min() == -39 and ex.max() == 40                  # frexp's exponent is one above the binade's
    bad = [(x.hex(), R.token(x), "%f" % x) for x in vals.tolist() if R.token(x) != "%f" % x]
    assert not bad, bad[:5]


@pytest.mark.parametrize("tag", TAGS)
def test_golden_motion_blocks(tag):
    gold = dict(np.load(os.path.join(GOLDEN, "bvh_parse.npz")))
    names, parents, pos, rot, offsets, order, frametime = R.golden_arrays(gold, tag)
    text = R.golden_file(os.path.join(GOLDEN, "bvh", tag + ".bvh"), tag)
    line = text.index(b"Frame Time:")
    block = text[text.index(b"\n", line) + 1:]
    M = R.columns(pos, rot, list(range(len(names))), order, tag == "mocha24_pos")     # the files list their joints depth-first
    assert M.shape == (40, 6 * len(names) if tag == "mocha24_pos" else 3 + 3 * len(names))
    assert R.motion_text(M, R.token) == block
    assert R.motion_text(M) == block
