"""tests/bvh_ref.py, the project's restatement of the reference's BVH loader, against what the reference's own bvh.load returned for the
three fixture files (tests/golden/bvh_parse.npz, written by tests/golden/make_golden_bvh.py): bit for bit in float64.  No GPU."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bvh_ref  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TAGS = ("mocha24_rot", "mocha24_pos", "mixamo22")


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(os.path.join(GOLDEN, "bvh_parse.npz")))


@pytest.mark.parametrize("tag", TAGS)
def test_restatement_equals_the_reference(gold, tag):
    with open(os.path.join(GOLDEN, "bvh", tag + ".bvh"), "rb") as f:
        got = bvh_ref.load(f.read())
    for k in ("rotations", "positions", "offsets"):
        want = gold[f"{tag}_{k}"]
        assert got[k].dtype == np.float64 and got[k].shape == want.shape
        assert np.array_equal(got[k].view(np.uint64), want.view(np.uint64)), (tag, k)
    assert np.array_equal(got["parents"], gold[f"{tag}_parents"])
    assert got["names"] == [str(n) for n in gold[f"{tag}_names"]]
    assert got["order"] == str(gold[f"{tag}_order"])
    assert got["frametime"] == float(gold[f"{tag}_frametime"])
    assert got["channels"] == (6 if tag == "mocha24_pos" else 3)


def test_fixture_files_are_what_the_issue_describes():
    with open(os.path.join(GOLDEN, "bvh", "mixamo22.bvh"), "rb") as f:
        text = f.read()
    assert text.endswith(b"\r\n\r\n") and text.count(b"\n") == text.count(b"\r\n") and b"ROOT mixamorig:Hips" in text


def test_motion_tokens_split():
    words, vals = bvh_ref.motion_tokens(b"1.5 -0.000000\t2e1 \r\n\r\n  .5\n")
    assert words == ["1.5", "-0.000000", "2e1", ".5"]
    assert np.array_equal(vals, [1.5, -0.0, 20.0, 0.5]) and np.signbit(vals[1])
