"""tests/clip_ingest_ref.py against the reference's own process_data (tests/golden/clip_ingest.npz, written by
tests/golden/make_golden_clip_ingest.py): no GPU.  Contacts and the windowing are exact; the floats of the plain cases lie within
clip_ingest_ref.E and those of the mirrored cases within E_MIRROR, the measured largest deviations, which the test prints."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import clip_ingest_ref as CR  # noqa: E402

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "clip_ingest.npz")
ROLES, TOES = (7, 9, 16, 1, 20), (5, 24)
FLOATS = ("pos", "vel", "rot", "ang")


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(GOLD))


def _run(gold, n, mirrored):
    return CR.process_clip(gold["rot"][:n], gold["pos"][:n], gold["parents"], str(gold["order"]), ROLES, TOES,
                           mirror_map=gold["mirror_map"] if mirrored else None)


@pytest.mark.parametrize("mirrored", [False, True], ids=["plain", "mirror"])
def test_fixture(gold, mirrored):
    tag, bound = ("mirror", CR.E_MIRROR) if mirrored else ("plain", CR.E)
    worst = {k: 0.0 for k in FLOATS}
    for n in gold["lengths"]:
        out = _run(gold, int(n), mirrored)
        assert np.array_equal(out["contact"], gold[f"{tag}_{n}_contact"]), (tag, n)
        for k in FLOATS:
            worst[k] = max(worst[k], float(np.abs(out[k] - gold[f"{tag}_{n}_{k}"]).max()))
    print(f"largest |restatement - reference|, {tag}:", {k: f"{v:.3g}" for k, v in worst.items()})
    assert max(worst.values()) <= bound, (tag, worst)
    assert max(worst.values()) >= bound / 10.0, ("the recorded deviation is more than ten times what is measured now", tag, worst)


def test_mirror_changes_the_clip(gold):
    a, b = gold["plain_100_pos"], gold["mirror_100_pos"]
    assert np.abs(a - b).max() > 1e-2 and gold["plain_100_contact"].any() and not gold["plain_100_contact"].all()
    assert not np.array_equal(gold["plain_100_contact"], gold["mirror_100_contact"])


@pytest.mark.parametrize("tag,step,pick", [("w30", 30, None), ("w1", 1, "w1_index")])
def test_windows_exact(gold, tag, step, pick):
    """divide applied to the reference's processed clip gives the reference's windows bit for bit, padding included."""
    full = {k: gold[f"plain_100_{k}"] for k in FLOATS + ("contact",)}
    w = CR.windows(full, 60, step)
    assert len(w["Ypos"]) == CR.window_count(100, 60, step) == (3 if step == 30 else 85)
    sel = slice(None) if pick is None else gold[pick]
    for key, name in (("Ypos", "pos"), ("Yvel", "vel"), ("Yrot", "rot"), ("Yang", "ang"), ("contact", "contact")):
        assert np.array_equal(w[key][sel], gold[f"{tag}_{name}"]), (tag, key)
    last = w["Yvel"][-1]
    m = min(60, 100 - (len(w["Ypos"]) - 1) * step)
    left = (60 - m) // 2 + (60 - m) % 2
    assert not last[:left].any() and not last[left + m:].any() and last[left:left + m].any()


def test_window_counts():
    assert [CR.window_count(n, 60, 1) for n in (31, 60, 100)] == [16, 45, 85]
    assert [CR.window_count(n, 60, 30) for n in (31, 100)] == [1, 3]
    assert CR.window_count(15, 60, 1) == 0
