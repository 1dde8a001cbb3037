"""tests/inertial_ref.py, the float64 restatement the inertialize kernel is held to, pinned without a GPU to tests/golden/inertialize.npz -
arrays the reference's own inertialize_transition_* / inertialize_update_* produced (tests/golden/make_golden_inertial.py)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import inertial_ref as R                                                    # noqa: E402

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "inertialize.npz")
TOL = 1e-12


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(GOLD))


def test_fixture_is_what_the_issue_describes(gold):
    g = gold
    F, n, V, _ = g["heads"].shape
    assert (F, n, V) == (24, 3, 22) and g["heads"].dtype == np.float32
    cut = g["ids"][1:] != g["ids"][:-1]
    assert not cut[:, 0].any()
    assert (np.nonzero(cut[:, 1])[0] + 1).tolist() == [5, 6, 9]
    assert g["hl"].tolist() == [0.02, 0.1, 1.0, 0.0]
    assert np.array_equal(g["heads"][5, 1, 0, 3:7], g["heads"][4, 1, 0, 3:7])          # a transition between identical rotations
    assert np.signbit(g["heads"][3, 0, 2, 0]) and g["heads"][3, 0, 2, 0] == 0           # the planted -0.0


def test_restatement_equals_the_reference_on_the_main_run(gold):
    g = gold
    F, n, V, _ = g["heads"].shape
    ref = R.InertialRef(n, V, halflife=0.1)
    for f in range(F):
        out = ref.step(g["heads"][f], ids=g["ids"][f])
        assert np.abs(out - g["out"][f]).max() <= TOL, f
        for name, mine in (("off_pos", ref.off_pos), ("off_vel", ref.off_vel), ("off_ang", ref.off_ang), ("off_rot", ref.off_rot)):
            assert np.abs(mine - g[name][f]).max() <= TOL, (name, f)
    assert ref.single_valued()
    w = np.concatenate(ref.monitor["w"])
    assert (w < 0).any(), "the fixture holds an offset with w < 0 before quat.abs"
    assert (np.concatenate(ref.monitor["len"]) == 0.0).any(), "the fixture holds the len < eps branch"
    # it really inertializes: at stream 1's first switch the raw positions jump (0.83), the output's do not (0.043; ordinary frames 0.053)
    raw = np.abs(g["heads"][5, 1, :, :3].astype(np.float64) - g["heads"][4, 1, :, :3]).max()
    smooth = np.abs(g["out"][5, 1, :, :3] - g["out"][4, 1, :, :3]).max()
    assert raw > 3 * smooth, (raw, smooth)


@pytest.mark.parametrize("i", range(4))
def test_restatement_equals_the_reference_at_every_half_life(gold, i):
    g = gold
    F, _, V, _ = g["heads"].shape
    ref = R.InertialRef(1, V, halflife=float(g["hl"][i]))
    for f in range(F):
        out = ref.step(g["heads"][f, 2:3], trigger=g["hl_trigger"][i, f:f + 1], valid=g["hl_valid"][i, f:f + 1])
        if g["hl_valid"][i, f]:
            assert np.abs(out[0] - g["hl_out"][i, f]).max() <= TOL, f
        else:
            assert np.isnan(out).all() and np.isnan(g["hl_out"][i, f]).all() and not ref.seen[0] and not ref.active[0]
    assert ref.single_valued()


def test_ids_and_triggers_are_the_same_transitions(gold):
    g = gold
    F, n, V, _ = g["heads"].shape
    a, b = R.InertialRef(n, V), R.InertialRef(n, V)
    for f in range(F):
        trig = (g["ids"][f] != g["ids"][f - 1]).astype(np.int32) if f else np.zeros(n, np.int32)
        assert np.array_equal(a.step(g["heads"][f], ids=g["ids"][f]), b.step(g["heads"][f], trigger=trig))


def test_a_stream_that_never_transitions_gets_its_input_back_bit_for_bit(gold):
    g = gold
    F, n, V, _ = g["heads"].shape
    ref = R.InertialRef(n, V)
    for f in range(F):
        out = ref.step(g["heads"][f], ids=g["ids"][f]).astype(np.float32)
        assert np.array_equal(out[0].view(np.uint32), g["heads"][f, 0].view(np.uint32)), f
    assert not ref.active[0] and ref.active[1] and ref.active[2]


def test_seeded_inputs_obey_the_two_conditions():
    """The seeded inputs of tests/test_inertialize_kernel.py, checked here on the CPU."""
    for seed, n, V in R.SEEDED:
        heads, ids = R.switched_streams(seed, 24, n, V)
        ref = R.InertialRef(n, V)
        for f in range(24):
            ref.step(heads[f], ids=ids[f])
        assert ref.single_valued(), (seed, n, V)
        assert ref.active[min(1, n - 1):].all() and (n == 1 or not ref.active[0])
