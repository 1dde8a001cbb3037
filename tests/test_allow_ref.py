"""Action-constrained matching without a GPU: the float64 restatement (tests/allow_ref.py) against the reference pin
(tests/golden/action_match.npz: scikit-learn's BallTree over the picked action's subset, train_CVAE.py:198-211) and against brute force;
the any / granule tables; the ``action_mask`` helper; the bindings' argument counts against the header's."""
import ctypes as C
import inspect
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import allow_ref as ar  # noqa: E402
import make_golden_action_match as gen  # noqa: E402
import scan_ref as sr  # noqa: E402

import mocha_sigasia2023_amd as M  # noqa: E402
from mocha_sigasia2023_amd import _C  # noqa: E402
from mocha_sigasia2023_amd.multi_character import allow_masks  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def fixture_problem():
    """(fixture, bank rows, seg_start, labels, queries, characters, masks) rebuilt from the fixture's seeds."""
    z = np.load(os.path.join(REPO, "tests", "golden", "action_match.npz"))
    assert [int(z["cnt_norm_seed"])] + z["char_seeds"].tolist() == [gen.CNT_NORM_SEED] + [c[0] for c in gen.CHARACTERS]
    assert z["char_runs"].tolist() == [list(c[1]) for c in gen.CHARACTERS] and z["query_seed"].tolist() == [gen.QUERY_SEED, gen.Q, gen.TRAPS]
    bk = gen.banks()
    q, cha, act = gen.queries(bk)
    assert np.array_equal(cha, z["character"]) and np.array_equal(act, z["action"])
    assert np.array_equal(bk[0][1], z["labels0"]) and np.array_equal(bk[1][1], z["labels1"])
    rows = np.concatenate([b[0] for b in bk])
    labels = np.concatenate([b[1] for b in bk])
    seg_start = np.concatenate([[0], np.cumsum([len(b[1]) for b in bk])])
    return z, rows, seg_start, labels, q, cha, [ar.action_mask([a]) for a in act]


def test_restatement_equals_the_reference_pin():
    z, rows, seg_start, labels, q, cha, masks = fixture_problem()
    idx, gidx, d2, applied = ar.search(q, rows, cha, seg_start, labels, masks, 1)
    assert np.array_equal(idx[:, 0], z["idx"]) and (applied == 1).all()
    assert np.allclose(np.sqrt(d2[:, 0]), z["dist"], rtol=1e-12, atol=0)        # float64 both: BallTree's reduced distance and the direct form
    # the index inside the subset, as BallTree returned it
    for i in range(len(cha)):
        lo = int(seg_start[cha[i]])
        picked = np.flatnonzero(labels[lo:int(seg_start[cha[i] + 1])] == z["action"][i])
        assert picked[z["subset_idx"][i]] == idx[i, 0] and gidx[i, 0] == lo + idx[i, 0]
    # the traps: the plain answer is a row of another action
    plain, _, _, ap0 = ar.search(q, rows, cha, seg_start, labels, [0] * len(cha), 1)
    assert np.array_equal(plain[:, 0], z["plain_idx"]) and (ap0 == 0).all()
    t = int(z["query_seed"][2])
    assert (plain[:t, 0] != idx[:t, 0]).all()
    assert ar.gaps_ok(q, rows, cha, seg_start, labels, masks, rows.view(np.uint32), 1) >= sr.MIN_GAP


def test_restatement_equals_brute_force_and_the_fallback_rule():
    r = np.random.default_rng(5)
    sizes = [1, 15, 16, 17, 33, 49]
    seg_start = np.concatenate([[0], np.cumsum(sizes)])
    N, D = int(seg_start[-1]), 64
    rows = r.standard_normal((N, D)).astype(np.float32)
    rows[40] = rows[35]                                                         # copies inside segment 3 (rows 32 .. 48 of the bank): local rows 3 and 8
    labels = r.integers(0, 4, N).astype(np.int32)
    labels[seg_start[1]:seg_start[2]] = 63                                      # a segment of one label: masks without bit 63 fall back
    labels[35], labels[40] = 1, 2
    Q = 40
    seg = r.integers(-1, 7, Q)
    masks = [int(m) for m in r.integers(0, 16, Q)]
    masks[0], masks[1], masks[2] = 0, ar.ALL, 1 << 63
    q = r.standard_normal((Q, D)).astype(np.float32)
    q[3], seg[3], masks[3] = rows[35], 3, ar.action_mask([2])                   # the lower copy is inadmissible: the higher one wins
    q[4], seg[4], masks[4] = rows[35], 3, ar.action_mask([1, 2])                # both admissible: the lower one wins
    for k in (1, 2, 5, 8):
        idx, gidx, d2, applied = ar.search(q, rows, seg, seg_start, labels, masks, k)
        assert np.array_equal(idx, ar.brute(q, rows, seg, seg_start, labels, masks, k)), k
        assert idx[3, 0] == 40 - seg_start[3] and idx[4, 0] == 35 - seg_start[3] and d2[3, 0] == 0 and d2[4, 0] == 0
        anys = ar.any_table(labels, seg_start)
        for i in range(Q):
            s = int(seg[i])
            if not 0 <= s < 6:
                assert applied[i] == 0 and (idx[i] == -1).all() and np.isposinf(d2[i]).all()
                continue
            want = 0 if masks[i] == 0 else (1 if masks[i] & anys[s] else -1)
            assert applied[i] == want
            if want != 1:                                                       # the unconstrained answer, to the bit
                pi, _, pd = sr.seg_search(q[i:i + 1], rows, seg[i:i + 1], seg_start, k)
                assert np.array_equal(pi[0], idx[i]) and np.array_equal(pd[0], d2[i])
            else:
                lab = labels[seg_start[s]:seg_start[s + 1]]
                got = idx[i][idx[i] >= 0]
                assert all((masks[i] >> int(lab[j])) & 1 for j in got)
                assert len(got) == min(k, sum((masks[i] >> int(v)) & 1 for v in lab))


def test_any_and_granule_tables():
    labels = np.array([0] * 16 + [1] * 1 + [5] * 15 + [63] * 17 + [2], np.int32)
    seg_start = [0, 17, 49, 50]
    assert ar.any_table(labels, seg_start) == [0b11, (1 << 5) | (1 << 63), 0b100]
    start, gran = ar.granule_table(labels, seg_start)
    assert start == [0, 2, 4, 5]
    # segment 0: 16 rows of label 0, then one of label 1; segment 1: 15 rows of label 5 then 17 of label 63 - its first granule holds both
    assert gran == [1, 2, (1 << 5) | (1 << 63), 1 << 63, 0b100]


def test_action_mask_helper():
    assert M.action_mask is not None and "action_mask" in M.__all__
    assert M.action_mask([]) == 0 and M.action_mask([0]) == 1 and M.action_mask([63]) == 1 << 63 and M.action_mask(3) == 8
    assert M.action_mask([1, 1, 5]) == 0b100010 and M.action_mask(np.array([2, 3])) == 0b1100 and M.action_mask(range(64)) == ar.ALL
    for bad in ([64], [-1], [1.5], 64, ["a"], [True]):
        with pytest.raises(ValueError):
            M.action_mask(bad)
    # host-side allow: one int for all, or one entry per query (an int mask, labels, None); checked before anything is launched
    cpu = "cpu"
    assert allow_masks(5, 3, cpu, "x").tolist() == [5, 5, 5]
    assert allow_masks([None, [0, 2], 1 << 63], 3, cpu, "x").tolist() == [0, 5, -(1 << 63)]
    assert allow_masks([ar.ALL], 1, cpu, "x").tolist() == [-1] and allow_masks([ar.ALL], 1, cpu, "x").dtype.is_floating_point is False
    assert np.array_equal(ar.as_int64([0, 5, 1 << 63, ar.ALL]), np.array([0, 5, -(1 << 63), -1]))
    for bad in ([[64]], [1 << 64], [-1], [1, 2]):
        with pytest.raises(ValueError):
            allow_masks(bad, 1, cpu, "x")


def _header_arg_counts():
    txt = open(os.path.join(REPO, "include", "mocha_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    out = {}
    for name, args in re.findall(r"\b(mocha_[a-z_0-9]+)\s*\(([^;{]*?)\)\s*;", code, flags=re.S):
        args = args.strip()
        out[name] = 0 if args in ("", "void") else args.count(",") + 1
    return out


NEW = ["mocha_bank_set_labels", "mocha_match_segmented_allow", "mocha_characterize_segmented_allow", "mocha_step_graph_segmented_allow",
       "mocha_live_step_allow", "mocha_live_step_raw_allow"]


def test_binding_argument_counts_equal_the_headers():
    counts = _header_arg_counts()
    sig = _C.SIGNATURES
    for n in NEW + ["mocha_match_segmented", "mocha_live_step_inert", "mocha_live_step_raw"]:
        assert n in counts, f"{n} is not declared in include/mocha_hip.h"
        assert len(sig[n][1]) == counts[n], (n, len(sig[n][1]), counts[n])
    # the constrained calls are the plain ones plus (allow, applied) - and k for the matcher, (k, temperature, w_k) for the characterize
    assert len(sig["mocha_match_segmented_allow"][1]) == len(sig["mocha_match_segmented"][1]) + 3
    assert len(sig["mocha_characterize_segmented_allow"][1]) == len(sig["mocha_characterize_soft_segmented"][1]) + 2
    assert sig["mocha_step_graph_segmented_allow"][1] == sig["mocha_characterize_segmented_allow"][1]
    assert sig["mocha_live_step_allow"][1] == sig["mocha_live_step_inert"][1] + [C.c_void_p, C.c_void_p]
    assert sig["mocha_live_step_raw_allow"][1] == sig["mocha_live_step_raw"][1] + [C.c_void_p, C.c_void_p]


def test_python_surface():
    P = inspect.signature
    assert P(M.MultiCharacterBank.__init__).parameters["labels"].default is None
    assert P(M.MultiCharacterBank.query).parameters["allow"].default is None
    assert P(M.MultiCharacterBank.characterize).parameters["allow"].default is None
    assert hasattr(M.MultiCharacterBank, "set_labels")
    assert P(M.MultiStreamCharacterizer.__init__).parameters["constrained"].default is False
    assert P(M.MultiStreamCharacterizer.step).parameters["allow"].default is None
    assert P(M.LiveSession.__init__).parameters["constrained"].default is False
    assert P(M.LiveSession.push).parameters["allow"].default is None and callable(M.LiveSession.set_allow)
    # the CVAE branch's seed match searches the whole character: it refuses the option before it looks at anything else
    with pytest.raises(ValueError, match="constrained"):
        M.LiveOursSession(None, None, None, None, None, None, None, None, constrained=True)
