"""The few-query scans and the segmented matchers against float64 at the kernel boundary (GPU cases: -m gpu; the reference pins and the
case-validity checks run everywhere).  The continuation of tests/test_match_kernels.py (its "family 4" and what was never in it).

What is held: match_stream.hip (mocha_match_stream<1|2|4|8, f32|bf16>, mocha_match_finish, mocha_match_topk_finish, mocha_match_refine),
match_scan8.hip (mocha_match_scan_adaptive<1|2|4>), match_segmented.hip (mocha_seg_plan, mocha_match_seg_scan, mocha_match_seg_finish),
match_seg_topk.hip (mocha_match_seg_keys, mocha_seg_topk_blend) and pointwise.hip's mocha_gather_blend / mocha_gather_rows.  The API tests
(test_edge_cases.py, test_scan8.py, test_multi_character.py, test_soft_match.py) run them only at D = 23040, only on the products of the
API's own earlier stages, and accept a near tie in place of the right index.  Here every launcher is called through
tests/gemm_probe/scan_probe.cpp on data the test AUTHORS, and the index must be the float64 answer with ties to the lowest row: NO near-tie
allowance.  The data pay for that: any two rows a result must order differ by exactly 0 (bit-identical copies) or by at least 1e-4 relative
in float64 d^2 (scan_ref.MIN_GAP, family 3's figure, about a hundred times the fp32 sum's error); that condition is asserted on the CPU
for every case (test_*_cases_are_valid), never skipped.

Family 4a - every row's key (launch_match_topk's keys, launch_match_scan16's and launch_match_scan8's keys behind the scratch head,
launch_match_seg_topk's keys) and the scan's per-workgroup minima: the decoded value against the float64 direct form through hold(),
relative, pooled per instance; the row in the low word exact; rows past the segment's end in the written range ~0; nothing else touched.
D in {chunk, 2 x chunk, 7680} (chunk = 1280 fp32, 1536 bf16), N in {1, 3, 15, 16, 17, 33, 257}, Q in {1, 2, 3, 4, 5, 8, 9, 17}: every (N, Q)
at D = chunk, two Latin rows of (N, Q) at the larger D.  Query 0's keys have the same bits whichever body computed them: the scan16 bodies
<1|2|4|8, bf16> and the segmented bodies <1|2|4|8> against launch_match_topk's <8>.  The byte image: D in {7680, 15360}, bytes and scales
from mp_to_i8, the value against the float64 distance to scale * (u8 - 128).
Family 4b - index and reported distance of launch_match_stream, _topk (k in {1, 2, 5, 8}), _scan16, _scan8, launch_match_segmented,
launch_match_seg_topk; winners at row 0, N - 1, both sides of the first 16-row workgroup, the last ragged workgroup, a bit-identical copy
of the winner at a higher row (same wave, next wave, next workgroup); fewer than k rows: -1 / +inf / 0; optional outputs null in turn; for
k = 1 the soft matcher's dist_k / idx0 / out equal launch_match_segmented's dist / idx and the enc row to the bit.
Family 4c - mocha_match_refine alone on authored keys (scan_ref.build_refine): keys = float64 distance + 0.9 of the stated bound
(rho_n + 2e-5 d) for the winner, - 0.9 for the decoys, every other row 1.1 bounds out and holding the TRAP row (the query itself: if a
pruned row were evaluated it would win).  Slices: per_slice = ceil(N / 64); keys in registers up to per_slice = 2 048 (N <= 131 072), re-read
beyond; index windows of 4 096 rows (a second window from N > 262 144).  N in {1, 63, 64, 65, 4097} at D in {256, 1536, 7680, 23040}; N in
{131072, 131073, 262145} at D = 256 (the bank is filled on the device; float64 over the candidate rows only); candidates 1, 2, 3, every
row; an all-identical bank; NaN keys; a query whose keys are all NaN; two launches on one scratch; the byte stage's mode words.
Family 5 - mocha_seg_plan alone (Q in {1, 7, 8, 9, 1023, 1024, 1025, 4096} x S in {1, 2, 5, Q + 3} x six id patterns), then the segmented
and soft launchers with device ids outside [0, S), segment sizes {1, 15, 16, 17, 33}, 1 .. 17 queries per segment, and a second soft group
whose segment is shorter than the first group's.
Weights and blends - w_k and mocha_gather_blend's implicit weights (read off a blend of unit rows) against the float64 softmax of the
distances the kernel itself reported / was given; the blends against the float64 weighted sum with the kernel's own weights;
temperatures {1e-3 x d, 1, 1e3}; mocha_gather_rows' clamping and bits.
Refusals - every hipErrorInvalidValue the launchers document and every PROBE_BAD_ARGUMENT of the contract in csrc/kernels.h; outputs keep
their guard pattern.

Kernel fix (family 4c found it; mocha_match_refine is on the streamed and live steps' path):
  NaN coarse keys were re-ranked instead of excluded.  The rule is "a NaN key never qualifies; no finite key at all: nothing is excluded",
  and the kernel's comments said so, but it formed d = sqrtf(fmaxf(key value, 0)) first and fmaxf(NaN, 0) is 0: a NaN key read as coarse
  distance 0 and ALWAYS qualified (and a query whose keys were all NaN took its bound from rho of the NaN minimum's row; every row still
  qualified, by the same accident).  Failing cases before the fix: n4097-d256-nan and n65-d1536-nan (a trap row with a NaN key won: idx 11
  for 0 and 4095, idx 4 for 64) and the pool after them; every other test of this file passed on the parent's kernel.  Now the smallest
  key is looked at first - NaN, +inf or the ~0 of an empty list means no finite key and every row is re-ranked - and a NaN key among finite
  ones returns false before the sqrt.  Finite keys take the same arithmetic as before.  The API-level suites pass unchanged (whole GPU
  suite: 1 751 passed = the parent's 1 674 + the 77 here); the demo benchmark alternating with the parent's library, 30 steps each:
  111.82 and 111.79 against 111.64 and 111.73 thousand frames/s.

Margins.  (4, 2) on the largest / rms error of the fp32 CPU evaluation (numpy's fp32 sum of the same direct form; the same softmax / blend
formula in fp32) for EVERY instance, the weights included: __expf did not need the 2-ulp-perturbed exponential (scan_ref.exp_2ulp is pinned
and unused).  Measured on an MI355X (77 GPU tests, every one passed, none skipped, no near tie accepted; 5.4 s for the file on the GPU box,
CPU references and case building included; the 9 CPU tests take 6 s), worst case largest ratio, then the rms ratio pooled over every
output of the instance (a case has fewer than 4 096 outputs, so the rms is held in the pool):
  keys f32 1.53, pooled 1.01 (24 920 keys)        keys b16 1.13 / 1.01 (24 920)         keys scan16 1.13 / 1.01 (24 920; the bits of keys b16)
  keys scan8 1.00 / 1.02 (1 749)                  keys seg f32 1.29 / 1.07 (5 427)      keys seg b16 1.52 / 1.06 (5 382)
  distances (relative, all within one fp32 ulp): stream 0.89 / 0.98 (f32 / b16, 342 each), topk 1.02 / 1.04 (1 766), scan16 1.25 (375),
  scan8 1.67 (20), refine 1.34 (101), segmented 0.95 / 0.87 (555), soft 0.99 / 1.02 (3 977 / 3 739)
  soft weights 1.58, pooled 0.90 (8 582)          soft blend 1.00 / 1.00 (7.2 M)        gather_blend 1.23 / 0.87 (141 372)
  mocha_gather_blend's implicit weights: 0.01 of the fp32 evaluation of its own scale-then-subtract form (the compiler contracts
  -dist * inv_temp - max into one fused multiply-add, so the product is never rounded), and against the DIFFERENCE-form yardstick - the
  bound the soft matcher is held to - 1.4 / 1.7 / 2.4 at temperatures 1e-3 d / 1 / 1e3: inside (4, 2) there as well.  That rests on the
  contraction; match_seg_topk.hip's subtract-first form does not.
Mutations, each built on a scratch copy (never committed; wrong numbers only, no access moves), failing tests of the 77 here / of the 52
tests of tests/test_edge_cases.py, test_scan8.py, test_multi_character.py and test_soft_match.py:
  (a) the refine's re-read branch taking rho one row off (rho[n - 1], row 0 its own): 6 (every case of N = 131 073 and 262 145 that is
      not all-identical - c3, c2, copy - and the pool) / 0.  The branch runs nowhere else.
  (b) mocha_match_topk_finish comparing v >= prev: 7 (all six (type, D) groups of test_scan_keys_indices_and_distances - pass r + 1 finds
      pass r's key again - and the body-bits test that reads what they leave) / 2 (test_top_k_query_and_soft_blend).
  (c) mocha_seg_plan splitting blocks at 7 instead of 8 in the count only: 12 (test_seg_plan at every Q >= 8, the segmented and soft
      cases with 8 or more queries of one segment, both second-group tests) / 6 (test_segmented_match_exact[False],
      test_characterize_segmented, test_segmented_topk_exact, test_soft_k1_is_the_hard_characterize).  The API-level files do see this one.
  (d) the soft blend's weights normalised over k instead of over the neighbours present: 7 (cases a, b, c of
      test_segmented_and_soft_matchers - the 1-row and 15-row segments at k = 2 .. 8 - and the pool) / 1 (test_short_segment_and_weights).
  (e) the refine rule without its 2e-5 d terms: 2 (n64-d7680-copy - a bit-identical copy of the winner with rho = 0 for both, where the
      terms are the whole bound - and the pool) / 0.  With a gap of >= 1e-4 in d^2 a decoy cannot sit inside 2 x 2e-5 d of the winner, so
      only the copy cases can show it.
"""
import functools
import itertools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import match_ref as mr  # noqa: E402
import scan_ref as sr  # noqa: E402
from test_match_kernels import DEFAULT_MARGIN, MARGINS, POOL, RATIOS, call, hold, hold_pool  # noqa: E402,F401
from test_pointwise_kernels import GUARD, SENTINEL, D as todev, Out, T, dev, same_bits  # noqa: E402

gpu = pytest.mark.gpu
ONE_ULP = float(np.spacing(np.float32(1.0)))
NS = (1, 3, 15, 16, 17, 33, 257)
QS = (1, 2, 3, 4, 5, 8, 9, 17)
KS = (1, 2, 5, 8)
QMAX = 17
CHUNK = {False: sr.CHUNK_F32, True: sr.CHUNK_BF16}
SCAN_PARAMS = [(bf16, D) for bf16 in (False, True) for D in (CHUNK[bf16], 2 * CHUNK[bf16], 7680)]


def combos(bf16, D):
    """(N, Q) pairs of one (type, D): all of them at D = chunk, two Latin rows (every N, every Q) at the larger D."""
    if D == CHUNK[bf16]:
        return list(itertools.product(NS, QS))
    return [(N, QS[(i + t) % len(QS)]) for t in (0, 3) for i, N in enumerate(NS)] + [(257, 17), (33, 9)]


@functools.lru_cache(maxsize=None)
def bank(bf16, D, N):
    """One bank per (type, D, N) with QMAX queries: a case of Q queries takes the first Q, so query 0 is the same under every body."""
    return sr.build_bank(f"{'b16' if bf16 else 'f32'}-d{D}-n{N}", N, D, QMAX, bf16, copies=(NS.index(N) + D // CHUNK[bf16]) % 2 == 1)


# =================================================================================================== no GPU: the restatements are what they claim
def test_reference_distance_and_neighbours_are_cdist_and_a_stable_sort():
    r = sr.rng("pin-dist")
    q, b = r.standard_normal((5, 96), dtype=np.float32), r.standard_normal((41, 96), dtype=np.float32)
    b[7] = b[3]; b[40] = b[3]                                                   # ties: the lower row first
    want = torch.cdist(T(q).double(), T(b).double()).pow(2).numpy()
    got = sr.dist2(q, b)
    assert np.allclose(got, want, rtol=1e-12, atol=0) and got.dtype == np.float64
    assert sr.dist2(q, b, np.float32).dtype == np.float32 and np.allclose(sr.dist2(q, b, np.float32), want, rtol=1e-5)
    idx, val = sr.knn(got, 8)
    order = torch.argsort(T(got), dim=1, stable=True)[:, :8].numpy()
    assert np.array_equal(idx, order) and np.array_equal(val, np.take_along_axis(got, order, 1))
    one = sr.dist2(b[3:4], b)
    assert list(sr.knn(one, 4)[0][0][:3]) == [3, 7, 40] and sr.nn(one)[0][0] == 3
    idx, val = sr.knn(got[:, :3], 5)                                            # fewer than k rows
    assert (idx[:, 3:] == -1).all() and np.isinf(val[:, 3:]).all() and (idx[:, :3] >= 0).all()


def test_reference_key_preserves_order_and_inverts():
    v = np.float32([0.0, 1e-45, 1e-30, 1.0, 1.0000001, 3e38, np.inf, -0.0, -1e-30, -2.5])
    k = sr.pack_key(v, np.zeros(len(v), np.int64))
    by_value = sorted(range(len(v)), key=lambda i: (float(v[i]), 0 if np.signbit(v[i]) else 1))
    assert sorted(range(len(v)), key=lambda i: int(k[i])) == by_value
    assert int(sr.pack_key(np.float32([np.nan]), [0])[0]) > int(k.max()) and int(sr.pack_key(np.float32([np.nan]), [5])[0]) < int(sr.NOKEY)
    back, row = sr.unpack_key(sr.pack_key(v, np.arange(len(v)) * 1000003))
    assert same_bits(back, v) and np.array_equal(row, np.arange(len(v)) * 1000003)
    assert int(sr.pack_key(np.float32([2.0]), [7])[0]) < int(sr.pack_key(np.float32([2.0]), [8])[0])      # ties to the lower row
    assert int(sr.pack_key(np.float32([1.0]), [3])[0]) == (0xBF800000 << 32) | 3
    assert np.isnan(sr.unpack_key(sr.pack_key(np.float32([np.nan]), [9]))[0][0])
    keys = sr.pack_key(np.arange(40, dtype=np.float32)[::-1].copy(), np.arange(40))[None]
    assert [int(x) & 0xFFFFFFFF for x in sr.wg_minima(keys)[0]] == [15, 31, 39]


def test_reference_candidate_rule_is_the_stated_inequality():
    r = sr.rng("pin-rule")
    d = (10 + r.random(200)).astype(np.float32)
    rho = (0.2 * r.random(200)).astype(np.float32)
    keys = sr.pack_key((d * d).astype(np.float32), np.arange(200))
    keys[17] = sr.pack_key(np.float32([np.nan]), [17])[0]
    got = sr.refine_candidates(keys, rho)
    dd = np.sqrt(sr.unpack_key(keys)[0].astype(np.float64))
    m = min((i for i in range(200) if i != 17), key=lambda i: (dd[i], i))
    want = [i for i in range(200) if i != 17 and (i == m or dd[i] - rho[i] - 2e-5 * dd[i] <= dd[m] + rho[m] + 2e-5 * dd[m])]
    assert list(got) == want and 1 < len(want) < 199
    allnan = sr.pack_key(np.full(9, np.nan, np.float32), np.arange(9))
    assert list(sr.refine_candidates(allnan, rho[:9])) == list(range(9))


def _sorted_plan(seg, S):
    order = sorted((int(s), q) for q, s in enumerate(seg) if 0 <= int(s) < S)
    out = []
    for s, q in order:
        if out and out[-1][0] == s and len(out[-1][1]) < 8:
            out[-1][1].append(q)
        else:
            out.append((s, [q]))
    return out


def test_reference_plan_is_a_sorted_list_cut_in_eights():
    r = sr.rng("pin-plan")
    for Q, S in ((1, 1), (9, 1), (40, 5), (100, 3), (17, 20)):
        seg = r.integers(-1, S + 1, Q)
        p = sr.plan(seg, S)
        assert p == _sorted_plan(seg, S)
        assert len(p) <= sr.blocks_bound(Q, S)
        assert sorted(q for _, qs in p for q in qs) == [q for q in range(Q) if 0 <= seg[q] < S]
    assert sr.plan([0] * 17, 1) == [(0, list(range(8))), (0, list(range(8, 16))), (0, [16])]
    assert sr.blocks_bound(17, 1) == 3 and sr.blocks_bound(16, 16) == 16 and sr.blocks_bound(4096, 1) == 512


def test_reference_weights_and_blend_are_torch_softmax_and_a_matmul():
    r = sr.rng("pin-soft")
    d = (100 + 3 * r.random((6, 8))).astype(np.float32)
    present = np.ones((6, 8), bool); present[2, 5:] = False; present[4, :] = False
    for t in (0.1, 1.0, 1e3):
        x = torch.where(T(present), -T(d).double() / float(np.float32(t)), torch.tensor(-np.inf, dtype=torch.float64))
        want = torch.nan_to_num(torch.softmax(x, 1), nan=0.0).numpy()
        for fn in (sr.weights_scaled, sr.weights_diff):
            w = fn(d, t, present)
            assert np.allclose(w, want, rtol=1e-9, atol=1e-300), (fn.__name__, t)
            assert (w[~present] == 0).all() and np.allclose(w.sum(1)[[0, 1, 2, 3, 5]], 1)
            assert fn(d, t, present, np.float32).dtype == np.float32
    # at a temperature far below the distances the fp32 evaluation of the scaled form loses digits the difference form keeps
    w64 = sr.weights_diff(d, 0.1, present)
    e_scaled = np.abs(sr.weights_scaled(d, 0.1, present, np.float32) - w64).max()
    e_diff = np.abs(sr.weights_diff(d, 0.1, present, np.float32) - w64).max()
    assert e_diff < 1e-6 and e_scaled > 4 * e_diff
    y = sr.exp_2ulp(np.float32([-3.0, -2.0, -1.0, 0.0]))
    off = np.abs(y.astype(np.float64) - np.exp(np.float64([-3, -2, -1, 0]))) / np.spacing(np.exp(np.float32([-3, -2, -1, 0])))
    assert (off > 1.0).all() and (off < 3.1).all(), off                         # 2 ulp of the result, give or take the fp32 result's own rounding
    enc = r.standard_normal((12, 20), dtype=np.float32)
    rows = r.integers(0, 12, (6, 8)); rows[~present] = -1
    w = sr.weights_diff(d, 1.0, present)
    want = np.stack([sum(w[q, j] * enc[rows[q, j]].astype(np.float64) for j in range(8) if rows[q, j] >= 0) + np.zeros(20) for q in range(6)])
    assert np.allclose(sr.blend(w, rows, enc), want, rtol=1e-12, atol=1e-15)


def test_reference_segmented_search_is_a_search_per_segment():
    k = seg_case("pin", False)
    for i, s in enumerate(k.seg):
        if 0 <= s < k.S:
            lo, hi = k.seg_start[s], k.seg_start[s + 1]
            d = torch.cdist(T(k.scan_query[i:i + 1]).double(), T(k.values[lo:hi]).double())[0].pow(2)
            order = torch.argsort(d, stable=True)[:8].numpy()
            n = len(order)
            assert np.array_equal(k.idx[i, :n], order) and (k.idx[i, n:] == -1).all() and np.array_equal(k.gidx[i, :n], order + lo)
        else:
            assert (k.idx[i] == -1).all() and np.isinf(k.d2_64[i]).all()


# =================================================================================================== no GPU: every authored case is valid
def test_scan_cases_are_valid_and_cover():
    """The gap condition of every bank, before anything is launched: the 9 nearest rows of every query (operands the scan sees) and the
    winner of the exact re-rank (fp32 rows) are separated by exactly 0 (bit-identical copies) or >= 1e-4 relative in float64 d^2; winners
    sit on every edge row; the copies come after their originals."""
    firsts, steps = set(), set()
    for bf16, D in SCAN_PARAMS:
        assert D % CHUNK[bf16] == 0
        pairs = combos(bf16, D)
        assert {n for n, _ in pairs} == set(NS) and {q for _, q in pairs} == set(QS)
        for N in NS:
            k = bank(bf16, D, N)
            assert k.gap is not None and k.gap >= sr.MIN_GAP, (k.name, k.gap)
            assert k.x_gap is not None and k.x_gap >= sr.MIN_GAP, (k.name, k.x_gap)
            w = int(sr.nn(k.d2_64[:1])[0][0])
            firsts.add((N, w))
            if k.twin is not None:
                assert k.twin > w and np.array_equal(k.bits[k.twin], k.bits[w]) and list(sr.knn(k.d2_64[:1], 2)[0][0]) == [w, k.twin]
                steps.add(k.twin - w)
            if N >= 18:
                assert len({int(v) for v in sr.nn(k.d2_64)[0]}) >= 2                # several anchors: the queries do not all share a winner
    assert {(257, 0), (257, 256)} & firsts and {w for n, w in firsts if n == 257} & {15, 16, 17, 255, 256, 240, 239} and steps >= {1}
    print("winner rows", sorted(firsts), "copy steps", sorted(steps))


REFINE_SMALL_N = (1, 63, 64, 65, 4097)
REFINE_SMALL_D = (256, 1536, 7680, 23040)
REFINE_LARGE_N = (131072, 131073, 262145)


def refine_specs():
    """name -> build_refine arguments.  Small banks: every (N, D) with the candidate count walking 1, 2, 3, all; large banks at D = 256."""
    specs = {}
    counts = (1, 2, 3, "all")
    for i, (N, D) in enumerate(itertools.product(REFINE_SMALL_N, REFINE_SMALL_D)):
        c = counts[(i + i // 4) % 4]
        if c == "all" and N * D > 4097 * 1536:
            c = 3                                                               # (every row of 4 097 x 7 680: 126 MB of float64 for nothing new)
        nq = 1 if c == "all" else (1, 3, 8, 2)[i % 4]
        c = c if c == "all" else min(c, max(1, N // nq))
        nq = nq if c == "all" else min(nq, N // c)
        specs[f"n{N}-d{D}-c{c}"] = dict(N=N, D=D, nq=nq, ncand=c)
    specs["n65-d256-all"] = dict(N=65, D=256, nq=1, ncand="all")
    specs["n4097-d1536-all"] = dict(N=4097, D=1536, nq=1, ncand="all")
    specs["n4097-d256-same"] = dict(N=4097, D=256, nq=2, ncand=1, allsame=True)
    specs["n64-d7680-copy"] = dict(N=64, D=7680, nq=2, ncand=2, copy=True)
    specs["n4097-d256-copy"] = dict(N=4097, D=256, nq=3, ncand=3, copy=True)
    specs["n4097-d256-nan"] = dict(N=4097, D=256, nq=3, ncand=3, nan_rows=40, all_nan_query=True)
    specs["n65-d1536-nan"] = dict(N=65, D=1536, nq=2, ncand=2, nan_rows=7, all_nan_query=True)
    for N in REFINE_LARGE_N:
        specs[f"n{N}-d256-c3"] = dict(N=N, D=256, nq=3, ncand=3)
        specs[f"n{N}-d256-c2"] = dict(N=N, D=256, nq=8, ncand=2)
    specs["n131073-d256-copy"] = dict(N=131073, D=256, nq=2, ncand=3, copy=True)
    specs["n262145-d256-same"] = dict(N=262145, D=256, nq=1, ncand=1, allsame=True)
    return specs


REFINE_SPECS = refine_specs()


@functools.lru_cache(maxsize=None)
def refine_case(name):
    return sr.build_refine(name, **REFINE_SPECS[name])


def test_refine_cases_are_valid_and_cover():
    """Every authored refine case on the CPU: the rule, evaluated in float64 AND in fp32 on the authored keys, keeps exactly the rows the
    case says; the scan's minimum names a decoy; the slice arithmetic puts candidates on both sides of every bound."""
    seen_counts, in_regs, windows = set(), set(), set()
    for name in REFINE_SPECS:
        k = refine_case(name)
        per = -(-k.N // sr.RF_SPLIT)
        assert per == k.per_slice
        in_regs.add(per <= sr.RF_KPT_ROWS)
        windows.add(-(-per // sr.RF_CAP))
        for i in range(k.nq):
            c64, c32 = sr.refine_candidates(k.keys[i], k.rho), sr.refine_candidates(k.keys[i], k.rho, np.float32)
            assert np.array_equal(c64, c32), (name, i)
            assert len(c64) == k.expect_cands[i], (name, i, len(c64), k.expect_cands[i])
            if k.expect_cands[i] < k.N:
                assert sorted(k.per_query[i]) == list(c64), (name, i)
            seen_counts.add(min(len(c64), 4) if len(c64) < k.N or k.N <= 3 else "all")
            m = int(k.wgmin[i].min() & np.uint64(0xFFFFFFFF))
            if 1 < k.expect_cands[i] and not np.isnan(sr.unpack_key(k.keys[i])[0]).all():
                assert m != k.winner[i], (name, i, "the coarse minimum is the winner")
        if k.N in REFINE_LARGE_N and not REFINE_SPECS[name].get("allsame"):
            rows = {v for mine in k.per_query for v in mine}
            lo_last = (k.N - 1) // per * per
            assert {0, per - 1, per, k.N - 1, lo_last} <= rows, (name, sorted(rows))
            if per > sr.RF_CAP:
                assert {sr.RF_CAP - 1, sr.RF_CAP, per + sr.RF_CAP} <= rows, (name, sorted(rows))
    assert seen_counts >= {1, 2, 3, "all"} and in_regs == {True, False} and windows == {1, 2}
    assert -(-131072 // 64) == 2048 and -(-131073 // 64) == 2049 and -(-262145 // 64) == 4097 and 63 * 4097 < 262145 < 64 * 4097


SEG_SIZES = (1, 15, 16, 17, 33)


def seg_specs():
    """name -> (sizes, ids).  Queries per segment 1, 2, 3, 4, 5 / 8, 9, 17, 1, 2 in shuffled order, ids outside [0, S) mixed in; the soft
    groups: 16 queries of the 33-row segment, then a 17th (and a 33rd) of a shorter one that is no multiple of 16 rows (15; the second group of g33: 17)."""
    r = sr.rng("seg-specs")
    specs = {}
    for name, counts in (("a", (1, 2, 3, 4, 5)), ("b", (8, 9, 17, 1, 2)), ("c", (5, 1, 8, 3, 9))):
        ids = [s for s, c in enumerate(counts) for _ in range(c)] + [-1, 5, -2 ** 31, 2 ** 31 - 1]
        specs[name] = (SEG_SIZES, [ids[i] for i in r.permutation(len(ids))])
    specs["pin"] = (SEG_SIZES, [4, 0, -1, 2, 2, 5, 1, 3, 3, 4])
    specs["g17"] = (SEG_SIZES, [4] * 16 + [1])
    specs["g33"] = (SEG_SIZES, [4] * 16 + [3] * 16 + [1])
    specs["g17bad"] = (SEG_SIZES, [4] * 15 + [7] + [3])
    specs["one"] = ((17,), [0, 0, 0])
    specs["bodies"] = (SEG_SIZES, [3] * 8 + [0] + [2] * 3 + [1] * 2)            # blocks of 8, 1, 3 and 2 queries in one group: the <8|1|4|2> bodies
    return specs


SEG_SPECS = seg_specs()
SEG_D = {False: (1280, 2560, 7680), True: (1536, 3072, 7680)}


@functools.lru_cache(maxsize=None)
def seg_case(name, bf16, D=None, spacing=0.1):
    sizes, ids = SEG_SPECS[name]
    D = CHUNK[bf16] if D is None else D
    return sr.build_segments(f"{name}-{'b16' if bf16 else 'f32'}-d{D}-s{spacing}", sizes, D, ids, bf16, spacing)


def test_segment_cases_are_valid_and_cover():
    per_seg = set()
    for name in SEG_SPECS:
        for bf16 in (False, True):
            k = seg_case(name, bf16)
            assert k.gap is not None and k.gap >= sr.MIN_GAP, (name, bf16, k.gap)
            per_seg |= {sum(1 for v in k.seg if v == s) for s in range(k.S)}
    assert per_seg >= {1, 2, 3, 4, 5, 8, 9, 17}
    k = seg_case("g17", False, spacing=2e-3)
    assert k.gap is not None and k.gap >= sr.MIN_GAP, k.gap
    for name in ("g17", "g33"):                                                 # item 4: the later group's segment is shorter, and ragged
        sizes, ids = SEG_SPECS[name]
        assert sizes[ids[-1]] < sizes[ids[0]] and sizes[ids[-1]] % 16 and len(ids) in (17, 33)


# =================================================================================================== GPU helpers
def nan_tail(a, rows=2):
    """A host fp32 array [n, cols] on the device in front of `rows` rows of NaN."""
    a = np.ascontiguousarray(a, np.float32)
    return todev(np.concatenate([a, np.full((rows, a.shape[1]), np.nan, np.float32)]))


def u16_tail(bits, rows=2):
    bits = np.ascontiguousarray(bits, np.uint16)
    return todev(np.concatenate([bits, np.full((rows, bits.shape[1]), 0x7FC0, np.uint16)]).view(np.int16))


def zeros64(words):
    return torch.zeros(int(words), dtype=torch.int64, device=dev())


def as_u64(t):
    return t.cpu().numpy().view(np.uint64)


class Raw:
    """A buffer of 32-bit words between sentinel guards whose elements need not all be written (a plan, a scratch)."""

    def __init__(self, words, fill=SENTINEL):
        self.words = int(words) + (int(words) & 1)
        self.buf = torch.full((2 * GUARD + self.words,), fill, dtype=torch.int32, device=dev())
        self.buf[:GUARD] = SENTINEL
        self.buf[GUARD + self.words:] = SENTINEL
        self.ptr = self.buf.data_ptr() + 4 * GUARD

    def host(self, what):
        h = self.buf.cpu().numpy()
        assert (h[:GUARD] == SENTINEL).all() and (h[GUARD + self.words:] == SENTINEL).all(), f"{what}: a guard word was overwritten"
        return h[GUARD:GUARD + self.words]

    def intact(self):
        return bool((self.buf == SENTINEL).all())


def hold_rel(inst, case, y, ref64, ref32, extra=None):
    """hold() on relative errors: every output divided by its own float64 value (distances of one case span a factor 200)."""
    s = np.where(np.asarray(ref64) > 0, ref64, 1.0).astype(np.float64)
    if extra is not None:
        e = np.where(extra[0] > 0, extra[0], 1.0)
        extra = (T(np.ravel(extra[0] / e)), T(np.ravel(extra[1].astype(np.float64) / e)))
    hold(inst, case, np.ravel(np.asarray(y, np.float64) / s), np.ravel(ref64 / s), np.ravel(np.asarray(ref32, np.float64) / s), ulp=ONE_ULP, extra=extra)


def ints(o, what):
    return o.check(what).view(np.int32)


_dev_cache = {}


def bank_on_device(k):
    """(bank, scan queries) of a build_bank case on the device, each in front of rows of NaN; cached per case."""
    if k.name not in _dev_cache:
        _dev_cache.clear()                                                      # one bank at a time
        b = u16_tail(k.bank16) if k.bf16 else nan_tail(k.rows)
        extra = (nan_tail(k.rows), nan_tail(k.query), todev(k.rho)) if k.bf16 else ()
        _dev_cache[k.name] = (b, nan_tail(k.scan_query)) + extra
    return _dev_cache[k.name]


def key_owner(Q, r):
    """The query whose keys row r of an 8-row key buffer holds after a launch that walked Q queries 8 at a time."""
    return r + 8 * ((Q - 1 - r) // 8)


_keys0 = {}


# =================================================================================================== families 4a / 4b: stream, topk, scan16
@gpu
@pytest.mark.parametrize("bf16,D", SCAN_PARAMS)
def test_scan_keys_indices_and_distances(bf16, D):
    """launch_match_stream, launch_match_topk and (bf16) launch_match_scan16 on every (N, Q) of this (type, D)."""
    L = sr.load()
    tag = "b16" if bf16 else "f32"
    for ci, (N, Q) in enumerate(combos(bf16, D)):
        k = bank(bf16, D, N)
        case = f"{tag}-d{D}-n{N}-q{Q}"
        dv = bank_on_device(k)
        dbank, dq = dv[0], dv[1]
        d64, d32 = k.d2_64[:Q], k.d2_32[:Q]
        extra = (k.d2_64, k.d2_32)
        ref_idx, ref_d2 = sr.knn(d64, sr.KMAX)
        rows = np.arange(Q)

        # ---- launch_match_stream: idx and dist (dist null every third case)
        words = L.sp_stream_scratch(Q, N)
        assert words == 8 * ((Q + 7) // 8) * ((N + 15) // 16)
        part = zeros64(words)
        idx, dist = Out((Q,)), (None if ci % 3 == 2 else Out((Q,)))
        rc = call(L.sp_match_stream, dbank.data_ptr(), int(bf16), dq.data_ptr(), Q, N, D, part.data_ptr(), words, idx.ptr, dist.ptr if dist else 0, 0)
        assert rc == 0, (case, rc)
        got = ints(idx, "stream idx")
        assert np.array_equal(got, ref_idx[:, 0]), (case, "stream", got, ref_idx[:, 0])
        if dist:
            hold_rel(f"scan: stream {tag} dist", case, dist.check("stream dist"), np.sqrt(ref_d2[:, 0]), np.sqrt(d32[rows, ref_idx[:, 0]]),
                     extra=(np.sqrt(extra[0]), np.sqrt(extra[1])))

        # ---- launch_match_topk: every row's key, the k nearest
        kk = KS[ci % 4]
        written = np.zeros((8, N), bool); written[:min(Q, 8)] = True
        keys, idxk, distk = Out((8, N), "f64", written), Out((Q, kk)), (None if ci % 3 == 1 else Out((Q, kk)))
        rc = call(L.sp_match_topk, dbank.data_ptr(), int(bf16), dq.data_ptr(), Q, N, D, kk, keys.ptr, 8 * N, idxk.ptr, distk.ptr if distk else 0, 0)
        assert rc == 0, (case, rc)
        kb = keys.check("topk keys").view(np.uint64)
        nrow = min(Q, 8)
        own = [key_owner(Q, r) for r in range(nrow)]
        val, row = sr.unpack_key(kb[:nrow])
        assert (row == np.arange(N)[None, :]).all(), (case, "the row in a key's low word")
        hold_rel(f"scan: keys {tag}", case, val, k.d2_64[own], k.d2_32[own], extra=extra)
        if Q <= 8:
            _keys0.setdefault((bf16, D, N), {})[("topk", Q)] = kb[0].copy()
        got = ints(idxk, "topk idx")
        assert np.array_equal(got, ref_idx[:, :kk]), (case, "topk", kk, got[:3], ref_idx[:3, :kk])
        if distk:
            dk = distk.check("topk dist")
            have = ref_idx[:, :kk] >= 0
            assert np.isposinf(dk[~have]).all(), (case, "a missing neighbour's distance")
            if have.any():
                sel = np.where(have, ref_idx[:, :kk], 0)
                hold_rel(f"scan: topk {tag} dist", case, dk[have], np.sqrt(ref_d2[:, :kk][have]), np.sqrt(np.take_along_axis(d32, sel, 1)[have]),
                         extra=(np.sqrt(extra[0]), np.sqrt(extra[1])))

        if not bf16:
            continue
        # ---- launch_match_scan16: the exact fp32 answer through the bf16 copy; its keys and minima behind the scratch head
        drows, dquery, drho = dv[2], dv[3], dv[4]
        words, head = L.sp_scan16_scratch_words(N), L.sp_scan16_head_words()
        assert words == head + 8 * N + 8 * ((N + 15) // 16) and head == 8 * 64 + 8 + 1
        x_idx, x_d2 = sr.nn(k.x_d2_64[:Q])
        scratch = Raw(2 * words, fill=0)
        outs = []
        for rep in range(2 if ci % 5 == 0 else 1):                              # twice on the same scratch: same bits, tickets left at zero
            idx, dist = Out((Q,)), (None if ci % 3 == 0 else Out((Q,)))
            rc = call(L.sp_match_scan16, dbank.data_ptr(), drho.data_ptr(), drows.data_ptr(), dq.data_ptr(), dquery.data_ptr(), Q, N, D,
                      scratch.ptr, words, idx.ptr, dist.ptr if dist else 0, 0)
            assert rc == 0, (case, rc)
            outs.append((ints(idx, "scan16 idx"), dist.check("scan16 dist") if dist else None))
        got, gd = outs[0]
        assert np.array_equal(got, x_idx), (case, "scan16", got, x_idx)
        if len(outs) > 1:
            assert np.array_equal(outs[1][0], got) and (gd is None or same_bits(outs[1][1], gd)), (case, "second launch")
        if gd is not None:
            hold_rel("scan: scan16 dist", case, gd, np.sqrt(x_d2), np.sqrt(k.x_d2_32[rows, x_idx]), extra=(np.sqrt(k.x_d2_64), np.sqrt(k.x_d2_32)))
        sc = scratch.host("scan16 scratch").view(np.uint64)
        assert not sc[8 * 64:head].any(), (case, "tickets / mode words not left at zero")
        k16 = sc[head:head + 8 * N].reshape(8, N)
        nwg = (N + 15) // 16
        wg = sc[head + 8 * N:head + 8 * N + 8 * nwg].reshape(8, nwg)
        assert np.array_equal(wg[:nrow], sr.wg_minima(k16[:nrow])), (case, "per-workgroup minima")
        val, row = sr.unpack_key(k16[:nrow])
        assert (row == np.arange(N)[None, :]).all()
        hold_rel("scan: keys scan16", case, val, k.d2_64[own], k.d2_32[own], extra=extra)
        if Q <= 8:
            _keys0[(bf16, D, N)][("scan16", Q)] = k16[0].copy()


@gpu
def test_query0_keys_do_not_depend_on_the_body():
    """The keys of query 0 of one bank, computed next to 0 .. 7 other queries by the <1|2|4|8> bodies (scan16) and by launch_match_topk's
    <8> body: the same bits."""
    if not _keys0:
        for bf16, D in SCAN_PARAMS[3:4]:
            test_scan_keys_indices_and_distances(bf16, D)
    n = 0
    for key, got in _keys0.items():
        first = next(iter(got.values()))
        for who, v in got.items():
            assert np.array_equal(v, first), (key, who)
            n += 1
    assert n >= 8
    bodies = {q for got in _keys0.values() for (who, q) in got if who == "scan16"}
    assert not any(k[0] for k in _keys0) or bodies >= {1, 2, 3, 5}


# =================================================================================================== the byte stage
S8_CASES = [(7680, 1, 1), (7680, 17, 2), (7680, 33, 3), (7680, 257, 4), (15360, 3, 4), (15360, 16, 1), (15360, 257, 2), (15360, 15, 3)]


@functools.lru_cache(maxsize=None)
def s8_bank(D, N):
    return sr.build_bank(f"s8-d{D}-n{N}", N, D, 4, True, copies=N % 2 == 1)


def _byte_image(k):
    """The byte image of a bank from the project's own mp_to_i8 (held in family 1): (bytes, scale, rho8) on the device and on the host."""
    M = mr.load()
    dx, dc = todev(k.rows), todev(k.centre)
    b8 = torch.zeros((k.N + 2) * k.D, dtype=torch.uint8, device=dev())          # (two rows of byte 0 behind the image: -128 scale, far away)
    sc, rh = torch.zeros(k.N, dtype=torch.float32, device=dev()), torch.zeros(k.N, dtype=torch.float32, device=dev())
    assert call(M.mp_to_i8, dx.data_ptr(), dc.data_ptr(), b8.data_ptr(), sc.data_ptr(), rh.data_ptr(), k.N, k.D, 0) == 0
    return b8, sc, rh, b8.cpu().numpy()[:k.N * k.D].reshape(k.N, k.D), sc.cpu().numpy()


@gpu
@pytest.mark.parametrize("D,N,Q", S8_CASES)
def test_scan8_keys_and_results(D, N, Q):
    """launch_match_scan8 with the mode words at zero: the keys behind the scratch head are the direct form against scale * (u8 - 128), the
    answer is the exact fp32 search's."""
    L = sr.load()
    k = s8_bank(D, N)
    case = f"s8-d{D}-n{N}-q{Q}"
    b8, sc, rh, u8, scale = _byte_image(k)
    img64 = scale.astype(np.float64)[:, None] * (u8.astype(np.float64) - 128)
    img32 = (scale[:, None] * (u8.astype(np.float32) - np.float32(128))).astype(np.float32)      # the fp32 evaluation rounds the image value once
    t64 = k.rows.astype(np.float64) - k.centre.astype(np.float64)[None, :]
    assert (rh.cpu().numpy().astype(np.float64) >= np.sqrt(((t64 - img64) ** 2).sum(1))).all()
    d64, d32 = sr.dist2(k.qc[:Q], img64), sr.dist2(k.qc[:Q], img32, np.float32)
    assert sr.gaps_ok(k.x_d2_64[:Q], k.rows.view(np.uint32), 1) is not None
    dbank, dq, drows, dquery, drho = bank_on_device(k)
    words, head = L.sp_scan16_scratch_words(N), L.sp_scan16_head_words()
    scratch = Raw(2 * words, fill=0)
    idx, dist = Out((Q,)), Out((Q,))
    rc = call(L.sp_match_scan8, b8.data_ptr(), sc.data_ptr(), rh.data_ptr(), dbank.data_ptr(), drho.data_ptr(), drows.data_ptr(), dq.data_ptr(),
              dquery.data_ptr(), Q, N, D, scratch.ptr, words, idx.ptr, dist.ptr, 0)
    assert rc == 0, (case, rc)
    x_idx, x_d2 = sr.nn(k.x_d2_64[:Q])
    got = ints(idx, "scan8 idx")
    assert np.array_equal(got, x_idx), (case, got, x_idx)
    hold_rel("scan: scan8 dist", case, dist.check("scan8 dist"), np.sqrt(x_d2), np.sqrt(k.x_d2_32[np.arange(Q), x_idx]),
             extra=(np.sqrt(k.x_d2_64), np.sqrt(k.x_d2_32)))
    s = scratch.host("scan8 scratch").view(np.uint64)
    assert not s[8 * 64:head - 1].any(), (case, "tickets")
    mode = s[head - 1:head].view(np.uint32)
    assert L.sp_scan8_mode_word() == head - 1 and mode[0] == 0 and mode[1] == 0, (case, mode)      # an uncrowded bank leaves the stage on
    k8 = s[head:head + 8 * N].reshape(8, N)
    val, row = sr.unpack_key(k8[:Q])
    assert (row == np.arange(N)[None, :]).all() and not k8[Q:].any()
    hold_rel("scan: keys scan8", case, val, d64, d32, extra=(sr.dist2(k.qc, img64), sr.dist2(k.qc, img32, np.float32)))
    nwg = (N + 15) // 16
    wg = s[head + 8 * N:head + 8 * N + 8 * nwg].reshape(8, nwg)
    assert np.array_equal(wg[:Q], sr.wg_minima(k8[:Q])), (case, "per-workgroup minima")


@gpu
def test_scan8_switches_itself_off_on_a_crowded_bank():
    """A bank of 13 x 64 identical rows: every row is a candidate, 13 > S8_DEGENERATE in every slice.  The first call scans the bytes and
    sets mode[1]; the second scans the bf16 copy: its keys are launch_match_scan16's bits.  Both answer row 0."""
    L = sr.load()
    N, D, Q = (sr.S8_DEGENERATE + 1) * sr.RF_SPLIT, 7680, 2
    r = sr.rng("s8-crowded")
    c = (0.1 * r.standard_normal(D, dtype=np.float32)).astype(np.float32)
    row = r.standard_normal(D, dtype=np.float32)
    k = sr.Case()
    k.name, k.N, k.D, k.bf16 = "s8-crowded", N, D, True
    k.rows, k.centre = np.repeat(row[None], N, 0), c
    k.query = (row[None] + 0.1 * r.standard_normal((Q, D), dtype=np.float32)).astype(np.float32)
    k.bank16 = mr.bf16_rne((k.rows - c[None]).astype(np.float32))
    k.scan_query = (k.query - c[None]).astype(np.float32)
    resid = np.sqrt((((k.rows[0].astype(np.float64) - c) - mr.bf16_value(k.bank16[0])) ** 2).sum())
    k.rho = np.full(N, np.nextafter(np.float32(1.001 * resid), np.float32(np.inf)), np.float32)
    b8, sc, rh, _, _ = _byte_image(k)
    dbank, dq, drows, dquery, drho = bank_on_device(k)
    words, head = L.sp_scan16_scratch_words(N), L.sp_scan16_head_words()
    scratch = Raw(2 * words, fill=0)
    want_d = np.sqrt(sr.dist2(k.query, k.rows[:1])[:, 0])
    modes, keys = [], []
    for rep in range(2):
        idx, dist = Out((Q,)), Out((Q,))
        rc = call(L.sp_match_scan8, b8.data_ptr(), sc.data_ptr(), rh.data_ptr(), dbank.data_ptr(), drho.data_ptr(), drows.data_ptr(), dq.data_ptr(),
                  dquery.data_ptr(), Q, N, D, scratch.ptr, words, idx.ptr, dist.ptr, 0)
        assert rc == 0
        assert (ints(idx, "idx") == 0).all() and np.allclose(dist.check("dist"), want_d, rtol=1e-6, atol=0), rep
        s = scratch.host("scratch").view(np.uint64)
        modes.append(tuple(int(v) for v in s[head - 1:head].view(np.uint32)))
        keys.append(s[head:head + Q * N].copy())
    assert modes == [(0, 1), (1, 1)], modes
    s16 = Raw(2 * words, fill=0)
    idx = Out((Q,))
    assert call(L.sp_match_scan16, dbank.data_ptr(), drho.data_ptr(), drows.data_ptr(), dq.data_ptr(), dquery.data_ptr(), Q, N, D, s16.ptr, words, idx.ptr, 0, 0) == 0
    k16 = s16.host("scan16 scratch").view(np.uint64)[head:head + Q * N]
    assert np.array_equal(keys[1], k16) and not np.array_equal(keys[0], k16)


# =================================================================================================== family 4c: the refine on authored keys
def _refine_bank(k):
    """The bank on the device: every row the trap, then the special rows; two rows of NaN behind it."""
    b = todev(k.trap).expand(k.N + 2, k.D).contiguous()
    b[k.N:] = float("nan")
    if len(k.srows):
        b[torch.from_numpy(k.srows).to(dev())] = todev(k.smat)
    return b


def _run_refine(L, k, b, scratch, *, nq=None, keys=None, rho16=None, rho8=None, mode=None, want_dist=True):
    nq = k.nq if nq is None else nq
    dk = todev((k.keys if keys is None else keys).view(np.int64))
    dw = todev(sr.wg_minima(k.keys if keys is None else keys).view(np.int64))
    dr = todev(k.rho if rho16 is None else rho16)
    d8 = None if rho8 is None else todev(rho8)
    dq = nan_tail(k.query)
    idx, dist = Out((nq,)), (Out((nq,)) if want_dist else None)
    rc = call(L.sp_match_refine, dk.data_ptr(), dw.data_ptr(), dw.shape[1], dr.data_ptr(), mr.ptr(d8), mode.ptr if mode else 0, b.data_ptr(),
              dq.data_ptr(), nq, k.N, k.D, idx.ptr, dist.ptr if dist else 0, scratch.ptr, L.sp_scan16_head_words(), 0)
    assert rc == 0, (k.name, rc)
    s = scratch.host("refine scratch").view(np.uint64)
    assert not s[8 * 64:8 * 64 + 8].any(), (k.name, "tickets not left at zero")
    return ints(idx, "refine idx"), (dist.check("refine dist") if dist else None)


@gpu
@pytest.mark.parametrize("name", list(REFINE_SPECS))
def test_refine_on_authored_keys(name):
    """The index is the float64 argmin over the rows the rule keeps although every decoy's key looks better than the winner's and every
    pruned row holds the trap; the distance is held against float64 on the winner's row; a second launch on the same scratch gives the same
    bits (dist null there in turn)."""
    L = sr.load()
    k = refine_case(name)
    b = _refine_bank(k)
    scratch = Raw(2 * L.sp_scan16_head_words(), fill=0)
    idx, dist = _run_refine(L, k, b, scratch)
    assert np.array_equal(idx, k.answer), (name, idx, k.answer)
    _refine_pool[name] = (dist.astype(np.float64) / k.d64, k.d32.astype(np.float64) / k.d64)      # held in test_refine_dist_pool
    idx2, dist2 = _run_refine(L, k, b, scratch, want_dist=name.endswith("c3"))
    assert np.array_equal(idx2, idx) and (dist2 is None or same_bits(dist2, dist)), name
    if REFINE_SPECS[name].get("allsame"):
        one = _run_refine(L, k, b, Raw(2 * L.sp_scan16_head_words(), fill=0), nq=1)      # the same bits as a run of one query
        assert one[0][0] == 0 and same_bits(one[1], np.ascontiguousarray(dist[:1])), name
        # ... and as a ONE-candidate run: every other row pruned by keys far out
        far = k.keys.copy()
        far[:, 1:] = sr.pack_key(np.full(k.N - 1, 1e30, np.float32), np.arange(1, k.N))[None]
        solo = _run_refine(L, k, b, Raw(2 * L.sp_scan16_head_words(), fill=0), keys=far)
        assert np.array_equal(solo[0], idx) and same_bits(solo[1], dist), (name, "one candidate against every row")


_refine_pool = {}


@gpu
def test_refine_dist_pool():
    """The refine's reported distance against float64 on the winner's row, bounded by the fp32 CPU evaluation of the same direct form; a
    case has 1 to 8 distances, so the relative errors of all cases are pooled (as test_match_kernels.test_selection_dist_pool does)."""
    for name in REFINE_SPECS:                                                  # (selected on its own: the cases this test pools are run here)
        if name not in _refine_pool:
            test_refine_on_authored_keys(name)
    got, r32 = (np.concatenate([v[j] for _, v in sorted(_refine_pool.items())]) for j in range(2))
    hold("scan: refine dist", f"{len(got)} distances, relative", got, np.ones_like(got), r32, ulp=ONE_ULP)


@gpu
def test_refine_byte_stage_mode_words():
    """mode[0] = 0 with rho8 given: the keys' bounds are rho8, and a slice with more than S8_DEGENERATE candidates sets mode[1] - exactly 12
    leave it, 13 set it.  mode[0] = 1: the bounds are rho16's; rho8 tiny and rho16 sound (and the other way round under mode[0] = 0) finds the
    winner only under the right reading."""
    L = sr.load()
    N, D = 4097, 256
    per = -(-N // sr.RF_SPLIT)
    for ncand, want in ((sr.S8_DEGENERATE, 0), (sr.S8_DEGENERATE + 1, 1)):
        rows = list(range(3 * per, 3 * per + ncand))                            # all in slice 3 (per_slice = 65 > 13)
        k = sr.build_refine(f"mode-{ncand}", N, D, 1, ncand, cand_rows=rows)
        assert sorted(sr.refine_candidates(k.keys[0], k.rho)) == rows and rows[-1] < 4 * per
        b = _refine_bank(k)
        tiny = np.full(N, 1e-6, np.float32)
        for m0, r16, r8 in ((0, tiny, k.rho), (1, k.rho, tiny)):
            mode = Raw(2, fill=0)
            mode.buf[GUARD] = m0
            idx, dist = _run_refine(L, k, b, Raw(2 * L.sp_scan16_head_words(), fill=0), rho16=r16, rho8=r8, mode=mode)
            assert np.array_equal(idx, k.answer), (ncand, m0, idx, k.answer)
            got = mode.host("mode")
            assert got[0] == m0 and got[1] == (want if m0 == 0 else 0), (ncand, m0, got)


# =================================================================================================== family 5: the plan alone
PLAN_Q = (1, 7, 8, 9, 1023, 1024, 1025, 4096)
PATTERNS = ("sorted", "reversed", "shuffled", "one", "bad", "bad-only")


def plan_ids(pattern, Q, S, r):
    ids = np.sort(r.integers(0, S, Q))
    if pattern == "reversed":
        ids = ids[::-1].copy()
    elif pattern == "shuffled":
        ids = r.permutation(ids)
    elif pattern == "one":
        ids = np.full(Q, S - 1)
    elif pattern in ("bad", "bad-only"):
        ids = r.permutation(ids).astype(np.int64)
        bad = np.array([-1, S, -2 ** 31, 2 ** 31 - 1])
        where = r.random(Q) < (0.3 if pattern == "bad" else 2.0)
        ids[where] = bad[r.integers(0, 4, int(where.sum()))]
    return ids.astype(np.int32)


def check_plan(plan, seg, S, what):
    want = sr.plan(seg, S)
    assert plan[0] == len(want) <= sr.blocks_bound(len(seg), S), (what, plan[0], len(want))
    for b, (s, qs) in enumerate(want):
        e = plan[1 + 10 * b:11 + 10 * b]
        assert e[0] == s and e[1] == len(qs) and list(e[2:2 + len(qs)]) == qs, (what, b, e, s, qs)


@gpu
@pytest.mark.parametrize("Q", PLAN_Q)
def test_seg_plan(Q):
    L = sr.load()
    assert L.sp_seg_max_q() == 4096 and L.sp_seg_topk_q() == 16 and L.sp_seg_topk_max_k() == 8
    for S, pattern in itertools.product((1, 2, 5, Q + 3), PATTERNS):
        seg = plan_ids(pattern, Q, S, sr.rng(f"plan-{Q}-{S}-{pattern}"))
        n = L.sp_seg_plan_ints(Q, S)
        assert n == 1 + 10 * sr.blocks_bound(Q, S)
        plan = Raw(n)
        rc = call(L.sp_seg_plan, todev(seg).data_ptr(), Q, S, plan.ptr, n, 0)
        assert rc == 0, (Q, S, pattern, rc)
        check_plan(plan.host("plan"), seg, S, (Q, S, pattern))


# =================================================================================================== segmented and soft matchers
def _seg_device(k):
    b = u16_tail(k.bank16) if k.bf16 else nan_tail(k.values)
    return b, nan_tail(k.scan_query), todev(k.seg), todev(k.seg_start), nan_tail(k.enc)


def _run_segmented(L, k, dv, max_rows, nulls=()):
    b, dq, dseg, dstart, _ = dv
    pw, pi = L.sp_seg_scratch_words(k.Q, max_rows), L.sp_seg_plan_ints(k.Q, k.S)
    part, plan = zeros64(pw + 1), Raw(pi)
    outs = {n: (None if n in nulls else Out((k.Q,))) for n in ("idx", "gidx", "dist")}
    rc = call(L.sp_match_segmented, b.data_ptr(), int(k.bf16), k.N, dq.data_ptr(), dseg.data_ptr(), k.Q, dstart.data_ptr(), k.S, max_rows, k.D,
              part.data_ptr(), pw, plan.ptr, pi, *[o.ptr if o else 0 for o in outs.values()], 0)
    assert rc == 0, (k.name, rc)
    check_plan(plan.host("plan"), k.seg, k.S, k.name)
    return {n: (None if o is None else (o.check(n) if n == "dist" else ints(o, n))) for n, o in outs.items()}


SOFT_OUTS = ("idx0", "idx_k", "dist_k", "w_k", "out")


def _run_soft(L, k, dv, max_rows, kk, temperature, nulls=(), enc=True):
    b, dq, dseg, dstart, denc = dv
    kw, pi = L.sp_seg_keys_words(max_rows), L.sp_seg_plan_ints(16, k.S)
    stride = kw // 16
    assert stride == -(-max_rows // 16) * 16
    keys, plan = Raw(2 * kw), Raw(pi)
    shapes = dict(idx0=(k.Q,), idx_k=(k.Q, kk), dist_k=(k.Q, kk), w_k=(k.Q, kk), out=(k.Q, k.D))
    outs = {n: (None if n in nulls else Out(shapes[n])) for n in SOFT_OUTS}
    rc = call(L.sp_match_seg_topk, b.data_ptr(), int(k.bf16), k.N, dq.data_ptr(), dseg.data_ptr(), k.Q, dstart.data_ptr(), k.S, max_rows, k.D,
              keys.ptr, kw, plan.ptr, pi, denc.data_ptr() if enc else 0, kk, temperature, *[o.ptr if o else 0 for o in outs.values()], 0)
    assert rc == 0, (k.name, rc)
    res = {n: (None if o is None else (ints(o, n) if n.startswith("idx") else o.check(n))) for n, o in outs.items()}
    res["keys"] = keys.host("soft keys").view(np.uint64)[:kw].reshape(16, stride)
    return res


def _valid(k):
    return (k.seg >= 0) & (k.seg < k.S)


def _check_soft(L, k, res, kk, temperature, tag, case, max_rows):
    """One soft launch against the restatement: neighbours, reported distances, the weights from THOSE distances, the blend from THOSE weights."""
    ok = _valid(k)
    want_idx = k.idx[:, :kk]
    if res["idx_k"] is not None:
        assert np.array_equal(res["idx_k"], want_idx), (case, res["idx_k"][:4], want_idx[:4])
    if res["idx0"] is not None:
        assert np.array_equal(res["idx0"], want_idx[:, 0]), case
    have = want_idx >= 0
    dk = res["dist_k"]
    if dk is not None:
        assert np.isposinf(dk[~have]).all(), case
        hold_rel(f"scan: soft {tag} dist", case, dk[have], np.sqrt(k.d2_64[:, :kk][have]), np.sqrt(k.d2_32[:, :kk][have]),
                 extra=(np.sqrt(k.d2_64[np.isfinite(k.d2_64)]), np.sqrt(k.d2_32[np.isfinite(k.d2_64)])))
    w = res["w_k"]
    if w is not None and dk is not None:
        assert (w[~have] == 0).all(), case
        dd = np.where(have, dk, 0)
        hold("scan: soft weights", case, w, sr.weights_diff(dd, temperature, have), sr.weights_diff(dd, temperature, have, np.float32))
        sums = w.sum(1)
        assert np.allclose(sums[have.any(1)], 1, atol=1e-6) and (sums[~have.any(1)] == 0).all(), case
    if res["out"] is not None and w is not None:
        g = np.where(have, k.gidx[:, :kk], -1)
        o = res["out"]
        assert same_bits(np.ascontiguousarray(o[~ok]), np.ascontiguousarray(np.repeat(k.enc[:1], int((~ok).sum()), 0))), (case, "an invalid id's out is enc[0]")
        if ok.any():
            hold("scan: soft blend", case, o[ok], sr.blend(w[ok], g[ok], k.enc), sr.blend(w[ok], g[ok], k.enc, np.float32))
    # family 4a: the keys of the LAST group of 16 queries (the buffer is reused group after group)
    q0 = (k.Q - 1) // 16 * 16
    stride = res["keys"].shape[1]
    for q in range(q0, k.Q):
        s = k.seg[q]
        if not 0 <= s < k.S:
            continue
        lo, n = int(k.seg_start[s]), k.sizes[s]
        n16 = -(-n // 16) * 16
        row = res["keys"][q - q0]
        val, r = sr.unpack_key(row[:n])
        assert np.array_equal(r, np.arange(n)) and (row[n:n16] == sr.NOKEY).all(), (case, q, "keys past the segment's end")
        full = sr.dist2(k.scan_query[q:q + 1], k.values[lo:lo + n])[0]
        full32 = sr.dist2(k.scan_query[q:q + 1], k.values[lo:lo + n], np.float32)[0]
        hold_rel(f"scan: keys seg {tag}", f"{case}-q{q}", val, full, full32, extra=(k.d2_64[np.isfinite(k.d2_64)], k.d2_32[np.isfinite(k.d2_64)]))
    return stride


@gpu
@pytest.mark.parametrize("bf16", [False, True])
@pytest.mark.parametrize("name", ["a", "b", "c", "one"])
def test_segmented_and_soft_matchers(name, bf16):
    """launch_match_segmented and launch_match_seg_topk on one multi-character bank: ids outside [0, S) give -1 / row 0 / +inf / weights 0 /
    enc[0] and leave the valid queries' bits alone; max_rows equal to and larger than the largest segment; outputs null in turn; k = 1 of the
    soft matcher is the hard matcher to the bit."""
    L = sr.load()
    tag = "b16" if bf16 else "f32"
    for di, D in enumerate(SEG_D[bf16] if name in ("a", "b") else SEG_D[bf16][:1]):
        k = seg_case(name, bf16, D)
        assert k.gap is not None and k.gap >= sr.MIN_GAP
        dv = _seg_device(k)
        ok = _valid(k)
        big = max(k.sizes)
        base = None
        for max_rows, nulls in ((big, ()), (big + 7, ("idx",)), (big, ("gidx",)), (big + 16, ("dist",))):
            res = _run_segmented(L, k, dv, max_rows, nulls)
            case = f"seg-{name}-{tag}-d{D}-m{max_rows}"
            if res["idx"] is not None:
                assert np.array_equal(res["idx"], k.idx[:, 0]), (case, res["idx"], k.idx[:, 0])
            if res["gidx"] is not None:
                assert np.array_equal(res["gidx"], np.where(ok, k.gidx[:, 0], 0)), case
            if res["dist"] is not None:
                assert np.isposinf(res["dist"][~ok]).all(), case
                hold_rel(f"scan: segmented {tag} dist", case, res["dist"][ok], np.sqrt(k.d2_64[ok, 0]), np.sqrt(k.d2_32[ok, 0]),
                         extra=(np.sqrt(k.d2_64[np.isfinite(k.d2_64)]), np.sqrt(k.d2_32[np.isfinite(k.d2_64)])))
                base = res if base is None else base
                assert same_bits(res["dist"], base["dist"]), (case, "max_rows changes no bit")
        # the valid queries alone, in the same order: the same bits (invalid ids in a launch change nothing for the others)
        if (~ok).any():
            sub = sr.Case()
            sub.__dict__.update(k.__dict__)
            sub.seg, sub.Q, sub.scan_query = k.seg[ok], int(ok.sum()), k.scan_query[ok]
            r2 = _run_segmented(L, sub, (dv[0], nan_tail(sub.scan_query), todev(sub.seg), dv[3], dv[4]), big)
            assert np.array_equal(r2["idx"], base["idx"][ok]) and same_bits(r2["dist"], np.ascontiguousarray(base["dist"][ok])), case
        # ---- the soft matcher
        dbar = float(np.sqrt(np.median(k.d2_64[ok, 0])))
        for kk, temperature, max_rows, nulls in ((1, 1.0, big, ()), (2, 1e-3 * dbar, big + 7, ("idx0",)), (5, 1.0, big, ("w_k",)), (8, 1e3, big, ("idx_k",)),
                                                 (8, 1e-3 * dbar, big + 16, ("dist_k",)), (5, 1e3, big, ("out",)), (2, 1.0, big, ())):
            if di and kk in (5,):
                continue
            case = f"soft-{name}-{tag}-d{D}-k{kk}-t{temperature:.3g}"
            res = _run_soft(L, k, dv, max_rows, kk, temperature, nulls)
            _check_soft(L, k, res, kk, temperature, tag, case, max_rows)
            if kk == 1:                                                         # promised in match_seg_topk.hip: the hard matcher's bits
                assert same_bits(res["dist_k"][:, 0].copy(), base["dist"]) and np.array_equal(res["idx0"], base["idx"]), case
                want = k.enc[np.where(ok, k.gidx[:, 0], 0)]
                assert same_bits(res["out"], want) and (res["w_k"][ok] == 1).all(), (case, "k = 1: out is the enc row")


@gpu
@pytest.mark.parametrize("bf16", [False, True])
def test_soft_matcher_second_group_and_body_bits(bf16):
    """Q = 17 and 33: the later group's segment is shorter than the first group's and no multiple of 16 rows - the keys a long segment left
    in the buffer must not be seen.  An invalid id in the middle of a group.  Tight shells (2e-3 in d^2) at temperature 1e-3 d: weights that
    are not 0 / 1.  Then the keys of a segment's first query against launch_match_topk's on that segment as a bank of its own: the segmented
    bodies <1|2|4|8> and the streaming <8> body give the same bits."""
    L = sr.load()
    tag = "b16" if bf16 else "f32"
    for name, spacing in (("g17", 0.1), ("g33", 0.1), ("g17bad", 0.1)) + ((("g17", 2e-3),) if not bf16 else ()):
        k = seg_case(name, bf16, None, spacing)
        assert k.gap is not None and k.gap >= sr.MIN_GAP
        dv = _seg_device(k)
        dbar = float(np.sqrt(np.median(k.d2_64[_valid(k), 0])))
        for kk, temperature in ((8, 1e-3 * dbar), (5, 1.0), (1, 1e3)):
            case = f"soft-{name}-{tag}-s{spacing}-k{kk}-t{temperature:.3g}"
            res = _run_soft(L, k, dv, max(k.sizes), kk, temperature)
            _check_soft(L, k, res, kk, temperature, tag, case, max(k.sizes))
            if spacing < 0.1 and kk == 8:
                w = res["w_k"]
                assert ((w > 0.01) & (w < 0.99)).sum() >= 3 * k.Q, (case, "the weights are all 0 / 1")
    for name in ("bodies",):
        k = seg_case(name, bf16)
        dv = _seg_device(k)
        res = _run_soft(L, k, dv, max(k.sizes), 1, 1.0)
        q0 = (k.Q - 1) // 16 * 16
        blocks = set()
        for q in range(q0, k.Q):
            s = k.seg[q]
            if not 0 <= s < k.S:
                continue
            lo, n = int(k.seg_start[s]), k.sizes[s]
            blocks.add(sum(1 for p in range(q0, k.Q) if k.seg[p] == s))
            sub = torch.cat([dv[0][lo:lo + n], dv[0][k.N:]])                    # the segment as a bank of its own, NaN rows behind it
            keys, idx = Out((8, n), "f64", np.arange(8)[:, None] < np.ones((1, n), int)), Out((1, 1))
            assert call(L.sp_match_topk, sub.data_ptr(), int(bf16), dv[1][q:].data_ptr(), 1, n, k.D, 1, keys.ptr, 8 * n, idx.ptr, 0, 0) == 0
            assert np.array_equal(keys.check("keys").view(np.uint64)[0], res["keys"][q - q0][:n]), (name, tag, q, "body bits")
        assert blocks == {1, 2, 3, 8}, blocks


# =================================================================================================== weights, blends, gathers
@gpu
def test_gather_blend_weights_and_blend():
    """mocha_gather_blend: its implicit weights, read off a blend of unit rows (w x 1 and sums with 0 are exact), against the float64 softmax
    of the distances it was given; then the blend of random rows against the float64 weighted sum with those weights.  Neighbours with an
    index < 0 or >= nrows are left out.  Temperatures {1e-3 x d, 1, 1e3} with the distances spread over three temperatures each time."""
    L = sr.load()
    r = sr.rng("gather-blend")
    Q, nrows = 33, 40
    for k, cols in ((1, 40), (2, 40), (5, 1028), (8, 256), (64, 64)):
        nrows = max(40, k)
        idx = np.stack([r.permutation(nrows)[:k] for _ in range(Q)]).astype(np.int32)
        if k > 1:
            idx[3, 1] = -1; idx[5, :] = -1; idx[7, k - 1] = nrows + 5
        present = (idx >= 0) & (idx < nrows)
        unit = np.zeros((nrows, max(cols, nrows + (-nrows) % 4)), np.float32)
        unit[np.arange(nrows), np.arange(nrows)] = 1
        src = r.standard_normal((nrows, cols), dtype=np.float32)
        for temperature in (0.1, 1.0, 1e3):
            case = f"k{k}-c{cols}-t{temperature:g}"
            dist = (100 + temperature * 3 * r.random((Q, k))).astype(np.float32)
            didx, ddist = todev(idx), todev(dist)
            o = Out((Q, unit.shape[1]))
            assert call(L.sp_gather_blend, nan_tail(unit).data_ptr(), didx.data_ptr(), ddist.data_ptr(), temperature, o.ptr, Q, k, unit.shape[1], nrows, 0) == 0
            wfull = o.check("unit blend")
            w = np.where(present, np.take_along_axis(wfull, np.where(present, idx, 0), 1), 0).astype(np.float32)
            assert np.allclose(wfull.sum(1), present.any(1).astype(np.float32), atol=1e-5), case
            w64 = sr.weights_scaled(dist, temperature, present)
            hold("scan: blend weights", case, w, w64, sr.weights_scaled(dist, temperature, present, np.float32))
            ediff = np.abs(sr.weights_diff(dist, temperature, present, np.float32) - w64).max()
            other = RATIOS.setdefault(f"scan: blend weights t={temperature:g} / difference-form yardstick", [0.0, 0.0])      # reported, not asserted
            other[0] = max(other[0], float(np.abs(w - w64).max() / max(ediff, 1e-300)))
            o = Out((Q, cols))
            assert call(L.sp_gather_blend, nan_tail(src).data_ptr(), didx.data_ptr(), ddist.data_ptr(), temperature, o.ptr, Q, k, cols, nrows, 0) == 0
            rows = np.where(present, idx, -1)
            hold("scan: gather_blend", case, o.check("blend"), sr.blend(w, rows, src), sr.blend(w, rows, src, np.float32))


@gpu
@pytest.mark.parametrize("cols", [4, 256, 1028])
def test_gather_rows_clamps_and_copies_bits(cols):
    L = sr.load()
    r = sr.rng(f"gather-rows-{cols}")
    nrows = 19
    src = r.standard_normal((nrows, cols), dtype=np.float32)
    src[4, 0] = np.float32(-0.0); src[6, cols - 1] = np.float32(1e-42)
    idx = np.array([0, 18, -5, nrows + 5, 4, 6, 6, -2 ** 31, 2 ** 31 - 1, 7], np.int32)
    o = Out((len(idx), cols))
    assert call(L.sp_gather_rows, nan_tail(src).data_ptr(), todev(idx).data_ptr(), o.ptr, len(idx), cols, nrows, 0) == 0
    assert same_bits(o.check("gather_rows"), src[np.clip(idx.astype(np.int64), 0, nrows - 1)])


# =================================================================================================== refusals: nothing is launched
@gpu
def test_scan_refusals():
    """Every hipErrorInvalidValue the launchers document and every PROBE_BAD_ARGUMENT of the contract (csrc/kernels.h); the outputs keep
    their guard pattern."""
    L = sr.load()
    BAD, INV = sr.BAD_ARGUMENT, sr.INVALID_VALUE
    k = bank(True, 7680, 17)
    dbank, dq, drows, dquery, drho = bank_on_device(k)
    N, D, Q = k.N, k.D, 2
    idx, dist = Out((64, 9)), Out((64, 9))                                      # (roomy: a refusal that launched after all must not run past them)
    part = zeros64(4096)
    head = L.sp_scan16_head_words()
    words = L.sp_scan16_scratch_words(N)
    scratch = zeros64(words)
    b, q, rw, qu, rh = dbank.data_ptr(), dq.data_ptr(), drows.data_ptr(), dquery.data_ptr(), drho.data_ptr()

    def refused(expect, fn, *args):
        assert call(fn, *args) == expect, (fn.__name__, args)
        assert idx.intact() and dist.intact(), fn.__name__

    # the streaming scan and the k-pass selection
    for kw in (dict(b=b + 2), dict(q=q + 4), dict(N=0), dict(N=2 ** 31), dict(D=0), dict(words=15), dict(idx=0), dict(part=0), dict(Q=0)):
        a = dict(dict(b=b, q=q, Q=Q, N=N, D=D, part=part.data_ptr(), words=4096, idx=idx.ptr), **kw)
        refused(BAD, L.sp_match_stream, a["b"], 1, a["q"], a["Q"], a["N"], a["D"], a["part"], a["words"], a["idx"], dist.ptr, 0)
    refused(INV, L.sp_match_stream, b, 1, q, Q, N, 1280, part.data_ptr(), 4096, idx.ptr, dist.ptr, 0)      # D off the bf16 chunk
    refused(INV, L.sp_match_stream, rw, 0, qu, Q, N, 1536, part.data_ptr(), 4096, idx.ptr, dist.ptr, 0)    # ... and off the fp32 chunk
    refused(BAD, L.sp_match_topk, b, 1, q, Q, N, D, 2, part.data_ptr(), 8 * N - 1, idx.ptr, dist.ptr, 0)
    refused(BAD, L.sp_match_topk, b, 1, q, Q, N, D, 2, part.data_ptr() + 4, 4096, idx.ptr, dist.ptr, 0)
    refused(INV, L.sp_match_topk, b, 1, q, Q, N, D, 0, part.data_ptr(), 4096, idx.ptr, dist.ptr, 0)
    refused(INV, L.sp_match_topk, b, 1, q, Q, N, 1280, 2, part.data_ptr(), 4096, idx.ptr, dist.ptr, 0)
    # the bf16-copy scan, the refine, the byte stage
    s16 = lambda **kw: (lambda a: (a["b"], rh, a["rw"], q, qu, a["Q"], a["N"], a["D"], a["s"], a["words"], idx.ptr, dist.ptr, 0))(
        dict(dict(b=b, rw=rw, Q=Q, N=N, D=D, s=scratch.data_ptr(), words=words), **kw))
    for kw in (dict(b=b + 8), dict(rw=rw + 4), dict(words=words - 1), dict(s=0), dict(N=0), dict(D=0)):
        refused(BAD, L.sp_match_scan16, *s16(**kw))
    for kw in (dict(D=1280), dict(D=1536 * 16), dict(D=768)):
        refused(INV, L.sp_match_scan16, *s16(**kw))
    dirty = zeros64(words)
    dirty[8 * 64 + 3] = 1                                                       # a ticket left behind by a launch that did not complete
    refused(BAD, L.sp_match_scan16, *s16(s=dirty.data_ptr()))
    keys = zeros64(8 * N + 64)
    rf = lambda **kw: (lambda a: (keys.data_ptr(), keys.data_ptr(), a["nwg"], rh, 0, 0, a["rw"], a["qu"], a["nq"], a["N"], a["D"], idx.ptr, dist.ptr,
                                  a["s"], a["words"], 0))(dict(dict(nwg=2, rw=rw, qu=qu, nq=2, N=N, D=D, s=scratch.data_ptr(), words=head), **kw))
    for kw in (dict(nq=9), dict(nq=0), dict(D=23040 + 256), dict(D=128), dict(D=384), dict(D=0), dict(N=0), dict(nwg=0), dict(words=head - 1), dict(rw=rw + 4),
               dict(qu=qu + 8), dict(s=dirty.data_ptr())):
        refused(BAD, L.sp_match_refine, *rf(**kw))
    s8 = lambda **kw: (lambda a: (b, rh, rh, b, rh, rw, q, qu, a["Q"], N, a["D"], a["s"], a["words"], idx.ptr, dist.ptr, 0))(
        dict(dict(Q=Q, D=D, s=scratch.data_ptr(), words=words), **kw))
    refused(INV, L.sp_match_scan8, *s8(Q=5))                                    # more than 4 queries for the byte stage
    refused(INV, L.sp_match_scan8, *s8(D=1536))                                 # D off the byte image's chunk
    refused(INV, L.sp_match_scan8, *s8(D=7680 * 4))                             # D > 23040
    refused(BAD, L.sp_match_scan8, *s8(words=words - 1))
    refused(BAD, L.sp_match_scan8, *s8(s=dirty.data_ptr()))
    # the gathers
    ii = todev(np.zeros(64, np.int32)).data_ptr()
    refused(INV, L.sp_gather_blend, rw, ii, rh, 0.0, dist.ptr, 1, 2, 8, N, 0)
    refused(INV, L.sp_gather_blend, rw, ii, rh, float("nan"), dist.ptr, 1, 2, 8, N, 0)
    refused(INV, L.sp_gather_blend, rw, ii, rh, -1.0, dist.ptr, 1, 2, 8, N, 0)
    refused(INV, L.sp_gather_blend, rw, ii, rh, 1.0, dist.ptr, 1, 0, 8, N, 0)
    refused(INV, L.sp_gather_blend, rw, ii, rh, 1.0, dist.ptr, 1, 65, 8, N, 0)
    refused(INV, L.sp_gather_blend, rw, ii, rh, 1.0, dist.ptr, 1, 2, 6, N, 0)
    refused(INV, L.sp_gather_blend, rw, ii, rh, 1.0, dist.ptr, 1, 2, 8, 0, 0)
    refused(BAD, L.sp_gather_blend, rw + 4, ii, rh, 1.0, dist.ptr, 1, 2, 8, N, 0)
    refused(BAD, L.sp_gather_blend, rw, ii, rh, 1.0, dist.ptr + 4, 1, 2, 8, N, 0)
    refused(INV, L.sp_gather_rows, rw, ii, dist.ptr, 1, 6, N, 0)
    refused(INV, L.sp_gather_rows, rw, ii, dist.ptr, 1, 8, 0, 0)
    refused(BAD, L.sp_gather_rows, rw, 0, dist.ptr, 1, 8, N, 0)
    refused(BAD, L.sp_gather_rows, rw + 8, ii, dist.ptr, 1, 8, N, 0)
    # the plan and the segmented matchers
    sk = seg_case("a", True, 1536)
    sb, sq, sseg, sstart, senc = _seg_device(sk)
    big = max(sk.sizes)
    plan = Raw(16 * 1024)
    pi = 16 * 1024
    segd = todev(np.zeros(5000, np.int32))
    for Qp, S in ((0, 1), (4097, 1), (4, 0)):
        refused(INV, L.sp_seg_plan, segd.data_ptr(), Qp, S, plan.ptr, pi, 0)
    refused(BAD, L.sp_seg_plan, segd.data_ptr(), 64, 64, plan.ptr, 10 * 64, 0)  # one int short
    refused(BAD, L.sp_seg_plan, 0, 4, 1, plan.ptr, pi, 0)
    assert plan.intact()
    pw = L.sp_seg_scratch_words(sk.Q, big)
    spart = zeros64(max(pw, 4097 * 4))

    def seg_args(**kw):
        a = dict(dict(b=sb.data_ptr(), rows=sk.N, q=sq.data_ptr(), Q=sk.Q, start=sstart.data_ptr(), S=sk.S, mr=big, D=sk.D, pw=pw, pi=pi), **kw)
        return (a["b"], 1, a["rows"], a["q"], sseg.data_ptr() if a["Q"] <= sk.Q else segd.data_ptr(), a["Q"], a["start"], a["S"], a["mr"], a["D"],
                spart.data_ptr(), a["pw"], plan.ptr, a["pi"])

    def table(v):
        return todev(np.asarray(v, np.int32)).data_ptr()

    bad_tables = (dict(start=table([0, 1, 1, 32, 49, 82])),                     # an EMPTY segment: its finish would read the next segment's row
                  dict(start=table([0, 1, 16, 32, 49, 49])),                    # ... the last one empty: a row past the bank
                  dict(start=table([1, 2, 16, 32, 49, 82])),                    # does not start at 0
                  dict(start=table([0, 16, 1, 32, 49, 82])),                    # decreasing
                  dict(rows=sk.N - 1),                                          # the table runs past the bank
                  dict(mr=big - 1), dict(mr=0), dict(S=0))
    for kw in bad_tables + (dict(pw=pw - 1), dict(pi=L.sp_seg_plan_ints(sk.Q, sk.S) - 1), dict(b=sb.data_ptr() + 8), dict(q=sq.data_ptr() + 4), dict(D=0), dict(Q=0)):
        refused(BAD, L.sp_match_segmented, *seg_args(**kw), idx.ptr, 0, dist.ptr, 0)
    refused(INV, L.sp_match_segmented, *seg_args(D=1280), idx.ptr, 0, dist.ptr, 0)
    refused(INV, L.sp_match_segmented, *seg_args(Q=4097), idx.ptr, 0, dist.ptr, 0)
    kw_ = L.sp_seg_keys_words(big)
    skeys = zeros64(kw_ + 64)

    def soft_args(**kw):
        a = dict(dict(b=sb.data_ptr(), rows=sk.N, q=sq.data_ptr(), start=sstart.data_ptr(), S=sk.S, mr=big, D=sk.D, kw=kw_, pi=pi, enc=senc.data_ptr(), k=2, t=1.0,
                      out=0), **kw)
        return (a["b"], 1, a["rows"], a["q"], sseg.data_ptr(), sk.Q, a["start"], a["S"], a["mr"], a["D"], skeys.data_ptr(), a["kw"], plan.ptr, a["pi"],
                a["enc"], a["k"], a["t"], 0, idx.ptr, dist.ptr, 0, a["out"], 0)

    for kw in bad_tables + (dict(kw=kw_ - 1), dict(pi=L.sp_seg_plan_ints(16, sk.S) - 1), dict(enc=senc.data_ptr() + 4), dict(D=0)):
        refused(BAD, L.sp_match_seg_topk, *soft_args(**kw))
    big_out = Out((sk.Q, sk.D))
    for kw in (dict(k=0), dict(k=9), dict(t=0.0), dict(t=-1.0), dict(t=float("nan")), dict(D=1280), dict(enc=0, out=big_out.ptr)):
        refused(INV, L.sp_match_seg_topk, *soft_args(**kw))
    assert big_out.intact() and plan.intact()


# =================================================================================================== last: the figures of the docstring
@gpu
def test_zz_worst_ratios_of_the_scans():
    """Last in the file: the worst ratio per instance over the cases that ran in this process, and every instance's pooled rms."""
    for inst, (a, b) in sorted(RATIOS.items()):
        if inst.startswith("scan:"):
            print(f"[scan] worst {inst:52s} max {a:.3f}  rms {b:.3f}")
    for inst in [i for i in POOL if i.startswith("scan:")]:
        hold_pool(inst)
