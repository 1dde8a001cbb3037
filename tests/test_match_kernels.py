"""The context matcher's kernels against float64, stage by stage (GPU cases: -m gpu; the CPU pins and the case-validity checks run everywhere).

The matcher is about 2 300 lines of HIP (csrc/match_mfma.hip, match_pass.hip, match_select2.hip, match_stream.hip, match_scan8.hip) and
every path through it is a cheap coarse stage, a pruning rule and an exact re-rank: the final index - all that tests/test_edge_cases.py,
test_scan8.py, test_hip_parity.py and test_bank.py see, always at D = 23040 - is right as long as the coarse stage's error stays inside the
bound the rule assumes, and cannot show a violation short of two rows sitting in exactly the wrong relation.  Here every launcher is called
directly through tests/gemm_probe/match_probe.cpp with intermediate products the test AUTHORS (query planes, score slabs, bnorm, qstat)
and each stage is held to its float64 restatement (tests/match_ref.py) and to the bound the next stage assumes of it.

Family 1 - bank-build and query-prep products (test_bank_products: rows {1, 3, 4, 257} x cols {256, 7680, 23040} x seven contents = 84 cases,
5 kernels each; guard words around every output).  to_bf16 / center_bf16: the bits of bf16_rne(x (-) c).  rownorm2_bf16: float64 sum of
squares of the same bf16 values, relative errors pooled over the 5 565 rows.  rowresid: rho >= ||(x - c) - b16|| in float64 with no
tolerance, rho <= (1 + 2e-5)(1.000001 r64 + 1e-6 n64).  to_i8: scale bits = fp32(max|x (-) c|) / 127 (1 for the zero row), bytes in [1, 255],
within 1 of the float64 value and equal to it more than 1e-4 from a tie, rho8 sound against the bytes and scale the kernel wrote, and
tight as above.
Family 2 - the coarse passes.  Instances: mocha_match_gemm_bf16_dma<4,1,nt> / <3,2,nt>, row-major and through the launch_tile_bf16 image,
with and without tickets (16); mocha_match_pass256<PFS,NT,.,NPL,TILED>, PFS 3 .. 6 (one plane) / 2 .. 4 (two), NT on / off, row-major and
through the launch_tile32_bf16 image (28).  test_coarse_pass_sweep: 184 cases (36 + 50 + 48 + 50 for the four (kernel, planes) groups),
D = 64 steps with steps walking 1 .. 3 R + 1 at ksplit 1 (R = the deepest ring / prefetch of the group: every branch of prologue, steady
state and tail of every instance), Q in {1, 9, 127, 128, 129, 257}, N in {1, 3, 127, 128, 129, 255, 256, 257, 260, 1027}, the regimes
normal / plane 0 zero / plane 1 = -plane 0 / index-revealing integers; EVERY variant of a group runs on every case of the group (1 712
launches), so every (instance, shape class), (instance, regime) and (shape class, regime) pair meets (test_pass_cases_are_a_pairwise_cover).
Two fixed cases close every group: index-revealing integers at D = 256 with Q = 257 (N = 260 and 3), where the positions k(q) cover every k.
test_coarse_pass_ragged_splits: steps 9 / ksplit 8 and (pass256) steps 17 / ksplit 16, empty slices' slabs zero in every element.
test_gemm_tickets_fold: K split 2 with slices of 1 .. 3 R + 1 steps, 9 / 8 and 12 / 4.  test_coarse_pass_full_depth: D = 23040, Q = 129,
N = 513, every K split the launcher accepts.  Asserted:
  (a) every slab against the float64 partial sum over its own K range (ceil split), bound = the error of the fp32 CPU evaluation of the
      same bf16 operands times MARGINS.  That evaluation is match_ref.coarse_ref: one running fp32 sum over the slab's K range that takes
      16 k at a time, the low plane's products before the high plane's (a stated order; a BLAS's own differs from one CPU to the next).
      A case of fewer than 4 096 outputs has its rms held in the group's pool only, and one of fewer than 1 024 takes the fp32
      evaluation's error from a 32 x 32 problem of the same depth and regime as well (q1-n3 has three samples of it).  plane 1 = -plane 0:
      float64 and the fp32 evaluation a1 b + a0 b are exactly 0 and leave nothing to scale; the bound is the fp32 evaluation's error on
      the one-plane product a0 b that passes through the accumulators;
  (b) soundness with the project's own numbers: bnorm from launch_rownorm2_bf16, |(bnorm - 2 sum_z S_z) - v64| <= 5e-5 (||a||^2 + ||b||^2)
      for every (q, n) of every case, whatever the regime; the fp32-bank route (exact-f32 GEMM with wsub = centre and a K split on the GEMM probe,
      launch_rownorm2) the same with 4e-6 (test_fp32_bank_route_is_inside_its_margin);
  (c) to the bit: image against row-major, NT against not, PFS against PFS (they move operands or change when a load is issued; every
      accumulator takes the same products in the same k order), run to run; with tickets slab 0 = the ticket-less run's slabs added in
      slab order from zero in fp32, the other slabs untouched, tickets zero afterwards, a second launch the same.  Between the two
      kernel families and between one and two planes only (a);
  (d) bank and queries sit in front of rows of NaN, the images in front of NaN: no NaN in S; guard words around S; every element of
      every slab written; index-revealing integers: S = bank[n][k(q)] to the bit in the slab that owns k(q), 0 in the others.
Family 3 - mocha_match_select and mocha_match_select2 on authored scores (32 cases, 216 queries; EVERY case on both kernels, three score
layouts - lds = N, lds = N + 3, slab_stride % 4 = 1 - and dist null / non-null).  match_ref.build_select places per query a winner at
NEAR ||q - c||^2, decoys a little behind it and far rows, and writes the slabs from the float64 score plus 0.9 of the bound stated in
match_select2.hip, + for the winner, - for everything else, so that EVERY decoy's coarse score is better than the winner's; rows inside
the bound 0, 1, 15 .. 17, 63 .. 65, 127 .. 129 and every row (copies), winner and candidates at rows 0, N - 1, both sides of 4 096, 16 384
and of the window bounds 64 / 128, the winner the lowest of a run of copies.  The validity of every case (the answer, the gap of exactly 0
or >= 1e-4, the realised error between 0.8 and 1.0 of the bound, the candidate count) is checked on the CPU
(test_select_cases_are_valid_and_cover).  Asserted: the index is the float64 argmin, ties to the lowest row; dist against the float64
direct form, pooled per kernel and bank type; NaN rows never win; a query without a finite score gets row 0 (select2: dist NaN; select
evaluates row 0 and reports its distance); NaN in other queries' scores leaves a query's bits alone.
Family 4 (launch_match_stream / _topk / _scan16 / _scan8, mocha_match_refine on authored keys and rho) and family 5 (the segmented and soft
matchers, the plan, the gathers) are held in tests/test_scan_kernels.py through tests/gemm_probe/scan_probe.cpp.

Kernel fixes (family 1 found both; rowresid and to_i8 are bank-set kernels, not on the step's path):
  1. rho underestimated on tiny rows.  Rows of size 1e-30: d^2 and t^2 leave the fp32 range, both sums came out 0 and rho = 0 against a
     float64 residual of 3e-32 .. 3e-31 (all 12 shapes, both kernels).  mocha_rowresid and mocha_to_i8 now also sum 2^64-scaled terms in
     the same pass and use those when ||x - c||^2 < 2^-40; larger rows take the old sums (to_i8: same bits as before).  The switch sits where
     nothing rests on denormals: above it every d^2 below the normal range together is worth 1e-19 sqrt(cols) against a slack of 1e-12;
     the "small" contents (1e-17, d^2 of 1e-39) pin the band below it.
  2. rowresid loose on rows with one large entry.  t = fl(x - c) carries 2^-24 |t| of rounding; with a 1e4 entry among unit ones that is
     5e-4 on a residual norm of 16, and rho exceeded the stated ceiling by up to 1.1e-5 relative (7 of 12 shapes; the CPU emulation of the
     kernel's formula gives the GPU's 16.030542 to the last digit).  The rounding can go either way, so it was no underestimate only
     because of the 1e-6 ||x - c|| term.  mocha_rowresid now recovers (x - c) - t with the two-sum and adds it to t - b16 (exact).
  tests/test_edge_cases.py, test_scan8.py, test_hip_parity.py and test_bank.py pass unchanged; the demo benchmark is unchanged (113.3 and 113.6
  against the parent's 113.4 and 113.4 thousand frames/s, alternating runs of 30 steps).

Margins.  (4, 2) on the largest / rms error of the fp32 CPU evaluation are the starting values and stay for every instance: nothing
measured comes near them, and nothing was tightened on one run.  Measured on an MI355X (67 GPU tests, every one passed; ratio = kernel
error / fp32 CPU error, every case prints its own with -s), worst case largest / rms (cases of >= 4 096 outputs), then the rms ratio pooled
over every output of the group:
  gemm<4,1> 2.17 / 1.42, pooled 1.40 (2.5 M outputs)      gemm<3,2> 1.69 / 1.44, pooled 1.42 (4.0 M)
  pass<1pl> 2.15 / 1.42, pooled 1.40 (5.9 M)              pass<2pl> 1.82 / 1.43, pooled 1.41 (6.6 M)
  D = 23040 alone: 1.12 - 2.15 / 1.28 - 1.43 over K splits 1 .. 16.  Every variant of a group has the group's figures: (c) holds to the bit.
  rownorm2_bf16 1.00 / 1.00 (5 565 rows, relative)        dist: select f32 1.00 / 1.00, select b16 1.00 / 1.00, select2 f32 0.87 / 1.01,
  select2 b16 1.00 / 1.03 (312 - 336 distances each, relative; all within one ulp)
  (b): |v - v64| at most 0.004 of the 5e-5 slack on the bf16 operands (the slack is there for the query's rounding, which (b) leaves out by
  taking v64 on the same operands), 0.027 of the 4e-6 slack on the fp32 route.
  rowresid: rho / r64 >= 1.00033 in every row with a residual, rho / ceiling <= 0.99998; to_i8 the same (1.00007, 0.99998).
Mutations, each built on a scratch copy (never committed; wrong numbers only, no access moves), failing tests of this file / of the 98 tests
of tests/test_edge_cases.py, test_scan8.py, test_hip_parity.py and test_bank.py:
  1. mocha_match_select2's candidate rule without the margin_rel term: 22 (21 of the 32 authored cases - every fp32-bank one, where the
     term is the whole bound, and the bf16 ones whose decoys sit beyond 2 ||dq|| ||b|| - and the fp32 NaN test) / 2.
  2. mocha_match_pass256 with two planes without its low-plane products: 4 (sweep, ragged and full depth of pass<2pl>, and the pool) / 0.
  3. mocha_rowresid without its 1e-6 ||b - c|| term: 0 / 0.  With kernel fix 2 the residual comes from the exact x - c and what is left for
     the term to cover is the fp32 sums' own error, which the factor 1.000001 covers in all 5 565 rows here.  On the PARENT's formula the
     same mutation underestimates 258 of the 518 rows of the three largest "outlier" cases (CPU emulation of that formula): there the term
     is what paid for the rounding of x - c.
  4. the slice length floored instead of ceiled (both coarse kernels): 7 (the ragged splits of all four groups - steps 9 / ksplit 8 drops
     a step, steps < ksplit computes nothing - pass256's full depth at K split 16, 360 = 16 x 22 + 8, and the pool) / 3.
Run time on the GPU box: 21 s for the file (attention file: 16 s), CPU references and case building included; the slowest tests are the
257 x 23040 bank products (2.6 s for seven contents) and the D = 23040 coarse cases (1.0 - 2.0 s for all K splits); a sweep of 36 - 50 cases
takes 0.6 - 1.4 s.  Every case ran and was measured.
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
import pointwise_ref as pr  # noqa: E402
from test_pointwise_kernels import D as todev, Out, T, dev, same_bits  # noqa: E402  (the guard pattern)

gpu = pytest.mark.gpu
DEFAULT_MARGIN = (4.0, 2.0)              # on the largest / on the rms error of the fp32 CPU evaluation (docstring, "Margins")
MARGINS = {}
RATIOS = {}
NAN16 = 0x7FC0


POOL = {}
MIN_RMS = 4096             # outputs below which a case's own rms is a handful of samples: it is held in the instance's pool only


def hold(inst, case, y, ref64, ref32, ulp=None, extra=None):
    """(a): y (numpy) against the float64 restatement, bounded by the fp32 CPU evaluation's own error times MARGINS[inst], plus one fp32 ulp
    of the largest reference value on the largest error.  extra = (ref64, ref32) of a larger problem of the same kind: a case of a few
    outputs (Q = 1, N = 3) has too few samples of the fp32 evaluation's error to size a bound with.  The rms error of a case of at least MIN_RMS outputs is held on its own; every
    case's squared errors also go to the instance's pool (hold_pool)."""
    y, ref64, ref32 = (T(np.asarray(a)) if not isinstance(a, torch.Tensor) else a for a in (y, ref64, ref32))
    emax, erms = pr.errors(y, ref64.double())
    bmax, brms = pr.errors(ref32, ref64.double())
    if extra is not None:                                                      # a handful of outputs: the fp32 evaluation's error is sampled on more of the same
        xmax, xrms = pr.errors(extra[1], extra[0].double())
        n, m = y.numel(), extra[0].numel()
        bmax, brms = max(bmax, xmax), ((brms * brms * n + xrms * xrms * m) / (n + m)) ** 0.5
    ulp = pr.ulp_of_largest(ref64.double()) if ulp is None else ulp
    mmax, mrms = MARGINS.get(inst, DEFAULT_MARGIN)
    rmax, rrms = emax / max(bmax, 1e-300), erms / max(brms, 1e-300)
    own = y.numel() >= MIN_RMS
    w = RATIOS.setdefault(inst, [0.0, 0.0])
    w[0], w[1] = max(w[0], rmax if emax > ulp else 0.0), max(w[1], rrms if own and erms > 0 else 0.0)
    pool = POOL.setdefault(inst, [0.0, 0.0, 0])
    pool[0] += erms * erms * y.numel(); pool[1] += brms * brms * y.numel(); pool[2] += y.numel()
    print(f"[match] {inst:22s} {case:40s} max {emax:.3e} ({rmax:6.2f} x fp32 cpu) rms {erms:.3e} ({rrms:5.2f} x) ulp {ulp:.2e}   worst so far {w[0]:.2f} / {w[1]:.2f}")
    assert emax <= mmax * bmax + ulp, (inst, case, (emax, erms), (bmax, brms), ulp)
    assert not own or erms <= mrms * brms + (ulp if bmax == 0 else 0), (inst, case, (emax, erms), (bmax, brms), ulp)


def hold_pool(inst):
    """The rms error over every output of every case of `inst` so far against the fp32 CPU evaluation's over the same outputs."""
    e2, b2, n = POOL[inst]
    ratio = (e2 / max(b2, 1e-300)) ** 0.5
    RATIOS.setdefault(inst + " pooled", [0.0, 0.0])[1] = ratio
    print(f"[match] {inst:22s} pooled over {n} outputs: rms {np.sqrt(e2 / n):.3e} ({ratio:5.2f} x fp32 cpu)")
    assert ratio <= MARGINS.get(inst, DEFAULT_MARGIN)[1], (inst, ratio)


def call(fn, *args):
    torch.cuda.synchronize()
    rc = fn(*args)
    torch.cuda.synchronize()
    return rc


def u16dev(a, tail_rows=0, cols=None):
    """uint16 host array on the device as int16, followed by `tail_rows` rows of bf16 NaN."""
    flat = np.ascontiguousarray(a).reshape(-1)
    if tail_rows:
        flat = np.concatenate([flat, np.full(tail_rows * cols, NAN16, np.uint16)])
    return torch.from_numpy(flat.view(np.int16).copy()).to(dev())


# =================================================================================================== no GPU: the restatements are what they claim
def test_bf16_rne_is_torch_bfloat16_and_rounds_ties_to_even():
    r = mr.rng("bf16")
    x = np.concatenate([r.standard_normal(4096, dtype=np.float32), np.float32([0, -0.0, 1e-40, 3e38, 1.0, -1.5]),
                        mr.contents("ties", 4, 256, r)[0].reshape(-1), mr.contents("tiny", 2, 256, r)[0].reshape(-1)])
    want = T(x).bfloat16().view(torch.int16).numpy().view(np.uint16)
    assert np.array_equal(mr.bf16_rne(x), want)
    # 1 + 2^-8 is half-way between 1 and 1 + 2^-7: the even neighbour is 1; 1 + 3 * 2^-8 goes up to 1 + 2^-6
    assert list(mr.bf16_rne(np.float32([1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, -(1 + 2.0 ** -8)]))) == [0x3F80, 0x3F82, 0xBF80]
    assert np.array_equal(mr.bf16_value(mr.bf16_rne(np.float32([1.0, -2.5]))), np.float32([1.0, -2.5]))


def test_contents_are_what_they_claim():
    r = mr.rng("contents")
    x, c = mr.contents("ties", 3, 256, r)
    assert (c == 0).all() and ((x.view(np.uint32) & 0xFFFF) == 0x8000).all()
    kept = (x.view(np.uint32) >> 16) & 1
    assert kept.min() == 0 and kept.max() == 1 and (x < 0).any() and (x > 0).any()
    trunc = (x.view(np.uint32) >> 16).astype(np.uint16)
    assert (mr.bf16_rne(x) != trunc).any() and (mr.bf16_rne(x) == trunc).any()          # truncation differs on the odd ones
    x, c = mr.contents("far", 3, 256, r)
    assert np.abs(c).min() >= 1e3 and np.abs(x.astype(np.float64) - c).max() < 10
    x, c = mr.contents("centre-row", 3, 256, r)
    assert np.array_equal(x[0], c)
    x, c = mr.contents("outlier", 3, 256, r)
    assert ((x == 1e4).sum(1) == 1).all()
    x, c = mr.contents("tiny", 3, 256, r)
    assert 0 < np.abs(x).max() < 1e-29 and float(np.float32(np.abs(x).max()) ** 2) == 0.0
    x, c = mr.contents("small", 3, 256, r)
    d = (x - c) - mr.bf16_value(mr.centred_bf16(x, c))
    assert float(np.float32(np.abs(x).max()) ** 2) > 1e-36 and 0 < float(np.abs(d).max()) ** 2 < 1.2e-38


def test_slices_are_the_ceil_split():
    """csrc/kernels.h and the coarse kernels: per = ceil(steps / ksplit) steps a slice; D = 23040 gives 360, 180, 90, 45 and 23 with a last
    slice of 15; a ragged split leaves empty slices."""
    assert [mr.slices(360, k)[0][1] for k in (1, 2, 4, 8, 16)] == [360, 180, 90, 45, 23]
    assert mr.slices(360, 16)[-1] == (345, 360)
    assert mr.slices(9, 8) == [(0, 2), (2, 4), (4, 6), (6, 8), (8, 9), (9, 9), (9, 9), (9, 9)]
    s = mr.slices(17, 16)
    assert s[8] == (16, 17) and all(a == b for a, b in s[9:]) and sum(b - a for a, b in s) == 17
    for steps, k in itertools.product(range(1, 40), (1, 2, 4, 8, 16)):
        sl = mr.slices(steps, k)
        assert sl[0][0] == 0 and all(sl[i][1] == sl[i + 1][0] for i in range(k - 1)) and sl[-1][1] == steps


def test_coarse_reference_slabs_add_up():
    r = mr.rng("coarse-ref")
    P, bank, _ = mr.pass_operands("normal", 5, 7, 64 * 9, 2, r)
    S64, S32 = mr.coarse_ref(P, bank, 9, 8)
    full64, _ = mr.coarse_ref(P, bank, 9, 1)
    assert torch.allclose(S64.sum(0), full64[0], rtol=0, atol=1e-9) and float(S64[5:].abs().max()) == 0.0
    a = mr.bf16_value(P[0]).astype(np.float64) + mr.bf16_value(P[1]).astype(np.float64)
    assert np.allclose(full64[0].numpy(), a @ mr.bf16_value(bank).astype(np.float64).T, rtol=0, atol=1e-9)
    assert float((S32.double() - S64).abs().max()) < 1e-4
    P, bank, kq = mr.pass_operands("index", 257, 3, 256, 2, r)
    assert sorted(set(kq.tolist())) == list(range(256))                          # Q = 257 at D = 256: the positions cover every k
    S64, _ = mr.coarse_ref(P, bank, 4, 1)
    assert np.array_equal(S64[0].numpy(), mr.bf16_value(bank).astype(np.float64)[:, kq].T)
    P, bank, _ = mr.pass_operands("p1-neg", 3, 4, 128, 2, r)
    assert float(mr.coarse_ref(P, bank, 2, 1)[0].abs().max()) == 0.0


# =================================================================================================== family 1: bank-build and query-prep products
F1_ROWS, F1_COLS = (1, 3, 4, 257), (256, 7680, 23040)
_f1_pool = {}


def _f1_launch(name, shape, kind, fn):
    o = Out(shape, kind)
    rc = call(fn, o)
    assert rc == 0, (name, rc)
    return o.check(name)


@gpu
@pytest.mark.parametrize("cols", F1_COLS)
@pytest.mark.parametrize("rows", F1_ROWS)
def test_bank_products(rows, cols):
    """to_bf16 / center_bf16: bits; rownorm2_bf16: pooled in test_rownorm2_bf16_pool; rowresid and to_i8: sound with no tolerance, tight to
    rho_ceiling; scale bits; bytes in [1, 255], within 1 of the float64 value and equal away from ties."""
    L = mr.load()
    for kind in mr.CONTENTS:
        case = f"r{rows}-c{cols}-{kind}"
        x, c = mr.contents(kind, rows, cols, mr.rng("f1-" + case))
        dx, dc = todev(x), todev(c)
        want = mr.centred_bf16(x, c)
        b_to = _f1_launch("to_bf16", (rows, cols), "u16", lambda o: L.mp_to_bf16(mr.ptr(dx), mr.ptr(dc), cols, o.ptr, rows * cols, 0))
        b_ce = _f1_launch("center_bf16", (rows, cols), "u16", lambda o: L.mp_center_bf16(mr.ptr(dx), mr.ptr(dc), o.ptr, rows, cols, 0))
        assert same_bits(b_to, want), (case, "to_bf16", int((b_to != want).sum()))
        assert same_bits(b_ce, want), (case, "center_bf16", int((b_ce != want).sum()))
        plain = _f1_launch("to_bf16", (rows, cols), "u16", lambda o: L.mp_to_bf16(mr.ptr(dx), 0, cols, o.ptr, rows * cols, 0))
        assert same_bits(plain, mr.bf16_rne(x)), (case, "to_bf16 without a centre")

        d16 = todev(want.view(np.int16))
        bn = _f1_launch("rownorm2_bf16", (rows,), "f32", lambda o: L.mp_rownorm2_bf16(mr.ptr(d16), o.ptr, rows, cols, 0))
        v = T(mr.bf16_value(want))
        _f1_pool[case] = (bn.astype(np.float64), (v.double() ** 2).sum(1).numpy(), (v * v).sum(1).double().numpy())

        rho = _f1_launch("rowresid", (rows,), "f32", lambda o: L.mp_rowresid(mr.ptr(dx), mr.ptr(dc), mr.ptr(d16), o.ptr, rows, cols, 0))
        r64, n64 = mr.resid_norms(x, c, mr.bf16_value(want).astype(np.float64))
        ceil = mr.rho_ceiling(r64, n64)
        print(f"[match] rowresid {case:28s} rho / r64 min {np.min(rho / np.maximum(r64, 1e-300)):.6f}   rho / ceiling max {np.max(rho / np.maximum(ceil, 1e-300)):.6f}")
        assert (rho.astype(np.float64) >= r64).all(), (case, "rowresid underestimates", rho[:4], r64[:4])
        assert (rho.astype(np.float64) <= ceil).all(), (case, "rowresid is loose", rho[:4], ceil[:4])

        o8, osc, orh = _Bytes(rows, cols), Out((rows,)), Out((rows,))
        rc = call(L.mp_to_i8, mr.ptr(dx), mr.ptr(dc), o8.ptr, osc.ptr, orh.ptr, rows, cols, 0)
        assert rc == 0
        u8, sc, rho8 = o8.check(), osc.check("to_i8 scale"), orh.check("to_i8 rho")
        assert same_bits(sc, mr.i8_scale(x, c)), (case, "scale", sc[:4], mr.i8_scale(x, c)[:4])
        if kind == "centre-row":
            assert sc[0] == 1.0
        assert u8.min() >= 1, (case, "byte 0")
        ideal = mr.i8_ideal(x, c, sc)
        near = np.rint(ideal)
        assert (np.abs(u8.astype(np.float64) - near) <= 1).all(), (case, "bytes")
        off_tie = np.abs(np.abs(ideal - np.floor(ideal)) - 0.5) > 1e-4
        assert (u8.astype(np.float64)[off_tie] == near[off_tie]).all(), (case, "bytes away from ties", int((u8.astype(np.float64)[off_tie] != near[off_tie]).sum()))
        r64, n64 = mr.resid_norms(x, c, sc.astype(np.float64)[:, None] * (u8.astype(np.float64) - 128))
        ceil = mr.rho_ceiling(r64, n64)
        print(f"[match] to_i8    {case:28s} rho / r64 min {np.min(rho8 / np.maximum(r64, 1e-300)):.6f}   rho / ceiling max {np.max(rho8 / np.maximum(ceil, 1e-300)):.6f}")
        assert (rho8.astype(np.float64) >= r64).all(), (case, "to_i8 rho underestimates", rho8[:4], r64[:4])
        assert (rho8.astype(np.float64) <= ceil).all(), (case, "to_i8 rho is loose", rho8[:4], ceil[:4])


class _Bytes:
    """A byte output between sentinel guards (0xAD bytes; 0 is never a legal byte of the image, 0xAD is, so `written` is not checked per element)."""

    def __init__(self, rows, cols):
        self.n = rows * cols
        self.shape = (rows, cols)
        self.buf = torch.full((self.n + 512,), 0, dtype=torch.uint8, device=dev())
        self.ptr = self.buf.data_ptr() + 256

    def check(self):
        h = self.buf.cpu().numpy()
        assert not h[:256].any() and not h[256 + self.n:].any(), "to_i8: a guard byte was overwritten"
        return h[256:256 + self.n].reshape(self.shape)                         # every legal byte is >= 1: an unwritten one shows as 0


@gpu
def test_rownorm2_bf16_pool():
    """One squared norm per row: a case has 1 to 257 outputs of very different sizes (1e-60 to 1e8), so every case's errors are taken
    relative to its own float64 value and pooled (as test_pointwise_kernels.test_rownorm2 pools per column)."""
    for rows, cols in itertools.product(F1_ROWS, F1_COLS):                      # (selected on its own: the cases this test pools are run here)
        if f"r{rows}-c{cols}-normal" not in _f1_pool:
            test_bank_products(rows, cols)
    assert len(_f1_pool) == len(F1_ROWS) * len(F1_COLS) * len(mr.CONTENTS)
    got, r64, r32 = [], [], []
    for case, (y, a, b) in sorted(_f1_pool.items()):
        s = np.where(a > 0, a, 1.0)
        assert (y[a == 0] == 0).all(), case
        got.append(y / s), r64.append(a / s), r32.append(b / s)
    hold("rownorm2_bf16", "all cases, relative", np.concatenate(got), np.concatenate(r64), np.concatenate(r32))


@gpu
def test_bank_product_refusals():
    L = mr.load()
    x, c = mr.contents("normal", 4, 256, mr.rng("f1-refuse"))
    dx, dc = todev(x), todev(c)
    o = Out((4, 256), "u16")
    for rc in (call(L.mp_to_bf16, mr.ptr(dx) + 4, mr.ptr(dc), 256, o.ptr, 1024, 0), call(L.mp_to_bf16, mr.ptr(dx), mr.ptr(dc), 256, o.ptr + 2, 1024, 0),
               call(L.mp_center_bf16, mr.ptr(dx), mr.ptr(dc) + 4, o.ptr, 4, 256, 0), call(L.mp_center_bf16, mr.ptr(dx), 0, o.ptr, 4, 256, 0),
               call(L.mp_center_bf16, mr.ptr(dx), mr.ptr(dc), o.ptr + 8, 4, 256, 0), call(L.mp_rowresid, mr.ptr(dx), mr.ptr(dc), 0, o.ptr, 4, 256, 0),
               call(L.mp_to_i8, mr.ptr(dx), mr.ptr(dc), o.ptr, 0, o.ptr, 4, 256, 0), call(L.mp_rownorm2_bf16, mr.ptr(dx), o.ptr, 0, 256, 0)):
        assert rc == mr.BAD_ARGUMENT and o.intact()
    assert call(L.mp_to_bf16, mr.ptr(dx), mr.ptr(dc), 254, o.ptr, 1016, 0) == mr.INVALID_VALUE and o.intact()      # the launchers' own
    assert call(L.mp_center_bf16, mr.ptr(dx), mr.ptr(dc), o.ptr, 4, 252, 0) == mr.INVALID_VALUE and o.intact()


# =================================================================================================== family 2: the coarse passes
QS = (1, 9, 127, 128, 129, 257)
NS = (1, 3, 127, 128, 129, 255, 256, 257, 260, 1027)
GROUPS = {                     # kernel family and planes -> (largest ring depth R, the variants run on every case, the operand regimes)
    "gemm<4,1>": dict(kind="gemm", planes=1, R=4, regimes=mr.REGIMES1,
                      variants=[dict(nt=nt, tiled=tl) for nt in (0, 1) for tl in (0, 1)]),
    "gemm<3,2>": dict(kind="gemm", planes=2, R=3, regimes=mr.REGIMES2,
                      variants=[dict(nt=nt, tiled=tl) for nt in (0, 1) for tl in (0, 1)]),
    "pass<1pl>": dict(kind="pass", planes=1, R=6, regimes=mr.REGIMES1,
                      variants=[dict(pfs=p, nt=nt, tiled=tl) for p in (3, 4, 5, 6) for nt in (0, 1) for tl in (0, 1)]),
    "pass<2pl>": dict(kind="pass", planes=2, R=4, regimes=mr.REGIMES2,
                      variants=[dict(pfs=p, nt=nt, tiled=tl) for p in (2, 3, 4) for nt in (0, 1) for tl in (0, 1)]),
}


def inst_name(group, v, tickets=0):
    g = GROUPS[group]
    if g["kind"] == "gemm":
        return f"gemm<{g['R']},{g['planes']},{'nt' if v['nt'] else 'ld'}>-{'img' if v['tiled'] else 'row'}" + ("-tk" if tickets else "")
    return f"pass<{v['pfs']},{'nt' if v['nt'] else 'ld'},{g['planes']},{'img' if v['tiled'] else 'row'}>"


# index-revealing integers at D = 256 with Q = 257: the positions k(q) cover EVERY k of the four 64-k stages, so a swizzle, stage-offset or
# piece error at any k position is off by whole integers; N = 260 (vector stores at a ragged tile) and 3.  In every group, on every variant.
EVERY_K = (dict(Q=257, N=260, steps=4, ksplit=1, regime="index"), dict(Q=257, N=3, steps=4, ksplit=1, regime="index"))


def _deal(group, salt):
    """Cases of a group: steps cycles 1 .. 3 R + 1 (ksplit 1: every branch of prologue, steady state and tail), Q, N and the regime are
    dealt by a seeded shuffle; the first salt whose deal is a pairwise cover of (Q, N, steps, regime) x regime / Q x N-class is taken."""
    g = GROUPS[group]
    r = mr.rng(f"deal-{group}-{salt}")
    nsteps = 3 * g["R"] + 1
    n = max(10 * len(g["regimes"]), 2 * nsteps) + 8
    ns, rg = r.permutation(len(NS)), r.permutation(len(g["regimes"]))
    out = []
    for i in range(n):
        out.append(dict(group=group, Q=QS[int(r.integers(len(QS)))], N=NS[ns[i % 10]], steps=i % nsteps + 1, ksplit=1,
                        regime=g["regimes"][rg[(i // 10 + i % 10) % len(g["regimes"])]]))
    return out


def _uncovered(cases, regimes):
    miss = []
    for key, vals in (("Q", QS), ("N", NS)):
        seen = {(c[key], c["regime"]) for c in cases}
        miss += [(key, v, rg) for v in vals for rg in regimes if (v, rg) not in seen]
    seen = {c["steps"] for c in cases}
    miss += [("steps", s) for s in range(1, max(seen) + 1) if s not in seen]
    return miss


@functools.lru_cache(None)
def pass_cases(group):
    for salt in range(256):
        cs = _deal(group, salt)
        if not _uncovered(cs, GROUPS[group]["regimes"]):
            return tuple(tuple(sorted(c.items())) for c in cs + [dict(c, group=group) for c in EVERY_K])
    raise AssertionError(group)


RAGGED = {"gemm": ((9, 8),), "pass": ((9, 8), (17, 16))}                   # (steps, ksplit): slices of two steps, one of one, the rest empty


def test_pass_cases_are_a_pairwise_cover():
    """Every (Q, regime), (N, regime) and every steps value 1 .. 3 R + 1 occurs in every group; every variant (instance) of a group runs on
    every case of the group, so every (instance, shape class) and (instance, regime) pair meets as well; all 60 (Q, N) pairs occur."""
    qn = set()
    for group, g in GROUPS.items():
        cs = [dict(c) for c in pass_cases(group)]
        assert not _uncovered(cs, g["regimes"])
        assert {c["steps"] for c in cs} == set(range(1, 3 * g["R"] + 2))
        for e in EVERY_K:
            assert dict(e, group=group) in cs, (group, e)
        qn |= {(c["Q"], c["N"]) for c in cs}
    print(f"[match] coarse-pass cases: {sum(len(pass_cases(g)) for g in GROUPS)}, launches {sum(len(pass_cases(g)) * len(GROUPS[g]['variants']) for g in GROUPS)}, (Q, N) pairs {len(qn)} of 60")
    assert len(qn) >= 45, len(qn)


class PassData:
    """Device operands of one coarse-pass problem: the query planes (plane 1 Q D elements after plane 0) and the bank, each followed by
    rows of NaN, and the two bank images made from that buffer by the image kernels (NaN behind them too)."""

    def __init__(self, P, bank, Q, N, Dk):
        L = mr.load()
        self.P, self.bank, self.Q, self.N, self.Dk, self.planes = P, bank, Q, N, Dk, P.shape[0]
        self.dq = u16dev(P, 8, Dk)
        self.db = u16dev(bank, 8, Dk)
        self.img = {}
        for which, elems, fn in (("gemm", L.mp_tiled_elems(N, Dk), L.mp_tile_bf16), ("pass", L.mp_tile32_elems(N, Dk), L.mp_tile32_bf16)):
            buf = torch.full((elems + 64,), NAN16, dtype=torch.int16, device=dev())
            assert call(fn, mr.ptr(self.db), mr.ptr(buf), elems, N, Dk, 0) == 0
            assert bool((buf[elems:] == NAN16).all()), "the image kernel wrote past its image"
            self.img[which] = (buf, elems)

    def run(self, kind, v, ksplit, tickets=None, expect=0):
        L = mr.load()
        out = Out((ksplit, self.Q, self.N))
        img, elems = self.img[kind] if v["tiled"] else (None, 0)
        qe = self.planes * self.Q * self.Dk
        if kind == "gemm":
            rc = call(L.mp_match_gemm_bf16, mr.ptr(self.dq), qe, self.Q * self.Dk, mr.ptr(self.db), out.ptr, self.Q, self.N, self.Dk, ksplit, self.planes,
                      mr.ptr(img), elems, v["nt"], mr.ptr(tickets), 0)
        else:
            rc = call(L.mp_match_pass256, mr.ptr(self.dq), qe, self.Q * self.Dk, mr.ptr(self.db), out.ptr, self.Q, self.N, self.Dk, ksplit,
                      v["pfs"] | (16 if v["nt"] else 0), self.planes, mr.ptr(img), elems, 0)
        assert rc == expect, (kind, v, rc)
        if expect:
            assert out.intact()
            return None
        S = out.check(f"S of {kind} {v}")                                       # guards intact, every element of every slab written
        assert not np.isnan(S).any(), "NaN from behind the operands reached S"
        return S


def _bnorm(data):
    o = Out((data.N,))
    assert call(mr.load().mp_rownorm2_bf16, mr.ptr(data.db), o.ptr, data.N, data.Dk, 0) == 0
    return o.check("bnorm")


def _check_pass(group, c, data, S_by_variant, kq):
    """(a) per slab and (b) soundness for the first variant; (c) every other variant of the group has the first one's bits: the image
    kernels only move the operands, the non-temporal hint and the prefetch depth only change WHEN a load is issued - every accumulator
    takes the same products in the same k order in all of them."""
    g = GROUPS[group]
    steps, ksplit, regime = c["steps"], c["ksplit"], c["regime"]
    names = [inst_name(group, v) for v in g["variants"]]
    first = S_by_variant[0]
    for nm, S in zip(names[1:], S_by_variant[1:]):
        assert same_bits(S, first), (nm, "differs from", names[0], c, float(np.abs(S - first).max()))
    S64, S32 = mr.coarse_ref(data.P, data.bank, steps, ksplit)
    for z, (s0, s1) in enumerate(mr.slices(steps, ksplit)):
        if s1 == s0:
            assert not (first[z] != 0).any(), (group, c, z, "the slab of an empty slice is not zero in every element")
    case = f"q{c['Q']}-n{c['N']}-s{steps}-k{ksplit}-{regime}"
    if regime == "index":
        assert np.array_equal(first.astype(np.float64), S64.numpy()), (group, case, "integers: S must be the bank entry to the bit")
        want = mr.bf16_value(data.bank)[:, kq].T
        if c["Q"] == 257 and steps == 4:
            assert sorted(set(kq.tolist())) == list(range(256)), "the positions do not cover every k"
        assert np.array_equal(mr.fold_f32(first), want), (group, case)
    def refs(P, bank, S64, S32):
        if regime != "p1-neg":
            return S64, S32
        # float64 and the fp32 evaluation a1 b + a0 b are both exactly 0: there is no error to scale.  What passes through the kernel's accumulators
        # is +- the one-plane product a0 b, each addition rounded at THAT size; the bound is the fp32 CPU evaluation's error on a0 b.
        one64, one32 = mr.coarse_ref(P[:1], bank, steps, ksplit)
        return S64, (one32.double() - one64).float()

    extra = None
    if c["Q"] * c["N"] < 1024 and regime != "index":
        Px, bx, _ = mr.pass_operands(regime, 32, 32, 64 * steps, g["planes"], mr.rng(f"extra-{group}-{case}"))
        extra = refs(Px, bx, *mr.coarse_ref(Px, bx, steps, ksplit))
    hold(group, case, first, *refs(data.P, data.bank, S64, S32), extra=extra)
    if True:                                                                   # (b), every regime
        bn = _bnorm(data)
        a = sum(mr.bf16_value(p).astype(np.float64) for p in data.P)
        b = mr.bf16_value(data.bank).astype(np.float64)
        v64 = (b * b).sum(1)[None, :] - 2 * (a @ b.T)
        v = (bn[None, :] - np.float32(2) * mr.fold_f32(first)).astype(np.float32)
        slack = mr.MARGIN_BF16 * ((a * a).sum(1)[:, None] + (b * b).sum(1)[None, :])
        ratio = float((np.abs(v.astype(np.float64) - v64) / slack).max())
        w = RATIOS.setdefault(group + " (b)", [0.0, 0.0])
        w[0] = max(w[0], ratio)
        print(f"[match] {group:22s} {case:40s} (b) |v - v64| / (5e-5 (|a|^2 + |b|^2)) max {ratio:.4f}")
        assert ratio <= 1.0, (group, case, ratio)


@gpu
@pytest.mark.parametrize("group", list(GROUPS))
def test_coarse_pass_sweep(group):
    g = GROUPS[group]
    for c in (dict(c) for c in pass_cases(group)):
        Dk = 64 * c["steps"]
        P, bank, kq = mr.pass_operands(c["regime"], c["Q"], c["N"], Dk, g["planes"], mr.rng(f"pass-{group}-{sorted(c.items())}"))
        data = PassData(P, bank, c["Q"], c["N"], Dk)
        res = [data.run(g["kind"], v, 1) for v in g["variants"]]
        again = data.run(g["kind"], g["variants"][0], 1)
        assert same_bits(again, res[0]), (group, c, "run to run")
        _check_pass(group, c, data, res, kq)
    hold_pool(group)


@gpu
@pytest.mark.parametrize("group", list(GROUPS))
def test_coarse_pass_ragged_splits(group):
    """Slices of two steps, one of one step, the rest empty: the empty ones' slabs are zeros, exactly, in every variant."""
    g = GROUPS[group]
    for (steps, ksplit), regime, (Q, N) in zip(RAGGED[g["kind"]] * len(g["regimes"]), [r for r in g["regimes"] for _ in RAGGED[g["kind"]]],
                                               ((129, 260), (9, 257), (257, 127), (128, 1027), (1, 3), (127, 256), (129, 129), (9, 128))):
        c = dict(group=group, Q=Q, N=N, steps=steps, ksplit=ksplit, regime=regime)
        P, bank, kq = mr.pass_operands(regime, Q, N, 64 * steps, g["planes"], mr.rng(f"ragged-{group}-{steps}-{regime}"))
        data = PassData(P, bank, Q, N, 64 * steps)
        _check_pass(group, c, data, [data.run(g["kind"], v, ksplit) for v in g["variants"]], kq)


@gpu
@pytest.mark.parametrize("group", ["gemm<4,1>", "gemm<3,2>"])
def test_gemm_tickets_fold(group):
    """With tickets, slab 0 is the ticket-less run's slabs added in slab order from zero in fp32 (to the bit: the fold reads back the very
    slabs the run without tickets leaves, and states the order), the other slabs are untouched, the tickets are all zero again, and a
    second launch on them gives the same bits.  K split 2 with slices of 1 .. 3 R + 1 steps, and the ragged split 9 / 8."""
    g = GROUPS[group]
    shapes = itertools.cycle(((129, 260), (9, 257), (257, 128), (128, 1027), (1, 3), (127, 255), (257, 256), (9, 1), (129, 129), (127, 127)))
    for (steps, ksplit), (Q, N) in zip([(2 * s, 2) for s in range(1, 3 * g["R"] + 2)] + [(9, 8), (12, 4)], shapes):
        regime = g["regimes"][steps % len(g["regimes"])]
        P, bank, kq = mr.pass_operands(regime, Q, N, 64 * steps, g["planes"], mr.rng(f"tickets-{group}-{steps}"))
        data = PassData(P, bank, Q, N, 64 * steps)
        plain = data.run("gemm", g["variants"][0], ksplit)
        ntk = ((Q + 127) // 128) * ((N + 127) // 128)
        for v in g["variants"]:
            tk = torch.zeros((ntk + 8,), dtype=torch.int32, device=dev())
            for _ in range(2):
                S = data.run("gemm", v, ksplit, tickets=tk)
                assert same_bits(S[0], mr.fold_f32(plain)), (inst_name(group, v, 1), Q, N, steps, ksplit)
                assert same_bits(S[1:], plain[1:]), (inst_name(group, v, 1), "slabs 1 .. were touched")
                assert not bool(tk.any()), "tickets are not zero again"
        if ksplit == 2 and steps == 2:
            c = dict(group=group, Q=Q, N=N, steps=steps, ksplit=ksplit, regime=regime)
            _check_pass(group, c, data, [plain], kq)
    tk = torch.ones((ntk + 8,), dtype=torch.int32, device=dev())
    data.run("gemm", g["variants"][0], ksplit, tickets=tk, expect=mr.BAD_ARGUMENT)          # tickets that are not zero at first use


@gpu
@pytest.mark.parametrize("group", list(GROUPS))
def test_coarse_pass_full_depth(group):
    """D = 23040, Q = 129, N = 513: every K split the launcher accepts - the one match_bf16_ksplit / match_pass256_ksplit returns for the shape
    among them - on the first and the last variant of the group ((c) between them), the others refused by the launcher."""
    g = GROUPS[group]
    L = mr.load()
    Q, N, steps = 129, 513, 360
    accepted = (1, 2, 4, 8) if g["kind"] == "gemm" else (1, 2, 4, 8, 16)
    chosen = L.mp_bf16_ksplit(Q, N) if g["kind"] == "gemm" else L.mp_pass256_ksplit(Q, N)
    assert chosen in accepted, chosen
    P, bank, kq = mr.pass_operands("normal", Q, N, 64 * steps, g["planes"], mr.rng(f"full-{group}"))
    data = PassData(P, bank, Q, N, 64 * steps)
    vs = [g["variants"][0], g["variants"][-1]]
    for ksplit in accepted:
        c = dict(group=group, Q=Q, N=N, steps=steps, ksplit=ksplit, regime="normal")
        res = [data.run(g["kind"], v, ksplit) for v in vs]
        assert same_bits(res[0], res[1])
        _check_pass(group, c, data, res[:1], kq)
    for ksplit in (3, 32) + ((16,) if g["kind"] == "gemm" else ()):
        data.run(g["kind"], vs[0], ksplit, expect=mr.INVALID_VALUE)


@gpu
def test_coarse_pass_refusals():
    """What no launcher checks: S off the 16-byte grid of its stores when N % 4 == 0, a second plane that is not Q D elements behind the
    first, an image shorter than the launcher reads, operands off the 16-byte grid; and the launchers' own refusals pass through."""
    L = mr.load()
    Q, N, Dk = 9, 260, 128
    P, bank, _ = mr.pass_operands("normal", Q, N, Dk, 2, mr.rng("refuse-pass"))
    d = PassData(P, bank, Q, N, Dk)
    out = Out((1, Q, N))
    qe = 2 * Q * Dk
    img, elems = d.img["gemm"]
    i32, e32 = d.img["pass"]
    bad = [
        call(L.mp_match_gemm_bf16, mr.ptr(d.dq), qe, Q * Dk, mr.ptr(d.db), out.ptr + 4, Q, N, Dk, 1, 2, 0, 0, 0, 0, 0),
        call(L.mp_match_pass256, mr.ptr(d.dq), qe, Q * Dk, mr.ptr(d.db), out.ptr + 8, Q, N, Dk, 1, 0, 2, 0, 0, 0),
        call(L.mp_match_gemm_bf16, mr.ptr(d.dq), qe, Q * Dk + 8, mr.ptr(d.db), out.ptr, Q, N, Dk, 1, 2, 0, 0, 0, 0, 0),
        call(L.mp_match_pass256, mr.ptr(d.dq), qe, 0, mr.ptr(d.db), out.ptr, Q, N, Dk, 1, 0, 2, 0, 0, 0),
        call(L.mp_match_pass256, mr.ptr(d.dq), qe // 2, Q * Dk, mr.ptr(d.db), out.ptr, Q, N, Dk, 1, 0, 2, 0, 0, 0),
        call(L.mp_match_gemm_bf16, mr.ptr(d.dq), qe, Q * Dk, mr.ptr(d.db), out.ptr, Q, N, Dk, 1, 2, mr.ptr(img), elems - 1, 0, 0, 0),
        call(L.mp_match_pass256, mr.ptr(d.dq), qe, Q * Dk, mr.ptr(d.db), out.ptr, Q, N, Dk, 1, 0, 2, mr.ptr(i32), e32 - 1, 0),
        call(L.mp_match_gemm_bf16, mr.ptr(d.dq) + 2, qe, Q * Dk, mr.ptr(d.db), out.ptr, Q, N, Dk, 1, 2, 0, 0, 0, 0, 0),
        call(L.mp_match_pass256, mr.ptr(d.dq), qe, Q * Dk, mr.ptr(d.db) + 4, out.ptr, Q, N, Dk, 1, 0, 2, 0, 0, 0),
        call(L.mp_match_pass256, mr.ptr(d.dq), qe, Q * Dk, 0, out.ptr, Q, N, Dk, 1, 0, 2, 0, 0, 0),
    ]
    assert bad == [mr.BAD_ARGUMENT] * len(bad) and out.intact(), bad
    assert call(L.mp_match_pass256, mr.ptr(d.dq), qe, Q * Dk, mr.ptr(d.db), out.ptr, Q, N, Dk, 1, 256, 2, 0, 0, 0) == mr.UNSUPPORTED and out.intact()
    own = [
        call(L.mp_match_pass256, mr.ptr(d.dq), qe, Q * Dk, mr.ptr(d.db), out.ptr, Q, N, Dk, 1, 5, 2, 0, 0, 0),       # PFS 5 with two planes
        call(L.mp_match_pass256, mr.ptr(d.dq), qe, Q * Dk, mr.ptr(d.db), out.ptr, Q, N, Dk, 1, 2, 1, 0, 0, 0),       # PFS 2 with one
        call(L.mp_match_pass256, mr.ptr(d.dq), qe, Q * Dk, mr.ptr(d.db), out.ptr, Q, N, Dk, 1, 0, 3, 0, 0, 0),       # three planes
        call(L.mp_match_gemm_bf16, mr.ptr(d.dq), qe, Q * Dk, mr.ptr(d.db), out.ptr, Q, N, Dk, 16, 2, 0, 0, 0, 0, 0),
    ]
    assert own == [mr.INVALID_VALUE] * len(own) and out.intact(), own


@gpu
def test_fp32_bank_route_is_inside_its_margin():
    """The fp32-bank route of do_match on the GEMM probe: S = qc (bank - centre)^T by the exact-f32 MFMA GEMM with wsub = centre and a K
    split, bnorm from launch_rownorm2 with the same centre; |(bnorm - 2 sum_z S_z) - v64| <= 4e-6 (||qc||^2 + ||b - c||^2) for every (q, n),
    v64 the same expression in float64 on the same fp32 operands (the centred weight rounded once to fp32, as the staging does)."""
    import gemm_probe as gp
    Q, N, Dk, ks = 129, 513, 2048, 4
    r = mr.rng("fp32-route")
    c = (0.1 * r.standard_normal(Dk, dtype=np.float32)).astype(np.float32)
    bank = (r.standard_normal((N, Dk), dtype=np.float32) + c).astype(np.float32)
    qc = r.standard_normal((Q, Dk), dtype=np.float32)
    dq, db, dc = todev(qc), todev(bank), todev(c)
    out, bn = Out((ks, Q, N)), Out((N,))
    p = gp.make_params(A=mr.ptr(dq), W=mr.ptr(db), C=out.ptr, wsub=mr.ptr(dc), M=Q, N=N, K=Dk, lda=Dk, ldc=N, ksplit=ks, slab_stride=Q * N)
    assert call(gp.run, p, "f32") == 0
    assert call(pr.load().pw_rownorm2, mr.ptr(db), mr.ptr(dc), bn.ptr, N, Dk, 0, 0) == 0
    S, bnorm = out.check("S of the fp32 route"), bn.check("bnorm")
    b = (bank - c[None, :]).astype(np.float32).astype(np.float64)
    a = qc.astype(np.float64)
    v64 = (b * b).sum(1)[None, :] - 2 * (a @ b.T)
    v = (bnorm[None, :] - np.float32(2) * mr.fold_f32(S)).astype(np.float32)
    ratio = float((np.abs(v.astype(np.float64) - v64) / (mr.MARGIN_F32 * ((a * a).sum(1)[:, None] + (b * b).sum(1)[None, :]))).max())
    RATIOS["fp32 route (b)"] = [ratio, 0.0]
    print(f"[match] fp32 route: |v - v64| / (4e-6 (|qc|^2 + |b - c|^2)) max {ratio:.4f}")
    assert ratio <= 1.0, ratio


# =================================================================================================== family 3: the two selections on authored scores
INSIDE = (0, 1, 15, 16, 17, 63, 64, 65, 127, 128, 129)
SEL_NS = (1, 2, 5, 4095, 4096, 4097, 4100, 16384, 16389, 20000)
SEL_QS = (1, 9, 17)
SEL_KS = (1, 2, 8, 16)


def _select_specs():
    """name -> keyword arguments of mr.build_select.  Every N of the issue at D = 256 in both modes, Q and ksplit cycling, the queries of a
    case walking through INSIDE from a moving start (every count meets both modes, both sides of both list capacities); every row a copy;
    the winner the lowest of a run of copies spread over the bank; D = 23040 with N <= 300."""
    specs = {}
    i = 0
    for N in SEL_NS:
        for mode in ("f32", "b16"):
            Q = 1 if N <= 5 else SEL_QS[i % 3]
            inside = [INSIDE[(3 * i + j) % len(INSIDE)] for j in range(Q)]
            specs[f"n{N}-{mode}"] = dict(N=N, D=256, Q=Q, ksplit=SEL_KS[i % 4], mode=mode, inside=inside, planes=1 + (i // 2) % 2 if mode == "b16" else 1)
            i += 1
    for j, (N, mode) in enumerate(((4100, "f32"), (4097, "b16"), (20000, "f32"), (16389, "b16"))):
        specs[f"n{N}-{mode}-all-inside"] = dict(N=N, D=256, Q=SEL_QS[j % 3], ksplit=SEL_KS[(j + 1) % 4], mode=mode, inside="all")
        specs[f"n{N}-{mode}-copies"] = dict(N=N, D=256, Q=9, ksplit=SEL_KS[j % 4], mode=mode, inside=[INSIDE[(j + q) % len(INSIDE)] for q in range(9)], dup=5)
    for j, (N, mode, Q) in enumerate(((300, "f32", 9), (300, "b16", 17), (257, "b16", 1), (5, "f32", 1))):
        specs[f"d23040-n{N}-{mode}"] = dict(N=N, D=23040, Q=Q, ksplit=SEL_KS[(j + 2) % 4], mode=mode, inside=[INSIDE[(j + 2 * q) % (8 if Q <= 9 else 5)] for q in range(Q)],
                                           planes=1 + j % 2 if mode == "b16" else 1)
    return specs


SELECT_SPECS = _select_specs()
KERNELS = ("select", "select2")            # every case runs on both


@functools.lru_cache(None)
def select_case(name):
    return mr.build_select(name, **SELECT_SPECS[name])


def test_select_cases_are_valid_and_cover():
    """build_select checks every case as it builds it: the float64 answer is the authored winner, its gap to the best other row is exactly
    zero or at least 1e-4 relative, every authored error lies between 0.8 and 1.0 of the bound, every decoy and copy looks better than
    the winner.  Here: the candidate rule, in float64 on the scores the kernel sees, keeps exactly the rows authored inside the bound (the
    same count with the threshold at 0.98 and at 1.02: no row hangs on an fp32 rounding), and the counts, placements and factors cover."""
    counts, factors = {(kern, mode): set() for kern in KERNELS for mode in ("f32", "b16")}, set()
    at = {"winner": set(), "decoy": set()}
    for name, spec in SELECT_SPECS.items():
        k = select_case(name)
        factors |= {("N", k.N), ("Q", k.Q), ("ks", k.ksplit), ("D", k.D)}
        factors |= {(kern, k.mode, what, v) for kern in KERNELS for what, v in (("N", k.N), ("ks", k.ksplit), ("D", k.D))}
        for i in range(k.Q):
            n = [len(mr.candidates(k, i, rel)) for rel in (0.98, 1.0, 1.02)]
            assert n[0] == n[1] == n[2] == k.inside[i] + 1, (name, i, n, k.inside[i])
            if spec["inside"] != "all" and not spec.get("dup"):
                for kern in KERNELS:
                    counts[kern, k.mode].add(k.inside[i])
            if spec["inside"] != "all" and k.N >= 4095:
                w, cp, dec = k.groups[i]
                for what, rows in (("winner", [w]), ("decoy", list(dec) + list(cp))):
                    at[what] |= {"last" if v == k.N - 1 else v for v in rows}
    for km in counts:                                                          # per (kernel, bank type): every inside count, every N, K split and D
        assert set(INSIDE) <= counts[km], (km, sorted(set(INSIDE) - counts[km]))
        assert {km + ("N", n) for n in SEL_NS} | {km + ("ks", s) for s in SEL_KS} | {km + ("D", d) for d in (256, 23040)} <= factors, km
    assert {("N", n) for n in SEL_NS} | {("Q", q) for q in SEL_QS} | {("ks", s) for s in SEL_KS} | {("D", 256), ("D", 23040)} <= factors
    # the winner, and a candidate, at both ends, on both sides of the register chunks and of the multiples of 64 / 128 that bound a list window
    edges = {0, "last", 63, 64, 127, 128, 4095, 4096, 16383, 16384}
    assert edges <= at["winner"] and edges <= at["decoy"], (sorted(map(str, edges - at["winner"])), sorted(map(str, edges - at["decoy"])))
    print(f"[match] selection cases: {len(SELECT_SPECS)}, queries {sum(select_case(n).Q for n in SELECT_SPECS)}")


LAYOUTS = ("tight", "pad3", "odd-stride")
_dist_pool = {}


def _run_select(k, kernel, layout, want_dist, S=None, expect=0):
    """One launch of `kernel` ("select" / "select2") on the case's authored slabs in `layout`: tight (lds = N, slab_stride = Q N: the
    16-byte score path when N % 4 == 0), pad3 (lds = N + 3, the pad columns hold -1e30: a score read from there would win), odd-stride
    (slab_stride = Q lds + 1)."""
    L = mr.load()
    S = k.S if S is None else S
    lds = k.N + (3 if layout == "pad3" else 0)
    stride = k.Q * lds + (1 if layout == "odd-stride" else 0)
    host = np.full((k.ksplit, stride), -1e30, np.float32)
    host[:, :k.Q * lds].reshape(k.ksplit, k.Q, lds)[:, :, :k.N] = S
    dS, dbn, dq, dc = todev(host), todev(k.bnorm), todev(k.query), todev(k.centre)
    dbank = todev(k.bank) if k.bank is not None else None
    db16 = u16dev(k.bank16) if k.bank16 is not None else None
    dqs = todev(k.qstat)
    idx, dist = Out((k.Q,)), (Out((k.Q,)) if want_dist else None)
    common = (mr.ptr(dS), k.ksplit, stride, lds, mr.ptr(dbn), mr.ptr(dq), mr.ptr(dc), mr.ptr(dbank), mr.ptr(db16))
    tail = (k.margin, k.Q, k.N, k.D, idx.ptr, dist.ptr if dist else 0, 0)
    if kernel == "select":
        rc = call(L.mp_match_select, *common, *tail)
    else:
        rc = call(L.mp_match_select2, *common, mr.ptr(dqs), *tail)
    assert rc == expect, (k.name, kernel, layout, rc)
    if expect:
        assert idx.intact() and (dist is None or dist.intact())
        return None, None
    return idx.check("idx").view(np.int32), (dist.check("dist") if dist else None)


@gpu
@pytest.mark.parametrize("name", list(SELECT_SPECS))
def test_selection_on_authored_scores(name):
    """Both kernels, dist null and non-null, the three score layouts: the index is the float64 argmin (ties to the lowest row) although
    every decoy's coarse score looks better than the winner's by up to 1.8 times the bound; dist is pooled in test_selection_dist_pool."""
    k = select_case(name)
    for kernel in KERNELS:
        # (a case authored with two query planes: mocha_match_select measures the ONE-plane residual itself, a larger bound than the errors
        # were authored against - it keeps more candidates and must return the same row)
        for layout, want_dist in itertools.product(LAYOUTS, (True, False)):
            idx, dist = _run_select(k, kernel, layout, want_dist)
            assert np.array_equal(idx, k.answer), (name, kernel, layout, want_dist, idx[:8], k.answer[:8])
            if want_dist:
                rows = np.arange(k.Q)
                ref64, ref32 = np.sqrt(k.d2_64[rows, k.answer]), np.sqrt(k.d2_32[rows, k.answer]).astype(np.float64)
                _dist_pool.setdefault(f"{kernel} {k.mode}", {})[(name, layout)] = (dist.astype(np.float64) / ref64, ref64 / ref64, ref32 / ref64)


@gpu
def test_selection_dist_pool():
    """dist: the direct-form distance of the answer against float64, bounded by the fp32 CPU evaluation of the same direct form; a case has
    1 to 17 distances, so the relative errors of all cases of a kernel and bank type are pooled."""
    ran = {name for pool in _dist_pool.values() for name, _ in pool}
    for name in SELECT_SPECS:                                                  # (selected on its own: the cases this test pools are run here)
        if name not in ran:
            test_selection_on_authored_scores(name)
    assert len(_dist_pool) == 4
    for inst, pool in sorted(_dist_pool.items()):
        got, r64, r32 = (np.concatenate([v[j] for _, v in sorted(pool.items())]) for j in range(3))
        hold(inst + " dist", f"{len(got)} distances, relative", got, r64, r32, ulp=float(np.spacing(np.float32(1.0))))


@gpu
@pytest.mark.parametrize("mode", ["f32", "b16"])
def test_selection_nan_and_inf_scores(mode):
    """NaN scores never win; NaN in the OTHER queries' score rows leaves a query's result alone to the bit; with every score of a query NaN,
    or +inf, the answer is row 0 - mocha_match_select2 reports dist NaN, mocha_match_select evaluates row 0 and reports its distance."""
    name = f"n4100-{mode}"
    k = select_case(name)
    clean = {kern: _run_select(k, kern, "tight", True) for kern in ("select", "select2")}
    S = k.S.copy()
    for i in range(k.Q):                                                       # the rows that look best, the winner excepted, and a run at the end
        order = [n for n in np.argsort(k.seen[i])[:40] if n != k.winner[i]]
        S[i % k.ksplit, i, order[::2]] = np.nan
        S[:, i, [n for n in range(k.N - 5, k.N) if n != k.winner[i]]] = np.nan
    for kern in ("select", "select2"):
        for layout in LAYOUTS:
            idx, dist = _run_select(k, kern, layout, True, S=S)
            # (mocha_match_select sums a row in an order chosen from the candidate count, which the NaN rows changed: no bit equality here)
            assert np.array_equal(idx, k.answer) and np.allclose(dist, clean[kern][1], rtol=1e-5, atol=0), (kern, layout)
    for fill, what in ((np.nan, "NaN"), (-np.inf, "+inf score")):
        S = k.S.copy()
        S[:, 1::2, :] = fill                                                   # every odd query: no finite score; the even ones must not notice
        for kern in ("select", "select2"):
            idx, dist = _run_select(k, kern, "tight", True, S=S)
            assert np.array_equal(idx[0::2], k.answer[0::2]) and same_bits(np.ascontiguousarray(dist[0::2]), np.ascontiguousarray(clean[kern][1][0::2])), (kern, what)
            assert (idx[1::2] == 0).all(), (kern, what, idx)
            if kern == "select2":
                assert np.isnan(dist[1::2]).all(), (kern, what, dist)
            else:
                d0 = np.sqrt(k.d2_64[1::2, 0])
                assert np.allclose(dist[1::2], d0, rtol=1e-5, atol=0), (kern, what, dist[1::2], d0)
            idx2, _ = _run_select(k, kern, "tight", False, S=S)
            assert np.array_equal(idx2, idx), (kern, what, "dist == null")


@gpu
def test_selection_refusals():
    """What no launcher checks: both banks or none, S / bnorm off the 16-byte grid of the vector score path, a score row longer than its
    leading dimension, slabs that overlap, D = 0 (which passes the launchers' D % 256); the launchers' own: a negative margin, D off 256."""
    L = mr.load()
    k = select_case("n4100-f32")
    dS, dbn, dq, dc, dbank, dqs = todev(k.S), todev(k.bnorm), todev(k.query), todev(k.centre), todev(k.bank), todev(k.qstat)
    idx = Out((k.Q,))
    ok = dict(S=mr.ptr(dS), ksplit=k.ksplit, slab_stride=k.Q * k.N, lds=k.N, bnorm=mr.ptr(dbn), query=mr.ptr(dq), centre=mr.ptr(dc), bank=mr.ptr(dbank),
              bank16=0, margin=k.margin, Q=k.Q, N=k.N, D=k.D)

    def both(expect, **kw):
        a = dict(ok, **kw)
        head = (a["S"], a["ksplit"], a["slab_stride"], a["lds"], a["bnorm"], a["query"], a["centre"], a["bank"], a["bank16"])
        tail = (a["margin"], a["Q"], a["N"], a["D"], idx.ptr, 0, 0)
        assert call(L.mp_match_select, *head, *tail) == expect and idx.intact(), kw
        assert call(L.mp_match_select2, *head, mr.ptr(dqs), *tail) == expect and idx.intact(), kw

    for kw in (dict(bank16=mr.ptr(dbank)), dict(bank=0), dict(S=mr.ptr(dS) + 4), dict(bnorm=mr.ptr(dbn) + 8), dict(lds=k.N - 4),
               dict(ksplit=2, slab_stride=k.Q * k.N - 4), dict(D=0), dict(query=mr.ptr(dq) + 4), dict(centre=0), dict(ksplit=0)):
        both(mr.BAD_ARGUMENT, **kw)
    for kw in (dict(margin=-1e-6), dict(margin=float("nan")), dict(D=k.D + 64)):
        both(mr.INVALID_VALUE, **kw)
    head = (ok["S"], ok["ksplit"], ok["slab_stride"], ok["lds"], ok["bnorm"], ok["query"], ok["centre"], ok["bank"], 0)
    assert call(L.mp_match_select2, *head, 0, k.margin, k.Q, k.N, k.D, idx.ptr, 0, 0) == mr.BAD_ARGUMENT and idx.intact()      # no qstat


@gpu
def test_zz_worst_ratios():
    """Last in the file: the worst ratio per instance over the cases that ran in this process (the figures of the docstring)."""
    for inst, (a, b) in sorted(RATIOS.items()):
        print(f"[match] worst {inst:26s} max {a:.3f}  rms {b:.3f}")
    for inst in POOL:
        hold_pool(inst)
