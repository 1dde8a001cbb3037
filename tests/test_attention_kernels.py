"""The attention kernels against float64 at the kernel boundary (GPU cases: -m gpu; the CPU pins of the reference run everywhere).

The twelve instances of csrc/attention.hip (mocha_attention_f32<DH,NKT,NQW>), csrc/attention_x3.hip (mocha_attention_x3<DH,PF2>,
mocha_attention_x3_split<256>) and csrc/attention_kv.hip (mocha_attention_x3_kv<256,HPW>) are launched directly through
tests/gemm_probe/attention_probe.cpp at every token count that is an edge of a tile or of the masking (1 .. 96, 97 .. 192 for the six-tile
instances), 1 .. 9 windows (the grid's padding to 8 and its early return), 1 .. 4 heads and every operand layout the contract allows - the
network itself only ever calls them with 90 x 90 tokens (182 x 182, 90 x 181 in the CVAE), behind GEMMs - and held to

  (a) the float64 restatement of the operation (tests/attention_ref.py; pinned without a GPU to torch's scaled_dot_product_attention and
      nn.MultiheadAttention by the test_reference_* functions below).  Bound: the error of the SAME restatement evaluated in fp32 by torch
      on the CPU against float64, times MARGINS[instance] = (on the largest error, on the rms error), plus one fp32 ulp of the largest
      output on the largest error.  The x3 and kv kernels get the bound of the f32 kernel;
  (b) the relations the code promises to the bit (PF2 true / false, reverse, kv_idx / the materialised gather, hsk = hsv = 0 / replicated
      rows, kv<256,4> / kv<256,2>, independence of B and of the window's position, run-to-run);
  (c) isolation: NaN in every other window's q, k and v rows leaves a window's bits alone;
  (d) untouched memory: 0x7FC0DEAD guard words in front of and behind every output and in the unused columns of a wide ldo, every
      element of rows < nq and columns < heads dh written; every refusal leaves the output intact.

Margins.  (4, 2) on the largest / rms error are the starting values and stay for every instance but five.  Measured on an MI355X (604 GPU
cases, 548 of them parity cases; ratio = kernel error / fp32 CPU error of the same restatement; every case prints its own with -s), worst
per instance, largest / rms, and the median rms ratio of the instance's peaked cases:
  f32<128,3,3> 1.58 / 1.18 (0.97)   f32<256,3,3> 3.03 / 1.97 (1.65)   f32<64,3,3> 2.28 / 1.54 (1.02)   f32<64,6,3> 2.53 / 1.84 (1.01)
  f32<64,6,6> 2.36 / 1.75 (1.00)   x3<128,true> 2.03 / 1.15 (0.79)   x3<128,false> 1.59 / 1.08   x3<256,true> 2.91 / 2.14 (1.37)
  x3<256,false> 1.71 / 1.44 (0.89)   x3 split<256> 1.34 / 1.02 (0.49)   kv<256,4> 4.17 / 2.74 (1.36)   kv<256,2> 2.24 / 1.58 (1.37)
Tightened to (4, 1.5): x3 split<256> and x3<128,false>.  Widened to (4.5, 3), just above what was measured: x3<256,true> (q65-k2 2.91 /
2.14 with 520 queries, q90-k90 2.13 with 90) and kv<256,4> (q2-k2, 72 queries, 4.17 / 2.74), and with them f32<256,3,3> (1.97, the
largest that stays inside the start), because an x3 or kv bound may not be looser than the f32 one of its head dim.  The reason is these
kernels' own summation order, measured inside the family: a score at head dim 256 is ONE fp32 running sum (f32: 128 MFMA steps of 2
products; x3, kv: 16 steps of six passes) and the peaked cases of all five such instances have a median ratio of 1.36 - 1.65, while
x3 split<256>, the same arithmetic as four partial sums of 64, has 0.49 and the single sums over 64 and 128 head dims have 0.8 - 1.0.  In
the peaked regime the output error of a query IS the score error of its top keys (d p / p = d logit, logits of a few tens), so that
factor comes through undamped and leaves the starting 2 too little room; kv<256,2> and x3<256,false> measured inside it and keep it.
Peaked cases and few queries.  Only the queries whose two largest logits lie close carry any error in the peaked regime, so a case's rms
error - the kernel's and the fp32 CPU evaluation's - is a sample of a fraction of its B heads nq (window, head, query) triples, and the
ratio of two handfuls has no bound: with the cases as first dealt, f32<256,3,3> q1-k95 (9 triples) measured 4.19 / 3.66, x3<256,true>
q2-k2 (8) 2.54, x3<128,true> q1-k65 (8) 2.32, f32<64,6,3> q2-k160 (2) 2.04 and, at 18 triples, 3.25 - in instances whose median is 1.0.
_enough_queries therefore gives a peaked case of fewer than 64 triples nine windows and, if need be, four heads (36 triples at nq = 1,
72 at nq = 2: the most the grid of B and heads has); the cover assertion still holds for every pair of factors.
(b) Every relation holds to the bit, kv<256,4> against kv<256,2> (pairs = 1) included: both add, per key tile, the k steps and inside one
the six plane pairs in the same order, whichever loop is outside.  Between split and the three-wave kernel and between kv and x3 only
(a) is asserted, as the code promises.
Kernel fix.  With ONE key the softmax weight is exactly 1 and the output is the value row; the fp32 CPU evaluation and the f32 kernel give
exactly that, the x3 and kv kernels were one ulp above it in magnitude in about 3 % of the elements, whole (query, head) rows at a time (25 cases
failed on an rms bound of 0).  Cause: the compiler contracted the product e * (1 / sum) into the first subtraction of the plane split, so the three
planes carried the unrounded product (1 + a fraction of 2^-24) instead of the fp32 weight.  mul_rn (csrc/device_utils.h) rounds the weight
before it is split, as attention.hip's is; the single-key cases are now exact in all twelve instances.  tests/test_gemm_engines.py and
tests/test_hip_parity.py pass unchanged and the demo benchmark is unchanged (115.6 against 115.6 thousand frames/s, alternating runs).
Mutations, each on a scratch copy (never committed), failing cases of this file / of tests/test_gemm_engines.py / of tests/test_hip_parity.py:
  1. mocha_attention_x3's mask compares key > nk: 87 (83 of the 106 parity cases of the four x3<DH,PF2> instances and their 4
     all-zero-query cases; the 23 that pass all have nk = 96 - no padded key - or nk = 1 - the clamped row is the one key again) / 10 of
     31 / 15 of 60.
  2. mocha_attention_f32 without the cross-half max exchange: 286 of the 306 parity cases of the five f32 instances (the 20 that pass are
     one-window tie cases, every logit of a query equal, so both halves hold the same maximum) / 10 of 31 / 0 of 60 (the network's default
     path takes the x3 kernels).
  3. mocha_attention_x3_kv without the third-plane products in P V: 99 (97 of the 100 kv parity cases and both all-zero-query cases; the
     3 that pass are peaked cases of one or two queries a window, whose weights are one-hot to the last bit, so that the loss is 2^-17 of
     a value against a bound set by the score error) / 3 of 31 / 0 of 60.
  (This file's counts with the final cases and margins; the two other files' from the runs of the first deal of the cases.)
Run time on the GPU box: 16 s for the file (pointwise file: 14 s), CPU references included; the slowest cases are the full-batch x3 ones
(260 (window, head) pairs in float64: 0.3 - 0.7 s).  Every case ran and was measured.
"""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attention_ref as ar  # noqa: E402
import pointwise_ref as pr  # noqa: E402
from test_pointwise_kernels import D, Out, T, normal, rng, same_bits  # noqa: E402  (the guard pattern and the named generators)

gpu = pytest.mark.gpu
# margin on the largest / on the rms error of the fp32 CPU evaluation, per instance (docstring, "Margins")
DEFAULT_MARGIN = (4.0, 2.0)
WIDE256 = (4.5, 3.0)                          # one running sum over 256 head dims: measured, docstring
MARGINS = {"x3 split<256>": (4.0, 1.5), "x3<128,false>": (4.0, 1.5), "f32<256,3,3>": WIDE256, "x3<256,true>": WIDE256, "kv<256,4>": WIDE256}

SMALL = (1, 2, 31, 32, 33, 64, 65, 90, 95, 96)
BIG = (97, 128, 129, 160, 181, 182, 192)
BS = (1, 7, 8, 9)
HEADS = (1, 2, 3, 4)
REGIMES = ("normal", "peaked", "tie")
WHICH = {"f32": ar.F32, "x3": ar.X3, "kv": ar.KV}


# =================================================================================================== the cases
def _inst(c):
    return ar.instance(WHICH[c["which"]], dh=c["dh"], nq=c["nq"], nk=c["nk"], B=c["B"], heads=c["heads"], split_max=c.get("split_max", 192),
                       pairs=c.get("pairs", 0))


def _uncovered(fam, cs):
    """The pairs of values of two factors of a family's cases that never meet.  Left out: (nq, nk) itself (the grid); the interleaved layout
    (it needs nq = nk); in the full-batch family (a band of the grid, two dozen cases) everything but instance x layout and instance x regime."""
    keys = ("nq", "nk", "inst", "B", "heads", "layout", "regime")
    rows = [dict(c, inst=_inst(c)) for c in cs]
    vals = {k: sorted({r[k] for r in rows}, key=str) for k in keys}
    missing = []
    for a in range(len(keys)):
        for b in range(a + 1, len(keys)):
            ka, kb = keys[a], keys[b]
            if {ka, kb} == {"nq", "nk"} or (fam == "x3 full" and {ka, kb} not in ({"inst", "layout"}, {"inst", "regime"})):
                continue
            if (fam == "f32 6x6" and {ka, kb} == {"inst", "nk"}) or (fam == "kv" and {ka, kb} == {"inst", "heads"}):
                continue                                                      # nk decides the instance; heads 2 and 6 are kv<256,2> whatever `pairs` says
            seen = {(r[ka], r[kb]) for r in rows}
            missing += [(ka, x, kb, y) for x in vals[ka] for y in vals[kb] if "qkv" not in (x, y) and (x, y) not in seen]
    return missing


def _latin(name, rows, cols, n):
    """(i, j) -> a value in range(n) such that, n <= min(rows, cols), every value meets every i and every j: (R[i] + C[j]) % n with R, C
    permutations chosen by the factor's name."""
    r = rng("latin-" + name)
    R, Cc = r.permutation(rows), r.permutation(cols)
    return lambda i, j: int((R[i] + Cc[j]) % n)


def _family(fam, which, nqs, nks, variants, layouts, heads=HEADS, keep=None, qkv=True):
    """One case per (nq, nk) of nqs x nks; the variant (what selects the instance), B, the head count, the layout and the input regime are
    dealt so that each of their values meets every nq and every nk (test_cases_are_a_pairwise_cover checks the rest)."""
    for salt in range(64):                                                    # the first deal that is a pairwise cover of the small factors too
        out = _deal(f"{fam}-{salt}", fam, which, nqs, nks, variants, layouts, heads, keep, qkv)
        if not _uncovered(fam, out):
            return out
    raise AssertionError(fam)


MIN_PEAKED = 64


def _enough_queries(c):
    """In the peaked regime a query's output error is ONE number, the score error of its top keys, and only the queries whose two largest
    logits lie close carry any: the rms error of a case - the kernel's and the fp32 CPU evaluation's that bounds it - is a sample of a
    fraction of its B heads nq (window, head, query) triples, and the ratio of two such samples has no bound when they are a handful
    (measured: 3.25 with 18 triples in an instance whose median is 1.0).  Below 64 triples a peaked case gets nine windows and, if that is
    not enough, four heads - 36 triples at nq = 1, 72 at nq = 2, the most the issue's grid of B and heads gives."""
    if c["regime"] == "peaked" and c["B"] * c["heads"] * c["nq"] < MIN_PEAKED:
        c = dict(c, B=9)
        if c["B"] * c["heads"] * c["nq"] < MIN_PEAKED:
            c["heads"] = 4
    return c


def _deal(name, fam, which, nqs, nks, variants, layouts, heads, keep, qkv):
    f = {k: _latin(f"{name}-{k}", len(nqs), len(nks), n) for k, n in
         (("variant", len(variants)), ("B", len(BS)), ("heads", len(heads)), ("layout", len(layouts)), ("regime", len(REGIMES)))}
    out = []
    for i, nq in enumerate(nqs):
        for j, nk in enumerate(nks):
            if keep is not None and not keep(i, j, nq, nk):
                continue
            c = dict(variants[f["variant"](i, j)])
            c.update(fam=fam, which=which, nq=nq, nk=nk, regime=REGIMES[f["regime"](i, j)])
            c.setdefault("B", BS[f["B"](i, j)])
            c.setdefault("heads", heads[f["heads"](i, j)])
            c["layout"] = layouts[f["layout"](i, j)]
            c = _enough_queries(c)
            out.append(c)
            if qkv and nq == nk:                                              # the interleaved buffer needs nq = nk: the diagonal, a second time
                out.append(dict(c, layout="qkv"))
    return out


LAYOUTS = ("sep", "wide", "shared", "hs")
FULL = (dict(B=65, heads=4), dict(B=257, heads=1), dict(B=86, heads=3), dict(B=129, heads=2))      # B heads > 256; 65, 257, 86, 129 pad the grid
MUST = ((1, 1), (96, 1), (1, 96))


def _full_pairs(i, j, nq, nk):
    """The full-batch x3 instances cost the CPU 260 (window, head) pairs a case: a diagonal band of the grid and the corners."""
    return (j - i) % 10 in (0, 3) or (nq, nk) in MUST


CASES = (
    _family("f32 small", "f32", SMALL, SMALL, (dict(dh=64), dict(dh=128), dict(dh=256)), LAYOUTS)
    + _family("f32 6x3", "f32", SMALL, BIG, (dict(dh=64),), LAYOUTS)
    + _family("f32 6x6", "f32", BIG, SMALL + BIG, (dict(dh=64),), LAYOUTS)
    + _family("x3 small", "x3", SMALL, SMALL, (dict(dh=128), dict(dh=256, split_max=0), dict(dh=256)), LAYOUTS + ("idx",))
    + _family("x3 full", "x3", SMALL, SMALL, tuple(dict(dh=dh, split_max=sm, **fb) for fb in FULL for dh, sm in ((128, 192), (256, 0))),
              LAYOUTS + ("idx",), keep=_full_pairs)
    + _family("kv", "kv", SMALL, SMALL, (dict(dh=256, pairs=0), dict(dh=256, pairs=1)), ("sep", "wide"), heads=(2, 4, 6, 4), qkv=False)
)


def _id(c):
    return f"{_inst(c)}-q{c['nq']}-k{c['nk']}-B{c['B']}-h{c['heads']}-{c['layout']}-{c['regime']}".replace(" ", "")


INSTANCES = ("f32<128,3,3>", "f32<256,3,3>", "f32<64,3,3>", "f32<64,6,3>", "f32<64,6,6>", "x3<128,true>", "x3<128,false>", "x3<256,true>",
             "x3<256,false>", "x3 split<256>", "kv<256,4>", "kv<256,2>")
# the smallest ordinary configuration of each instance: the relations (b), the isolation (c) and the all-zero queries run on these
REACH = {
    "f32<128,3,3>": dict(which="f32", dh=128, nq=33, nk=31, B=9, heads=2), "f32<256,3,3>": dict(which="f32", dh=256, nq=33, nk=31, B=9, heads=2),
    "f32<64,3,3>": dict(which="f32", dh=64, nq=90, nk=90, B=9, heads=4), "f32<64,6,3>": dict(which="f32", dh=64, nq=90, nk=181, B=9, heads=4),
    "f32<64,6,6>": dict(which="f32", dh=64, nq=182, nk=182, B=9, heads=4),
    "x3<128,true>": dict(which="x3", dh=128, nq=33, nk=31, B=9, heads=2), "x3<128,false>": dict(which="x3", dh=128, nq=33, nk=31, B=65, heads=4),
    "x3<256,true>": dict(which="x3", dh=256, nq=33, nk=31, B=9, heads=4, split_max=0),
    "x3<256,false>": dict(which="x3", dh=256, nq=33, nk=31, B=65, heads=4, split_max=0),
    "x3 split<256>": dict(which="x3", dh=256, nq=33, nk=31, B=9, heads=4),
    "kv<256,4>": dict(which="kv", dh=256, nq=33, nk=31, B=9, heads=4), "kv<256,2>": dict(which="kv", dh=256, nq=33, nk=31, B=9, heads=4, pairs=1),
}


def reach(inst, **kw):
    c = dict(REACH[inst], layout="sep", regime="normal", fam="reach")
    c.update(kw)
    return c


# =================================================================================================== inputs, launches, the bound
class Case:
    """Host operands of a case (torch fp32 2-D views with their leading dimensions) and the launch parameters that describe them."""

    def __init__(self, c, name=None):
        self.c = c = dict(c)
        self.which = WHICH[c["which"]]
        B, h, dh, nq, nk, lay = c["B"], c["heads"], c["dh"], c["nq"], c["nk"], c["layout"]
        self.B, self.heads, self.dh, self.nq, self.nk = B, h, dh, nq, nk
        H = h * dh
        r = rng(name or ("attn-" + _id(c)))
        self.hsk = self.hsv = -1
        self.kv_idx, self.kv_rows = None, 0
        nwin = B                                                             # windows of keys / values
        ldq = ldk = ldv = ldo = H
        if lay == "wide":
            ldq, ldk, ldv, ldo = H + 4, H + 8, H + 12, H + 8
        elif lay == "shared":
            self.hsk = self.hsv = 0
            ldk = ldv = dh
        elif lay == "hs":
            self.hsk, self.hsv = dh + 4, dh + 8
            ldk, ldv = (h - 1) * self.hsk + dh, (h - 1) * self.hsv + dh
        elif lay == "idx":
            self.kv_rows = nwin = 5
            self.kv_idx = np.array(([-3, 7, 2, 2, 0, 4, 5, 1, 3] * (B // 9 + 1))[:B] if B > 1 else [7], dtype=np.int32)
        if self.which == ar.KV:
            ldk = ldv = 256
        self.ldo = ldo
        if lay == "qkv":                                                      # one interleaved buffer, as the encoder and the CVAE use
            assert nq == nk
            self.base = [normal(r, B * nq, 3 * H)]
            self.q, self.k, self.v = self.base[0][:, :H], self.base[0][:, H:2 * H], self.base[0][:, 2 * H:]
        else:
            self.base = [normal(r, B * nq, ldq), normal(r, nwin * nk, ldk), normal(r, nwin * nk, ldv)]
            self.q, self.k, self.v = self.base
        self.scale = float(dh) ** -0.5
        reg = c["regime"]
        if reg == "peaked":                                                   # logits ~ N(0, 9^2): they span a few tens, the softmax is nearly one-hot
            self.q *= np.float32(3)
            self.k *= np.float32(3)
        elif reg == "tie":                                                    # even windows: every key row the same; odd ones: every third
            for w in range(nwin):                                             # (self.k may be a view of the interleaved buffer: no reshape)
                win = self.k[w * nk:(w + 1) * nk]
                win[::(3 if w & 1 else 1)] = win[:1].copy()
        elif reg == "zeroq":
            self.q[:] = 0

    def to_device(self, img=None):
        """Device copies, tight: each buffer ends with its last row.  img: the kv launcher's image, if it is not to be encoded from k and v."""
        dv = [D(b) for b in self.base]
        if len(dv) == 1:
            H = self.heads * self.dh
            p = dv[0].data_ptr()
            self.ptrs, self.lds = (p, p + 4 * H, p + 8 * H), (3 * H,) * 3
        else:
            self.ptrs, self.lds = tuple(t.data_ptr() for t in dv), tuple(b.shape[1] for b in self.base)
        self.dv = dv
        self.d_idx = D(self.kv_idx)
        self.d_img = None
        if img is not None:
            self.d_img = D(img)
        elif self.which == ar.KV:
            img = ar.kv_encode(self.k.reshape(self.B, self.nk, 256), self.v.reshape(self.B, self.nk, 256))
            K, V = pr.kv_decode(img)                                          # the operands the kernel is given ARE the fp32 rows: the planes sum back exactly
            assert np.array_equal(ar.planes_value(K.transpose(1, 0, 2, 3))[:, :self.nk].reshape(-1, 256), self.k.astype(np.float64))
            assert np.array_equal(ar.planes_value(V.transpose(1, 0, 2, 3))[:, :self.nk].reshape(-1, 256), self.v.astype(np.float64))
            self.d_img = D(img)
        return self

    def params(self, out_ptr, **over):
        kw = dict(q=self.ptrs[0], k=self.ptrs[1], v=self.ptrs[2], out=out_ptr, ldq=self.lds[0], ldk=self.lds[1], ldv=self.lds[2], ldo=self.ldo,
                  B=self.B, heads=self.heads, dh=self.dh, nq=self.nq, nk=self.nk, scale=self.scale, hsk=self.hsk, hsv=self.hsv,
                  split_max=self.c.get("split_max", 192), pairs=self.c.get("pairs", 0), kv_idx=ar.ptr(self.d_idx), kv_rows=self.kv_rows,
                  kv=ar.ptr(self.d_img))
        kw.update(over)
        return ar.make_params(**kw)

    def new_out(self, B=None):
        B = self.B if B is None else B
        w = np.zeros((max(B, 1) * self.nq, self.ldo), dtype=bool)
        w[:B * self.nq, :self.heads * self.dh] = True
        return Out(w.shape, written=w)

    def launch(self, expect=0, B=None, **over):
        """One launch under the (d) checks.  Returns [B, nq, heads dh] fp32 (None for a refusal, whose buffers must be intact)."""
        out = self.new_out(B)
        if B is not None:
            over["B"] = B
        torch.cuda.synchronize()
        rc = ar.load().at_attention(self.params(out.ptr, **over), self.which, 0)
        torch.cuda.synchronize()
        assert rc == expect, (self.c, over, rc, expect)
        if expect != 0:
            assert out.intact(), (self.c, over, "a refused launch wrote")
            return None
        B = self.B if B is None else B
        return out.check(str(self.c))[:B * self.nq, :self.heads * self.dh].reshape(B, self.nq, self.heads * self.dh).copy()

    def reference(self, dtype):
        t = [T(a).to(dtype) for a in (self.q, self.k, self.v)]
        hs = dict(hsk=0, hsv=0) if self.which == ar.KV else dict(hsk=self.hsk, hsv=self.hsv)
        return ar.attention(*t, B=self.B, heads=self.heads, dh=self.dh, nq=self.nq, nk=self.nk, scale=self.scale, kv_idx=self.kv_idx,
                            kv_rows=self.kv_rows, **hs)


RATIOS = {}


def hold(inst, case, y, ref64, ref32):
    """(a): y (numpy fp32) against the float64 restatement, bounded by the fp32 CPU evaluation's own error."""
    y = T(np.asarray(y))
    assert bool(torch.isfinite(y).all()), (inst, case, "a NaN or an infinity in the output")
    emax, erms = ar.errors(y, ref64)
    bmax, brms = ar.errors(ref32, ref64)
    ulp = ar.ulp_of_largest(ref64)
    mmax, mrms = MARGINS.get(inst, DEFAULT_MARGIN)
    rmax, rrms = emax / max(bmax, 1e-300), erms / max(brms, 1e-300)
    w = RATIOS.setdefault(inst, [0.0, 0.0])
    w[0], w[1] = max(w[0], rmax if emax > ulp else 0.0), max(w[1], rrms if brms > 0 or erms > 0 else 0.0)
    print(f"[attention] {inst:14s} {case:52s} max {emax:.3e} ({rmax:6.2f} x fp32 cpu) rms {erms:.3e} ({rrms:5.2f} x) ulp {ulp:.2e}   worst so far {w[0]:.2f} / {w[1]:.2f}")
    assert emax <= mmax * bmax + ulp and erms <= mrms * brms, (inst, case, (emax, erms), (bmax, brms), ulp)


# =================================================================================================== no GPU: the reference is what it claims
def _loops(q, k, v, B, heads, dh, nq, nk, scale, hsk, hsv, bk):
    out = torch.zeros((B, nq, heads * dh), dtype=q.dtype)
    for b in range(B):
        for h in range(heads):
            for i in range(nq):
                qi = q[b * nq + i, h * dh:(h + 1) * dh]
                s = torch.stack([scale * (qi * k[bk[b] * nk + j, h * hsk:h * hsk + dh]).sum() for j in range(nk)])
                w = torch.exp(s - s.max())
                w = w / w.sum()
                out[b, i, h * dh:(h + 1) * dh] = sum(w[j] * v[bk[b] * nk + j, h * hsv:h * hsv + dh] for j in range(nk))
    return out


def test_reference_is_the_formula_of_kernels_h():
    """attention_ref.attention against plain loops over (window, head, query, key) with explicit strides: wide rows, hsk != hsv, hsk = hsv =
    0, a clamped kv_idx."""
    g = torch.Generator().manual_seed(21)
    B, heads, dh, nq, nk = 3, 2, 8, 3, 5
    q = torch.randn((B * nq, heads * dh + 4), generator=g, dtype=torch.float64)
    for hsk, hsv, idx, rows in ((-1, -1, None, 0), (12, 16, None, 0), (0, 0, None, 0), (-1, 12, [-2, 9, 1], 4)):
        wins = rows or B
        k = torch.randn((wins * nk, 3 * dh + 12), generator=g, dtype=torch.float64)
        v = torch.randn((wins * nk, 3 * dh + 16), generator=g, dtype=torch.float64)
        got = ar.attention(q, k, v, B=B, heads=heads, dh=dh, nq=nq, nk=nk, scale=0.4, hsk=hsk, hsv=hsv, kv_idx=idx, kv_rows=rows)
        bk = list(range(B)) if idx is None else [min(max(x, 0), rows - 1) for x in idx]
        want = _loops(q, k, v, B, heads, dh, nq, nk, 0.4, dh if hsk < 0 else hsk, dh if hsv < 0 else hsv, bk)
        assert float((got - want).abs().max()) < 1e-14


def test_reference_is_scaled_dot_product_attention():
    g = torch.Generator().manual_seed(22)
    for B, heads, dh, nq, nk in ((2, 4, 64, 90, 181), (3, 2, 128, 33, 96), (1, 4, 256, 96, 1)):
        q = torch.randn((B * nq, heads * dh), generator=g, dtype=torch.float64)
        k = torch.randn((B * nk, heads * dh), generator=g, dtype=torch.float64) * 2
        v = torch.randn((B * nk, heads * dh), generator=g, dtype=torch.float64)
        got = ar.attention(q, k, v, B=B, heads=heads, dh=dh, nq=nq, nk=nk, scale=dh ** -0.5)
        sp = lambda x, n: x.reshape(B, n, heads, dh).permute(0, 2, 1, 3)      # noqa: E731
        want = F.scaled_dot_product_attention(sp(q, nq), sp(k, nk), sp(v, nk), scale=dh ** -0.5).permute(0, 2, 1, 3).reshape(B, nq, heads * dh)
        assert float((got - want).abs().max()) < 1e-13


def test_reference_is_multihead_attention_with_identity_projections():
    """The CVAE shape: head dim 64, 4 heads, 90 queries x 181 keys, against nn.MultiheadAttention whose projections are the identity."""
    g = torch.Generator().manual_seed(23)
    B, heads, dh, nq, nk = 2, 4, 64, 90, 181
    E = heads * dh
    mha = torch.nn.MultiheadAttention(E, heads, bias=True, batch_first=True, dtype=torch.float64)
    with torch.no_grad():
        mha.in_proj_weight.copy_(torch.eye(E, dtype=torch.float64).repeat(3, 1))
        mha.in_proj_bias.zero_()
        mha.out_proj.weight.copy_(torch.eye(E, dtype=torch.float64))
        mha.out_proj.bias.zero_()
    q = torch.randn((B, nq, E), generator=g, dtype=torch.float64)
    k = torch.randn((B, nk, E), generator=g, dtype=torch.float64)
    v = torch.randn((B, nk, E), generator=g, dtype=torch.float64)
    with torch.no_grad():
        want = mha(q, k, v, need_weights=False)[0]
    got = ar.attention(q.reshape(-1, E), k.reshape(-1, E), v.reshape(-1, E), B=B, heads=heads, dh=dh, nq=nq, nk=nk, scale=dh ** -0.5)
    assert float((got - want).abs().max()) < 1e-13


def test_reference_kv_idx_is_a_gather():
    g = torch.Generator().manual_seed(24)
    B, heads, dh, nq, nk, rows = 6, 2, 128, 7, 9, 4
    q = torch.randn((B * nq, heads * dh), generator=g, dtype=torch.float64)
    k = torch.randn((rows * nk, heads * dh), generator=g, dtype=torch.float64)
    v = torch.randn((rows * nk, heads * dh), generator=g, dtype=torch.float64)
    idx = np.array([-1, 4, 2, 2, 0, 3], dtype=np.int32)
    sel = torch.tensor([0, 3, 2, 2, 0, 3])
    kw = dict(B=B, heads=heads, dh=dh, nq=nq, nk=nk, scale=0.1)
    got = ar.attention(q, k, v, kv_idx=idx, kv_rows=rows, **kw)
    want = ar.attention(q, k.reshape(rows, nk, -1)[sel].reshape(B * nk, -1), v.reshape(rows, nk, -1)[sel].reshape(B * nk, -1), **kw)
    assert torch.equal(got, want)


def test_reference_kv_encode_inverts_kv_decode():
    r = rng("kv-encode")
    for n in (1, 31, 90, 96):
        K, V = normal(r, 2, n, 256) * 5, normal(r, 2, n, 256)
        img = ar.kv_encode(K, V)
        assert img.shape == (2, pr.KV_IMG_BYTES) and img.dtype == np.uint8
        k, v = pr.kv_decode(img)                                              # [B, 3, 96, 256]
        assert np.array_equal(k[:, :, :n], pr.plane_chain(K).transpose(1, 0, 2, 3)) and np.array_equal(v[:, :, :n], pr.plane_chain(V).transpose(1, 0, 2, 3))
        assert not k[:, :, n:].any() and not v[:, :, n:].any()
    assert np.array_equal(ar.kv_encode(K, V), img) and not np.array_equal(ar.kv_encode(V, K), img)


def test_probe_refuses_what_no_launcher_checks():
    """The probe's own sane() (host code; no GPU is touched)."""
    lib = ar.load()
    assert lib.at_kv_img_bytes() == pr.KV_IMG_BYTES
    one = 4096
    good = dict(q=one, k=one, v=one, out=one, kv=one, ldq=256, ldk=256, ldv=256, ldo=256, B=2, heads=2, dh=128, nq=9, nk=9, scale=0.1)

    def sane(which, **kw):
        return lib.at_sane(ar.make_params(**dict(good, **kw)), which)
    for which in (ar.F32, ar.X3, ar.KV):
        assert sane(which) == 0
        assert sane(which, nq=0) == 0 and sane(which, nk=500) == 0 and sane(which, dh=32) == 0 and sane(which, B=0) == 0      # the launchers' to refuse
        for bad in (dict(q=0), dict(out=0), dict(q=one + 4), dict(out=one + 8), dict(ldq=258), dict(ldo=254), dict(ldq=252), dict(ldo=128),
                    dict(scale=0.0), dict(scale=-1.0), dict(scale=float("inf")), dict(scale=float("nan")), dict(B=1 << 21), dict(heads=65)):
            assert sane(which, **bad) == ar.BAD_ARGUMENT, (which, bad)
    for which in (ar.F32, ar.X3):
        for bad in (dict(k=0), dict(v=0), dict(k=one + 4), dict(v=one + 12), dict(ldk=255), dict(ldv=130), dict(ldk=252), dict(ldv=128),
                    dict(heads=0), dict(heads=-1), dict(hsk=130), dict(hsv=6), dict(hsk=132), dict(hsv=132, ldv=256),
                    dict(kv_idx=one), dict(kv_idx=one, kv_rows=0)):
            assert sane(which, **bad) == ar.BAD_ARGUMENT, (which, bad)
        assert sane(which, hsk=0, hsv=0, ldk=128, ldv=128) == 0 and sane(which, hsk=132, ldk=260) == 0 and sane(which, kv_idx=one, kv_rows=1) == 0
    assert sane(ar.KV, kv=0) == ar.BAD_ARGUMENT and sane(ar.KV, kv=one + 8) == ar.BAD_ARGUMENT
    assert sane(ar.KV, heads=0) == 0 and sane(ar.KV, heads=3, ldq=384, ldo=384) == 0      # the kv launcher's to refuse
    assert sane(3) == ar.BAD_ARGUMENT


def test_cases_are_a_pairwise_cover():
    """Every instance is reached; per family every (nq, nk) of the issue's grid is there (the full-batch family: a band and the corners);
    every value of every other factor meets every nq, every nk and every value of every other factor."""
    assert {_inst(c) for c in CASES} == set(INSTANCES) == {_inst(reach(i)) for i in INSTANCES}
    assert all(_inst(reach(i)) == i for i in INSTANCES)
    pairs = {(c["nq"], c["nk"]) for c in CASES}
    assert set(MUST) | {(182, 182), (90, 181), (90, 90)} <= pairs
    fams = {}
    for c in CASES:
        fams.setdefault(c["fam"], []).append(c)
    grids = {"f32 small": (SMALL, SMALL), "f32 6x3": (SMALL, BIG), "f32 6x6": (BIG, SMALL + BIG), "x3 small": (SMALL, SMALL), "kv": (SMALL, SMALL)}
    for fam, (nqs, nks) in grids.items():
        assert {(c["nq"], c["nk"]) for c in fams[fam]} == {(a, b) for a in nqs for b in nks}, fam
    full = fams["x3 full"]
    assert {c["nq"] for c in full} == set(SMALL) == {c["nk"] for c in full} and set(MUST) <= {(c["nq"], c["nk"]) for c in full}
    assert all(c["B"] * c["heads"] > 256 for c in full) and {c["B"] for c in full} == {65, 257, 86, 129}
    for fam, cs in fams.items():
        assert not _uncovered(fam, cs), (fam, _uncovered(fam, cs))
    assert {_inst(c) for c in CASES if c["layout"] == "qkv"} == set(INSTANCES[:10]) - {"f32<64,6,3>"}      # (nq <= 96 < nk has no diagonal)
    assert {c["B"] for c in CASES} >= set(BS) and {c["heads"] for c in CASES if c["which"] != "kv"} == set(HEADS)


# =================================================================================================== GPU: (a) float64 parity, under (d)
@gpu
@pytest.mark.parametrize("c", CASES, ids=_id)
def test_parity(c):
    case = Case(c).to_device()
    y = case.launch()
    hold(_inst(c), _id(c), y, case.reference(torch.float64), case.reference(torch.float32))


@gpu
@pytest.mark.parametrize("inst", INSTANCES)
def test_zero_queries_give_the_mean_of_the_values(inst):
    c = reach(inst, regime="zeroq")
    case = Case(c).to_device()
    y = case.launch()
    ref64 = case.reference(torch.float64)
    v = T(case.v).double().reshape(case.B, case.nk, -1)
    mean = v.mean(1, keepdim=True)[:, :, :case.heads * case.dh] if case.which != ar.KV else v.mean(1, keepdim=True).repeat(1, 1, case.heads)
    assert float((ref64 - mean).abs().max()) < 1e-14
    hold(inst, _id(c), y, ref64, case.reference(torch.float32))


# =================================================================================================== GPU: (b) relations to the bit
@gpu
@pytest.mark.parametrize("inst", INSTANCES)
def test_two_runs_agree_and_windows_do_not_depend_on_the_batch(inst):
    """The same launch twice; a window alone (B = 1, pointers moved to it) and the first B - 1, B - 2 windows; a copy of a window at
    another place of the batch.  The full-batch instances stay full: 72 and 65 windows, copies at 0, 37 and 64."""
    c = reach(inst, layout="wide")
    case = Case(c)
    B, nq, nk = case.B, case.nq, case.nk
    src, places = (5, (0, B - 1)) if B == 9 else (37, (0, 64))
    qw, kw, vw = (a.reshape(B, -1, a.shape[1]) for a in (case.q, case.k, case.v))
    for pl in places:
        qw[pl], kw[pl], vw[pl] = qw[src], kw[src], vw[src]
    case.to_device()
    y = case.launch()
    assert same_bits(y, case.launch()), (inst, "two runs differ")
    for pl in places:
        assert same_bits(y[pl], y[src]), (inst, "a window's bits depend on its place", pl)
    if B == 9:
        for n in (8, 7):                                                      # 8: a full group of the grid; 7: one workgroup per head returns early
            assert same_bits(case.launch(B=n), y[:n]), (inst, "B", n)
        step = [4 * src * nq * case.lds[0], 4 * src * nk * case.lds[1], 4 * src * nk * case.lds[2]]
        over = dict(q=case.ptrs[0] + step[0], k=case.ptrs[1] + step[1], v=case.ptrs[2] + step[2])
        if case.which == ar.KV:
            over["kv"] = ar.ptr(case.d_img) + src * pr.KV_IMG_BYTES
        assert same_bits(case.launch(B=1, **over)[0], y[src]), (inst, "a window alone")
    else:
        big = Case(dict(c, B=72))
        for a, b in zip(big.base, case.base):
            a[:b.shape[0]] = b
        big.to_device()
        assert same_bits(big.launch()[:B], y), (inst, "B 72 / 65")


@gpu
@pytest.mark.parametrize("dh", (128, 256))
def test_x3_prefetch_depth_and_reverse(dh):
    """x3<DH,true> (B heads <= 256) and x3<DH,false> (> 256) give a window the same bits: the first nine and the windows 40 .. 48 of a
    65-window batch launched on their own.  reverse = 1 changes nothing in either; 257 windows x 1 head the same."""
    for B, heads in ((65, 4), (257, 1)):
        c = reach(f"x3<{dh},false>", B=B, heads=heads, nq=90, nk=33, layout="hs", regime="peaked")
        case = Case(c).to_device()
        assert _inst(c) == f"x3<{dh},false>"
        y = case.launch()
        assert same_bits(case.launch(reverse=1), y), (dh, B, "reverse, full batch")
        for first in (0, 40):
            over = dict(q=case.ptrs[0] + 4 * first * case.nq * case.lds[0], k=case.ptrs[1] + 4 * first * case.nk * case.lds[1],
                        v=case.ptrs[2] + 4 * first * case.nk * case.lds[2])
            assert _inst(dict(c, B=9)) == f"x3<{dh},true>"
            ys = case.launch(B=9, **over)
            assert same_bits(ys, y[first:first + 9]), (dh, B, first, "PF2 true / false")
            assert same_bits(case.launch(B=9, reverse=1, **over), ys), (dh, B, first, "reverse, small batch")


@gpu
@pytest.mark.parametrize("inst", ("x3<128,true>", "x3<128,false>", "x3<256,true>", "x3<256,false>", "x3 split<256>"))
def test_kv_idx_is_the_materialised_gather(inst):
    c = reach(inst, layout="idx", nq=90, nk=65)
    case = Case(c).to_device()
    y = case.launch()
    sel = np.clip(case.kv_idx, 0, case.kv_rows - 1)
    flat = Case(dict(c, layout="sep"))
    flat.q[:] = case.q
    flat.k[:] = case.k.reshape(case.kv_rows, case.nk, -1)[sel].reshape(flat.k.shape)
    flat.v[:] = case.v.reshape(case.kv_rows, case.nk, -1)[sel].reshape(flat.v.shape)
    assert same_bits(flat.to_device().launch(), y), inst
    # one index for every window, at both ends of the clamp
    for i, row in ((-5, 0), (99, case.kv_rows - 1)):
        case.d_idx = D(np.full(case.B, i, dtype=np.int32))
        flat.k[:] = np.tile(case.k.reshape(case.kv_rows, case.nk, -1)[row], (case.B, 1))
        flat.v[:] = np.tile(case.v.reshape(case.kv_rows, case.nk, -1)[row], (case.B, 1))
        assert same_bits(flat.to_device().launch(), case.launch()), (inst, i)


@gpu
@pytest.mark.parametrize("inst", INSTANCES[:10])
def test_shared_rows_are_the_replicated_rows(inst):
    """hsk = hsv = 0 with ldk = ldv = dh (the folded decoder) against the same rows once per head at stride dh."""
    c = reach(inst, layout="shared", regime="peaked")
    case = Case(c).to_device()
    rep = Case(dict(c, layout="sep"))
    rep.q[:] = case.q
    rep.k[:] = np.tile(case.k, (1, case.heads))
    rep.v[:] = np.tile(case.v, (1, case.heads))
    assert same_bits(rep.to_device().launch(), case.launch()), inst


@gpu
@pytest.mark.parametrize("heads", (4, 8))
def test_kv_head_quads_and_head_pairs_agree(heads):
    """kv<256,4> and kv<256,2> (pairs = 1) add the same products to every score and output in the same order (attention_kv.hip: per key
    tile the k steps and, inside one, the six plane pairs, whichever of the two loops is outside): the same bits.  And both against the
    three-wave x3 kernel on the fp32 rows by (a) alone, in test_parity."""
    for nq, nk, reg in ((90, 90, "normal"), (33, 31, "peaked"), (96, 1, "tie"), (1, 96, "normal")):
        c = reach("kv<256,4>", heads=heads, nq=nq, nk=nk, regime=reg, layout="wide")
        case = Case(c).to_device()
        assert _inst(c) == "kv<256,4>" and _inst(dict(c, pairs=1)) == "kv<256,2>"
        assert same_bits(case.launch(pairs=1), case.launch()), (heads, nq, nk)


# =================================================================================================== GPU: (c) isolation
@gpu
@pytest.mark.parametrize("inst", INSTANCES)
def test_a_window_reads_only_its_own_rows(inst):
    """Every other window's q, k and v rows (for kv: its whole image) NaN: the chosen window - the first, one inside, the last - keeps its
    bits.  nq < 96 and nk < 96 (192): a padded row read across the window's end would leak through 0 * NaN."""
    small = {"f32<64,6,3>": dict(nq=33, nk=130), "f32<64,6,6>": dict(nq=100, nk=130)}.get(inst, dict(nq=33, nk=31))
    c = reach(inst, layout="wide", **small)
    case = Case(c).to_device()
    y = case.launch()
    B = case.B
    for w in (0, B // 2, B - 1):
        nan = Case(c)
        for a in nan.base:
            win = a.reshape(B, -1, a.shape[1])
            keep = win[w].copy()
            win[:] = np.nan
            win[w] = keep
        img = None
        if nan.which == ar.KV:                                                # the image: every bf16 of the other windows a NaN (no zero rows either)
            img = np.full((B, pr.KV_IMG_BYTES // 2), 0x7FC0, dtype=np.uint16)
            img[w] = ar.kv_encode(case.k.reshape(B, case.nk, 256)[w:w + 1], case.v.reshape(B, case.nk, 256)[w:w + 1]).view(np.uint16)[0]
            img = img.view(np.uint8)
        nan.to_device(img)
        yn = nan.launch()
        assert same_bits(yn[w], y[w]), (inst, w, "a window's output depends on its neighbours' rows")
        assert np.isnan(np.delete(yn, w, 0)).all()


# =================================================================================================== GPU: (d) refusals
@gpu
def test_refusals():
    bad = ar.INVALID_VALUE
    f = lambda inst, **kw: Case(reach(inst, B=2, **kw)).to_device()           # noqa: E731
    for nq, nk in ((0, 9), (9, 0), (193, 9), (9, 193)):
        case = f("f32<64,3,3>")
        case.launch(expect=bad, nq=nq, nk=nk)
    for inst in ("x3<128,true>", "x3 split<256>", "kv<256,4>", "kv<256,2>"):
        for nq, nk in ((0, 9), (9, 0), (97, 9), (9, 97)):
            f(inst).launch(expect=bad, nq=nq, nk=nk)
    f("f32<64,3,3>").launch(expect=bad, dh=32)
    f("f32<128,3,3>").launch(expect=bad, nk=97)                              # the six-tile instances are head dim 64 only
    f("f32<128,3,3>").launch(expect=bad, nq=97)
    f("x3<128,true>", heads=1).launch(expect=bad, dh=64)
    f("kv<256,4>", heads=2).launch(expect=bad, dh=128)
    f("kv<256,4>").launch(expect=bad, heads=3)
    f("kv<256,4>").launch(expect=bad, heads=0)
    for inst in ("f32<256,3,3>", "f32<64,6,6>"):                             # launch_attention has no gathered form: refused, not ignored
        case = f(inst)
        case.launch(expect=bad, kv_idx=ar.ptr(D(np.zeros(2, dtype=np.int32))), kv_rows=2)
    for inst in INSTANCES:                                                    # no windows: success, nothing written
        case = Case(reach(inst)).to_device()
        out = case.new_out(0)
        assert ar.load().at_attention(case.params(out.ptr, B=0), case.which, 0) == 0 and out.intact(), inst
