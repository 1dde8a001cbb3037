"""Every GEMM instance of the library against float64 at the kernel boundary: gathers, epilogues, tile edges (GPU cases: -m gpu).

The GEMM is a family of kernels and batch size alone chooses among them (launch_gemm: mocha_gemm_skinny16 / mocha_gemm_skinny /
mocha_gemm_f32<64,2,2,1,1> / <64,4,1,1,2> / <128,2,2,2,2>; launch_gemm_x3: 64 x 64, 64 x 128, 128 x 64, 128 x 128 tiles and the persistent
mocha_gemm_x3p with three epilogue instances; gemm_h2.hip's four tiles; gemm_x3r.hip's three epilogue instances).  Each of them carries its
own copy of the temporal-conv gather and of the epilogue.  Here every instance is launched directly (tests/gemm_probe) with every gather
configuration and epilogue the network uses, at the smallest whole number of windows that reaches it and one window more, and held to

  (a) a float64 CPU reference built from what the operation means (tests/gemm_probe/__init__.py: the gather restated once in numpy
      integer arithmetic from the formula in csrc/kernels.h; test_reference_gather_is_the_convolution_it_stands_for pins that restatement
      to torch's own reflect-pad / upsample / conv / AvgPool, without a GPU).  Bound: the error of the SAME operation evaluated in fp32 by
      torch on the CPU against that float64 result (in torch's own summation order and as one k-ordered chain, the larger: see below),
      times MARGIN_MAX on the largest and MARGIN_RMS on the rms error, plus one fp32 ulp of the largest output on the largest error.  Inputs are unit normal, weights scaled by 1 / sqrt(K): a wrong source row, a wrong
      rowbias row or a wrong tap is an O(1) error - five to six orders above the bound - so the outcome does not hang on the margin.
      The two-plane fp16 engine keeps the bound tests/test_gemm_f16x2.py asserts for plain rows: no worse than the exact-f32 kernels on
      the same case (1.02 x rms, 1.5 x max, + 1e-9).
  (b) untouched memory: C has sentinel rows after M and sentinel columns from N to ldc (the split upsample conv's second half: also the
      128 columns in front of its offset; raw K-split slabs: guard rows between the slabs) - bit-intact afterwards.
  (c) bit identity: persistent on / off (all three of its epilogue instances, gathered cases included) and x3r against x3 - and both
      again with so few workgroups (64 persistent, 8 of x3r) that each walks several tiles / panels: with the defaults every case here
      has fewer tiles than workgroups, and the code that sets those schedules apart would not run (VARIANTS).
  (e) the fp16 engine's c_amax vector: per window exactly the largest magnitude stored.
  (d) the instance: each case asserts, from the exported selection predicates, the kernel it reached - and that an engine that must
      refuse the case (R = 4 on the plane engines, rowbias on x3r, a handful of windows on every plane engine) does refuse it.

GEMM sites of the network (mocha_api.cpp) -> case family here, and the instance each takes at 1 / 8 / 128 / 585 windows with the
library's defaults (plane engine on where it supports the launch, else the exact-f32 kernels) - asserted by test_site_instances:

  site                 family (parameters)                                    1          8          128          585
  emb.joint_block      n256 K 960, rowbias mod 6                              skinny16   skinny16   x3<64x128>   x3p<2>
  emb.gcn_joint        gcn_joint: 360 rows / window, K 192, rowbias mod 6     skinny16   skinny     x3p<2>       x3p<2>
  emb.tcn_joint_pool   n256 K 1280, bias (and as one launch: G4)              skinny16   skinny16   x3<64x128>   x3p<0>
  emb.gcn_body         n256 K 512, rowbias mod 6                              skinny16   skinny16   x3<64x128>   x3p<2>
  emb.tcn_body         G1, bias (+ rowbias mod 90)                            skinny16   skinny16   x3<64x128>   x3p<0> / x3p<2>
  enc.qkv              n1536 K 256, none                                      skinny16   x3<64x128> x3<128x128>  x3<128x128>
  xf.out_proj (enc)    n256 K 512, bias + residual                            skinny16   skinny16   x3<64x128>   x3p<1>
  xf.ff1               n512 K 256, bias + GELU                                skinny16   skinny16   x3<64x128>   x3p<0>
  xf.ff2               n256 K 512, bias + residual                            skinny16   skinny16   x3<64x128>   x3p<1>
  dec.q                n1024 K 256, none                                      skinny16   x3<64x128> x3<128x128>  x3<128x128>
  xf.out_proj (dec)    n256 K 1024, bias + residual                           skinny16   skinny16   x3<64x128>   x3p<1>
  dec.style1           style1: M = windows, N 1024, K 256, bias + LeakyReLU   skinny16   skinny16   skinny16     skinny16
  dec.style2           style2: N 1024, K 1024, bias (<= 192 windows)          skinny16   skinny16   skinny16     -
  dec.style2 per layer style2l: N 512, K 512, lda = ldc = 1024 (> 192)        -          -          -            skinny16
  mot.gcn_body         n256 K 512, rowbias mod 6                              skinny16   skinny16   x3<64x128>   x3p<2>
  mot.tcn_body         G1, bias                                               skinny16   skinny16   x3<64x128>   x3p<0>
  mot.gcn_joint        n192 K 256, a_lrelu + bias                             skinny16   skinny16   x3<64x64>    x3<128x64>
  mot.tcn_joint        G2 (V 22 / 24), bias; from 256 windows G2a + G2b       skinny16   skinny     x3p<0>       x3p<0> (both halves)
  mot.tcn_joint unfolded  G3, bias                                            skinny     skinny     x3<128x64>   x3<128x64>
  CVAE linear1 / in_proj  n512 K 256 bias + ReLU / n768 K 256 bias            (the f32 / x3 tiers of those families)

The fp32 reference error and its summation order.  torch's fp32 GEMM on the CPU is a BLAS that sums K in an order of its own choosing, and
that choice decides its error: measured on the CPU alone (no kernel involved; unit-normal data as here, M = 90, N = 256), its rms error
against float64 equals that of ONE k-ordered chain per element to 1 % for K <= 384 (K 128 / 256 / 320: 2.02 / 2.88 / 3.20e-7 both ways), and
from K = 512 on it stays near 2.9e-7 - K is cut into blocks there - while the chain's goes on as 1.8e-8 sqrt(K), which is what fp32
rounding of a running sum predicts (2^-23 sqrt(0.54 / 12) sqrt(K / 2)): chain / BLAS = 1.4, 2.0, 3.9 x rms and 1.8, 3.3, 7.4 x max at
K = 512, 1280, 4096, and the BLAS figure moves with M as well (the 4-frame mean, K 1280: 1.9 x at 90 rows, 3.3 x at 180).  The exact-f32 kernels ARE one
k-ordered chain per element (v_mfma_f32_32x32x2_f32, gemm_f32.hip), so at K = 1280 a correct kernel sits 2.5 x above the BLAS rms error
(G4, 90 rows: 3.27e-7 against 1.32e-7) and no constant margin on the BLAS figure alone is right for every K.  The bound therefore takes the
fp32 CPU error in both orders - torch's GEMM on all rows, and torch fp32 accumulating the K products in k order (gemm_probe._matmul) on
CHAIN_ROWS evenly spaced rows - and uses the larger, per statistic.  For K <= 384 that changes nothing.  Both are the reference's own
error; neither comes from a kernel.  The chain counts only for kernels that keep one fp32 accumulator per output element over the whole
of K: the exact-f32 tiles and every tile of the plane engines (one MFMA accumulator over all K steps; at K = 1280 / 4096 they sit 2.2 /
3.7 x above the BLAS rms figure, as the chain does).  skinny16 and skinny cut K four ways (chains of at most 320 products here, shorter
than the BLAS's blocks) and are held to the BLAS figure alone.

Margins.  MARGIN_MAX = 4 and MARGIN_RMS = 2 were the starting values.  Measured on an MI355X (all 317 cases, 1 096 launches; ratio = kernel
error / fp32 CPU error as above; every case prints its own with -s), worst per instance, max / rms:
  skinny16 0.99 / 0.94   skinny 1.32 / 1.29   f32<64,2,2,1,1> 2.17 / 1.01   f32<64,4,1,1,2> 1.75 / 1.01   f32<128,2,2,2,2> 1.23 / 1.01
  x3<64x64> 1.31 / 0.86  x3<64x128> 1.31 / 0.86  x3<128x64> 1.36 / 0.85  x3<128x128> 1.62 / 0.88  x3p<0> 1.62 / 0.86  x3p<1> 1.61 / 0.88
  x3p<2> 1.50 / 0.86     x3r<-1> 1.31 / 0.84  x3r<0> 1.37 / 0.85  x3r<1> 1.15 / 0.80
  h2<64x64> 0.88 / 0.68  h2<64x128> 1.05 / 0.72  h2<128x64> 1.09 / 0.68  h2<128x128> 0.94 / 0.72  (h2 is asserted against the f32 kernels)
The rms ratio never exceeds 1.01 where the chain counts - the exact-f32 tiles reproduce the chain's rms to 1 %, the plane engines are below
it - and 1.29 for the four-way K split against the BLAS figure alone (K = 1280: four chains of 320 against the BLAS's blocks), so
MARGIN_RMS is tightened to 1.5 (the factor tests/test_gemm_engines.py allows between two engines; what is left covers a
fused against an unfused multiply-add in the chain and a BLAS that blocks K elsewhere on another CPU).  The largest error is the extreme
of 10^4 - 10^7 samples and scatters accordingly (up to 2.17); MARGIN_MAX stays 4.
Two mutations, on a scratch copy (never committed).  The upper reflect of mocha_gemm_x3p as 2 * T_full - 1 - tf: fails all twelve epilogues
of G1 at 273 windows and bias / bias_rb90 at 272 (x3p<0>, <1>, <2>; O(1) errors); G2 / G2a / G2b / G3 cannot see it - with tshift = 2
the upsampled frames 56 - 59 are all source frame 14, so their cases are no protection against an off-by-one at the upper reflect, only
G1's are; tests/test_hip_parity.py passes.  rowbias[row % (rb_mod + 1)] in mocha_gemm_skinny: fails every rowbias case of the skinny tier
(n256 K 256 / 512 / 960 with rb6, rb90, bias_rb90, rb6_res; G1; G2/24 rb6_res; gcn_joint; M = 799 / 801); test_hip_parity.py fails
test_characterize_vs_oracle[33-16] and test_fused_pose_normalisation.
Run time on the GPU box: 36 - 42 s for the file (317 cases; the slowest case 0.8 s), CPU references on 16 threads included.
"""
import os
import sys
import zlib

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gemm_probe as gp  # noqa: E402

MARGIN_MAX, MARGIN_RMS = 4.0, 1.5
SENTINEL = 0x7FC0DEAD      # as int32: a quiet NaN with a payload no kernel produces
GUARD_ROWS, GUARD_COLS = 8, 16
CHAIN_ROWS = 512           # rows (evenly spaced, first and last included) on which the fp32 reference is also summed as one k-ordered chain

# ------------------------------------------------------------------------------------------------ gather configurations (mocha_api.cpp)
G1 = dict(T_out=15, V=6, ntaps=3, pad=1, stride=1, R=1, T_full=15, tshift=0, Cc=256, T_src=15, tstep=1)


def G2(V):
    return dict(T_out=15, V=V, ntaps=3, pad=2, stride=4, tstep=4, R=1, T_full=60, tshift=2, Cc=64, T_src=15)


def G2a(V):
    return dict(G2(V), ntaps=2)


def G2b(V):
    return dict(G2(V), ntaps=2, pad=-2)


def G3(V):
    return dict(T_out=60, V=V, ntaps=5, pad=2, stride=1, R=1, T_full=60, tshift=2, Cc=64, T_src=15, tstep=1)


G4 = dict(T_out=15, V=6, ntaps=5, pad=2, stride=4, R=4, T_full=60, tshift=0, Cc=256, T_src=60, tstep=1, ascale=0.25)

# ------------------------------------------------------------------------------------------------ epilogues
EPILOGUES = {
    "none": {}, "bias": dict(bias=1), "rb6": dict(rb=6), "rb90": dict(rb=90), "bias_gelu": dict(bias=1, act=1), "bias_lrelu": dict(bias=1, act=2),
    "bias_relu": dict(bias=1, act=3), "bias_res": dict(bias=1, res=1), "alrelu_bias": dict(bias=1, a_lrelu=1), "bias_rb90": dict(bias=1, rb=90),
    "rb6_res": dict(rb=6, res=1), "alrelu": dict(a_lrelu=1),
}

# ------------------------------------------------------------------------------------------------ families and the windows that reach each tier
# tier = the exact-f32 launcher's INSTANCE (the constants are named after the rows of its tile, 16 / 32 / 64 / 128; they are instance names,
# not heights); the plane engines' tiles follow it (T64 -> 64-row tiles, T128 -> 128-row tiles / persistent).  T128 is the 128 x 64 tile
# f32<64,4,1,1,2>.  The 128 x 128 tile f32<128,2,2,2,2> is a further instance that no window count of the network's launches reaches
# (the launcher keeps it for K >= 4096 and the matcher's raw slabs; no gather has such a K): it is named in full where it is meant,
# and gets plain rows with bias + residual and raw slabs only.
T16, T32, T64, T128 = "skinny16", "skinny", "f32<64,2,2,1,1>", "f32<64,4,1,1,2>"
FAMILIES = {
    # name: rows per window, N, K, gather, {tier: (smallest windows, one more)}
    "n256": dict(rpw=90, N=256, K=256, tiers={T16: (1, 2), T32: (9, 10), T64: (33, 34), T128: (272, 273)}),
    "G1": dict(rpw=90, N=256, K=768, g=G1, tiers={T16: (1, 2), T32: (9, 10), T64: (33, 34), T128: (272, 273)}),
    "gcn_joint": dict(rpw=360, N=256, K=192, tiers={T16: (1, 2), T32: (3, 4), T64: (9, 10), T128: (68, 69)}),
    "n512": dict(rpw=90, N=512, K=256, tiers={T16: (1, 2), T32: (9, 10), T64: (16, 17), T128: (136, 137)}),
    "n768": dict(rpw=90, N=768, K=256, tiers={T16: (1, 2), T32: (9,), T64: (10, 11), T128: (90, 91)}),
    "n1024": dict(rpw=90, N=1024, K=256, tiers={T16: (1, 2), T64: (8, 9), T128: (67, 68)}),
    "n1536": dict(rpw=90, N=1536, K=256, tiers={T16: (1, 2), T64: (5, 6), T128: (45, 46)}),
    "n192": dict(rpw=90, N=192, K=256, tiers={T16: (1, 2), T32: (9, 10), T64: (45, 46), T128: (363, 364)}),
    "style1": dict(rpw=1, N=1024, K=256, tiers={T16: (1, 2), T64: (641, 642), T128: (6017, 6018)}),
    "style2": dict(rpw=1, N=1024, K=1024, tiers={T16: (1, 2), T32: (193, 194), T64: (641, 642)}),
    "style2l": dict(rpw=1, N=512, K=512, lda=1024, ldc=1024, tiers={T16: (1, 2), T32: (769, 770), T64: (1409, 1410), T128: (12161, 12162)}),
    "G2/22": dict(rpw=330, N=256, K=192, g=G2(22), tiers={T16: (1, 2), T32: (3, 4), T64: (9, 10), T128: (75, 76)}),
    "G2/24": dict(rpw=360, N=256, K=192, g=G2(24), tiers={T16: (1, 2), T32: (3, 4), T64: (9, 10), T128: (68, 69)}),
    "G2a/22": dict(rpw=330, N=128, K=128, g=G2a(22), ldc=256, tiers={T16: (1, 2), T32: (3, 4), T64: (19, 20), T128: (149, 150)}),
    "G2b/22": dict(rpw=330, N=128, K=128, g=G2b(22), ldc=256, coff=128, tiers={T16: (1, 2), T32: (3, 4), T64: (19, 20), T128: (149, 150)}),
    "G2b/24": dict(rpw=360, N=128, K=128, g=G2b(24), ldc=256, coff=128, tiers={T16: (1, 2), T32: (3, 4), T64: (17, 18), T128: (137, 138)}),
    "G3/22": dict(rpw=1320, N=64, K=320, g=G3(22), tiers={T32: (1, 2), T64: (10, 11), T128: (75, 76)}),
    "G4": dict(rpw=90, N=256, K=1280, g=G4, tiers={T64: (1, 2), T128: (272, 273)}),
}
ALL_TIERS = (T16, T32, T64, T128)


def _problem(fam, windows, epi, tier, **over):
    f = FAMILIES[fam]
    d = dict(fam=fam, M=windows * f["rpw"], rpw=f["rpw"], N=f["N"], K=f["K"], g=f.get("g"), epi=epi, tier=tier,
             lda=f.get("lda"), ldc=f.get("ldc"), coff=f.get("coff", 0), ksplit=1, wsub=0)
    d.update(over)
    d["name"] = (f"{fam}-K{d['K']}-{epi}-" + (f"w{windows}" if windows else f"M{d['M']}") + (f"-ks{d['ksplit']}" if d["ksplit"] > 1 else "")
                 + ("-wsub" if d["wsub"] else ""))
    return d


def _problems():
    out = []

    def add(fam, epis, which=(0, 1), tiers=ALL_TIERS, **over):
        for tier in tiers:
            ws = FAMILIES[fam]["tiers"].get(tier)
            if not ws:
                continue
            for i in which:
                if i < len(ws):
                    for e in epis:
                        out.append(_problem(fam, ws[i], e, tier, **over))

    # every epilogue on plain rows at the smallest window count of every instance; none / bias again one window more
    add("n256", list(EPILOGUES), which=(0,))
    add("n256", ["none", "bias"], which=(1,))
    # the body tcn gather with every epilogue one window past the threshold; its two site epilogues at the threshold
    add("G1", list(EPILOGUES), which=(1,))
    add("G1", ["bias", "bias_rb90"], which=(0,))
    # the other gather configurations as the network launches them, both window counts
    for fam in ("G2/22", "G2/24", "G2a/22", "G2b/22", "G2b/24", "G3/22", "G4"):
        add(fam, ["bias"])
    add("G2/24", ["none", "rb6_res"], which=(0,), tiers=(T16, T32, T64, T128))
    add("G3/22", ["alrelu", "bias_res"], which=(1,))
    # the network's plain-row sites with their own K / N / epilogue
    add("n256", ["rb6"], which=(0,), K=960)
    add("n256", ["bias"], which=(0,), K=1280)
    add("n256", ["rb6", "bias_res"], which=(1,), K=512)
    add("n256", ["bias_res"], which=(0,), K=1024)
    add("gcn_joint", ["rb6"])
    add("n512", ["bias_gelu", "bias_relu"])
    add("n768", ["bias"])
    add("n1024", ["none"])
    add("n1536", ["none"])
    add("n192", ["alrelu_bias"])
    add("n192", ["none", "rb90", "bias_res", "bias_gelu"], which=(0,), tiers=(T64, T128))
    add("style1", ["bias_lrelu"])
    add("style2", ["bias"])
    add("style2l", ["bias"], which=(0,))
    # plain rows at tile height - 1 / + 1 of every instance (M is given directly; `tier` still names the exact-f32 instance)
    for tier, h, k in ((T16, 16, 1), (T16, 16, 12), (T32, 32, 25), (T64, 64, 47), (T128, 128, 192)):
        for dm in (-1, 1):
            for e in ("bias_res", "rb6"):
                out.append(_problem("n256", 0, e, tier, M=h * k + dm))
    for dm in (-1, 1):                                                  # N = 192: the 64-wide tiles (64 x 64, 128 x 64)
        out.append(_problem("n192", 0, "alrelu_bias", T64, M=64 * 64 + dm))
        out.append(_problem("n192", 0, "alrelu_bias", T128, M=128 * 256 + dm))
        out.append(_problem("n512", 0, "bias_gelu", T64, M=128 * 65 + dm))     # x3r: a ragged last panel
        out.append(_problem("n512", 0, "none", T64, M=128 * 65 + dm))
    # the register-resident instance's three epilogues at the first whole number of windows it takes (8192 rows) and one more; a wider launch
    for w in (92, 93):
        for e in ("none", "bias", "bias_gelu"):
            out.append(_problem("n512", w, e, T64))
    out.append(_problem("n1536", 92, "bias", T128))
    # raw K-split slabs (the matcher's launch shape): no epilogue, slab z = the partial sum over its K range
    for ks in (2, 4):
        out.append(_problem("n256", 0, "none", "f32<64,4,1,1,2>", M=257, K=512, ksplit=ks))
        out.append(_problem("n512", 0, "none", "f32<128,2,2,2,2>", M=8000 // ks, K=4096, ksplit=ks))      # 256 wide tiles: one per CU either way
        out.append(_problem("n192", 0, "none", "f32<64,4,1,1,2>", M=129, K=512, ksplit=ks))
        # ... with the centred bank: a K vector subtracted from every W row as it is staged (exact-f32 kernels only; the plane engines
        # take the vector when the image is packed and refuse it in a launch)
        out.append(_problem("n256", 0, "none", "f32<64,4,1,1,2>", M=257, K=512, ksplit=ks, wsub=1))
        out.append(_problem("n512", 0, "none", "f32<128,2,2,2,2>", M=8000 // ks, K=4096, ksplit=ks, wsub=1))
    # the 128 x 128 exact-f32 tile with an epilogue: long K (the launcher keeps the wide tile from K = 4096), more tiles than mid-size launches have
    out.append(_problem("n512", 0, "bias_res", "f32<128,2,2,2,2>", M=128 * 96 + 1, K=4096))
    seen = {}
    for p in out:
        seen.setdefault(p["name"], p)
    return list(seen.values())


PROBLEMS = _problems()
# engine variants: the x3 launcher with the library's defaults, with 64 x 64 tiles forced on 128-multiples, and with the persistent instance off
# ... with 64 instead of 768 persistent workgroups, and with 8 instead of 256 workgroups of the register-resident instance.  With the defaults no
# case here has more tiles than workgroups (at most 416 tiles of 128 x 128; 65 - 192 panels), so every workgroup would take ONE tile and
# the code that sets these schedules apart - the K loop crossing into the next tile, the epilogue running over the next tile's loads, the
# skipped padded tiles, x3r's whole panels and the carry from one unit to the next - would not run.  64 workgroups walk 6 - 7 tiles each;
# 8 take 8 - 24 whole panels each, then a share of the rest.  Both run only on the cases that reach those instances (RESCHEDULED).
VARIANTS = {"f32": ("f32", {}), "x3": ("x3", {}), "x3/t64": ("x3", dict(tile64_below=1 << 30)), "x3/nop": ("x3", dict(persistent=0)),
            "x3/p64": ("x3", dict(persistent=64)), "h2": ("h2", {}), "x3r": ("x3r", {}), "x3r/g8": ("x3r", dict(x3r_grid=8))}
RESCHEDULED = {"x3/p64": "x3p", "x3r/g8": "x3r"}      # variant -> the instances it re-schedules; other cases would repeat "x3" / "x3r" launch for launch
# kernels that keep ONE fp32 accumulator per output element over the whole of K (the exact-f32 tiles: an fmaf chain; every plane tile: one
# MFMA accumulator over the K steps) - the others (skinny16, skinny) cut K four ways, into chains of at most 320 products here
ONE_ACCUMULATOR = ("f32<", "x3", "h2<")


def walk(variant, pr):
    """(units of work, workgroups) of a re-scheduled launch, as its launcher counts them: 128 x 128 tiles of the XCD-padded tile order
    against the persistent workgroups; 128-row panels against x3r's workgroups."""
    m_tiles = (pr["M"] + 127) // 128
    if variant == "x3/p64":
        return (m_tiles if m_tiles < 8 else (m_tiles + 7) // 8 * 8) * (pr["N"] // 128), 64
    return m_tiles, 8


def expected_instance(variant, pr):
    """The instance the case is MEANT to reach (None = the engine must refuse it), from the case's declared tier."""
    tier, N, e, g = pr["tier"], pr["N"], EPILOGUES[pr["epi"]], pr["g"]
    raw = pr["ksplit"] > 1
    engine = VARIANTS[variant][0]
    if engine == "f32":
        return tier
    if pr["wsub"]:
        return None                                                            # the centred bank's vector: exact-f32 kernels only
    big = tier in ("f32<64,4,1,1,2>", "f32<128,2,2,2,2>")
    if engine == "x3r":
        ok = (g is None and not raw and pr["K"] == 256 and N % 256 == 0 and not e.get("res") and not e.get("rb")
              and e.get("act", 0) <= 1 and (e.get("bias") or not e.get("act")) and pr["M"] >= 8192)
        return ("x3r<%d>" % (1 if e.get("act") else 0 if e.get("bias") else -1)) if ok else None
    if raw:
        return "x3<128x128>" if engine == "x3" else None                       # h2 takes no K split
    if tier in (T16, T32) or (g is not None and g["R"] != 1):
        return None                                                            # a handful of windows; the 4-frame mean
    odd = N % 128 != 0
    if engine == "h2":
        return ("h2<128x64>" if big else "h2<64x64>") if odd else ("h2<128x128>" if big else "h2<64x128>")
    if odd:
        return "x3<128x64>" if big else "x3<64x64>"
    if not big:
        return "x3<64x64>" if variant == "x3/t64" else "x3<64x128>"
    if variant == "x3/nop" or N > 512:
        return "x3<128x128>"
    return "x3p<%d>" % (1 if e.get("res") else 2 if e.get("rb") else 0)


# ------------------------------------------------------------------------------------------------ no GPU: the reference is what it claims to be
def _conv_weights(N, C, taps, gen):
    return torch.randn((N, C, taps), generator=gen, dtype=torch.float64)


def test_reference_gather_is_the_convolution_it_stands_for():
    """The numpy restatement of the gather (gemm_probe.gather_rows) against the torch float64 ops it replaces, to 1e-12:
    3 taps = reflect pad 1 + conv over 15 frames; 5 taps with tshift 2 = repeat_interleave(4) + reflect pad 2 + conv over 60 frames;
    R 4 / stride 4 / ascale 0.25 = the 5-tap conv followed by AvgPool over 4 frames; the stride-4 / tstep-4 form with folded weights
    (one output row per source frame, 4 phases x 64 columns) and its two 2-tap halves = that same 5-tap result."""
    gen = torch.Generator().manual_seed(3)
    B = 3

    def as_rows(x):                  # (B, C, T, V) -> rows (b, t, v) x C
        return x.permute(0, 2, 3, 1).reshape(-1, x.shape[1])

    def gemm(src_rows, M, g, Wk):    # Wk [N][taps][C] flattened k = tap * C + c
        return gp.reference(src_rows, Wk.reshape(Wk.shape[0], -1), M, Wk.shape[0], Wk.shape[1] * Wk.shape[2], g=g)

    # G1: 3 taps over 15 frames
    V, C, N = 6, 256, 32
    x = torch.randn((B, C, 15, V), generator=gen, dtype=torch.float64)
    w = _conv_weights(N, C, 3, gen)
    ref = F.conv2d(F.pad(x, (0, 0, 1, 1), mode="reflect"), w.unsqueeze(-1))
    got = gemm(as_rows(x), B * 15 * V, G1, w.permute(0, 2, 1))
    assert float((got - as_rows(ref)).abs().max()) < 1e-12
    # G3: 5 taps over the x4 nearest-upsampled frames, read through t >> 2
    V, C, N = 22, 64, 64
    y = torch.randn((B, C, 15, V), generator=gen, dtype=torch.float64)
    w5 = _conv_weights(N, C, 5, gen)
    up = y.repeat_interleave(4, dim=2)
    ref5 = F.conv2d(F.pad(up, (0, 0, 2, 2), mode="reflect"), w5.unsqueeze(-1))          # (B, N, 60, V)
    got5 = gemm(as_rows(y), B * 60 * V, G3(V), w5.permute(0, 2, 1))
    assert float((got5 - as_rows(ref5)).abs().max()) < 1e-12
    # G4: 5 taps + AvgPool(4) over 60 frames as one operand
    V4, C4 = 6, 256
    z = torch.randn((B, C4, 60, V4), generator=gen, dtype=torch.float64)
    w4 = _conv_weights(N, C4, 5, gen)
    ref4 = F.avg_pool2d(F.conv2d(F.pad(z, (0, 0, 2, 2), mode="reflect"), w4.unsqueeze(-1)), (4, 1))
    got4 = gemm(as_rows(z), B * 15 * V4, G4, w4.permute(0, 2, 1))
    assert float((got4 - as_rows(ref4)).abs().max()) < 1e-12
    # G2: output frame 4 s + ph of the 5-tap conv reads upsampled frames 4 s + ph + d - 2 (d < 5), i.e. source frames s - 1, s, s + 1 (tap j =
    # (ph + d - 2) // 4 + 1) with the reflection at the upsampled ends; weights folded per (phase, tap) give all four phases of source
    # frame s as one row of 4 x 64 columns
    Wf = torch.zeros((4, N, 3, C), dtype=torch.float64)
    for ph in range(4):
        for d in range(5):
            Wf[ph, :, (ph + d - 2) // 4 + 1] += w5[:, :, d]
    Wf = Wf.reshape(4 * N, 3, C)
    ref2 = ref5.reshape(B, N, 15, 4, V).permute(0, 2, 4, 3, 1).reshape(B * 15 * V, 4 * N)          # rows (b, s, v), columns (phase, n)
    got2 = gemm(as_rows(y), B * 15 * V, G2(V), Wf)
    assert float((got2 - ref2).abs().max()) < 1e-12
    # ... and the two 2-tap halves: phases 0, 1 never read source frame s + 1, phases 2, 3 never s - 1
    assert float(Wf[:2 * N, 2].abs().max()) == 0.0 and float(Wf[2 * N:, 0].abs().max()) == 0.0
    gota = gemm(as_rows(y), B * 15 * V, G2a(V), Wf[:2 * N, :2])
    gotb = gemm(as_rows(y), B * 15 * V, G2b(V), Wf[2 * N:, 1:])
    assert float((torch.cat([gota, gotb], 1) - ref2).abs().max()) < 1e-12


def test_case_table_is_complete():
    """Every instance of every engine is the declared target of at least one case, every gather configuration and every epilogue appears,
    and every engine has cases it must refuse."""
    want = {"skinny16", "skinny", "f32<64,2,2,1,1>", "f32<64,4,1,1,2>", "f32<128,2,2,2,2>", "x3<64x64>", "x3<64x128>", "x3<128x64>", "x3<128x128>",
            "x3p<0>", "x3p<1>", "x3p<2>", "h2<64x64>", "h2<64x128>", "h2<128x64>", "h2<128x128>", "x3r<-1>", "x3r<0>", "x3r<1>"}
    got, refused = set(), set()
    for pr in PROBLEMS:
        for v in VARIANTS:
            inst = expected_instance(v, pr)
            (got.add(inst) if inst else refused.add(VARIANTS[v][0]))
    assert want <= got, want - got
    assert refused == {"x3", "h2", "x3r"}
    assert {pr["fam"] for pr in PROBLEMS} >= set(FAMILIES) and {pr["epi"] for pr in PROBLEMS} == set(EPILOGUES)
    assert len({pr["name"] for pr in PROBLEMS}) == len(PROBLEMS)
    # persistent on / off pairs for all three epilogue instances and for gathered cases; x3r against x3 with bias and bias + GELU
    pers = {(expected_instance("x3", pr), pr["g"] is not None) for pr in PROBLEMS if (expected_instance("x3", pr) or "").startswith("x3p")}
    assert {i for i, _ in pers} == {"x3p<0>", "x3p<1>", "x3p<2>"} and {g for _, g in pers} == {False, True}
    # the re-scheduled variants give EVERY workgroup several units: each epilogue instance of the persistent kernel, its gathered launches
    # (G1, G2 and both halves) and a_lrelu, with at least 5 tiles per workgroup; each x3r instance with whole panels and a remainder
    multi = {(expected_instance("x3/p64", pr), pr["fam"].split("/")[0], bool(EPILOGUES[pr["epi"]].get("a_lrelu"))) for pr in PROBLEMS
             if (expected_instance("x3/p64", pr) or "").startswith("x3p") and walk("x3/p64", pr)[0] >= 5 * walk("x3/p64", pr)[1]}
    assert {i for i, _, _ in multi} == {"x3p<0>", "x3p<1>", "x3p<2>"} and {f for _, f, _ in multi} >= {"G1", "G2", "G2a", "G2b"} and {a for _, _, a in multi} == {False, True}
    for pr in PROBLEMS:
        if (expected_instance("x3/p64", pr) or "").startswith("x3p"):
            assert walk("x3/p64", pr)[0] >= 5 * 64, pr["name"]
            assert walk("x3/p64", pr)[0] <= 768, pr["name"]                   # ... and ONE tile each with the default: "x3" and "x3/p64" are two schedules
    carry = {expected_instance("x3r/g8", pr) for pr in PROBLEMS if expected_instance("x3r/g8", pr)
             and walk("x3r/g8", pr)[0] // 8 >= 1 and walk("x3r/g8", pr)[0] % 8 != 0}
    assert carry == {"x3r<-1>", "x3r<0>", "x3r<1>"}, carry


# ------------------------------------------------------------------------------------------------ GPU
def dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return torch.device("cuda:0")


def _params_for(pr, variant, ptr=None):
    """probe_params of a case (ptr: name -> device address; None = selection only)."""
    f, e, g = FAMILIES[pr["fam"]], EPILOGUES[pr["epi"]], pr["g"]
    N, K, M = pr["N"], pr["K"], pr["M"]
    lda = pr["lda"] or (g["Cc"] if g else K)
    ldc = pr["ldc"] or N + GUARD_COLS
    ptr = ptr or dict(A=1, W=1, C=1, bias=1, rowbias=1, residual=1, wsub=1)
    kw = dict(A=ptr["A"], W=ptr["W"], C=ptr["C"], M=M, N=N, K=K, lda=lda, ldc=ldc, ksplit=pr["ksplit"],
              rows_per_win=pr["rpw"] if pr["rpw"] >= 64 else 1024)
    if pr["ksplit"] > 1:
        kw["slab_stride"] = (M + GUARD_ROWS) * ldc
    if pr["wsub"]:
        kw["wsub"] = ptr["wsub"]
    if ptr.get("c_amax"):
        kw["c_amax"] = ptr["c_amax"]
    if e.get("bias"):
        kw["bias"] = ptr["bias"]
    if e.get("rb"):
        kw.update(rowbias=ptr["rowbias"], rb_mod=e["rb"])
    if e.get("res"):
        kw.update(residual=ptr["residual"], ldr=N + 32)
    kw.update(act=e.get("act", 0), a_lrelu=e.get("a_lrelu", 0))
    if g:
        kw.update(gather=1, **g)
    kw.update(VARIANTS[variant][1])
    return gp.make_params(**kw)


def _data(pr):
    gen = torch.Generator().manual_seed(zlib.crc32(pr["name"].encode()))
    e, g = EPILOGUES[pr["epi"]], pr["g"]
    N, K, M = pr["N"], pr["K"], pr["M"]
    lda = pr["lda"] or (g["Cc"] if g else K)
    src_rows = M // (g["T_out"] * g["V"]) * g["T_src"] * g["V"] if g else M
    d = dict(A=torch.randn((src_rows, lda), generator=gen), W=torch.randn((N, K), generator=gen) / np.sqrt(K))
    d["bias"] = torch.randn((N,), generator=gen) if e.get("bias") else None
    d["rowbias"] = torch.randn((e["rb"] + 1, N), generator=gen) if e.get("rb") else None      # one spare row behind the rb_mod rows the launch may read
    d["residual"] = torch.randn((M, N + 32), generator=gen) if e.get("res") else None
    d["wsub"] = torch.randn((K,), generator=gen) / np.sqrt(K) if pr["wsub"] else None
    return d


def _reference(pr, d, dtype, **how):
    e, g = EPILOGUES[pr["epi"]], pr["g"]
    c = {k: (v.to(dtype) if v is not None else None) for k, v in d.items()}
    kw = dict(g=g, a_lrelu=bool(e.get("a_lrelu")), **how)
    if c["wsub"] is not None:
        c["W"] = c["W"] - c["wsub"]                                    # one rounding per weight in fp32, as the kernel's subtraction on staging
    if pr["ksplit"] > 1:
        per = pr["K"] // pr["ksplit"]                                  # K / ksplit is a whole number of 32-wide slabs in every raw case
        return torch.stack([gp.reference(c["A"], c["W"], pr["M"], pr["N"], pr["K"], kslice=(z * per, (z + 1) * per), **kw) for z in range(pr["ksplit"])])
    return gp.reference(c["A"], c["W"], pr["M"], pr["N"], pr["K"], bias=c["bias"], rowbias=c["rowbias"], rb_mod=e.get("rb", 1), act=e.get("act", 0),
                        residual=c["residual"], **kw)


def _launch(pr, variant, dd):
    """One launch into a fresh sentinel-filled C.  Returns (return code, result on the CPU or None, guards intact).  The fp16 engine is also
    given a zeroed c_amax vector and must leave in it, per window of rows_per_win rows, exactly the largest magnitude it stored."""
    N, M, ks = pr["N"], pr["M"], pr["ksplit"]
    ldc = pr["ldc"] or N + GUARD_COLS
    coff = pr["coff"]
    Cbuf = torch.full((ks, M + GUARD_ROWS, ldc), SENTINEL, dtype=torch.int32, device=dev())
    ptr = {k: (v.data_ptr() if v is not None else 0) for k, v in dd.items()}
    ptr["C"] = Cbuf.data_ptr() + 4 * coff
    camax = None
    if VARIANTS[variant][0] == "h2":
        rpw = pr["rpw"] if pr["rpw"] >= 64 else 1024
        camax = torch.zeros(((M + rpw - 1) // rpw + GUARD_ROWS,), dtype=torch.float32, device=dev())
        ptr["c_amax"] = camax.data_ptr()
    p = _params_for(pr, variant, ptr)
    torch.cuda.synchronize()
    rc = gp.run(p, VARIANTS[variant][0])
    torch.cuda.synchronize()
    if rc != 0:
        return rc, None, bool((Cbuf == SENTINEL).all())
    body = Cbuf[:, :M, coff:coff + N]
    out = body.contiguous().view(torch.float32).cpu()
    mask = torch.ones_like(Cbuf, dtype=torch.bool)
    mask[:, :M, coff:coff + N] = False
    intact = bool((Cbuf[mask] == SENTINEL).all())
    written = bool((body != SENTINEL).all())
    if camax is not None:
        nwin = (M + rpw - 1) // rpw
        stored = body[0].contiguous().view(torch.float32).abs().amax(1)
        want = torch.stack([stored[w * rpw:(w + 1) * rpw].max() for w in range(nwin)])
        assert torch.equal(camax[:nwin], want), ("c_amax", float((camax[:nwin] - want).abs().max()))
        assert float(camax[nwin:].abs().max()) == 0.0, "c_amax written past the last window"
    return rc, (out if ks > 1 else out[0]), intact and written


def _err(y, ref64):
    d = y.double() - ref64
    return float(d.abs().max()), float(d.pow(2).mean().sqrt())


@pytest.mark.gpu
@pytest.mark.timeout(600)
@pytest.mark.parametrize("pr", PROBLEMS, ids=[p["name"] for p in PROBLEMS])
def test_gemm_instance(pr):
    d = _data(pr)
    ref64 = _reference(pr, d, torch.float64)
    rows = torch.arange(pr["M"]) if pr["M"] <= CHAIN_ROWS else torch.linspace(0, pr["M"] - 1, CHAIN_ROWS).long()
    e_blas = _err(_reference(pr, d, torch.float32), ref64)
    e_chain = _err(_reference(pr, d, torch.float32, rows=rows, chain=True), ref64[..., rows, :])
    e32 = (max(e_blas[0], e_chain[0]), max(e_blas[1], e_chain[1]))
    print(f"[gemm-instances] {pr['name']:34s} fp32 cpu: torch GEMM max {e_blas[0]:.3e} rms {e_blas[1]:.3e}, k-ordered chain max {e_chain[0]:.3e} rms {e_chain[1]:.3e}")
    ulp = float(np.spacing(np.float32(ref64.abs().max())))
    dd = {k: (v.to(dev()) if v is not None else None) for k, v in d.items()}
    res, errs, base = {}, {}, {}
    for variant, (engine, _) in VARIANTS.items():
        want = expected_instance(variant, pr)
        if variant in RESCHEDULED and not (want or "").startswith(RESCHEDULED[variant]):
            continue
        p = _params_for(pr, variant)
        sel = gp.select(p)
        if want is None:                                                # (d) the engine must refuse: its predicate says no and the probe reports it
            assert not sel[engine], (variant, sel)
            rc, _, intact = _launch(pr, variant, dd)
            assert rc == gp.UNSUPPORTED and intact, (variant, rc, intact)
            continue
        assert engine == "f32" or sel[engine], (variant, sel)
        assert gp.instance(engine, p, sel) == want, (variant, gp.instance(engine, p, sel), want, sel)      # (d)
        rc, y, intact = _launch(pr, variant, dd)
        assert rc == 0, (variant, rc)
        assert intact, f"{variant} ({want}): a guard word of C was overwritten, or an element of C was not written"      # (b)
        base[variant] = e32 if want.startswith(ONE_ACCUMULATOR) else e_blas
        res[variant], errs[variant] = y, _err(y, ref64)
        print(f"[gemm-instances] {pr['name']:34s} {variant:7s} {want:18s} max {errs[variant][0]:.3e} ({errs[variant][0] / max(base[variant][0], 1e-30):5.2f} x fp32 cpu)  "
              f"rms {errs[variant][1]:.3e} ({errs[variant][1] / max(base[variant][1], 1e-30):5.2f} x)  ulp {ulp:.2e}")
    for variant, (emax, erms) in errs.items():                             # (a)
        if variant == "h2":
            assert erms <= errs["f32"][1] * 1.02 + 1e-9 and emax <= errs["f32"][0] * 1.5 + 1e-9, (variant, errs[variant], errs["f32"])
        else:
            b = base[variant]
            assert emax <= MARGIN_MAX * b[0] + ulp and erms <= MARGIN_RMS * b[1], (variant, (emax, erms), b, ulp)
    x3s = [v for v in ("x3", "x3/t64", "x3/nop", "x3/p64", "x3r", "x3r/g8") if v in res]      # (c) every schedule of the plane engine: same products, same order per element
    for v in x3s[1:]:
        assert torch.equal(res[x3s[0]], res[v]), (x3s[0], v, float((res[x3s[0]] - res[v]).abs().max()))


def _f32_instance(fam, windows, **over):
    pr = _problem(fam, windows, "none", None, **over)
    p = _params_for(pr, "f32")
    return gp.instance("f32", p, gp.select(p))


def test_window_counts_are_the_smallest_that_reach_each_instance():
    """Host code only (the selection predicates): runs without a GPU."""
    for fam, f in FAMILIES.items():
        for tier, ws in f["tiers"].items():
            for w in ws:
                assert _f32_instance(fam, w) == tier, (fam, tier, w)
            if ws[0] > 1:
                assert _f32_instance(fam, ws[0] - 1) != tier, (fam, tier, ws[0])


SITES = [
    # site, family, epilogue, overrides, instance at 1 / 8 / 128 / 585 windows (library defaults: x3 where it supports the launch, else exact f32)
    ("emb.joint_block", "n256", "rb6", dict(K=960), ("skinny16", "skinny16", "x3<64x128>", "x3p<2>")),
    ("emb.gcn_joint", "gcn_joint", "rb6", {}, ("skinny16", "skinny", "x3p<2>", "x3p<2>")),
    ("emb.tcn_joint_pool", "n256", "bias", dict(K=1280), ("skinny16", "skinny16", "x3<64x128>", "x3p<0>")),
    ("emb.gcn_body", "n256", "rb6", dict(K=512), ("skinny16", "skinny16", "x3<64x128>", "x3p<2>")),
    ("emb.tcn_body", "G1", "bias", {}, ("skinny16", "skinny16", "x3<64x128>", "x3p<0>")),
    ("emb.tcn_body+pos", "G1", "bias_rb90", {}, ("skinny16", "skinny16", "x3<64x128>", "x3p<2>")),
    ("enc.qkv", "n1536", "none", {}, ("skinny16", "x3<64x128>", "x3<128x128>", "x3<128x128>")),
    ("xf.out_proj enc", "n256", "bias_res", dict(K=512), ("skinny16", "skinny16", "x3<64x128>", "x3p<1>")),
    ("xf.ff1", "n512", "bias_gelu", {}, ("skinny16", "skinny16", "x3<64x128>", "x3p<0>")),
    ("xf.ff2", "n256", "bias_res", dict(K=512), ("skinny16", "skinny16", "x3<64x128>", "x3p<1>")),
    ("dec.q", "n1024", "none", {}, ("skinny16", "x3<64x128>", "x3<128x128>", "x3<128x128>")),
    ("xf.out_proj dec", "n256", "bias_res", dict(K=1024), ("skinny16", "skinny16", "x3<64x128>", "x3p<1>")),
    ("dec.style1", "style1", "bias_lrelu", {}, ("skinny16", "skinny16", "skinny16", "skinny16")),
    ("dec.style2", "style2", "bias", {}, ("skinny16", "skinny16", "skinny16", None)),
    ("dec.style2 per layer", "style2l", "bias", {}, (None, None, None, "skinny16")),
    ("mot.gcn_body", "n256", "rb6", dict(K=512), ("skinny16", "skinny16", "x3<64x128>", "x3p<2>")),
    ("mot.tcn_body", "G1", "bias", {}, ("skinny16", "skinny16", "x3<64x128>", "x3p<0>")),
    ("mot.gcn_joint", "n192", "alrelu_bias", {}, ("skinny16", "skinny16", "x3<64x64>", "x3<128x64>")),
    ("mot.tcn_joint V22", "G2/22", "bias", {}, ("skinny16", "skinny", "x3p<0>", None)),
    ("mot.tcn_joint V24", "G2/24", "bias", {}, ("skinny16", "skinny", "x3p<0>", None)),
    ("mot.tcn_joint a", "G2a/22", "bias", {}, (None, None, None, "x3p<0>")),
    ("mot.tcn_joint b", "G2b/22", "bias", {}, (None, None, None, "x3p<0>")),
    ("mot.tcn_joint b V24", "G2b/24", "bias", {}, (None, None, None, "x3p<0>")),
    ("mot.tcn_joint unfolded", "G3/22", "bias", {}, ("skinny", "skinny", "x3<128x64>", "x3<128x64>")),
]


def test_site_instances():
    """Host code only (the selection predicates; runs without a GPU).  The mapping in the module docstring: every GEMM site of run_embed, the encoder, the decoder and run_to_mot is a family of the case
    table, and takes these instances at 1, 8, 128 and 585 windows."""
    fams = {(pr["fam"], pr["epi"], pr["K"]) for pr in PROBLEMS}
    for site, fam, epi, over, want in SITES:
        assert (fam, epi, over.get("K", FAMILIES[fam]["K"])) in fams, site
        for w, inst in zip((1, 8, 128, 585), want):
            if inst is None:
                continue
            pr = _problem(fam, w, epi, None, **over)
            p = _params_for(pr, "x3")
            sel = gp.select(p)
            got = gp.instance("x3", p, sel) if sel["x3"] else gp.instance("f32", p, sel)
            assert got == inst, (site, w, got, inst)
