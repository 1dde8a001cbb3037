"""The norm and pointwise kernels against float64 at the kernel boundary (GPU cases: -m gpu; the CPU pins of the references run everywhere).

csrc/pointwise.hip (instance norm, AdaIN, the embed / body / joint front ends, the final projection, the float64 style MLP, the window
sums, the bank utilities) and mocha_absmax of gemm_h2.hip are launched directly through tests/gemm_probe/pointwise_probe.cpp at the
smallest shapes that reach each instance and each edge of the launchers' contracts (n = 2 .. 96 tokens, V <= 32, Cin <= 16, any row
count) - the network itself only ever calls them with 90 tokens, 22 / 24 joints and whole windows - and held to

  (a) a float64 restatement of what the operation means (tests/pointwise_ref.py; pinned without a GPU to the oracle, to torch's own
      reflect pad / bfloat16 and to an independent encoder by the test_reference_* functions below).  Bound: the error of the SAME
      restatement evaluated in fp32 by torch on the CPU against float64, times MARGINS[kernel] = (on the largest error, on the rms error),
      plus one fp32 ulp of the largest output on the largest error.  The float64 kernels, mean64, the column statistics and absmax have
      DERIVED bounds instead (stated where they are asserted);
  (b) the relations the code promises to the bit: copy_out = the gathered rows, zc = zn - centre, the bf16 planes of zc, the key / value
      image = the plane chain of the normalised / the input rows at the (un)swizzled position, qstat's layout, embed_sums =
      window_sums(embed_front), y32 = y64 rounded once, sub_rows and center_rows' out32 = numpy fp32;
  (c) bit identity across launch variants: reverse 0 / 1 for every kernel that takes it, split / unsplit for instnorm and AdaIN,
      max_wgs for the plane embed front, every combination of optional outputs of the instance norm;
  (d) untouched memory: every output has 0x7FC0DEAD guard words in front of it, behind it and in unused columns, every element the case
      asked for is written, every output it did not ask for is null; every refusal leaves all buffers intact.

Margins.  (4, 2) on the largest / rms error were the starting values.  Measured on an MI355X (175 GPU cases, about 4 000 launches; ratio =
kernel error / fp32 CPU error of the same restatement; every case prints its own with -s), worst per kernel, largest / rms:
  instnorm 1.78 / 1.23 (rms per n: 1.00 at n = 2 and 7, 1.02 at 8, 1.18 at 9, 0.97 - 1.23 from 88 to 96: the kernel adds 8 strided token
  groups and then the groups in order, torch adds the tokens in an order of its own)
  adain (closed) 1.18 / 1.00   adain (literal) 1.30 / 1.02   embed_front 1.67 / 1.04   embed_front_x3 1.55 / 1.09   embed_sums 1.32 / 1.00
  window_sums - / 1.00 (never above one ulp)   body_front 1.00 / 1.00   joint_expand 1.24 / 1.00   rownorm2 - / 0.75   final_proj 3.11 / 1.75
The rms ratio stays at or below 1.23 everywhere but in final_proj, so the rms margin is tightened to 1.5 (DEFAULT_MARGIN, the value
tests/test_gemm_instances.py arrived at).  final_proj keeps the starting (4, 2): its large ratios are all Cout = 3 (rows1320-C3: 2.42 - 3.11 /
1.48 - 1.75; Cout = 16: 0.92 / 0.93) - the kernel is one k-ordered chain of 64 products per output on the fp32 matrix pipe whatever Cout is,
while torch's CPU matmul sums a 3-column product differently (and more accurately) than a 16-column one; the starting margin holds it, so it
is not widened.
Derived bounds, worst error / bound: linear_f64 0.19, mean64 0.12; qstat 0.47 and center_rows' qstat 0.31 of (4 x the fp32 CPU sum's error
+ one ulp), relative error at most 1.1e-7; column statistics and absmax within one ulp everywhere.
Mutations, each on a scratch copy (never committed), new file / tests/test_hip_parity.py:
  1. inorm_stats divides by n instead of n - 1: all 18 test_instnorm and all 8 test_adain cases fail / 21 of 60 fail (encoder, decoder,
     generator_forward, characterize, pose normalisation, decoder folding, pair).
  2. mocha_embed_sums_x3's upper reflect as 119 - r: all 18 test_embed_sums cases fail at their first launch (float64: errors of 0.9 - 1.5 against a bound
     of 1e-6; the bit identity with window_sums(embed_front) comes after it in the case), nothing else / 18 of 60 fail (mot_embedding, fused_encode, ...).
  3. mocha_final_proj de-normalises with row v instead of v + 1: the three de-normalising test_final_proj cases fail, nothing else / 1 of 60
     fails (test_fused_pose_normalisation).
Run time on the GPU box: 14 s for the file (the slowest case 0.5 s: the 64 x 64 float64 tile against numpy.longdouble), CPU references included.
Every case ran and was measured; no kernel needed a fix.

A note on V * Cin = 513: with V <= 32 and Cin <= 16 no pair has that product (513 = 27 x 19), so the refusal case is (27, 19), which the
Cin limit refuses as well; the product limit cannot be reached on its own.
"""
import itertools
import os
import sys
import zlib

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pointwise_ref as pr  # noqa: E402

gpu = pytest.mark.gpu
SENTINEL = 0x7FC0DEAD
GUARD = 64                                  # sentinel words in front of and behind every output
# margin on the largest / on the rms error of the fp32 CPU evaluation, per kernel (section 4 of the docstring)
MARGINS = {"final_proj": (4.0, 2.0)}
DEFAULT_MARGIN = (4.0, 1.5)


def rng(name):
    return np.random.Generator(np.random.PCG64(zlib.crc32(name.encode())))


def normal(r, *shape):
    return r.standard_normal(shape, dtype=np.float32)


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return torch.device("cuda:0")


def D(a):
    """A host array (or None) on the device."""
    return None if a is None else T(a).to(dev())


class Out:
    """An output buffer between sentinel guards.  kind: f32 / f64 / u16; `written` (bool array of `shape`, default all): the elements
    the launch must write - every other one (unused columns of a wide leading dimension) must stay a sentinel."""
    KINDS = {"f32": (torch.int32, np.float32, 4), "f64": (torch.int64, np.float64, 8), "u16": (torch.int16, np.uint16, 2)}

    def __init__(self, shape, kind="f32", written=None):
        self.tdt, self.ndt, size = self.KINDS[kind]
        self.shape = tuple(int(s) for s in shape)
        n = int(np.prod(self.shape))
        self.words = (n * size + 3) // 4
        self.words += self.words & 1
        self.buf = torch.full((2 * GUARD + self.words,), SENTINEL, dtype=torch.int32, device=dev())
        self.fresh = self._body(torch.full((self.words,), SENTINEL, dtype=torch.int32), n)
        self.body = self._body(self.buf[GUARD:GUARD + self.words], n)
        self.written = torch.ones(self.shape, dtype=torch.bool) if written is None else T(written)
        self.ptr = self.body.data_ptr()

    def _body(self, words, n):
        return words.view(self.tdt)[:n].view(self.shape)

    def intact(self):
        """Nothing at all was written (a refusal)."""
        return bool((self.buf == SENTINEL).all())

    def check(self, what):
        host = self.buf.cpu()
        body = self._body(host[GUARD:GUARD + self.words], int(np.prod(self.shape)))
        assert bool((host[:GUARD] == SENTINEL).all()) and bool((host[GUARD + self.words:] == SENTINEL).all()), f"{what}: a guard word was overwritten"
        assert bool((body[~self.written] == self.fresh[~self.written]).all()), f"{what}: an element outside the output was overwritten"
        assert bool((body[self.written] != self.fresh[self.written]).all()), f"{what}: an element of the output was not written"
        return body.numpy().view(self.ndt)


RATIOS = {}


def hold(kernel, case, y, ref64, ref32):
    """(a): y (numpy fp32) against the float64 restatement, bounded by the fp32 CPU evaluation's own error."""
    y = T(np.asarray(y))
    emax, erms = pr.errors(y, ref64)
    bmax, brms = pr.errors(ref32, ref64)
    ulp = pr.ulp_of_largest(ref64)
    mmax, mrms = MARGINS.get(kernel, DEFAULT_MARGIN)
    rmax, rrms = emax / max(bmax, 1e-300), erms / max(brms, 1e-300)
    w = RATIOS.setdefault(kernel, [0.0, 0.0])
    w[0], w[1] = max(w[0], rmax if emax > ulp else 0.0), max(w[1], rrms)
    print(f"[pointwise] {kernel:14s} {case:44s} max {emax:.3e} ({rmax:6.2f} x fp32 cpu) rms {erms:.3e} ({rrms:5.2f} x) ulp {ulp:.2e}   worst so far {w[0]:.2f} / {w[1]:.2f}")
    assert emax <= mmax * bmax + ulp and erms <= mrms * brms, (kernel, case, (emax, erms), (bmax, brms), ulp)


def both(fn, *args, **kw):
    """The restatement `fn` in float64 and in fp32: tensors among the arguments are converted, everything else passes."""
    def conv(a, dt):
        return a.to(dt) if isinstance(a, torch.Tensor) and a.is_floating_point() else a
    out = []
    for dt in (torch.float64, torch.float32):
        out.append(fn(*[conv(a, dt) for a in args], **{k: conv(v, dt) for k, v in kw.items()}))
    return out


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


# =================================================================================================== no GPU: the references are what they claim
def test_reference_norms_are_the_oracles():
    """pointwise_ref.instnorm / adain_literal against oracle.mocha_oracle.mean_variance_norm / adain in float64, to 1e-12."""
    from oracle import mocha_oracle as O
    g = torch.Generator().manual_seed(11)
    x = torch.randn((3, 9, 256), generator=g, dtype=torch.float64) * 3 + 1
    out, mean = pr.instnorm(x)
    assert float((out - O.mean_variance_norm(x.permute(0, 2, 1)).permute(0, 2, 1)).abs().max()) < 1e-12
    assert float((mean - x.mean(1)).abs().max()) < 1e-13
    sty = torch.randn((3, 7, 256), generator=g, dtype=torch.float64)
    sd = {"p.style.2.weight": torch.randn((64, 256), generator=g, dtype=torch.float64) / 16, "p.style.2.bias": torch.randn((64,), generator=g, dtype=torch.float64),
          "p.style.4.weight": torch.randn((512, 64), generator=g, dtype=torch.float64) / 8, "p.style.4.bias": torch.randn((512,), generator=g, dtype=torch.float64)}
    s = F.linear(F.leaky_relu(F.linear(sty.mean(1), sd["p.style.2.weight"], sd["p.style.2.bias"]), 0.2), sd["p.style.4.weight"], sd["p.style.4.bias"])
    xad, qin = pr.adain_literal(x, s[:, :256], s[:, 256:])
    want = O.adain(sd, "p", x, sty)
    assert float((xad - want).abs().max()) < 1e-12
    assert float((qin - O.mean_variance_norm(want.permute(0, 2, 1)).permute(0, 2, 1)).abs().max()) < 1e-9
    xc, qc = pr.adain_closed(x, s[:, :256], s[:, 256:])                     # well-conditioned here: both orders agree
    assert float((xc - xad).abs().max()) < 1e-12 and float((qc - qin).abs().max()) < 1e-9


def test_reference_embed_front_is_the_first_stage_of_mot_embedding(golden_dir):
    """pointwise_ref.embed_front against oracle.mocha_oracle.mot_embedding's own 1x1 conv (its `emb_conv1` stage), LeakyReLU, and - hop by
    hop - the oracle's spatial_conv with an identity 1x1 conv, then the joint -> part pool, in float64 with the real graph constants."""
    from oracle import mocha_oracle as O
    from mocha_sigasia2023_amd import synthetic_state_dict
    z = np.load(os.path.join(golden_dir, "graph_constants.npz"))
    for layout in ("mocha", "mixamo"):
        sd = {k: T(v).double() for k, v in synthetic_state_dict(seed=5, gain=1.5, layout=layout).items()}
        A_j, pool = T(z[f"{layout}_A_j"]).double(), T(z[f"{layout}_pool"]).double()
        assert torch.equal(A_j, sd["mot_embedding.2.A_j"]) and torch.equal(pool, sd["mot_embedding.3.weight"])
        V, Cin = A_j.shape[1], sd["mot_embedding.1.weight"].shape[1]
        X = torch.randn((2, 60, V, Cin), generator=torch.Generator().manual_seed(3), dtype=torch.float64)
        st = {}
        O.mot_embedding(sd, X, st)
        h = F.leaky_relu(st["emb_conv1"], O.LRELU_SLOPE)                    # (B, 64, T, V)
        eye = torch.eye(64, dtype=torch.float64).reshape(64, 64, 1, 1)
        hops = [torch.einsum("nctv,vw->nctw", O.spatial_conv(h, A_j[k:k + 1], eye, None), pool) for k in range(3)]      # each (B, 64, T, 6)
        want = torch.stack(hops, 1).permute(0, 3, 4, 1, 2).reshape(2 * 60, 6, 192)                                      # (b, t), p, (k, c)
        AP = torch.einsum("kvw,wp->kvp", A_j, pool)
        got = pr.embed_front(X.reshape(120, V, Cin), sd["mot_embedding.1.weight"].reshape(64, Cin), sd["mot_embedding.1.bias"], AP)
        assert float((got - want).abs().max()) < 1e-12
        # the pose normalisation: z-score with the root row's statistics in front, root dropped
        Xr = torch.randn((5, V + 1, Cin), dtype=torch.float64, generator=torch.Generator().manual_seed(4))
        m, s = torch.randn((V + 1) * Cin, dtype=torch.float64, generator=torch.Generator().manual_seed(5)), torch.rand((V + 1) * Cin, dtype=torch.float64, generator=torch.Generator().manual_seed(6)) + 0.5
        a = pr.embed_front(Xr, sd["mot_embedding.1.weight"].reshape(64, Cin), sd["mot_embedding.1.bias"], AP, m, s, 1)
        b = pr.embed_front(((Xr - m.reshape(V + 1, Cin)) / s.reshape(V + 1, Cin))[:, 1:], sd["mot_embedding.1.weight"].reshape(64, Cin), sd["mot_embedding.1.bias"], AP)
        assert float((a - b).abs().max()) < 1e-12


def test_reference_window_sums_are_reflect_pad_and_pooling():
    """pointwise_ref.window_sums against F.pad(mode="reflect") and, per tap, the average over 4 frames at stride 4, to 1e-12."""
    y = torch.randn((3, 60, 6, 20), generator=torch.Generator().manual_seed(8), dtype=torch.float64)
    got = pr.window_sums(y)                                                 # (B, 15, 6, 5 * 20)
    pad = F.pad(y.permute(0, 3, 1, 2), (0, 0, 2, 2), mode="reflect")       # (B, C, 64, 6)
    for dt in range(5):
        want = F.avg_pool2d(pad[:, :, dt:dt + 60], (4, 1)).permute(0, 2, 3, 1)       # frames dt .. dt + 59 of the padded line, pooled by 4
        assert float((got[..., dt * 20:(dt + 1) * 20] - want).abs().max()) < 1e-12


def test_reference_final_proj_row_map():
    """The phased row map in words: output row (window, t, joint) reads channels (t & 3) * 64 .. + 63 of input row (window, t >> 2, joint);
    de-normalisation by row joint + 1.  Against plain loops."""
    g = torch.Generator().manual_seed(9)
    V, Co = 5, 3
    z = torch.randn((2, 15, V, 256), generator=g, dtype=torch.float64)
    W6, b6 = torch.randn((Co, 64), generator=g, dtype=torch.float64), torch.randn((Co,), generator=g, dtype=torch.float64)
    ym, ys = torch.randn(((V + 1) * Co,), generator=g, dtype=torch.float64), torch.rand(((V + 1) * Co,), generator=g, dtype=torch.float64) + 0.5
    got = pr.final_proj(z, W6, b6, V, ym, ys, phased=True).reshape(2, 60, V, Co)
    for w, t, v in itertools.product(range(2), (0, 1, 3, 4, 58, 59), range(V)):
        zz = z[w, t >> 2, v, (t & 3) * 64:(t & 3) * 64 + 64]
        y = F.leaky_relu(zz, 0.2) @ W6.T + b6
        y = y * ys.reshape(V + 1, Co)[v + 1] + ym.reshape(V + 1, Co)[v + 1]
        assert float((got[w, t, v] - y).abs().max()) < 1e-12


def test_reference_bf16_is_torch_bfloat16():
    """Round to nearest even in integer arithmetic against torch.Tensor.to(torch.bfloat16): 4 million random bit patterns (NaNs left
    out), every tie of a block of exponents, subnormals, the largest finite values, signed zeros and infinities."""
    r = rng("bf16")
    bits = r.integers(0, 1 << 32, size=1 << 22, dtype=np.uint64).astype(np.uint32)
    ties = (np.arange(0, 1 << 16, dtype=np.uint32) << 16) | 0x8000           # exactly half way, every upper half (NaNs removed below)
    near = np.concatenate([ties - 1, ties + 1])
    sub = r.integers(0, 1 << 23, size=1 << 16, dtype=np.uint64).astype(np.uint32) | (r.integers(0, 2, size=1 << 16, dtype=np.uint64).astype(np.uint32) << 31)
    special = np.array([0, 0x80000000, 0x7F800000, 0xFF800000, 0x7F7FFFFF, 0x7F7F8000, 0x7F7F7FFF, 1, 0x007FFFFF, 0x00008000, 0x00018000], dtype=np.uint32)
    u = np.concatenate([bits, ties, near, sub, special])
    u = u[(u & 0x7FFFFFFF) <= 0x7F800000]
    x = u.view(np.float32)
    want = T(x).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    got = pr.bf16_bits(x)
    assert np.array_equal(got, want)
    assert np.array_equal(pr.bf16_value(got), T(x).to(torch.bfloat16).float().numpy())
    assert pr.bf16_bits(np.array([np.nan], dtype=np.float32))[0] & 0x7FC0 == 0x7FC0
    # the chain leaves at most 2^-24 |x| and its planes sum back to x for ordinary values
    v = normal(r, 100000) * 10
    p = pr.bf16_value(pr.plane_chain(v))
    assert np.array_equal((p[0] + p[1]) + p[2], v)


def _kv_encode(K, V):
    """An encoder of the key / value image written independently of pointwise_ref.kv_decode, byte by byte from the layout comment of
    csrc/attention_kv.hip: K, V uint16 [B, 3, 96, 256] -> uint8 [B, KV_IMG_BYTES]."""
    B = K.shape[0]
    img = np.zeros((B, pr.KV_IMG_BYTES), dtype=np.uint8)
    for op, src in ((0, K), (1, V)):
        for c, pl, row in itertools.product(range(8), range(3), range(96)):
            base = (op * 8 + c) * pr.KV_STAGE_BYTES + pl * 96 * 64 + row * 64
            for piece in range(4):
                at = piece ^ ((row >> 2) & 3) if op == 0 else piece
                d0 = 32 * c + 8 * piece
                img[:, base + 16 * at:base + 16 * at + 16] = np.ascontiguousarray(src[:, pl, row, d0:d0 + 8]).view(np.uint8)
    return img


def test_reference_kv_image_decoder_round_trip():
    r = rng("kvimg")
    K = r.integers(0, 1 << 16, size=(2, 3, 96, 256), dtype=np.uint64).astype(np.uint16)
    V = r.integers(0, 1 << 16, size=(2, 3, 96, 256), dtype=np.uint64).astype(np.uint16)
    k, v = pr.kv_decode(_kv_encode(K, V))
    assert np.array_equal(k, K) and np.array_equal(v, V)
    # the K and V images of the same rows differ only by the swizzle: same 16-byte pieces, piece j of row r at j ^ ((r >> 2) & 3)
    img = _kv_encode(K, K).reshape(2, 2, 8, 3, 96, 4, 16)
    for row in (0, 3, 4, 9, 14, 95):
        for piece in range(4):
            assert np.array_equal(img[:, 0, :, :, row, piece ^ ((row >> 2) & 3)], img[:, 1, :, :, row, piece])


def test_probe_refuses_what_no_launcher_checks():
    """The probe's own sane() (host code; no GPU is touched: it returns before any launch)."""
    lib = pr.load()
    one = 4096                                                              # never dereferenced: every call below returns before launching
    assert lib.pw_final_proj(one, one, one, one, 60 * 22 + 1, 15, 22, 0, 0, 1, 0, 0) == pr.BAD_ARGUMENT       # phased, not whole windows
    assert lib.pw_final_proj(one, one, one, one, 10, 15, 22, one, 0, 0, 0, 0) == pr.BAD_ARGUMENT             # ymean without ystd
    assert lib.pw_final_proj(0, one, one, one, 10, 15, 22, 0, 0, 0, 0, 0) == pr.BAD_ARGUMENT
    assert lib.pw_linear_f64(one, 32, 32, one, 0, one, 0, 64, 4, 32, 32, 2, 0, 0) == pr.BAD_ARGUMENT         # ldx < (L - 1) xcol + K
    assert lib.pw_linear_f64(one, 64, 32, one, 0, one, 0, 63, 4, 32, 32, 2, 0, 0) == pr.BAD_ARGUMENT         # ldy < L N
    assert lib.pw_embed_front(one, one, one, one, one, 4, 22, 15, one, 0, 0, 0, 512, 0) == pr.BAD_ARGUMENT   # xmean without xstd
    assert lib.pw_column_mean(one, 4, 64, one, one, 100, 0) == pr.BAD_ARGUMENT                               # scratch too small
    assert lib.pw_absmax(one, 2, 5, 0, 1.0, 0.0, 0) == pr.BAD_ARGUMENT
    q = pr.pw_inorm()
    q.B, q.n, q.x, q.zn = 1, 9, one, one                                    # zn without gm / gs
    assert lib.pw_instnorm(q, 1, 0) == pr.BAD_ARGUMENT
    q = pr.pw_inorm()
    q.B, q.n, q.x, q.zn, q.gm, q.gs, q.centre, q.zc16, q.plane_stride = 2, 9, one, one, one, one, one, one, 2 * 9 * 256 - 1      # planes overlap
    assert lib.pw_instnorm(q, 1, 0) == pr.BAD_ARGUMENT


# =================================================================================================== GPU: instance norm
IN_N = (2, 7, 8, 9, 88, 89, 90, 95, 96)
SPLITS = {"split": 1 << 30, "unsplit": 0}


def _inorm_inputs(name, B, n):
    r = rng(name)
    scale = r.uniform(0.01, 30.0, (B, 1, 256)).astype(np.float32)
    x = (normal(r, B, n, 256) + 1.5 * normal(r, B, 1, 256)) * scale         # the offset is proportional to the scale
    x[:, :, 12:16] = 4.25                                                   # zero variance, sums exact
    d = dict(x=x.astype(np.float32), gm=normal(r, n, 256), gs=r.uniform(0.5, 2.0, (n, 256)).astype(np.float32), centre=normal(r, n, 256))
    return d


def _inorm_launch(B, n, dd, split_max, want, reverse=0, table=None, row_idx=None, table_rows=0, use_extra=1, expect=0):
    """One launch.  want: names among out, mean_out, zn, zc, zc16, zc16x2, qstat, copy_out, kvimg, mean64.  Returns name -> numpy."""
    outs = {}
    if "out" in want: outs["out"] = Out((B, n, 256))
    if "mean_out" in want: outs["mean_out"] = Out((B, 256))
    if "zn" in want: outs["zn"] = Out((B, n, 256))
    if "zc" in want: outs["zc"] = Out((B, n, 256))
    if "zc16" in want: outs["zc16"] = Out((1, B, n, 256), "u16")
    if "zc16x2" in want: outs["zc16"] = Out((2, B, n, 256), "u16")
    if "qstat" in want: outs["qstat"] = Out((B, pr.QSTAT_PARTS, 2))
    if "copy_out" in want: outs["copy_out"] = Out((B, n, 256))
    if "kvimg" in want: outs["kvimg"] = Out((B, pr.KV_IMG_BYTES // 2), "u16")
    if "mean64" in want: outs["mean64"] = Out((B, 256), "f64")
    q = pr.pw_inorm()
    q.B, q.n, q.split_max, q.reverse = B, n, split_max, reverse
    q.x = pr.ptr(dd["x"]) if table is None else 0
    for k in ("out", "mean_out", "zn", "zc", "zc16", "qstat", "copy_out", "kvimg", "mean64"):
        setattr(q, k, outs[k].ptr if k in outs else 0)
    if "zn" in want or "gm" in want:
        q.gm, q.gs = pr.ptr(dd["gm"]), pr.ptr(dd["gs"])
    if ("zc" in want or "zc16" in want or "zc16x2" in want or "centre" in want) and "nocentre" not in want:
        q.centre = pr.ptr(dd["centre"])
    if "zc16x2" in want or "stride" in want:
        q.plane_stride = B * n * 256
    if table is not None:
        q.table, q.table_rows = pr.ptr(table), table_rows
    if row_idx is not None:
        q.row_idx = pr.ptr(row_idx)
    torch.cuda.synchronize()
    rc = pr.load().pw_instnorm(q, use_extra, 0)
    torch.cuda.synchronize()
    assert rc == expect, (want, rc, expect)
    if expect != 0:
        assert all(o.intact() for o in outs.values()), (want, "a refused launch wrote")
        return None
    return {k: o.check(f"instnorm {want} {k}") for k, o in outs.items()}


def _fp32_sum_error(terms64):
    """terms64 (..., N) float64 values that are exact fp32 numbers' squares: the error of their fp32 CPU sum (torch) against float64."""
    return float((terms64.float().sum(-1).double() - terms64.sum(-1)).abs().max())


def _check_inorm(case, B, n, d, ref, res, xin, split):
    """Every assertion that applies to the outputs a launch produced."""
    (out64, mean64r), (out32, mean32) = ref["out"]
    if "out" in res:
        hold("instnorm", f"{case} out", res["out"], out64, out32)
        assert np.all(res["out"][:, :, 12:16] == 0.0), "a zero-variance channel is not exactly 0"
    if "mean_out" in res:
        hold("instnorm", f"{case} mean", res["mean_out"], mean64r, mean32)
    if "mean64" in res:
        bound = n * 2.0 ** -53 * np.abs(xin.astype(np.float64)).mean(1)      # derived: n float64 additions of exact fp32 values and one division
        err = np.abs(res["mean64"].astype(np.longdouble) - xin.astype(np.longdouble).sum(1) / n).astype(np.float64)
        print(f"[pointwise] mean64         {case:44s} worst error / bound {float((err / np.maximum(bound, 1e-300)).max()):.3f}")
        assert np.all(err <= bound), (case, "mean64", float(err.max()))
    if "zn" in res:
        hold("instnorm", f"{case} zn", res["zn"], ref["zn"][0], ref["zn"][1])
        zc = (res["zn"] - d["centre"][None]).astype(np.float32)            # (b) from the kernel's own zn, in numpy fp32
        if "zc" in res:
            assert same_bits(res["zc"], zc), (case, "zc != zn - centre")
            hold("instnorm", f"{case} zc", res["zc"], ref["zc"][0], ref["zc"][1])
        left = zc
        if "zc16" in res:
            p0 = pr.bf16_bits(zc)
            assert np.array_equal(res["zc16"][0], p0), (case, "plane 0 != bf16(zc)")
            left = (zc - pr.bf16_value(p0)).astype(np.float32)
            if res["zc16"].shape[0] == 2:
                p1 = pr.bf16_bits(left)
                assert np.array_equal(res["zc16"][1], p1), (case, "plane 1 != bf16(zc - plane 0)")
                left = (left - pr.bf16_value(p1)).astype(np.float32)
        else:
            left = np.zeros_like(zc)
        if "qstat" in res:
            qs = res["qstat"].astype(np.float64)                             # (B, part, {||zc||^2, ||left||^2})
            t = np.stack([zc.astype(np.float64) ** 2, left.astype(np.float64) ** 2], -1)      # (B, n, 256, 2)
            parts = t.reshape(B, n, 4, 64, 2).transpose(0, 2, 4, 1, 3).reshape(B, 4, 2, n * 64)  # per channel quarter
            whole = t.transpose(0, 3, 1, 2).reshape(B, 2, n * 256)
            if split == "unsplit":
                assert np.all(res["qstat"][:, 1:] == 0.0), (case, "qstat parts 1..3 of a one-workgroup window are not 0")
            else:                                                          # part y = channels 64 y .. 64 y + 63
                tol = 4 * _fp32_sum_error(T(parts)) + float(np.spacing(np.float32(parts.sum(-1).max())))
                e = float(np.abs(qs - parts.sum(-1)).max())
                print(f"[pointwise] qstat parts    {case:44s} error {e:.3e} bound {tol:.3e}")
                assert e <= tol, (case, "qstat part", e, tol)
            tol = 4 * _fp32_sum_error(T(whole)) + float(np.spacing(np.float32(whole.sum(-1).max())))
            e = float(np.abs(qs.sum(1) - whole.sum(-1)).max())
            print(f"[pointwise] qstat          {case:44s} error {e:.3e} bound {tol:.3e} (relative {e / float(whole.sum(-1).max()):.2e})")
            assert e <= tol, (case, "qstat", e, tol)
    if "copy_out" in res:
        assert same_bits(res["copy_out"], xin), (case, "copy_out != the gathered rows")
    if "kvimg" in res:
        K, V = pr.kv_decode(res["kvimg"].view(np.uint8).reshape(B, pr.KV_IMG_BYTES))
        assert not K[:, :, n:].any() and not V[:, :, n:].any(), (case, "rows n .. 95 of the images are not zero")
        assert np.array_equal(V[:, :, :n], pr.plane_chain(xin).transpose(1, 0, 2, 3)), (case, "V image != the plane chain of the input")
        if "out" in res:
            assert np.array_equal(K[:, :, :n], pr.plane_chain(res["out"]).transpose(1, 0, 2, 3)), (case, "K image != the plane chain of out")


@gpu
@pytest.mark.parametrize("B", (1, 3))
@pytest.mark.parametrize("n", IN_N)
def test_instnorm(n, B):
    case = f"n{n}-B{B}"
    d = _inorm_inputs("inorm-" + case, B, n)
    dd = {k: D(v) for k, v in d.items()}
    x = T(d["x"])
    o = both(pr.instnorm, x)
    zn = [(o[i][0] - T(d["gm"]).to(o[i][0].dtype)) / T(d["gs"]).to(o[i][0].dtype) for i in (0, 1)]
    ref = dict(out=o, zn=zn, zc=[zn[i] - T(d["centre"]).to(zn[i].dtype) for i in (0, 1)])
    combos = [("out", "mean_out"), ("out",), ("zn",), ("zn", "zc"), ("zn", "zc16"), ("zn", "zc16x2"), ("zn", "zc", "zc16x2"),
              ("zn", "zc", "qstat"), ("zn", "zc16", "qstat"), ("zn", "zc16x2", "qstat"), ("zn", "zc", "zc16x2", "qstat"), ("out", "mean64")]
    everything = ("out", "mean_out", "zn", "zc", "zc16x2", "qstat", "mean64") + (("kvimg",) if n >= 88 else ())
    seen = {}
    for split, smax in SPLITS.items():
        first = {}
        for want in combos + [everything]:
            res = _inorm_launch(B, n, dd, smax, want)
            _check_inorm(f"{case} {split} {'+'.join(want)}", B, n, d, ref, res, d["x"], split)
            for k, v in res.items():                                       # (c) an output does not depend on which others were asked for
                key = k if k != "zc16" else f"zc16x{v.shape[0]}"              # (qstat: ||zc||^2 does not; the second word is what the planes asked for leave out)
                v = v[..., 0].copy() if k == "qstat" else v
                assert same_bits(first.setdefault(key, v), v), (case, split, want, k)
            full = res
        if n >= 88:                                                         # the image as the decoder launches it: no out
            img = _inorm_launch(B, n, dd, smax, ("kvimg",))
            _check_inorm(f"{case} {split} kvimg alone", B, n, d, ref, img, d["x"], split)
            assert same_bits(img["kvimg"], first["kvimg"]), (case, split, "the image depends on out")
        rev = _inorm_launch(B, n, dd, smax, everything, reverse=1)           # (c) reverse
        for k, v in rev.items():
            assert same_bits(v, full[k]), (case, split, "reverse", k)
        seen[split] = first
    for k, v in seen["split"].items():                                      # (c) split against unsplit (qstat: another layout by contract)
        if k != "qstat":
            assert same_bits(v, seen["unsplit"][k]), (case, "split / unsplit", k)
    if B == 3:                                                              # no extras struct at all: the launcher's defaults
        res = _inorm_launch(B, n, dd, 0, ("out", "mean_out", "zn"), use_extra=0)
        for k, v in res.items():
            assert same_bits(v, seen["split"][k]), (case, "no extras", k)
    # gathered rows: a negative index, one past the table (both clamped) and a repeat
    tr = 4
    table = np.concatenate([d["x"], _inorm_inputs("inorm-t-" + case, tr, n)["x"]])[:tr]
    idx = np.array([-3, tr + 5, tr - 1][:B] if B > 1 else [tr + 5], dtype=np.int32)
    rows = np.clip(idx, 0, tr - 1)
    xin = table[rows]
    og = both(pr.instnorm, T(xin))
    zg = [(og[i][0] - T(d["gm"]).to(og[i][0].dtype)) / T(d["gs"]).to(og[i][0].dtype) for i in (0, 1)]
    refg = dict(out=og, zn=zg, zc=[zg[i] - T(d["centre"]).to(zg[i].dtype) for i in (0, 1)])
    for split, smax in SPLITS.items():
        want = ("out", "mean_out", "zn", "zc", "copy_out") + (("kvimg",) if n >= 88 else ())
        res = _inorm_launch(B, n, dd, smax, want, table=D(table), row_idx=D(idx), table_rows=tr)
        _check_inorm(f"{case} {split} gather", B, n, d, refg, res, xin, split)


@gpu
def test_instnorm_refusals():
    B, n = 2, 90
    d = _inorm_inputs("inorm-refuse", B, 97)
    dd = {k: D(v) for k, v in d.items()}
    bad = pr.INVALID_VALUE
    for nn in (1, 97):
        _inorm_launch(B, nn, dd, 1 << 30, ("out", "mean_out", "zn"), expect=bad)
        _inorm_launch(B, nn, dd, 0, ("out",), expect=bad)
    _inorm_launch(B, 87, dd, 1 << 30, ("out", "kvimg"), expect=bad)
    _inorm_launch(B, n, dd, 1 << 30, ("zn", "zc", "nocentre"), expect=bad)
    _inorm_launch(B, n, dd, 1 << 30, ("zc", "gm", "centre"), expect=bad)      # zc without zn
    _inorm_launch(B, n, dd, 1 << 30, ("zn", "qstat"), expect=bad)
    _inorm_launch(B, n, dd, 1 << 30, ("zn", "zc", "stride"), expect=bad)      # plane_stride without zc16
    _inorm_launch(B, n, dd, 1 << 30, ("out",), row_idx=D(np.zeros(B, dtype=np.int32)), expect=bad)      # row_idx without table


# =================================================================================================== GPU: AdaIN
def _adain_launch(dd, gb, gb_off, gb_stride, B, n, closed, idx, gb_rows, smax, reverse=0, expect=0):
    xad, qin = Out((B, n, 256)), Out((B, n, 256))
    torch.cuda.synchronize()
    rc = pr.load().pw_adain(pr.ptr(dd), gb.data_ptr() + 4 * gb_off, gb_stride, xad.ptr, qin.ptr, B, n, closed, pr.ptr(idx), gb_rows, smax, reverse, 0)
    torch.cuda.synchronize()
    assert rc == expect, (rc, expect)
    if expect:
        assert xad.intact() and qin.intact()
        return None
    return xad.check("adain xad"), qin.check("adain qin")


@gpu
@pytest.mark.parametrize("B", (1, 3))
@pytest.mark.parametrize("n", (2, 9, 90, 96))
def test_adain(n, B):
    case = f"n{n}-B{B}"
    r = rng("adain-" + case)
    rows = 4                                                                # rows of the gamma / beta table (>= B)
    for closed in (1, 0):
        x = normal(r, B, n, 256) * r.uniform(0.01, 30.0, (B, 1, 256)).astype(np.float32)
        g = (normal(r, rows, 256) * 2.0).astype(np.float32)
        if closed:                                                          # the inputs of tests/test_adain_identity.py
            b = (normal(r, rows, 256) * 10.0).astype(np.float32)
            g[:, 0:8] = (-1.0 + r.uniform(-1e-3, 1e-3, (rows, 8))).astype(np.float32)
            g[:, 8:12] = -3.0
            x[:, :, 12:16] = 4.25
        else:                                                               # |1 + gamma| >= 0.5: the literal order is well-conditioned everywhere
            b = normal(r, rows, 256)
            g1 = 1.0 + g
            g = (np.where(np.abs(g1) < 0.5, np.copysign(0.5, g1) + g1, g1) - 1.0).astype(np.float32)
            assert np.abs(1.0 + g.astype(np.float64)).min() >= 0.5 - 1e-6
        dx = D(x)
        fn = pr.adain_closed if closed else pr.adain_literal
        for stride, idx in itertools.product((512, 1024), (None, np.array([-2, rows + 3, 0][:B] if B > 1 else [rows + 3], dtype=np.int32))):
            layer = 1 if stride == 1024 else 0                              # the second layer's constants: gb + 512 (mocha_api.cpp)
            tab = normal(r, rows, stride)
            tab[:, layer * 512:layer * 512 + 256], tab[:, layer * 512 + 256:layer * 512 + 512] = g, b
            sel = np.arange(B) if idx is None else np.clip(idx, 0, rows - 1)
            ref64, ref32 = both(fn, T(x), T(g[sel]), T(b[sel]))
            got = {}
            for split, smax in SPLITS.items():
                name = f"{case} closed{closed} s{stride} {'idx' if idx is not None else 'rows'} {split}"
                xad, qin = _adain_launch(dx, D(tab), layer * 512, stride, B, n, closed, D(idx), rows, smax)
                kern = "adain" if closed else "adain literal"
                hold(kern, name + " xad", xad, ref64[0], ref32[0])
                hold(kern, name + " qin", qin, ref64[1], ref32[1])
                if closed:
                    assert np.all(qin[:, :, 12:16] == 0.0), (name, "qin of a zero-variance channel is not exactly 0")
                got[split] = (xad, qin)
                rx, rq = _adain_launch(dx, D(tab), layer * 512, stride, B, n, closed, D(idx), rows, smax, reverse=1)
                assert same_bits(rx, xad) and same_bits(rq, qin), (name, "reverse")
            assert same_bits(got["split"][0], got["unsplit"][0]) and same_bits(got["split"][1], got["unsplit"][1]), (case, "split / unsplit")


@gpu
def test_adain_refusals():
    x, gb = D(normal(rng("adain-r"), 2, 97, 256)), D(normal(rng("adain-g"), 4, 1024))
    for n, stride, idx, rows in ((1, 512, None, 0), (97, 512, None, 0), (90, 508, None, 0), (90, 514, None, 0), (90, 512, D(np.zeros(2, dtype=np.int32)), 0)):
        _adain_launch(x, gb, 0, stride, 2, n, 1, idx, rows, 1 << 30, expect=pr.INVALID_VALUE)


# =================================================================================================== GPU: embed front, embed sums, window sums
VC = ((22, 15), (24, 15), (25, 15), (32, 15), (32, 16), (6, 3))
NORMS = ("none", "zscore", "rawroot")
MAXWIN = 35


def _embed_inputs(name, V, Cin, norm, frames):
    r = rng(name)
    raw = 1 if norm == "rawroot" else 0
    d = dict(X=normal(r, frames, V + raw, Cin), W1=normal(r, 64, Cin) / np.float32(np.sqrt(Cin)), b1=normal(r, 64), AP=normal(r, 3, V, 6) / np.float32(np.sqrt(V)),
             xmean=None if norm == "none" else normal(r, (V + raw) * Cin), xstd=None if norm == "none" else r.uniform(0.5, 2.0, (V + raw) * Cin).astype(np.float32))
    return d, raw


def _embed_ref(d, raw, frames):
    t = {k: (None if v is None else T(v)) for k, v in d.items()}
    return both(pr.embed_front, t["X"][:frames], t["W1"], t["b1"], t["AP"], t["xmean"], t["xstd"], raw)


def _embed_front_launch(dd, frames, V, Cin, raw, planes, max_wgs=512, expect=0):
    out = Out((frames, 6, 192))
    torch.cuda.synchronize()
    rc = pr.load().pw_embed_front(pr.ptr(dd["X"]), pr.ptr(dd["W1"]), pr.ptr(dd["b1"]), pr.ptr(dd["AP"]), out.ptr, frames, V, Cin, pr.ptr(dd["xmean"]),
                                  pr.ptr(dd["xstd"]), raw, planes, max_wgs, 0)
    torch.cuda.synchronize()
    assert rc == expect, (rc, expect)
    if expect:
        assert out.intact()
        return None
    return out.check("embed_front")


@gpu
@pytest.mark.parametrize("norm", NORMS)
@pytest.mark.parametrize("V,Cin", VC)
def test_embed_front(V, Cin, norm):
    case = f"V{V}-C{Cin}-{norm}"
    d, raw = _embed_inputs("embed-" + case, V, Cin, norm, 60)
    dd = {k: D(v) for k, v in d.items()}
    ref64, ref32 = _embed_ref(d, raw, 60)
    for frames in (1, 5, 60):
        for planes in (0, 1):
            y = _embed_front_launch(dd, frames, V, Cin, raw, planes)
            hold("embed_front_x3" if planes else "embed_front", f"{case} f{frames}", y, ref64[:frames], ref32[:frames])
    # every wave takes several frames and the last round is partial: 21 frames over 2 workgroups of 4 waves - same bits as one frame per wave
    y2 = _embed_front_launch(dd, 21, V, Cin, raw, 1, max_wgs=2)
    hold("embed_front_x3", f"{case} f21 wgs2", y2, ref64[:21], ref32[:21])
    assert same_bits(y2, _embed_front_launch(dd, 21, V, Cin, raw, 1)), (case, "max_wgs changes the result")


@gpu
def test_embed_front_grid_stride():
    """8 195 frames: the smallest count at which the exact-f32 build's 2 048 workgroups of 4 waves take a second frame (three of them)."""
    V, Cin, frames = 22, 15, 8195
    d, raw = _embed_inputs("embed-stride", V, Cin, "rawroot", frames)
    dd = {k: D(v) for k, v in d.items()}
    ref64, ref32 = _embed_ref(d, raw, frames)
    y = _embed_front_launch(dd, frames, V, Cin, raw, 0)
    hold("embed_front", "V22-C15-rawroot f8195", y, ref64, ref32)
    hold("embed_front", "V22-C15-rawroot f8195 tail", y[8192:], ref64[8192:], ref32[8192:])


def _window_sums_launch(y, B, C, expect=0, rows=None):
    u = Out((B, 15, 6, 5 * C))
    torch.cuda.synchronize()
    rc = pr.load().pw_window_sums(pr.ptr(y), u.ptr, B * 90 if rows is None else rows, C, 0)
    torch.cuda.synchronize()
    assert rc == expect, (rc, expect)
    if expect:
        assert u.intact()
        return None
    return u.check("window_sums")


@gpu
@pytest.mark.parametrize("norm", NORMS)
@pytest.mark.parametrize("V,Cin", VC)
def test_embed_sums(V, Cin, norm):
    case = f"V{V}-C{Cin}-{norm}"
    d, raw = _embed_inputs("esums-" + case, V, Cin, norm, MAXWIN * 60)
    dd = {k: D(v) for k, v in d.items()}
    f64, f32 = _embed_ref(d, raw, MAXWIN * 60)
    ref64, ref32 = (pr.window_sums(f.reshape(MAXWIN, 60, 6, 192)) for f in (f64, f32))
    for nwin, wgs in ((1, 512), (2, 512), (3, 7), (2, 1), (35, 512)):
        res = []
        for reverse in (0, 1):
            u = Out((nwin, 15, 6, 960))
            torch.cuda.synchronize()
            rc = pr.load().pw_embed_sums(pr.ptr(dd["X"]), pr.ptr(dd["W1"]), pr.ptr(dd["b1"]), pr.ptr(dd["AP"]), u.ptr, nwin, V, Cin, pr.ptr(dd["xmean"]),
                                         pr.ptr(dd["xstd"]), raw, wgs, reverse, 0)
            torch.cuda.synchronize()
            assert rc == 0, rc
            res.append(u.check("embed_sums"))
        assert same_bits(res[0], res[1]), (case, nwin, wgs, "reverse")
        hold("embed_sums", f"{case} w{nwin} wgs{wgs}", res[0], ref64[:nwin], ref32[:nwin])
        ends = [0, 14]                                                      # the pooled frames whose taps are reflected
        hold("embed_sums", f"{case} w{nwin} wgs{wgs} reflected", res[0][:, ends], ref64[:nwin, ends], ref32[:nwin, ends])
        # (b) the same additions in the same order as window_sums on the plane front end's frames
        fr = _embed_front_launch(dd, nwin * 60, V, Cin, raw, 1)
        two = _window_sums_launch(D(fr), nwin, 192)
        assert same_bits(res[0], two), (case, nwin, wgs, "embed_sums != window_sums(embed_front)")


@gpu
@pytest.mark.parametrize("B", (1, 2, 5))
@pytest.mark.parametrize("C", (256, 192))
def test_window_sums(C, B):
    y = normal(rng(f"wsums-{C}-{B}"), B, 60, 6, C) + np.float32(0.5)
    ref64, ref32 = both(pr.window_sums, T(y))
    hold("window_sums", f"C{C}-B{B}", _window_sums_launch(D(y), B, C), ref64, ref32)


@gpu
def test_embed_and_window_sums_refusals():
    d, raw = _embed_inputs("embed-refuse", 33, 17, "zscore", 60)
    dd = {k: D(v) for k, v in d.items()}
    for V, Cin in ((33, 15), (22, 17), (27, 19), (33, 17)):
        _embed_front_launch(dd, 4, V, Cin, raw, 0, expect=pr.INVALID_VALUE)
        _embed_front_launch(dd, 4, V, Cin, raw, 1, expect=pr.INVALID_VALUE)
        u = Out((1, 15, 6, 960))
        rc = pr.load().pw_embed_sums(pr.ptr(dd["X"]), pr.ptr(dd["W1"]), pr.ptr(dd["b1"]), pr.ptr(dd["AP"]), u.ptr, 1, V, Cin, pr.ptr(dd["xmean"]), pr.ptr(dd["xstd"]), raw, 512, 0, 0)
        assert rc == pr.INVALID_VALUE and u.intact()
    assert 27 * 19 == 513
    y = D(normal(rng("ws-refuse"), 2, 60, 6, 256))
    _window_sums_launch(y, 2, 256, expect=pr.INVALID_VALUE, rows=91)
    _window_sums_launch(y, 2, 128, expect=pr.INVALID_VALUE)


# =================================================================================================== GPU: body front, joint expand, final projection
def _simple(fn, outshape, *args):
    out = Out(outshape)
    torch.cuda.synchronize()
    rc = fn(out.ptr, *args)
    torch.cuda.synchronize()
    return rc, out


@gpu
@pytest.mark.parametrize("frames", (1, 3, 4, 5, 15, 30))
def test_body_front(frames):
    r = rng(f"body-{frames}")
    x, Ab = normal(r, frames, 6, 256), normal(r, 2, 6, 6) / np.float32(np.sqrt(6))
    ref64, ref32 = both(pr.body_front, T(x), T(Ab))
    dx, dA = D(x), D(Ab)
    res = []
    for reverse in (0, 1):
        rc, out = _simple(lambda o: pr.load().pw_body_front(pr.ptr(dx), pr.ptr(dA), o, frames, reverse, 0), (frames, 6, 512))
        assert rc == 0
        res.append(out.check("body_front"))
    hold("body_front", f"f{frames}", res[0], ref64, ref32)
    assert same_bits(res[0], res[1]), "reverse"


@gpu
@pytest.mark.parametrize("frames", (1, 4, 15, 17))
@pytest.mark.parametrize("V", (22, 24, 1, 21, 25, 32))
def test_joint_expand(V, frames):
    r = rng(f"jexp-{V}-{frames}")
    g, AU = normal(r, frames, 6, 192), normal(r, 3, 6, V) / np.float32(np.sqrt(18))
    ref64, ref32 = both(pr.joint_expand, T(g), T(AU))
    dg, dA = D(g), D(AU)
    res = []
    for reverse in (0, 1):
        rc, out = _simple(lambda o: pr.load().pw_joint_expand(pr.ptr(dg), pr.ptr(dA), o, frames, V, reverse, 0), (frames, V, 64))
        assert rc == 0
        res.append(out.check("joint_expand"))
    hold("joint_expand", f"V{V}-f{frames}", res[0], ref64, ref32)
    assert same_bits(res[0], res[1]), "reverse"


@gpu
def test_joint_expand_and_final_proj_refusals():
    g, AU = D(normal(rng("jr"), 4, 6, 192)), D(normal(rng("ja"), 3, 6, 33))
    rc, out = _simple(lambda o: pr.load().pw_joint_expand(pr.ptr(g), pr.ptr(AU), o, 4, 33, 0, 0), (4, 33, 64))
    assert rc == pr.INVALID_VALUE and out.intact()
    z, W, b = D(normal(rng("fz"), 10, 64)), D(normal(rng("fw"), 17, 64)), D(normal(rng("fb"), 17))
    rc, out = _simple(lambda o: pr.load().pw_final_proj(pr.ptr(z), pr.ptr(W), pr.ptr(b), o, 10, 17, 22, 0, 0, 0, 0, 0), (10, 17))
    assert rc == pr.INVALID_VALUE and out.intact()


def _final_proj_case(case, z, rows, V, Cout, denorm, phased):
    r = rng("fproj-" + case)
    W6, b6 = normal(r, Cout, 64) / np.float32(8), normal(r, Cout)
    ym = ys = None
    if denorm:                                                              # the root row would make a wrong offset an O(1) .. O(1000) error
        ym, ys = normal(r, V + 1, Cout), r.uniform(0.5, 2.0, (V + 1, Cout)).astype(np.float32)
        ym[0], ys[0] = 1000.0, 100.0
    t = [None if a is None else T(a) for a in (z, W6, b6, ym, ys)]
    ref64, ref32 = both(pr.final_proj, t[0], t[1], t[2], V, t[3], t[4], phased=phased)
    dz, dW, db, dm, dsd = (D(a) for a in (z, W6, b6, ym, ys))
    res = []
    for reverse in (0, 1):
        rc, out = _simple(lambda o: pr.load().pw_final_proj(pr.ptr(dz), pr.ptr(dW), pr.ptr(db), o, rows, Cout, V, pr.ptr(dm), pr.ptr(dsd), int(phased), reverse, 0), (rows, Cout))
        assert rc == 0, rc
        res.append(out.check("final_proj"))
    hold("final_proj", case, res[0], ref64, ref32)
    assert same_bits(res[0], res[1]), (case, "reverse")


@gpu
@pytest.mark.parametrize("denorm", (0, 1))
@pytest.mark.parametrize("Cout", (3, 15, 16))
def test_final_proj(Cout, denorm):
    for rows in (1, 127, 128, 129, 1320):
        case = f"rows{rows}-C{Cout}-d{denorm}"
        _final_proj_case(case, normal(rng("fz-" + case), rows, 64), rows, 22, Cout, denorm, False)
    for wins, V in itertools.product((1, 2), (22, 24)):
        case = f"phased-w{wins}-V{V}-C{Cout}-d{denorm}"
        _final_proj_case(case, normal(rng("fz-" + case), wins, 15, V, 256), wins * 60 * V, V, Cout, denorm, True)


# =================================================================================================== GPU: float64 linear
def _linear_cases():
    out = []
    nk = list(itertools.product((7, 33, 512, 1024), (32, 256, 512)))
    for mi, M in enumerate((1, 16, 17, 33)):
        for i, (N, K) in enumerate(nk):
            j = i + mi
            out.append(dict(M=M, N=N, K=K, lmode=("L1", "L2", "L2x0")[j % 3], act=(0, 2)[(j // 3) % 2], outs=("both", "y64", "y32")[(j + j // 3) % 3]))
    for act in (0, 2):
        out.append(dict(M=961, N=1024, K=32, lmode="L2", act=act, outs="both"))
    return out


LINEAR = _linear_cases()


def _linear_launch(c, X, W, bias, ldx, xcol, L, outs, act=None, K=None, expect=0):
    M, N = c["M"], c["N"]
    ldy = L * N + 3
    wr = np.zeros((M, ldy), dtype=bool)
    wr[:, :L * N] = True
    y64 = Out((M, ldy), "f64", wr) if outs in ("both", "y64") else None
    y32 = Out((M, ldy), "f32", wr) if outs in ("both", "y32") else None
    torch.cuda.synchronize()
    rc = pr.load().pw_linear_f64(pr.ptr(X), ldx, xcol, pr.ptr(W), pr.ptr(bias), y64.ptr if y64 else 0, y32.ptr if y32 else 0, ldy, M, N,
                                 c["K"] if K is None else K, L, c["act"] if act is None else act, 0)
    torch.cuda.synchronize()
    assert rc == expect, (c, rc, expect)
    if expect:
        assert all(o.intact() for o in (y64, y32) if o)
        return None, None
    return (y64.check("linear y64")[:, :L * N] if y64 else None), (y32.check("linear y32")[:, :L * N] if y32 else None)


def test_linear_case_table_reaches_every_instance():
    """Host arithmetic only: the rows kernel (M <= 16), 32 x 32 tiles (fewer than 512 tiles of 64 x 64) and 64 x 64 tiles, each with both
    activations, every N, K, block mode and output mode."""
    def inst(c):
        L = 1 if c["lmode"] == "L1" else 2
        return "rows" if c["M"] <= 16 else "t32" if ((c["N"] + 63) // 64) * ((c["M"] + 63) // 64) * L < 512 else "t64"
    got = {(inst(c), c["act"]) for c in LINEAR}
    assert got == {(i, a) for i in ("rows", "t32", "t64") for a in (0, 2)}
    for i in ("rows", "t32"):
        mine = [c for c in LINEAR if inst(c) == i]
        assert {c["N"] for c in mine} == {7, 33, 512, 1024} and {c["K"] for c in mine} == {32, 256, 512}
        assert {c["lmode"] for c in mine} == {"L1", "L2", "L2x0"} and {c["outs"] for c in mine} == {"both", "y64", "y32"}


@gpu
@pytest.mark.parametrize("c", LINEAR, ids=[f"M{c['M']}-N{c['N']}-K{c['K']}-{c['lmode']}-act{c['act']}-{c['outs']}" for c in LINEAR])
def test_linear_f64(c):
    M, N, K = c["M"], c["N"], c["K"]
    L = 1 if c["lmode"] == "L1" else 2
    xcol = 0 if c["lmode"] == "L2x0" else K
    ldx = (L - 1) * xcol + K + 2                                            # wider than the columns read; even (16-byte row loads)
    r = rng("lin-%s" % sorted(c.items()))
    X, W, bias = r.standard_normal((M, ldx)), r.standard_normal((L * N, K)) / np.sqrt(K), r.standard_normal(L * N)
    ref, mag = pr.linear_f64(X, W, bias, N, K, L, xcol, c["act"])
    bound = K * 2.0 ** -53 * mag                                            # derived: K fused multiply-adds per element, each rounding <= 2^-53 of the running sum <= sum |x||w|
    dX, dW, db = D(X), D(W), D(bias)
    y64, y32 = _linear_launch(c, dX, dW, db, ldx, xcol, L, "both")
    err = np.abs(y64.astype(np.longdouble) - ref).astype(np.float64)
    print(f"[pointwise] linear_f64     {str(c):80s} worst error / bound {float((err / bound).max()):.3f}")
    assert np.all(err <= bound), (c, float((err / bound).max()))
    assert same_bits(y32, y64.astype(np.float32)), (c, "y32 is not y64 rounded once")
    if c["outs"] != "both":                                                 # the other output null: the same bits
        a, b = _linear_launch(c, dX, dW, db, ldx, xcol, L, c["outs"])
        assert same_bits(a, y64) if a is not None else same_bits(b, y32), (c, "an output depends on the other")
    nb, _ = pr.linear_f64(X, W, None, N, K, L, xcol, c["act"])              # no bias
    z64, _ = _linear_launch(c, dX, dW, None, ldx, xcol, L, "y64")
    assert np.all(np.abs(z64.astype(np.longdouble) - nb).astype(np.float64) <= bound), (c, "no bias")


@gpu
def test_linear_f64_refusals():
    c = dict(M=4, N=8, K=64, act=0)
    X, W = D(np.zeros((4, 70))), D(np.zeros((8, 64)))
    _linear_launch(c, X, W, None, 66, 0, 1, "both", K=48, expect=pr.INVALID_VALUE)
    _linear_launch(c, X, W, None, 66, 0, 1, "both", K=16, expect=pr.INVALID_VALUE)
    _linear_launch(c, X, W, None, 67, 0, 1, "both", expect=pr.INVALID_VALUE)
    _linear_launch(c, X, W, None, 66, 0, 1, "both", act=1, expect=pr.INVALID_VALUE)
    assert pr.load().pw_linear_f64(pr.ptr(X), 66, 0, pr.ptr(W), 0, 0, 0, 16, 4, 8, 64, 1, 0, 0) == pr.INVALID_VALUE


# =================================================================================================== GPU: bank utilities
@gpu
def test_rownorm2():
    """One squared norm per row: a case has 1 or 5 outputs, too few for an rms, so the cases are pooled - each row's norm divided by its
    number of columns (in float64, on both sides) - and held together; each case's guards and its reverse launch are checked on its own."""
    got, r64, r32 = [], [], []
    for cols, rows in itertools.product((4, 1020, 1024, 1028, 23040), (1, 5)):
        r = rng(f"rn2-{cols}-{rows}")
        x, sub = normal(r, rows, cols) + np.float32(0.5), normal(r, cols)
        dx, ds = D(x), D(sub)
        for s in (None, sub):
            ref64, ref32 = both(lambda a, b: ((a - b) ** 2).sum(1) if b is not None else (a ** 2).sum(1), T(x), None if s is None else T(s))
            res = []
            for reverse in (0, 1):
                rc, out = _simple(lambda o: pr.load().pw_rownorm2(pr.ptr(dx), pr.ptr(ds) if s is not None else 0, o, rows, cols, reverse, 0), (rows,))
                assert rc == 0
                res.append(out.check("rownorm2"))
            assert same_bits(res[0], res[1]), (cols, rows, "reverse")
            e, b = float(np.abs(res[0] - ref64.numpy()).max()), float((ref32.double() - ref64).abs().max())
            print(f"[pointwise] rownorm2       c{cols}-r{rows}-{'sub' if s is not None else 'plain'}: error {e:.3e}, fp32 cpu {b:.3e}, ulp {pr.ulp_of_largest(ref64):.2e}")
            got.append(res[0].astype(np.float64) / cols), r64.append(ref64 / cols), r32.append(ref32.double() / cols)
    hold("rownorm2", "all cases, per column", np.concatenate(got), torch.cat(r64), torch.cat(r32))


@gpu
def test_sub_rows_is_numpy_fp32():
    r = rng("subrows")
    for rows, cols in ((3, 1028), (1, 4), (7, 23040)):                     # 771 float4: not a multiple of the 256 a workgroup takes
        x, sub = normal(r, rows, cols), normal(r, cols)
        dx, ds = D(x), D(sub)
        rc, out = _simple(lambda o: pr.load().pw_sub_rows(pr.ptr(dx), pr.ptr(ds), o, rows, cols, 0), (rows, cols))
        assert rc == 0 and same_bits(out.check("sub_rows"), x - sub[None])
    rc, out = _simple(lambda o: pr.load().pw_sub_rows(pr.ptr(dx), pr.ptr(ds), o, 2, 6, 0), (2, 6))
    assert rc == pr.INVALID_VALUE and out.intact()


def _center_rows(dx, dc, rows, cols, mode, reverse=0, expect=0, qstat=True, nplanes=None, both_outputs=False):
    planes = Out((2 if mode == "p2" else 1, rows, cols), "u16") if mode in ("p1", "p2") or both_outputs else None
    o32 = Out((rows, cols)) if mode == "f32" or both_outputs else None
    qs = Out((rows, pr.QSTAT_PARTS, 2)) if qstat else None
    torch.cuda.synchronize()
    rc = pr.load().pw_center_rows(pr.ptr(dx), pr.ptr(dc), planes.ptr if planes else 0, nplanes if nplanes is not None else (2 if mode == "p2" else 1),
                                  o32.ptr if o32 else 0, qs.ptr if qs else 0, rows, cols, reverse, 0)
    torch.cuda.synchronize()
    assert rc == expect, (mode, rc, expect)
    if expect:
        assert all(o.intact() for o in (planes, o32, qs) if o)
        return None
    return (planes.check("center_rows planes") if planes else None), (o32.check("center_rows out32") if o32 else None), qs.check("center_rows qstat")


@gpu
@pytest.mark.parametrize("cols", (4, 2048, 2052, 23040))
def test_center_rows(cols):
    rows = 5
    r = rng(f"crows-{cols}")
    x, c = normal(r, rows, cols) * np.float32(3), normal(r, cols)
    dx, dc = D(x), D(c)
    z = (x - c[None]).astype(np.float32)
    for mode in ("f32", "p1", "p2"):
        planes, o32, qs = _center_rows(dx, dc, rows, cols, mode)
        left = np.zeros_like(z)
        if mode == "f32":
            assert same_bits(o32, z), (cols, "out32 != x - centre")
        else:
            chain = pr.plane_chain(z, 2)
            assert np.array_equal(planes[0], chain[0]), (cols, mode, "plane 0")
            left = (z - pr.bf16_value(chain[0])).astype(np.float32)
            if mode == "p2":
                assert np.array_equal(planes[1], chain[1]), (cols, mode, "plane 1")
                left = (left - pr.bf16_value(chain[1])).astype(np.float32)
        assert np.all(qs[:, 1:] == 0.0), (cols, mode, "qstat parts 1..3")
        t = np.stack([z.astype(np.float64) ** 2, left.astype(np.float64) ** 2], 1)        # (rows, 2, cols)
        tol = 4 * _fp32_sum_error(T(t)) + float(np.spacing(np.float32(t.sum(-1).max())))
        e = float(np.abs(qs[:, 0].astype(np.float64) - t.sum(-1)).max())
        print(f"[pointwise] center_rows    c{cols}-{mode:4s} qstat error {e:.3e} bound {tol:.3e} (relative {e / float(t.sum(-1).max()):.2e})")
        assert e <= tol, (cols, mode, e, tol)
        rev = _center_rows(dx, dc, rows, cols, mode, reverse=1)
        for a, b in zip((planes, o32, qs), rev):
            assert a is None or same_bits(a, b), (cols, mode, "reverse")


@gpu
def test_center_rows_refusals():
    x, c = D(normal(rng("cr-r"), 2, 8)), D(normal(rng("cr-c"), 8))
    bad = pr.INVALID_VALUE
    _center_rows(x, c, 2, 8, "f32", both_outputs=True, expect=bad)
    qs = Out((2, pr.QSTAT_PARTS, 2))
    assert pr.load().pw_center_rows(pr.ptr(x), pr.ptr(c), 0, 1, 0, qs.ptr, 2, 8, 0, 0) == bad and qs.intact()      # neither planes nor out32
    _center_rows(x, c, 2, 8, "p1", nplanes=3, expect=bad)
    _center_rows(x, c, 2, 8, "p1", qstat=False, expect=bad)
    _center_rows(x, c, 2, 6, "f32", expect=bad)                             # cols not a multiple of 4


@gpu
@pytest.mark.parametrize("cols", (64, 23040))
def test_column_mean_and_stats(cols):
    """Held to the float64 result rounded to fp32, within ONE fp32 ulp.  Derived: the kernels accumulate in float64 (relative error
    <= N 2^-53, far below half an fp32 ulp, 2^-24), so only the final rounding to fp32 can differ from the reference's.  The data
    carries a per-column offset 1e3 times its spread: an fp32 accumulation would lose three digits of the std and fail."""
    r = rng(f"cstats-{cols}")
    spread = r.uniform(0.1, 3.0, cols).astype(np.float32)
    full = (normal(r, 1000, cols) + np.float32(1e3) * np.sign(normal(r, cols))) * spread
    dfull = D(full)
    nd = pr.load().pw_column_mean_scratch_doubles(cols)
    assert nd >= cols
    for N in (1, 3, 4, 5, 17, 1000):
        x64 = full[:N].astype(np.float64)
        m64, s64 = x64.mean(0), x64.std(0)

        def within_one_ulp(got, want, what):
            w32 = want.astype(np.float32)
            ok = np.abs(got.astype(np.float64) - w32.astype(np.float64)) <= np.spacing(np.abs(w32)).astype(np.float64)
            assert np.all(ok), (cols, N, what, int((~ok).sum()))
        scratch = Out((nd,), "f64")
        rc, mean = _simple(lambda o: pr.load().pw_column_mean(pr.ptr(dfull), N, cols, o, scratch.ptr, nd, 0), (cols,))
        assert rc == 0
        within_one_ulp(mean.check("column_mean"), m64, "column_mean")
        assert bool((scratch.buf[:GUARD] == SENTINEL).all()) and bool((scratch.buf[GUARD + scratch.words:] == SENTINEL).all())
        sd = Out((cols,))
        rc, mean = _simple(lambda o: pr.load().pw_column_stats(pr.ptr(dfull), N, cols, o, sd.ptr, 0), (cols,))
        assert rc == 0
        within_one_ulp(mean.check("column_stats mean"), m64, "column_stats mean")
        within_one_ulp(sd.check("column_stats sd"), s64, "column_stats sd")
        rc, mean = _simple(lambda o: pr.load().pw_column_stats(pr.ptr(dfull), N, cols, o, 0, 0), (cols,))      # sd null: the mean-only path
        assert rc == 0
        within_one_ulp(mean.check("column_stats mean only"), m64, "column_stats mean only")
    rc, mean = _simple(lambda o: pr.load().pw_column_stats(pr.ptr(dfull), 4, 65, o, 0, 0), (65,))
    assert rc == pr.INVALID_VALUE and mean.intact()


# =================================================================================================== GPU: absmax
ABSMAX = ((1, 1), (3, 5), (3, 4099), (1, 8193), (2, 12291))


@gpu
@pytest.mark.parametrize("nwin,per", ABSMAX)
def test_absmax(nwin, per):
    """out[w] = max(prefill, mul * max|window w| + add), within one fp32 ulp of the float64 evaluation (derived: max is exact, the
    multiply-add rounds once).  A window of few windows is cut into slices of at least 4 096 floats: per // 4096 of them."""
    r = rng(f"absmax-{nwin}-{per}")
    slices = max(1, per // 4096)
    cuts = [per * k // slices for k in range(1, slices)]
    plant = sorted({0, per - 1} | {c - 1 for c in cuts} | set(cuts))
    for off, (mul, add) in itertools.product((0, 1, 2, 3), ((1.0, 0.0), (1.5, 0.25))):
        for pos in plant:
            x = r.uniform(-1, 1, nwin * per + 8).astype(np.float32)
            x[:off] = 50.0                                                  # in front of the first window and behind the last: not part of any
            x[off + nwin * per:] = 50.0
            for w in range(nwin):
                x[off + w * per + pos] = (3.0 + w) * (-1.0) ** w
            dx = D(x)
            pre = np.zeros(nwin, dtype=np.float32)
            if nwin > 1 or off & 1:                                         # above the result: it stays (a single window: every other launch)
                pre[nwin - 1] = 100.0
            out = Out((nwin,))
            out.body.copy_(T(pre).view(torch.int32).to(dev()))
            torch.cuda.synchronize()
            rc = pr.load().pw_absmax(dx.data_ptr() + 4 * off, nwin, per, out.ptr, mul, add, 0)
            torch.cuda.synchronize()
            assert rc == 0
            host = out.buf.cpu()
            assert bool((host[:GUARD] == SENTINEL).all()) and bool((host[GUARD + out.words:] == SENTINEL).all())
            got = host[GUARD:GUARD + nwin].numpy().view(np.float32)
            m = np.abs(x[off:off + nwin * per].astype(np.float64)).reshape(nwin, per).max(1)
            assert np.array_equal(m, 3.0 + np.arange(nwin)), "the planted value is the largest"
            want = np.maximum(pre.astype(np.float64), np.float64(np.float32(mul)) * m + np.float64(np.float32(add)))
            assert np.all(np.abs(got.astype(np.float64) - want) <= np.spacing(want.astype(np.float32)).astype(np.float64)), (nwin, per, off, pos, got, want)


@gpu
def test_absmax_refusals():
    x = D(np.ones(65536 + 8, dtype=np.float32))
    for nwin, mul, add in ((4, 0.0, 0.0), (4, 1.0, -0.5), (65536, 1.0, 0.0)):
        out = Out((nwin,))
        rc = pr.load().pw_absmax(pr.ptr(x), nwin, 1, out.ptr, mul, add, 0)
        torch.cuda.synchronize()
        assert rc == pr.INVALID_VALUE and out.intact(), (nwin, mul, add, rc)
