"""The grouped GEMM at the kernel boundary (mocha_linear_grouped -> mocha_gemm_grouped, cvae_grouped.hip): G groups of m rows, group g on
the weights of slot which[g] of a bank of Cw = 3 slots, against float64 on the CPU - every group with its own slot's weights.

Cases: m in {1, 15, 16, 17, 90, 181, 182} (one row, one row short of a tile, a tile, one row more, the sampler's three sizes: 5 tiles + 10
rows, 11 tiles + 5 / 6 rows) x (N, K) in {(256, 256), (768, 256), (512, 256), (256, 512), (16, 16)} (the sampler's four shapes and the
smallest launch: one column tile, ONE k group, so three of the four waves have no work) x the epilogues none / bias / bias + ReLU /
bias + residual with ldr > N; G = 3 with which = [2, 0, 2] (repeated, not ascending) and G = 1.

(a) accuracy: the rule of tests/test_gemm_instances.py - error <= 4 x (largest) and 1.5 x (rms) of the same product in fp32 by torch on the
    CPU, plus one fp32 ulp of the largest output on the largest error.  The kernel cuts K four ways (one chain per wave of at most
    K / 4 products, two alternating accumulators), so it is held to the BLAS figure alone, as that file holds the skinny tiers.
    Inputs unit normal, weights scaled by 1 / sqrt(K): a wrong slot, row or column is an error of order 1.
(b) invalid groups - which = -1, which = Cw, an unstored slot - are zeros, and a valid group beside them keeps its bits.
(c) stores: guard words (0xA5A5A5A5) before and after y and, with ldc > N, between the rows stay bit-intact; every element of y is written.
(d) to the bit: a group alone (G = 1) equals the same group at position 0 and at position 2 of G = 3 beside other slots; run to run.
(e) refusals: N % 16, K % 16, m < 1, ldc < N, NULL pointers -> MOCHA_ERR_ARG, nothing written.

Mutations (scratch builds, each run once against this file):
  which[0] for which[g] in mocha_gemm_grouped                         -> every G = 3 case fails (a) (group 1 computed with slot 2)
  row tiles cut across the whole G * m instead of per group           -> the m in {15, 17, 90, 181, 182} cases fail (a); m = 1 and m = 16 pass
(recorded in the pull request's summary with the observed counts)."""
import ctypes as C

import numpy as np
import pytest
import torch

import mocha_sigasia2023_amd as M

pytestmark = pytest.mark.gpu

ERR_ARG = -1
CW = 3
MS = (1, 15, 16, 17, 90, 181, 182)
SHAPES = ((256, 256), (768, 256), (512, 256), (256, 512), (16, 16))
EPILOGUES = ("none", "bias", "bias_relu", "bias_res")
MARGIN_MAX, MARGIN_RMS = 4.0, 1.5
GUARD = np.uint32(0xA5A5A5A5).view(np.int32).item()
PAD = 64                                                                    # guard words in front of and behind y


@pytest.fixture(scope="module")
def ctx():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    g = M.Generator(device="cuda:0")
    return g._ctx


def _data(m, N, K, G=3):
    rng = np.random.Generator(np.random.PCG64(1000 * m + N + K))
    return dict(x=torch.from_numpy(rng.standard_normal((G, m, K)).astype(np.float32)),
                w=torch.from_numpy((rng.standard_normal((CW, N, K)) / np.sqrt(K)).astype(np.float32)),
                b=torch.from_numpy(rng.standard_normal((CW, N)).astype(np.float32)),
                r=torch.from_numpy(rng.standard_normal((G, m, N + 12)).astype(np.float32)))


def _reference(d, which, epi, dtype):
    out = []
    for g, slot in enumerate(which):
        y = d["x"][g].to(dtype) @ d["w"][slot].to(dtype).T
        if epi != "none":
            y = y + d["b"][slot].to(dtype)
        if epi == "bias_relu":
            y = torch.relu(y)
        if epi == "bias_res":
            y = y + d["r"][g][:, :y.shape[1]].to(dtype)
        out.append(y)
    return torch.stack(out)


def _launch(ctx, x, w, b, r, which, stored, epi, ldc, check=True):
    """x (G,m,K), r (G,m,ldr) on the CPU -> (rc, y (G,m,N), guards intact and every element written)."""
    dev = torch.device("cuda:0")
    G, m, K = x.shape
    N = w.shape[1]
    xd, wd, bd, rd = x.contiguous().to(dev), w.to(dev), b.to(dev), r.contiguous().to(dev)
    wh = torch.tensor(list(which), dtype=torch.int32, device=dev)
    st = torch.tensor(list(stored), dtype=torch.int32, device=dev)
    buf = torch.full((2 * PAD + G * m * ldc,), GUARD, dtype=torch.int32, device=dev)
    y = buf[PAD:]
    p = lambda t: C.c_void_p(t.data_ptr())                                   # noqa: E731
    rc = ctx.lib.mocha_linear_grouped(ctx.h, p(xd), p(wd), p(bd) if epi != "none" else None, p(wh), p(st), p(y), ldc, G, m, N, K, CW,
                                      3 if epi == "bias_relu" else 0, p(rd) if epi == "bias_res" else None, r.shape[2] if epi == "bias_res" else 0,
                                      C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    body = buf[PAD:PAD + G * m * ldc].reshape(G * m, ldc)
    out = body[:, :N].contiguous().view(torch.float32).reshape(G, m, N).cpu()
    ok = bool((buf[:PAD] == GUARD).all()) and bool((buf[PAD + G * m * ldc:] == GUARD).all()) and bool((body[:, N:] == GUARD).all())
    if check and rc == 0:
        ok = ok and bool((body[:, :N] != GUARD).all())
    return rc, out, ok


def _err(y, ref64):
    d = y.double() - ref64
    return float(d.abs().max()), float(d.pow(2).mean().sqrt())


@pytest.mark.parametrize("N,K", SHAPES, ids=[f"n{n}k{k}" for n, k in SHAPES])
@pytest.mark.parametrize("m", MS)
def test_grouped_gemm(ctx, m, N, K):
    d = _data(m, N, K)
    which, all_stored = [2, 0, 2], [1, 1, 1]
    for e, epi in enumerate(EPILOGUES):
        ldc = N + 8 if e % 2 else N                                        # guard words between the rows on every other epilogue
        ref64 = _reference(d, which, epi, torch.float64)
        e_blas = _err(_reference(d, which, epi, torch.float32), ref64)
        ulp = float(np.spacing(np.float32(ref64.abs().max())))
        rc, y, ok = _launch(ctx, d["x"], d["w"], d["b"], d["r"], which, all_stored, epi, ldc)
        assert rc == 0, (epi, rc, ctx.lib.mocha_last_error(ctx.h))
        assert ok, f"{epi}: a guard word was overwritten or an element of y was not written"                               # (c)
        emax, erms = _err(y, ref64)
        print(f"[linear-grouped] m {m:3d} n{N} k{K} {epi:9s} max {emax:.3e} ({emax / max(e_blas[0], 1e-30):5.2f} x fp32 cpu) "
              f"rms {erms:.3e} ({erms / max(e_blas[1], 1e-30):5.2f} x)  ulp {ulp:.2e}")
        assert emax <= MARGIN_MAX * e_blas[0] + ulp and erms <= MARGIN_RMS * e_blas[1], (epi, (emax, erms), e_blas, ulp)     # (a)
        # (d) run to run; a group alone against its place in the batch: position 2 here, position 0 of the reversed batch beside slot 0
        rc2, y2, ok2 = _launch(ctx, d["x"], d["w"], d["b"], d["r"], which, all_stored, epi, ldc)
        assert rc2 == 0 and ok2 and torch.equal(y.view(torch.int32), y2.view(torch.int32)), (epi, "run to run")
        rc1, alone, ok1 = _launch(ctx, d["x"][2:3], d["w"], d["b"], d["r"][2:3], [2], all_stored, epi, ldc)
        assert rc1 == 0 and ok1 and torch.equal(alone[0].view(torch.int32), y[2].view(torch.int32)), (epi, "alone vs position 2")
        rev = torch.tensor([2, 1, 0])
        rc3, y3, ok3 = _launch(ctx, d["x"][rev], d["w"], d["b"], d["r"][rev], [2, 0, 2], all_stored, epi, ldc)
        assert rc3 == 0 and ok3 and torch.equal(alone[0].view(torch.int32), y3[0].view(torch.int32)), (epi, "alone vs position 0")
        # G = 1 against float64 on its own
        e1 = _err(alone[0], ref64[2])
        assert e1[0] <= MARGIN_MAX * e_blas[0] + ulp, (epi, "G = 1", e1, e_blas)
        # (b) which = -1, which = Cw, an unstored slot: zeros; the valid group beside them keeps the bits it has alone
        x4 = torch.cat([d["x"], d["x"][2:3]]); r4 = torch.cat([d["r"], d["r"][2:3]])
        rc4, y4, ok4 = _launch(ctx, x4, d["w"], d["b"], r4, [-1, CW, 1, 2], [1, 0, 1], epi, ldc)
        assert rc4 == 0 and ok4, (epi, "invalid groups")
        assert not y4[:3].view(torch.int32).any(), (epi, "an invalid group is not all zeros", float(y4[:3].abs().max()))
        assert torch.equal(y4[3].view(torch.int32), alone[0].view(torch.int32)), (epi, "a valid group beside invalid ones")


def test_refusals(ctx):
    d = _data(16, 32, 32)
    args = (d["x"], d["w"], d["b"], d["r"], [2, 0, 2], [1, 1, 1], "bias_res")
    rc, _, ok = _launch(ctx, *args, 32)
    assert rc == 0 and ok
    dev = torch.device("cuda:0")
    t = torch.zeros(4096, device=dev)
    wh = torch.zeros(4, dtype=torch.int32, device=dev)
    buf = torch.full((4096,), GUARD, dtype=torch.int32, device=dev)
    p = lambda a: C.c_void_p(a.data_ptr())                                   # noqa: E731
    good = dict(x=p(t), w=p(t), b=p(t), which=p(wh), stored=p(wh), y=p(buf), ldc=32, G=3, m=16, N=32, K=32, Cw=3, act=0, res=p(t), ldr=32)
    order = ["x", "w", "b", "which", "stored", "y", "ldc", "G", "m", "N", "K", "Cw", "act", "res", "ldr"]
    cases = [("N % 16", dict(N=24)), ("K % 16", dict(K=40)), ("m < 1", dict(m=0)), ("ldc < N", dict(ldc=16)), ("ldc % 4", dict(ldc=34)),
             ("ldr < N", dict(ldr=16)), ("act", dict(act=1)), ("Cw", dict(Cw=0)), ("G < 0", dict(G=-1)),
             ("x", dict(x=None)), ("w", dict(w=None)), ("which", dict(which=None)), ("stored", dict(stored=None)), ("y", dict(y=None))]
    for name, over in cases:
        a = dict(good, **over)
        assert ctx.lib.mocha_linear_grouped(ctx.h, *[a[k] for k in order], None) == ERR_ARG, name
    assert ctx.lib.mocha_linear_grouped(None, *[good[k] for k in order], None) == ERR_ARG
    torch.cuda.synchronize()
    assert bool((buf == GUARD).all())
    assert ctx.lib.mocha_linear_grouped(ctx.h, *[dict(good, G=0)[k] for k in order], None) == 0      # nothing to do
    torch.cuda.synchronize()
    assert bool((buf == GUARD).all())
