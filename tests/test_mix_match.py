"""mocha_match_mix_segmented through the C ABI on the MI355X (run with -m gpu): per window up to four (character, six body-part weights)
components, each matched in its own character, the weights normalised per part, the part-wise blend of the matched entries.

Three characters of 5, 17 and 33 rows - below, across and two past the scan's 16-row granule - as an fp32 bank, as a bf16 bank, and on a
resident bank between an empty (retired) slot and a never-filled one.  Q in {1, 3, 9} windows x J in {1, 2, 4} components; with Q = 9
every window's component 0 names the 33-row character (J = 4: component 2 as well), so that character has 9 / 18 pseudo-queries and a
second and third 8-query block open.  Ids: loaded characters, ids outside the table, empty slots, the same id twice in a window; weights:
random, with zeros, NaN, negatives and infinities sprinkled in, weightless components, and (Q >= 3) a window with nothing present.

Held: idx / dist = mocha_match_segmented for (that query, that id), bit for bit, -1 / +inf where the component is not present;
wnorm = tests/mix_ref.py in fp32, bit for bit; out = the torch composition in the kernel's order, bit for bit, and within (J + 1) 2^-23
sum_j |w_j e_j| of the float64 blend (J products and J sums of half an ulp each, doubled); guard words around every output intact."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mix_ref as R  # noqa: E402
from mocha_sigasia2023_amd import Generator, MultiCharacterBank, ResidentCharacterBank, weights  # noqa: E402

pytestmark = pytest.mark.gpu
D = 90 * 256
SIZES = (5, 17, 33)
GUARD = 16
NAN, INF = float("nan"), float("inf")


def dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return torch.device("cuda:0")


def vp(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


@pytest.fixture(scope="module")
def model():
    return Generator(layout="mixamo", device=dev()).load_state_dict(weights.synthetic_state_dict(1777, 1.0, "mixamo")).eval()


@pytest.fixture(scope="module")
def data():
    """Per character: rows (n, D) and encoded features (n, 90, 256), unrelated to the rows so that a wrong row shows in the blend; a pool
    of 9 queries, each a noisy copy of a row of one character (so its match there is known) and far from everything else."""
    g = torch.Generator(device="cpu"); g.manual_seed(20)
    rows = [torch.randn((n, D), generator=g) for n in SIZES]
    encs = [torch.randn((n, 90, 256), generator=g) for n in SIZES]
    near = [(2, 32), (1, 16), (0, 4), (2, 15), (1, 0), (2, 16), (0, 0), (1, 15), (2, 31)]          # (character, row): granule edges
    q = torch.stack([rows[c][r] + 0.05 * torch.randn((D,), generator=g) for c, r in near])
    d = dev()
    return dict(rows=[r.to(d) for r in rows], encs=[e.to(d) for e in encs], q=q.to(d), near=near)


def _bank(model, data, kind):
    """-> (bank object, id of each of the three characters, ids that name nothing, global first row of each character, encoded rows in
    bank order as the kernels gather them (row 0 first))."""
    pairs = list(zip(data["rows"], data["encs"]))
    if kind != "resident":
        mb = MultiCharacterBank(model, pairs, bf16=(kind == "bf16"), dec_cache=False)
        first = [mb.rows(c)[0] for c in range(3)]
        return mb, [0, 1, 2], [-1, 3, 1000, -2 ** 31], first, mb.encoded
    rb = ResidentCharacterBank(model, capacity_rows=160, max_characters=6, max_rows_per_character=48, dec_cache=False)
    big = rb.add(*pairs[2])                                # slot 0, rows 0 .. 32: bank row 0 stays a live character's
    gone = rb.add(data["rows"][1][:16].contiguous(), data["encs"][1][:16].contiguous())
    small = rb.add(*pairs[0])
    mid = rb.add(*pairs[1])
    rb.retire(gone)
    assert (big, gone, small, mid) == (0, 1, 2, 3)
    ids = [small, mid, big]
    first = [rb.rows(s)[0] for s in ids]
    assert first[2] == 0
    enc = torch.zeros((160, 90, 256), device=dev())
    for c in range(3):
        enc[first[c]: first[c] + SIZES[c]] = data["encs"][c]
    return rb, ids, [-1, gone, 4, 5, 6, 77], first, enc


def _problem(Q, J, cid, bad, seed):
    """ids (Q,J) and weights (Q,J,6) on the host."""
    r = np.random.default_rng(seed)
    pick = np.array(cid + bad)
    p = np.array([0.8 / len(cid)] * len(cid) + [0.2 / len(bad)] * len(bad))
    ids = r.choice(pick, size=(Q, J), p=p)
    w = r.random((Q, J, 6)).astype(np.float32) + np.float32(0.05)
    junk = np.array([0.0, -0.0, NAN, -1.5, INF, -INF], dtype=np.float32)
    hit = r.random((Q, J, 6)) < 0.2
    w[hit] = r.choice(junk, size=int(hit.sum()))
    if J >= 2:                                             # the same id twice in window 0, both usable
        ids[0, J - 1] = ids[0, 0] = cid[1]
        w[0, 0] = 0.3; w[0, J - 1] = 0.6
    if Q >= 3 and not (Q == 9 and J == 1):                 # nothing present in window 1: bad ids, or no usable weight
        ids[1] = bad[0]
        if J >= 2:
            ids[1, 1] = cid[0]
            w[1, 1] = 0.0
    if Q == 3 and J >= 2:                                  # a one-hot splice by body part in window 2
        ids[2, 0], ids[2, 1] = cid[0], cid[2]
        w[2] = 0.0
        w[2, 0] = [1, 0, 1, 1, 0, 0]; w[2, 1] = [0, 1, 0, 0, 1, 1]
    if Q == 9:                                             # >= 9 pseudo-queries of the 33-row character: a second 8-query block
        lo = 0 if J == 1 else 2
        ids[lo:, 0] = cid[2]
        w[lo:, 0, 0] = 0.5
        if J >= 2:
            ids[4:, 1] = cid[2]
            w[4:, 1, 1] = 0.25
    if J == 4:
        w[Q - 1, 2] = 0.0                                  # a weightless component
        w[Q - 1, 3] = [NAN, -1, INF, 0, -0.0, -INF]        # and one with nothing usable
    return ids.astype(np.int32), w


def _guarded(shape, dtype, fill):
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device=dev())
    return buf, buf[GUARD: GUARD + n].view(*shape)


def _guards_intact(buf, fill):
    return bool((buf[:GUARD] == fill).all()) and bool((buf[-GUARD:] == fill).all())


@pytest.mark.parametrize("kind", ["fp32", "bf16", "resident"])
def test_match_mix(model, data, kind):
    m = model
    bank, cid, bad, first, enc = _bank(m, data, kind)
    loaded = {c: n for c, n in zip(cid, SIZES)}
    first_of = dict(zip(cid, first))
    tok = torch.arange(90, device=dev()) % 6
    seen_none = seen_second_block = 0
    for Q in (1, 3, 9):
        q = data["q"][:Q].contiguous()
        for J in (1, 2, 4):
            ids_h, w_h = _problem(Q, J, cid, bad, 100 * Q + J)
            ids, w = torch.from_numpy(ids_h).to(dev()), torch.from_numpy(w_h).to(dev())
            # the hard matcher on (that query, that id), every pair
            hard_d, hard_i = bank.query(q.repeat_interleave(J, 0).contiguous(), ids.reshape(-1))
            hard_i, hard_d = hard_i.reshape(Q, J).cpu().numpy(), hard_d.reshape(Q, J).cpu().numpy()
            pres = R.present(ids_h, w_h, set(cid))
            assert ((hard_i >= 0) == np.isin(ids_h, cid)).all()
            seen_none += int((~pres.any(1)).sum())
            seen_second_block += int(max((ids_h[pres] == c).sum() for c in cid) >= 9) if pres.any() else 0
            ibuf, idx = _guarded((Q, J), torch.int32, 0x5A5A5A5)
            dbuf, dist = _guarded((Q, J), torch.float32, -777.0)
            wbuf, wn = _guarded((Q, J, 6), torch.float32, -777.0)
            obuf, out = _guarded((Q, 90, 256), torch.float32, -777.0)
            m._ctx.call("mocha_match_mix_segmented", vp(q), Q, vp(ids), vp(w), J, vp(idx), vp(dist), vp(wn), vp(out), None)
            torch.cuda.synchronize()
            tag = (kind, Q, J)
            assert _guards_intact(ibuf, 0x5A5A5A5) and _guards_intact(dbuf, -777.0) and _guards_intact(wbuf, -777.0) and _guards_intact(obuf, -777.0), tag
            # index and distance: the hard matcher's, bit for bit; -1 / +inf where not present
            want_i = np.where(pres, hard_i, -1)
            want_d = np.where(pres, hard_d, np.float32(INF))
            assert np.array_equal(idx.cpu().numpy(), want_i), (tag, idx.cpu().numpy(), want_i)
            assert np.array_equal(dist.cpu().numpy().view(np.uint32), want_d.astype(np.float32).view(np.uint32)), tag
            # the normalised weights: mix_ref in fp32, bit for bit
            wn_ref = R.normalise(w_h, pres)
            assert np.array_equal(wn.cpu().numpy().view(np.uint32), wn_ref.view(np.uint32)), (tag, wn.cpu().numpy(), wn_ref)
            assert (wn_ref[~pres] == 0).all()
            # out: the torch composition in the kernel's order - masked where the weight is 0, j ascending, products and sums rounded
            # separately; a window with nothing present holds bank row 0
            grow = np.where(pres, want_i + np.vectorize(lambda c: first_of.get(int(c), 0))(ids_h), 0)
            grow_t = torch.from_numpy(grow).to(dev())
            comp = torch.zeros((Q, 90, 256), device=dev())
            for j in range(J):
                wt = wn[:, j][:, tok]                                                  # (Q, 90): the weight of every token
                term = wt[:, :, None] * enc[grow_t[:, j]]
                comp = torch.where((wt != 0)[:, :, None], comp + term, comp)
            none = torch.from_numpy(~pres.any(1)).to(dev())
            comp[none] = enc[0]
            assert torch.equal(out, comp), (tag, float((out - comp).abs().max()))
            # ... and the float64 blend
            feats = enc[grow_t].cpu().numpy()
            F64 = R.blend(wn_ref, feats, np.float64)
            mag = (np.abs(wn_ref[:, :, np.arange(90) % 6, None].astype(np.float64) * feats)).sum(1)
            err = np.abs(out.cpu().numpy().astype(np.float64) - F64)
            live = pres.any(1)
            print(f"{tag}: max |out - float64 blend| / bound = {float((err[live] / ((J + 1) * 2.0 ** -23 * mag[live] + 1e-300)).max()) if live.any() else 0:.3f}")
            assert (err[live] <= (J + 1) * 2.0 ** -23 * mag[live]).all(), tag
            # the optional outputs left out: the same rows
            idx2 = torch.full((Q, J), 9, dtype=torch.int32, device=dev())
            m._ctx.call("mocha_match_mix_segmented", vp(q), Q, vp(ids), vp(w), J, vp(idx2), None, None, None, None)
            assert torch.equal(idx2, idx), tag
            # the Python route is the same call
            d_p, i_p, w_p, o_p = bank.query(q, mix=(ids, w))
            assert torch.equal(i_p, idx) and torch.equal(d_p, dist) and torch.equal(w_p, wn) and torch.equal(o_p, out), tag
    assert seen_none >= 2 and seen_second_block >= 2


def test_one_effective_component_is_the_entry_itself(model, data):
    """Weight on one component only (whatever its scale): wnorm is exactly 1 there, out the matched entry's bits, and the known match."""
    bank, cid, bad, first, enc = _bank(model, data, "fp32")
    Q = 9
    q = data["q"]
    near = data["near"]
    ids = torch.tensor([[bad[0], c, 1 - min(c, 1)] for c, _ in near], dtype=torch.int32, device=dev())
    w = torch.zeros((Q, 3, 6), device=dev())
    w[:, 0] = 5.0                                          # on an id that names nothing: not present
    w[:, 1] = torch.tensor([1e-30, 0.3, 7.0, 1e30, 1.0, 2.0, 0.5, 3e38, 1e-45], device=dev())[:, None]
    dist, idx, wn, out = bank.query(q, mix=(ids, w))
    torch.cuda.synchronize()
    assert idx[:, 1].tolist() == [r for _, r in near] and bool((idx[:, 0] == -1).all()) and bool((idx[:, 2] == -1).all())
    assert bool((wn[:, 1] == 1).all()) and bool((wn[:, 0] == 0).all()) and bool((wn[:, 2] == 0).all())
    want = torch.stack([data["encs"][c][r] for c, r in near])
    assert torch.equal(out, want)
