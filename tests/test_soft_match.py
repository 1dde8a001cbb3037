"""Soft context matching on a multi-character bank on the MI355X (run with -m gpu): the k nearest rows of every query within its OWN
character's rows, the softmax weights, the blended character feature, the soft characterize and its captured step
(mocha_match_topk_segmented, mocha_characterize_soft_segmented, mocha_step_graph_soft_segmented; MultiCharacterBank.query(k=),
.characterize(soft=), MultiStreamCharacterizer(soft=)).

Top-k bank: segments of [3, 16, 17, 200, 2049] rows - fewer rows than k, exactly one scan workgroup, a one-row tail chunk, several
chunks, a chunk count that is no multiple of anything convenient - all of them searched, plus a sixth segment of 40 rows that no query
names.  Noise rows with, per query, two noisy copies in its own segment (the second 1e-3 farther), a CLOSER decoy in another segment, and
in the 17-row segment an exact duplicate pair at local rows 15 and 16 - a tie that straddles two scan workgroups - with one query on it.
The data come from SEED, chosen so that in float64 no two of a query's first 9 distances (fp32 rows) are closer than 1e-5 relative
except that planted tie (the fixture asserts it): fp32 arithmetic cannot reorder them, so every returned row must be the float64 row.

The blend itself is not exposed by the library; it is checked through the soft characterize: (a) bit for bit against the staged route
whose blend the test computes in the kernel's order, (b) against the oracle decoder fed the float64 blend."""
import ctypes as C

import numpy as np
import pytest
import torch

from mocha_sigasia2023_amd import Generator, MultiCharacterBank, MultiStreamCharacterizer, synthetic, weights
from oracle import mocha_oracle as O

pytestmark = pytest.mark.gpu
D = 90 * 256
TOL = 1e-4
SIZES = [3, 16, 17, 200, 2049, 40]
USED = [0, 1, 2, 3, 4]                  # segment 5 stays unused
DUP = (2, 15, 16)                       # segment, local rows of the exact duplicate pair
SEED = 35
POOL = 48                               # queries in the pool; query 0 sits on the duplicate pair
KS = (1, 2, 5, 8)


def dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return torch.device("cuda:0")


def _bf16_round(a):
    u = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) >> 16
    return (u.astype(np.uint32) << 16).view(np.float32)


def make_topk_data(seed):
    """(bank (N, D) fp32, queries (POOL, D) fp32, ids (POOL,), starts, pairs) on the host, from `seed` alone.  pairs: per segment a
    dict {frozenset({a, b}): owner} of the local rows that hold query `owner`'s two copies (1e-3 apart as seen from that query, but nearly equidistant -
    a few 1e-7 relative - from every OTHER query of the segment), and the exact duplicate pair (owner -1)."""
    rng = np.random.default_rng(seed)
    starts = np.concatenate([[0], np.cumsum(SIZES)]).astype(np.int64)
    bank = rng.standard_normal((int(starts[-1]), D), dtype=np.float32)
    q = rng.standard_normal((POOL, D), dtype=np.float32)
    # ids: the duplicate's query, one query per small segment first, then a mix weighted to the large segments
    ids = np.concatenate([[DUP[0], 0, 1, 2, 3, 4], rng.choice(USED, POOL - 6, p=[0.06, 0.14, 0.14, 0.26, 0.40])]).astype(np.int64)
    free = [rng.permutation(n).tolist() for n in SIZES]
    for r in DUP[1:]:
        free[DUP[0]].remove(r)
    pairs = [{} for _ in SIZES]
    pairs[DUP[0]][frozenset(DUP[1:])] = -1
    s, r0, r1 = DUP
    bank[starts[s] + r1] = bank[starts[s] + r0]
    q[0] = bank[starts[s] + r0] + 0.02 * rng.standard_normal(D, dtype=np.float32)
    for i in range(1, POOL):
        s = int(ids[i])
        noise = 0.02 * rng.standard_normal(D, dtype=np.float32)
        if len(free[s]) >= 2:
            a, b = free[s].pop(), free[s].pop()
            bank[starts[s] + a] = q[i] + noise
            bank[starts[s] + b] = q[i] + np.float32(1.001) * noise
            pairs[s][frozenset((a, b))] = i
        decoy = [t for t in USED if t != s and len(free[t]) >= 1]
        if decoy:
            t = decoy[i % len(decoy)]
            bank[starts[t] + free[t].pop()] = q[i] + np.float32(0.5) * noise
    return bank, q, ids, starts, pairs


def tie_free_gaps(order, d, own):
    """Relative gaps between consecutive float64 distances of a query's first rows, without the planted near-ties `own` (the segment's
    pairs, see make_topk_data) where the two rows of a pair are neighbours in the order."""
    dd = d[order]
    gaps = (dd[1:] - dd[:-1]) / dd[1:]
    at = [c for c in range(len(order) - 1) if frozenset((int(order[c]), int(order[c + 1]))) in own]
    return np.delete(gaps, at)


def float64_order(searched, qs, ids, starts, nkeep=9):
    """Per query: (rows of its own segment in ascending float64 distance, ties to the lower row; those distances), the first nkeep."""
    out = []
    for i in range(qs.shape[0]):
        s = int(ids[i])
        rows = searched[int(starts[s]): int(starts[s + 1])].double()
        d = (rows - qs[i].double()[None]).pow(2).sum(1).sqrt()
        order = torch.sort(d, stable=True).indices[:nkeep]
        out.append((order.cpu().numpy(), d.cpu().numpy()))
    return out


@pytest.fixture(scope="module")
def model():
    sd = weights.synthetic_state_dict(1777, 1.0, "mixamo")
    return Generator(layout="mixamo", device=dev()).load_state_dict(sd).eval(), sd


@pytest.fixture(scope="module")
def topk(model):
    bank_np, q_np, ids, starts, pairs = make_topk_data(SEED)
    bank, q = torch.from_numpy(bank_np).to(dev()), torch.from_numpy(q_np).to(dev())
    centre = bank_np.astype(np.float64).mean(0).astype(np.float32)
    searched16 = torch.from_numpy(_bf16_round(bank_np - centre)).to(dev())
    qc = q - torch.from_numpy(centre).to(dev())
    ref32 = float64_order(bank, q, ids, starts)
    ref16 = float64_order(searched16, qc, ids, starts)
    # the seed's property, in float64 alone: no near-tie among a query's first k + 1 = 9 distances except the planted ones.  A query's OWN
    # two copies are 1e-3 apart and count as distinct answers; only another query's pair, or the duplicate, may be a near-tie
    for i, (order, d) in enumerate(ref32):
        own = {p for p, owner in pairs[int(ids[i])].items() if owner != i}
        gaps = tie_free_gaps(order, d, own)
        if i == 0:
            assert tuple(order[:2]) == DUP[1:] and d[order[0]] == d[order[1]], order[:3]
        assert gaps.size == 0 or gaps.min() >= 1e-5, (i, int(ids[i]), gaps.min())
    return dict(bank=bank, q=q, ids=ids, starts=starts, pairs=pairs, ref={False: (bank, q, ref32), True: (searched16, qc, ref16)})


def _selection(Q, ids):
    """Pool indices of a launch of Q queries: mixed and repeated ids; from 16 on the first group of 16 holds 8 / 4 / 2 / 1 / 1 queries of
    segments 4 / 3 / 2 / 1 / 0, so that the 8-, 4-, 2- and 1-query scan bodies all run."""
    by = {s: [i for i in range(POOL) if ids[i] == s] for s in USED}
    if Q == 1:
        return [0]
    if Q == 3:
        return [0, 1, by[4][0]]
    if Q == 8:
        return [0, 1, 2] + by[4][:3] + [by[3][0], 0]
    if Q == 9:
        return by[4][:5] + [1, 0, by[3][0], by[4][0]]
    first = by[4][:8] + by[3][:4] + [0, 3] + [2] + [1]
    assert len(first) == 16 and len(by[4]) >= 8 and len(by[3]) >= 4
    if Q == 16:
        return first
    rest = [i for i in range(POOL) if i not in first]
    return first + rest[:Q - 16 - 2] + [0, 1]


def _topk_call(m, mb, q, ids_dev, k):
    """mocha_match_topk_segmented itself (MultiCharacterBank.query takes the hard call for k = 1)."""
    mb._ensure()
    Q = q.shape[0]
    idx = torch.empty((Q, k), dtype=torch.int32, device=q.device)
    dist = torch.empty((Q, k), dtype=torch.float32, device=q.device)
    m._ctx.call("mocha_match_topk_segmented", C.c_void_p(q.data_ptr()), Q, C.c_void_p(ids_dev.data_ptr()), k, C.c_void_p(idx.data_ptr()),
                C.c_void_p(dist.data_ptr()), None)
    return dist, idx


@pytest.mark.parametrize("bf16", [False, True])
def test_segmented_topk_exact(model, topk, bf16):
    m, _ = model
    bank, starts, ids_all = topk["bank"], topk["starts"], topk["ids"]
    searched, qs_all, ref = topk["ref"][bf16]
    mb = MultiCharacterBank(m, [(bank[starts[c]:starts[c + 1]], bank[starts[c]:starts[c + 1]].view(-1, 90, 256)) for c in range(len(SIZES))],
                            bf16=bf16, dec_cache=False)
    swaps, pairs = 0, topk["pairs"]
    for Q in (1, 3, 8, 9, 16, 37):
        sel = np.array(_selection(Q, ids_all))
        assert len(sel) == Q
        ids = ids_all[sel]
        ids_dev = torch.from_numpy(ids.astype(np.int32)).to(dev())
        q = topk["q"][torch.from_numpy(sel).to(dev())].contiguous()
        dist1, idx1 = mb.query(q, ids_dev)                              # the hard 1-NN of the same queries
        for k in KS:
            dist, idx = _topk_call(m, mb, q, ids_dev, k)
            if k > 1:
                dist_p, idx_p = mb.query(q, ids_dev, k=k)               # the Python route is the same call
                assert torch.equal(idx_p, idx) and torch.equal(dist_p, dist)
            torch.cuda.synchronize()
            # column 0 is the hard matcher's answer, index and distance, to the bit (k = 1: the whole result)
            assert torch.equal(idx[:, 0], idx1[:, 0]), (Q, k)
            assert torch.equal(dist[:, 0], dist1[:, 0]), (Q, k, float((dist[:, 0] - dist1[:, 0]).abs().max()))
            idx_h, dist_h = idx.cpu().numpy(), dist.cpu().numpy()
            for j, i in enumerate(sel):
                order, d64 = ref[i]
                n = SIZES[int(ids[j])]
                have = min(k, n)
                assert (idx_h[j, have:] == -1).all() and np.isposinf(dist_h[j, have:]).all(), (Q, k, j)     # fewer rows than k
                assert len(set(idx_h[j, :have].tolist())) == have
                for c in range(have):
                    got = int(idx_h[j, c])
                    assert 0 <= got < n, (Q, k, j, c, got)
                    if got != int(order[c]):
                        assert abs(d64[got] - d64[order[c]]) <= 2e-6 * d64[order[c]], (Q, k, j, c, got, int(order[c]), d64[got], d64[order[c]])
                        # fp32 bank: the seed leaves no float64 near-tie but the planted ones, so only the two rows of a planted pair may swap
                        assert bf16 or pairs[int(ids[j])].get(frozenset((got, int(order[c]))), i) != i, (Q, k, j, c, got, int(order[c]))
                        swaps += 1
                    assert abs(float(dist_h[j, c]) - d64[got]) <= 1e-5 * d64[got] + 1e-6, (Q, k, j, c, float(dist_h[j, c]), d64[got])
                if i == 0 and k >= 2:
                    assert idx_h[j, :2].tolist() == list(DUP[1:]), idx_h[j]       # the tie: lower row first
                    assert dist_h[j, 0] == dist_h[j, 1]
    print(f"bf16={bf16}: {swaps} accepted float64 near-ties (columns that hold the other row of a planted pair)")


def test_short_segment_and_weights(model, topk):
    """k = 5 on the top-k bank through the soft characterize: the 3-row segment's columns 3.. are -1 / weight 0, the rows are those of the
    matcher on the same queries, and the weights are the float64 softmax of the RETURNED distances to 1e-6."""
    m, _ = model
    bank, starts = topk["bank"], topk["starts"]
    mean, std = synthetic.cnt_norm(7)
    mb = MultiCharacterBank(m, [(bank[starts[c]:starts[c + 1]], bank[starts[c]:starts[c + 1]].view(-1, 90, 256)) for c in range(len(SIZES))],
                            dec_cache=False)
    W, k = 10, 5
    ids = np.array([0, 4, 2, 0, 1, 3, 4, 4, 2, 0])
    src = torch.from_numpy(synthetic.pose_windows(9, W, 22)).to(dev())
    for T in (2.0, 0.05, 40.0):
        Y, idx_k, w_k = mb.characterize(src, ids, mean, std, return_index=True, soft=(k, T))
        _, _, nm = m.encode(src, mean, std)
        dist, idx = mb.query(nm.reshape(W, D), ids, k=k)
        torch.cuda.synchronize()
        assert torch.equal(idx_k, idx)
        assert bool(torch.isfinite(Y).all())
        d, w = dist.cpu().numpy().astype(np.float64), w_k.cpu().numpy()
        for i in range(W):
            have = min(k, SIZES[ids[i]])
            assert (idx_k[i, have:] == -1).all() and (w[i, have:] == 0).all() and np.isposinf(d[i, have:]).all()
            e = np.exp(-(d[i, :have] - d[i, :have].min()) / T)
            assert np.abs(w[i, :have] - e / e.sum()).max() <= 1e-6, (T, i, w[i], e / e.sum())
        assert np.abs(w.sum(1) - 1).max() <= 1e-6


def _plant(bank, starts, sizes, q, ids, g, scale, used):
    """Two noisy copies of query i in its own segment (distinct rows), a closer one in another used segment with room."""
    free = [torch.randperm(n, device=bank.device, generator=g).tolist() for n in sizes]
    for i, s in enumerate(ids):
        noise = scale * torch.randn((D,), device=bank.device, generator=g)
        if len(free[s]) >= 2:
            r0, r1 = free[s].pop(), free[s].pop()
            bank[starts[s] + r0] = q[i] + noise
            bank[starts[s] + r1] = q[i] + 1.001 * noise
        decoy = [t for t in used if t != s and len(free[t]) >= 1]
        if decoy:
            t = decoy[i % len(decoy)]
            bank[starts[t] + free[t].pop()] = q[i] + 0.5 * noise


@pytest.fixture(scope="module")
def chars(model):
    """Three characters (64, 200, 500 rows) with planted copies of 24 windows' own features; windows' characters mixed."""
    m, sd = model
    V, W = 22, 24
    mean, std = synthetic.cnt_norm(7)
    g = torch.Generator(device=dev()); g.manual_seed(5)
    sizes = [64, 200, 500]
    starts = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    src = torch.from_numpy(synthetic.pose_windows(5, W, V)).to(dev())
    _, _, nm0 = m.encode(src, mean, std)
    nm0 = nm0.reshape(W, D)
    bank = torch.randn((int(starts[-1]), D), device=dev(), generator=g)
    ids = np.array([2, 0, 1, 2, 2, 1, 0, 0, 1, 2, 1, 1, 0, 2, 2, 2, 0, 1, 1, 0, 2, 0, 1, 2])
    gap = (torch.cdist(nm0, nm0) + 1e30 * torch.eye(W, device=dev())).min().item()
    _plant(bank, starts, sizes, nm0, ids, g, 0.1 * gap / D ** 0.5, range(3))
    banks = [(bank[starts[c]:starts[c + 1]].contiguous(), bank[starts[c]:starts[c + 1]].reshape(-1, 90, 256).contiguous()) for c in range(3)]
    mb = MultiCharacterBank(m, banks)
    return dict(m=m, sd=sd, mean=mean, std=std, src=src, nm0=nm0, bank=bank, starts=starts, sizes=sizes, ids=ids, banks=banks, mb=mb)


def test_soft_characterize(chars):
    m, mb, src, ids, starts = chars["m"], chars["mb"], chars["src"], chars["ids"], chars["starts"]
    mean, std = chars["mean"], chars["std"]
    k, T, W = 4, 2.0, len(ids)
    Y, idx_k, w_k = mb.characterize(src, ids, mean, std, return_index=True, soft=(k, T))
    assert torch.equal(Y, mb.characterize(src, ids, mean, std, soft=(k, T)))
    # (a) the staged route: encode -> z-score -> top-k -> blend of the returned rows with the returned weights (fp32, j ascending, every
    # product and sum rounded on its own: the kernel's order) -> decoder -> to_mot; the same kernels on the same values: bit-identical
    enc, _, nm = m.encode(src, mean, std)
    dist, idx = mb.query(nm.reshape(W, D), ids, k=k)
    assert torch.equal(idx, idx_k) and bool((idx >= 0).all())
    rows = idx.long() + torch.from_numpy(starts[ids]).to(dev())[:, None]
    enc_bank = chars["bank"].reshape(-1, 90, 256)
    blend = torch.zeros((W, 90, 256), device=dev())
    for j in range(k):
        blend = blend + w_k[:, j, None, None] * enc_bank[rows[:, j]]
    Ys = m.to_mot(m.decoder(enc, blend))
    torch.cuda.synchronize()
    assert torch.equal(Y, Ys), float((Y - Ys).abs().max())
    # the weights of the returned distances (float64 softmax), and the planted pair in front with nearly equal weights
    d = dist.cpu().numpy().astype(np.float64)
    e = np.exp(-(d - d.min(1, keepdims=True)) / T)
    assert np.abs(w_k.cpu().numpy() - e / e.sum(1, keepdims=True)).max() <= 1e-6
    # (b) against the oracle decoder fed the float64 blend of the returned rows and weights, on a sample
    ost = O.to_torch_state(chars["sd"])
    sel = np.array([0, 1, 2, 7, 13])
    b64 = (w_k.double()[:, :, None, None] * enc_bank.double()[rows]).sum(1)
    print(f"max |fp32 blend (kernel order) - float64 blend| = {float((blend.double() - b64).abs().max()):.3e}")
    assert float((blend.double() - b64).abs().max()) <= 1e-5
    with torch.no_grad():
        eo, _ = O.encode(ost, src.cpu()[sel])
        Yo = O.to_mot(ost, O.decoder(ost, eo, b64.float().cpu()[sel])).numpy()
    err = np.abs(Y.cpu().numpy()[sel] - Yo).max()
    print(f"max |Y_soft - Y_oracle(float64 blend)| = {err:.3e}")
    assert err < TOL


@pytest.mark.parametrize("dec_cache", [True, False])
def test_soft_k1_is_the_hard_characterize(chars, dec_cache):
    """soft = (1, T): weight 1.0 and 0 + 1 * x are exact, so the soft route must give the hard route's Y to the bit - with the bank's
    cached decoder constants (the hard route reads them, the soft route recomputes them per call) and without."""
    m, src, ids = chars["m"], chars["src"], chars["ids"]
    mb = chars["mb"] if dec_cache else MultiCharacterBank(m, chars["banks"], dec_cache=False)
    Yh, ih = mb.characterize(src, ids, chars["mean"], chars["std"], return_index=True)
    for T in (2.0, 0.01, 300.0):
        Y, idx_k, w_k = mb.characterize(src, ids, chars["mean"], chars["std"], return_index=True, soft=(1, T))
        torch.cuda.synchronize()
        assert torch.equal(idx_k[:, 0], ih) and bool((w_k == 1.0).all())
        assert torch.equal(Y, Yh), (dec_cache, T, float((Y - Yh).abs().max()))
    chars["mb"].activate()


@pytest.mark.parametrize("S_w", [1, 5, 16])
def test_soft_multi_stream_replay_equals_eager(chars, S_w):
    m, mb, src = chars["m"], chars["mb"], chars["src"]
    soft = (4, 2.0)
    rng = np.random.default_rng(S_w)
    mb.activate()
    ms = MultiStreamCharacterizer(mb, chars["mean"], chars["std"], streams=S_w, soft=soft)
    gens = []
    for step in range(3):
        w = rng.permutation(len(chars["ids"]))[:S_w]
        ids = rng.integers(0, 3, S_w).astype(np.int32)
        ms.input.copy_(src[w])
        ms.characters.copy_(torch.from_numpy(ids))                  # new ids in place: the captured step reads them
        Y, idx_k, wk = ms.step()
        Y, idx_k, wk = Y.clone(), idx_k.clone(), wk.clone()
        gens.append(m._ctx.generation())
        Ye, ie, we = mb.characterize(src[w], ids, chars["mean"], chars["std"], return_index=True, soft=soft)
        assert torch.equal(Y, Ye) and torch.equal(idx_k, ie) and torch.equal(wk, we), step
    assert gens[0] == gens[-1], gens                                # captured once: only the ids changed, nothing was replaced
    m.profile_start()                                               # a step that had to capture again would refuse while profiling
    try:
        Y, idx_k, wk = ms.step()
    finally:
        m.profile_stop()
    assert torch.equal(Y, Ye) and torch.equal(idx_k, ie)


def test_soft_refusals(chars):
    m, mb = chars["m"], chars["mb"]
    mb.activate()
    lib, h = m._ctx.lib, m._ctx.h
    q = chars["nm0"][:2].contiguous()
    ids = torch.zeros((2,), dtype=torch.int32, device=dev())
    idx = torch.full((2, 8), 7, dtype=torch.int32, device=dev())
    vp = lambda t: C.c_void_p(t.data_ptr())                          # noqa: E731
    gen = m._ctx.generation()
    assert lib.mocha_match_topk_segmented(h, vp(q), 2, vp(ids), 0, vp(idx), None, None) == -1
    assert lib.mocha_match_topk_segmented(h, vp(q), 2, vp(ids), 9, vp(idx), None, None) == -1
    assert lib.mocha_match_topk_segmented(h, vp(q), 2, None, 4, vp(idx), None, None) == -1
    Y = torch.empty((2, 60, 22, 15), device=dev())
    X = chars["src"][:2].contiguous()
    mean = torch.from_numpy(chars["mean"]).to(dev()); std = torch.from_numpy(chars["std"]).to(dev())
    for fn in (lib.mocha_characterize_soft_segmented, lib.mocha_step_graph_soft_segmented):
        w = torch.zeros((2, 8), device=dev())
        assert fn(h, vp(X), 2, vp(ids), 4, 0.0, vp(mean), vp(std), vp(Y), vp(idx), vp(w), 0, None) == -1
        assert fn(h, vp(X), 2, vp(ids), 9, 1.0, vp(mean), vp(std), vp(Y), vp(idx), vp(w), 0, None) == -1
        assert fn(h, vp(X), 2, None, 4, 1.0, vp(mean), vp(std), vp(Y), vp(idx), vp(w), 0, None) == -1
    torch.cuda.synchronize()
    assert bool((idx == 7).all()) and m._ctx.generation() == gen     # nothing was launched, nothing replaced
    with pytest.raises(ValueError):
        mb.characterize(X, [0, 1], mean, std, soft=(9, 1.0))
    with pytest.raises(ValueError):
        mb.query(q, [0, 1], k=0)
