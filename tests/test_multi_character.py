"""Multi-character bank on the MI355X (run with -m gpu): several characters as row segments of one bank, every query / window matched
exactly within its OWN character's rows (mocha_bank_set_segments, mocha_match_segmented, mocha_characterize_segmented,
mocha_step_graph_segmented; MultiCharacterBank, MultiStreamCharacterizer).

Inputs as in test_fullsize_parity.py::test_config4_*: synthetic weights, banks of noise with planted noisy copies of the queries' own
features (two per query, the farther one 1e-3 further away: distinct answers and near-ties), and - so that searching the wrong rows would
show - a CLOSER copy of every query planted in another character's rows.  Indices are checked against a float64 brute-force search of each
query's own segment; a mismatch is accepted only as a float64 near-tie (relative gap <= 2e-6).  No test here feeds out-of-range ids."""
import ctypes as C

import numpy as np
import pytest
import torch

from mocha_sigasia2023_amd import ContextBank, Generator, MultiCharacterBank, MultiStreamCharacterizer, synthetic, weights
from oracle import mocha_oracle as O

pytestmark = pytest.mark.gpu
D = 90 * 256
TOL = 1e-4
SIZES = [1, 7, 300, 2048, 4099]
USED = [0, 2, 3, 4]                     # segment 1 stays unused


def dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return torch.device("cuda:0")


def _bf16_round(a):
    u = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) >> 16
    return (u.astype(np.uint32) << 16).view(np.float32)


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


def _check_idx(idx, dist, qs, ids, searched, starts, sizes):
    """idx / dist against the float64 search of each query's own segment of `searched` (the fp32 rows, or bf16(b - centre) with centred
    queries qs).  Returns the number of accepted near-ties."""
    nt = 0
    for s in sorted(set(ids.tolist())):
        m = np.nonzero(ids == s)[0]
        rows = searched[starts[s]: starts[s] + sizes[s]].double()
        qm = qs[torch.from_numpy(m).to(qs.device)].double()
        best = torch.cdist(qm, rows).argmin(dim=1).cpu().numpy()
        for j, i in enumerate(m):
            got = int(idx[i])
            assert 0 <= got < sizes[s], (i, got)
            d_got = float((qm[j] - rows[got]).norm())
            if got != best[j]:
                d_best = float((qm[j] - rows[int(best[j])]).norm())
                assert d_got - d_best <= 2e-6 * d_best, (i, s, got, int(best[j]), d_got, d_best)
                nt += 1
            assert abs(float(dist[i]) - d_got) <= 1e-5 * d_got + 1e-6, (i, float(dist[i]), d_got)
    return nt


@pytest.fixture(scope="module")
def model():
    sd = weights.synthetic_state_dict(1777, 1.0, "mixamo")
    return Generator(layout="mixamo", device=dev()).load_state_dict(sd).eval(), sd


@pytest.mark.parametrize("bf16", [False, True])
def test_segmented_match_exact(model, bf16):
    m, _ = model
    g = torch.Generator(device=dev()); g.manual_seed(11)
    rng = np.random.default_rng(11)
    starts = np.concatenate([[0], np.cumsum(SIZES)]).astype(np.int64)
    N = int(starts[-1])
    bank = torch.randn((N, D), device=dev(), generator=g)
    QA = 300
    q_all = torch.randn((QA, D), device=dev(), generator=g)
    ids_all = np.sort(rng.choice(USED, QA))                # runs ...
    ids_all[QA // 2:] = rng.permutation(ids_all[QA // 2:])  # ... and shuffled order
    _plant(bank, starts, SIZES, q_all, ids_all, g, 0.02, USED)
    mb = MultiCharacterBank(m, [(bank[starts[c]:starts[c + 1]], bank[starts[c]:starts[c + 1]].view(-1, 90, 256)) for c in range(len(SIZES))],
                            bf16=bf16, dec_cache=False)
    assert [mb.rows(c) for c in range(len(SIZES))] == [(int(starts[c]), int(starts[c + 1])) for c in range(len(SIZES))]
    searched, qs_all = bank, q_all
    if bf16:
        bank_np = bank.cpu().numpy()
        centre = bank_np.astype(np.float64).mean(0).astype(np.float32)
        searched = torch.from_numpy(_bf16_round(bank_np - centre)).to(dev())
        qs_all = q_all - torch.from_numpy(centre).to(dev())
    ties = 0
    for Q in (1, 3, 8, 9, 37, 300):
        sel = rng.permutation(QA)[:Q]
        if Q >= 8:
            sel[Q // 2] = sel[0]                               # a repeated query
        ids = ids_all[sel]
        dist, idx = mb.query(q_all[sel], torch.from_numpy(ids).to(dev()))
        torch.cuda.synchronize()
        ties += _check_idx(idx[:, 0].cpu().numpy(), dist[:, 0].cpu().numpy(), qs_all[sel], ids, searched, starts, SIZES)
    assert ties <= 3 or bf16, ties
    with pytest.raises(ValueError):
        mb.query(q_all[:2], [0, 5])                           # host ids are checked before any launch


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


def test_characterize_segmented(chars):
    m, mb, src, ids, starts, sizes = chars["m"], chars["mb"], chars["src"], chars["ids"], chars["starts"], chars["sizes"]
    Y, idx = mb.characterize(src, ids, chars["mean"], chars["std"], return_index=True)
    torch.cuda.synchronize()
    idx = idx.cpu().numpy()
    _, _, nm = m.encode(src, chars["mean"], chars["std"])
    dist, idx_q = mb.query(nm.reshape(len(ids), D), ids)
    assert np.array_equal(idx, idx_q[:, 0].cpu().numpy())          # the batched characterize matches as the query does
    _check_idx(idx, dist[:, 0].cpu().numpy(), nm.reshape(len(ids), D), ids, chars["bank"], starts, sizes)
    # Y against the oracle on a sample: encode the source windows, decode on the matched row of each window's own character
    ost = O.to_torch_state(chars["sd"])
    sel = np.array([0, 1, 2, 7, 13])
    rows = torch.from_numpy(starts[ids[sel]] + idx[sel])
    with torch.no_grad():
        eo, _ = O.encode(ost, src.cpu()[sel])
        Yo = O.to_mot(ost, O.decoder(ost, eo, chars["bank"].reshape(-1, 90, 256).cpu()[rows])).numpy()
    assert np.abs(Y.cpu().numpy()[sel] - Yo).max() < TOL
    # against ContextBank(one character).characterize on the same windows: the same kernels on the same rows (the encoder of the same batch
    # size, the decoder constants of the same entry, computed per row) - expected bit-identical
    for c in range(3):
        w = np.nonzero(ids == c)[0]
        cb = ContextBank(m, *chars["banks"][c])
        Yc, ic = cb.characterize(src[w], chars["mean"], chars["std"], return_index=True)
        Ys, iseg = mb.characterize(src[w], [c] * len(w), chars["mean"], chars["std"], return_index=True)
        assert np.array_equal(ic.cpu().numpy(), iseg.cpu().numpy()) and np.array_equal(iseg.cpu().numpy(), idx[w])
        err = float((Yc - Ys).abs().max())
        print(f"character {c}: {len(w)} windows, max |Y_segmented - Y_ContextBank| = {err:.3e}")
        assert err <= 1e-5


@pytest.mark.parametrize("S_w", [3, 8])
def test_multi_stream_replay_equals_eager(chars, S_w):
    m, mb, src = chars["m"], chars["mb"], chars["src"]
    rng = np.random.default_rng(S_w)
    mb.characterize(src[:S_w], [0] * S_w, chars["mean"], chars["std"])   # eager first: weight images made on first use exist before capture
    ms = MultiStreamCharacterizer(mb, chars["mean"], chars["std"], streams=S_w)
    gens = []
    for k in range(4):
        w = rng.permutation(len(chars["ids"]))[:S_w]
        ids = rng.integers(0, 3, S_w).astype(np.int32)
        ms.input.copy_(src[w])
        ms.characters.copy_(torch.from_numpy(ids))                  # new ids in place: the captured step reads them
        Y, idx = ms.step()
        Y, idx = Y.clone(), idx.clone()
        gens.append(m._ctx.generation())
        Ye, ie = mb.characterize(src[w], ids, chars["mean"], chars["std"], return_index=True)
        assert torch.equal(Y, Ye) and torch.equal(idx, ie), k
    assert gens[1] == gens[-1], gens                                # only the ids changed: no re-capture, nothing replaced
    ids = [k % 3 for k in range(S_w)]
    Y, idx = ms.step(src[:S_w], ids)                                # windows and host ids as arguments
    Ye, ie = mb.characterize(src[:S_w], ids, chars["mean"], chars["std"], return_index=True)
    assert Y.shape == (S_w, 60, 22, 15) and torch.equal(Y, Ye) and torch.equal(idx, ie)
    assert m._ctx.generation() == gens[-1]


def test_union_calls_and_table_cleared(chars):
    m, mb = chars["m"], chars["mb"]
    q = chars["nm0"][:5].contiguous()
    mb.activate()
    lib, h = m._ctx.lib, m._ctx.h
    idx_s = torch.empty((5,), dtype=torch.int32, device=dev()); dist_s = torch.empty((5,), device=dev())
    m._ctx.call("mocha_match", C.c_void_p(q.data_ptr()), 5, C.c_void_p(idx_s.data_ptr()), C.c_void_p(dist_s.data_ptr()), None)
    union = ContextBank(m, mb.cnt_nm, mb.encoded)                      # plain mocha_bank_set of the concatenation: clears the table
    dist_u, idx_u = union.query(q)
    torch.cuda.synchronize()
    assert torch.equal(idx_s, idx_u[:, 0]) and torch.equal(dist_s, dist_u[:, 0])
    ids = torch.zeros((5,), dtype=torch.int32, device=dev())
    rc = lib.mocha_match_segmented(h, C.c_void_p(q.data_ptr()), 5, C.c_void_p(ids.data_ptr()), C.c_void_p(idx_s.data_ptr()), None, None)
    assert rc == -3                                                    # MOCHA_ERR_STATE: no segment table
    dist_m, _ = mb.query(q, [0] * 5)                                  # the multi-character bank makes itself current again
    assert bool(torch.isfinite(dist_m).all())
