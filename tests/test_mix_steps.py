"""Character mixing through the characterize calls on the MI355X (run with -m gpu): MultiCharacterBank.characterize(mix=) /
mocha_characterize_mix_segmented, MultiStreamCharacterizer(mix=J) / mocha_step_graph_mix_segmented, and the refusals.

Three characters of 64, 200 and 500 rows with planted copies of 24 windows' own features (the set-up of tests/test_soft_match.py: 24
windows and banks of more than 16 rows, so that the literal decoder's float64 style MLP and the bank's cached decoder constants come
from the same tiled kernel).  24 windows are two groups of the mixing matcher (16 + 8)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mix_ref as R  # noqa: E402
from mocha_sigasia2023_amd import (Generator, LiveOursSession, LiveSession, MultiCharacterBank, MultiStreamCharacterizer,  # noqa: E402
                                   synthetic, weights)
from oracle import mocha_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu
D = 90 * 256
TOL = 1e-4                               # tests/test_soft_match.py: the soft route against the oracle decoder fed the float64 blend
SIZES = [64, 200, 500]
IDS = np.array([2, 0, 1, 2, 2, 1, 0, 0, 1, 2, 1, 1, 0, 2, 2, 2, 0, 1, 1, 0, 2, 0, 1, 2])


def dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return torch.device("cuda:0")


def _plant(bank, starts, q, ids, g, scale):
    """Two noisy copies of query i in its own character (distinct rows), a closer one in another character."""
    free = [torch.randperm(n, device=bank.device, generator=g).tolist() for n in SIZES]
    for i, s in enumerate(ids):
        noise = scale * torch.randn((D,), device=bank.device, generator=g)
        r0, r1 = free[s].pop(), free[s].pop()
        bank[starts[s] + r0] = q[i] + noise
        bank[starts[s] + r1] = q[i] + 1.001 * noise
        t = [t for t in range(3) if t != s][i % 2]
        bank[starts[t] + free[t].pop()] = q[i] + 0.5 * noise


@pytest.fixture(scope="module")
def chars():
    sd = weights.synthetic_state_dict(1777, 1.0, "mixamo")
    m = Generator(layout="mixamo", device=dev()).load_state_dict(sd).eval()
    W = len(IDS)
    mean, std = synthetic.cnt_norm(7)
    g = torch.Generator(device=dev()); g.manual_seed(5)
    starts = np.concatenate([[0], np.cumsum(SIZES)]).astype(np.int64)
    src = torch.from_numpy(synthetic.pose_windows(5, W, 22)).to(dev())
    _, _, nm0 = m.encode(src, mean, std)
    nm0 = nm0.reshape(W, D)
    bank = torch.randn((int(starts[-1]), D), device=dev(), generator=g)
    gap = (torch.cdist(nm0, nm0) + 1e30 * torch.eye(W, device=dev())).min().item()
    _plant(bank, starts, nm0, IDS, g, 0.1 * gap / D ** 0.5)
    banks = [(bank[starts[c]:starts[c + 1]].contiguous(), bank[starts[c]:starts[c + 1]].reshape(-1, 90, 256).contiguous()) for c in range(3)]
    mb = MultiCharacterBank(m, banks)
    return dict(m=m, sd=sd, mean=mean, std=std, src=src, nm0=nm0, bank=bank, starts=starts, banks=banks, mb=mb)


def _general_mix(W, J, seed):
    """ids (W,J) over the three characters with a few ids that name nothing, weights (W,J,6) with zeros and junk; every window keeps at
    least one present component."""
    r = np.random.default_rng(seed)
    ids = r.integers(0, 3, (W, J)).astype(np.int32)
    w = (r.random((W, J, 6)) + 0.05).astype(np.float32)
    w[r.random((W, J, 6)) < 0.15] = 0.0
    if J >= 2:
        ids[r.random((W, J)) < 0.1] = 7
        w[3, 1] = 0.0
        w[5, 0, 2] = float("nan"); w[6, J - 1, 4] = -1.0
    bad = ids.max(1) > 2
    ids[bad, 0] = IDS[:W][bad]                                   # (a bad id somewhere: make sure component 0 is a character ...)
    w[:, 0, 0] = np.maximum(w[:, 0, 0], 0.1)                     # ... with a usable weight)
    return ids, w


@pytest.mark.parametrize("dec_cache", [True, False])
def test_one_effective_component_is_the_hard_characterize(chars, dec_cache):
    """One component with usable weight: its normalised weight is exactly 1 and 0 + 1 * x is exact, so the mix route must give the hard
    route's Y to the bit - with the bank's cached decoder constants (the hard route reads them, the mix route recomputes them per call,
    the literal flow of the soft route) and without."""
    m, src = chars["m"], chars["src"]
    mb = chars["mb"] if dec_cache else MultiCharacterBank(m, chars["banks"], dec_cache=False)
    W = len(IDS)
    Yh, ih = mb.characterize(src, IDS, chars["mean"], chars["std"], return_index=True)
    scale = torch.from_numpy(np.random.default_rng(1).uniform(1e-3, 50.0, W).astype(np.float32)).to(dev())
    other = torch.from_numpy(((IDS + 1) % 3).astype(np.int32)).to(dev())
    own = torch.from_numpy(IDS.astype(np.int32)).to(dev())
    for slot in (0, 1):                                           # the effective component first, or second behind one of weight 0
        ids = torch.stack([own, other] if slot == 0 else [other, own], 1).contiguous()
        w = torch.zeros((W, 2, 6), device=dev())
        w[:, slot] = scale[:, None]
        Y, idx, wn = mb.characterize(src, None, chars["mean"], chars["std"], return_index=True, mix=(ids, w))
        torch.cuda.synchronize()
        assert torch.equal(idx[:, slot], ih) and bool((idx[:, 1 - slot] == -1).all())
        assert bool((wn[:, slot] == 1.0).all()) and bool((wn[:, 1 - slot] == 0.0).all())
        assert torch.equal(Y, Yh), (dec_cache, slot, float((Y - Yh).abs().max()))
    # J = 1 with a weight per window is the same statement
    Y1 = mb.characterize(src, None, chars["mean"], chars["std"], mix=(own[:, None], scale[:, None]))
    assert torch.equal(Y1, Yh)
    chars["mb"].activate()


@pytest.mark.parametrize("J", [2, 4])
def test_general_weights(chars, J):
    m, mb, src, starts = chars["m"], chars["mb"], chars["src"], chars["starts"]
    mean, std = chars["mean"], chars["std"]
    mb.activate()
    W = len(IDS)
    ids_h, w_h = _general_mix(W, J, 40 + J)
    ids, w = torch.from_numpy(ids_h).to(dev()), torch.from_numpy(w_h).to(dev())
    Y, idx, wn = mb.characterize(src, None, mean, std, return_index=True, mix=(ids, w))
    assert torch.equal(Y, mb.characterize(src, None, mean, std, mix=(ids_h, w_h)))               # host data, no index asked
    # the staged route: encode -> z-score -> query(mix=) -> decoder on its blend -> to_mot; the same kernels on the same values
    enc, _, nm = m.encode(src, mean, std)
    dist, idx_q, wn_q, out = mb.query(nm.reshape(W, D), mix=(ids, w))
    assert torch.equal(idx_q, idx) and torch.equal(wn_q, wn)
    Ys = m.to_mot(m.decoder(enc, out))
    torch.cuda.synchronize()
    assert torch.equal(Y, Ys), float((Y - Ys).abs().max())
    pres = R.present(ids_h, w_h, {0, 1, 2})
    assert pres.any(1).all() and (~pres).any() and np.array_equal(idx.cpu().numpy() >= 0, pres)
    assert np.array_equal(wn.cpu().numpy(), R.normalise(w_h, pres))
    # component 0 names the window's own character wherever the draw left it there: the planted copy is its match
    hard_i = mb.query(chars["nm0"], IDS)[1][:, 0]
    same = torch.from_numpy((ids_h[:, 0] == IDS) & pres[:, 0]).to(dev())
    assert int(same.sum()) >= 6 and torch.equal(idx[:, 0][same], hard_i[same])
    # against the oracle decoder fed the float64 blend, on a sample of windows
    ost = O.to_torch_state(chars["sd"])
    sel = np.array([0, 1, 2, 7, 13, 17, 23])
    rows = np.where(pres, idx.cpu().numpy() + starts[np.clip(ids_h, 0, 2)], 0)
    feats = chars["bank"].reshape(-1, 90, 256)[torch.from_numpy(rows[sel]).to(dev())].cpu().numpy()
    b64 = R.blend(wn.cpu().numpy()[sel], feats, np.float64)
    print(f"J={J}: max |fp32 blend - float64 blend| = {float(np.abs(out.cpu().numpy()[sel] - b64).max()):.3e}")
    with torch.no_grad():
        eo, _ = O.encode(ost, src.cpu()[sel])
        Yo = O.to_mot(ost, O.decoder(ost, eo, torch.from_numpy(b64).float())).numpy()
    err = np.abs(Y.cpu().numpy()[sel] - Yo).max()
    print(f"J={J}: max |Y_mix - Y_oracle(float64 blend)| = {err:.3e}")
    assert err < TOL


@pytest.mark.parametrize("S_w,J", [(1, 2), (3, 2), (16, 4)])
def test_mix_multi_stream_replay_equals_eager(chars, S_w, J):
    m, mb, src = chars["m"], chars["mb"], chars["src"]
    rng = np.random.default_rng(10 * S_w + J)
    mb.activate()
    ms = MultiStreamCharacterizer(mb, chars["mean"], chars["std"], streams=S_w, mix=J)
    gens = []
    for step in range(3):
        win = rng.permutation(len(IDS))[:S_w]
        ids_h, w_h = _general_mix(len(IDS), J, 70 + step)
        ids_h, w_h = ids_h[win], w_h[win]
        if step == 1:
            w_h[0] = 0.0                                             # a stream with nothing present: idx -1, weights 0
        ms.input.copy_(src[win])
        if step == 2:
            Y, idx, wn = ms.step(mix=(ids_h, w_h))                    # through the argument ...
        else:
            ms.mix_ids.copy_(torch.from_numpy(ids_h))                 # ... or written in place: the captured step reads them
            ms.mix_weights.copy_(torch.from_numpy(w_h))
            Y, idx, wn = ms.step()
        Y, idx, wn = Y.clone(), idx.clone(), wn.clone()
        gens.append(m._ctx.generation())
        Ye, ie, we = mb.characterize(src[win], None, chars["mean"], chars["std"], return_index=True, mix=(ids_h, w_h))
        torch.cuda.synchronize()
        assert torch.equal(idx, ie) and torch.equal(wn, we), step
        keep = torch.from_numpy(R.present(ids_h, w_h, {0, 1, 2}).any(1)).to(dev())      # (a window with nothing present: Y unspecified)
        assert torch.equal(Y[keep], Ye[keep]), step
        if step == 1:
            assert bool((idx[0] == -1).all()) and bool((wn[0] == 0).all()) and not bool(keep[0])
    assert gens[0] == gens[-1], gens                                  # captured once: new ids and weights replace nothing
    m.profile_start()                                                 # a step that had to capture again would refuse while profiling
    try:
        Y, idx, wn = ms.step()
    finally:
        m.profile_stop()
    assert torch.equal(idx, ie) and torch.equal(Y[keep], Ye[keep])


def test_mix_refusals(chars):
    m, mb = chars["m"], chars["mb"]
    mb.activate()
    lib, h = m._ctx.lib, m._ctx.h
    vp = lambda t: C.c_void_p(t.data_ptr())                           # noqa: E731
    q = chars["nm0"][:2].contiguous()
    ids = torch.zeros((2, 4), dtype=torch.int32, device=dev())
    w = torch.ones((2, 4, 6), device=dev())
    idx = torch.full((2, 4), 7, dtype=torch.int32, device=dev())
    wn = torch.full((2, 4, 6), 7.0, device=dev())
    Y = torch.full((2, 60, 22, 15), 7.0, device=dev())
    X = chars["src"][:2].contiguous()
    mean = torch.from_numpy(chars["mean"]).to(dev()); std = torch.from_numpy(chars["std"]).to(dev())
    gen = m._ctx.generation()
    for J in (0, 5, -1):
        assert lib.mocha_match_mix_segmented(h, vp(q), 2, vp(ids), vp(w), J, vp(idx), None, vp(wn), None, None) == -1
        assert b"components" in lib.mocha_last_error(h)
    assert lib.mocha_match_mix_segmented(h, vp(q), 2, None, vp(w), 2, vp(idx), None, vp(wn), None, None) == -1
    assert lib.mocha_match_mix_segmented(h, vp(q), 2, vp(ids), None, 2, vp(idx), None, vp(wn), None, None) == -1
    assert lib.mocha_match_mix_segmented(h, vp(q), 2, vp(ids), vp(w), 2, None, None, vp(wn), None, None) == -1
    assert lib.mocha_match_mix_segmented(h, None, 2, vp(ids), vp(w), 2, vp(idx), None, vp(wn), None, None) == -1
    for fn in (lib.mocha_characterize_mix_segmented, lib.mocha_step_graph_mix_segmented):
        for J in (0, 5):
            assert fn(h, vp(X), 2, vp(ids), vp(w), J, vp(mean), vp(std), vp(Y), vp(idx), vp(wn), 0, None) == -1
        assert fn(h, vp(X), 2, None, vp(w), 2, vp(mean), vp(std), vp(Y), vp(idx), vp(wn), 0, None) == -1
        assert fn(h, vp(X), 2, vp(ids), None, 2, vp(mean), vp(std), vp(Y), vp(idx), vp(wn), 0, None) == -1
    assert lib.mocha_step_graph_mix_segmented(h, vp(X), 17, vp(ids), vp(w), 2, vp(mean), vp(std), vp(Y), vp(idx), vp(wn), 0, None) == -1
    assert lib.mocha_step_graph_mix_segmented(h, vp(X), 2, vp(ids), vp(w), 2, vp(mean), vp(std), vp(Y), None, vp(wn), 0, None) == -1
    torch.cuda.synchronize()
    assert bool((idx == 7).all()) and bool((wn == 7).all()) and bool((Y == 7).all()) and m._ctx.generation() == gen      # nothing launched
    # no segment table: MOCHA_ERR_STATE
    from mocha_sigasia2023_amd import ContextBank
    ContextBank(m, chars["banks"][0][0], chars["banks"][0][1])
    assert lib.mocha_match_mix_segmented(h, vp(q), 2, vp(ids), vp(w), 2, vp(idx), None, vp(wn), None, None) == -3
    assert lib.mocha_characterize_mix_segmented(h, vp(X), 2, vp(ids), vp(w), 2, vp(mean), vp(std), vp(Y), vp(idx), vp(wn), 0, None) == -3
    torch.cuda.synchronize()
    assert bool((idx == 7).all()) and bool((Y == 7).all())
    mb.activate()
    gen = m._ctx.generation()
    # the Python layer: mix does not combine with soft, allow / constrained, inertial or the Ours sessions, and J is 1 .. 4
    mix = ([0, 1], [0.5, 0.5])
    with pytest.raises(ValueError, match="does not combine"):
        mb.characterize(X, None, mean, std, mix=mix, soft=(2, 1.0))
    with pytest.raises(ValueError, match="does not combine"):
        mb.characterize(X, None, mean, std, mix=mix, allow=[1, 1])
    with pytest.raises(ValueError, match="does not combine"):
        mb.characterize(X, [0, 1], mean, std, mix=mix)
    with pytest.raises(ValueError, match="does not combine"):
        mb.query(q, mix=mix, k=2)
    with pytest.raises(ValueError, match="does not combine"):
        mb.query(q, mix=mix, allow=[1, 1])
    for J in (0, 5):
        with pytest.raises(ValueError):
            MultiStreamCharacterizer(mb, mean, std, streams=2, mix=J)
        with pytest.raises(ValueError):
            LiveSession(mb, mean, std, streams=2, mix=J)
        with pytest.raises(ValueError):
            mb.query(q, mix=(np.zeros((2, J), np.int32), np.ones((2, J), np.float32)))
    with pytest.raises(ValueError, match="does not combine"):
        MultiStreamCharacterizer(mb, mean, std, streams=2, mix=2, soft=(2, 1.0))
    with pytest.raises(ValueError, match="does not combine"):
        MultiStreamCharacterizer(mb, mean, std, streams=2, mix=2, constrained=True)
    for kw in (dict(soft=(2, 1.0)), dict(inertial=0.1), dict(constrained=True)):
        with pytest.raises(ValueError, match="does not combine"):
            LiveSession(mb, mean, std, streams=2, mix=2, **kw)
    with pytest.raises(ValueError, match="mix= is not supported"):
        LiveOursSession(mb, mean, std, None, None, None, None, None, streams=2, mix=2)
    assert m._ctx.generation() == gen
