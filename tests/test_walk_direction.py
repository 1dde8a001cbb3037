"""Option "walk" (include/mocha_hip.h): the order in which the row-walking kernels of the batch path touch their row blocks - 0 upwards,
1 alternating from step to step (the default), 2 every eligible launch downwards.  Only the map from workgroup (or walk step) to row block
is mirrored, so every result must be bit-identical between the three settings.  The window counts are the smallest that reach each kernel
instance and each edge of its tile walk (comments at the cases)."""
import numpy as np
import pytest
import torch

from mocha_sigasia2023_amd import ContextBank, Generator, StreamingCharacterizer, synthetic, weights

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SEED, GAIN = 1777, 1.0


@pytest.fixture(scope="module")
def norm():
    mean, std = synthetic.cnt_norm(13)
    return torch.from_numpy(mean).to(DEV), torch.from_numpy(std).to(DEV)


def _model(layout):
    return Generator(layout=layout, device=DEV).load_state_dict(weights.synthetic_state_dict(seed=SEED, gain=GAIN, layout=layout)).eval()


@pytest.fixture(scope="module")
def model22():
    return _model("mixamo")                    # 22 joints


@pytest.fixture(scope="module")
def model24():
    return _model("mocha")                     # 24 joints: the shipped layout


def _windows(seed, n, V):
    return torch.from_numpy(synthetic.pose_windows(seed, n, V)).to(DEV)


def _pair(model, src, cha, norm):
    out = model.characterize_pair(src, cha, norm[0], norm[1], return_index=True, return_bank=True)
    torch.cuda.synchronize()
    return [t.clone() for t in out]            # Y, idx, cha_encoded, cha_cnt_nm


def _same(a, b, what):
    for name, x, y in zip(("Y", "idx", "cha_encoded", "cha_cnt_nm"), a, b):
        assert torch.equal(x, y), f"{what}: {name} differs"


def _pair_all_walks(model, n_src, n_cha, norm, options=()):
    src, cha = _windows(901, n_src, model.V), _windows(902, n_cha, model.V)
    for k, v in options:
        model.set_option(k, v)
    try:
        res = []
        for walk in (0, 1, 2):
            model.set_option("walk", walk)
            res.append(_pair(model, src, cha, norm))
    finally:
        model.set_option("walk", 1)
    assert torch.isfinite(res[0][0]).all()
    _same(res[0], res[1], f"{n_cha} + {n_src} windows, walk 1 against 0")
    _same(res[0], res[2], f"{n_cha} + {n_src} windows, walk 2 against 0")


# 280 windows: 25 200 rows = 196 full 128-row tiles + one of 112 rows; the encoder's N = 256 launches have 2 x 197 tiles and the decoder's and
# to_mot's (277 windows) 2 x 195 - from 192 m-tiles at N = 256 a launch is no longer mid-size, so they take the persistent instance; with 8
# workgroups it walks ~50 rounds, the mirrored walk starting at the partial tile
@pytest.mark.parametrize("n_cha,n_src", [(3, 277), (277, 3)])
def test_full_batch_persistent_many_rounds(model22, norm, n_cha, n_src):
    try:
        _pair_all_walks(model22, n_src, n_cha, norm, options=(("gemm_persistent", 8),))
    finally:
        model22.set_option("gemm_persistent", 768)


# the same shapes on the shipped layout with the default 768 workgroups: one round, the grid smaller than the (padded) tile count
@pytest.mark.parametrize("n_cha,n_src", [(3, 277), (277, 3)])
def test_full_batch_shipped_layout(model24, norm, n_cha, n_src):
    _pair_all_walks(model24, n_src, n_cha, norm)


# 17 windows: 1 530 rows = 12 m-tiles of 128 (24 of 64) - the XCD-aware order with padded m-tiles, the 64-row and 64 x 64 mid-size tiles
def test_xcd_order_mid_size(model22, norm):
    _pair_all_walks(model22, 8, 9, norm)


# 5 windows: fewer than 8 m-tiles - the plain tile order
def test_plain_order(model22, norm):
    _pair_all_walks(model22, 2, 3, norm)


def test_three_calls_chunked(norm):
    """encode + ContextBank + characterize with 7 windows in chunks of 4: the walk order starts over with every chunk."""
    m = _model("mixamo").reserve(4)
    src, cha = _windows(901, 7, m.V), _windows(902, 7, m.V)
    res = []
    for walk in (0, 1, 2):
        m.set_option("walk", walk)
        enc, cnt, nm = m.encode(cha, norm[0], norm[1])
        bank = ContextBank(m, nm, enc)
        Y, idx = bank.characterize(src, norm[0], norm[1], return_index=True)
        torch.cuda.synchronize()
        res.append([Y.clone(), idx.clone(), enc.clone(), nm.clone()])
    _same(res[0], res[1], "three calls, walk 1 against 0")
    _same(res[0], res[2], "three calls, walk 2 against 0")


def test_captured_step(model22, norm):
    """One window through the captured per-window step: walk = 1 replays the bits of walk = 0, and a replay does not move the generation."""
    m = model22
    enc, cnt, nm = m.encode(_windows(902, 5, m.V), norm[0], norm[1])
    bank = ContextBank(m, nm, enc)
    win = _windows(901, 1, m.V)
    try:
        m.set_option("walk", 0)
        sc = StreamingCharacterizer(bank, norm[0], norm[1])
        Y, idx = sc.step(win[0])
        torch.cuda.synchronize()
        Y0, i0 = Y.clone(), idx.clone()
        m.set_option("walk", 1)
        Y, idx = sc.step(win[0])                # captured again: the option moved the generation
        torch.cuda.synchronize()
        assert torch.equal(Y, Y0) and torch.equal(idx, i0)
        gen = m._ctx.generation()
        for _ in range(2):
            Y, idx = sc.step(win[0])
            torch.cuda.synchronize()
            assert torch.equal(Y, Y0) and torch.equal(idx, i0)
        assert m._ctx.generation() == gen
    finally:
        m.set_option("walk", 1)


def test_two_contexts_two_streams(norm):
    """Two contexts with different walk values on two streams at once: each returns what it returns alone."""
    models = [_model("mixamo"), _model("mixamo")]
    models[0].set_option("walk", 1)
    models[1].set_option("walk", 2)
    src, cha = _windows(901, 8, 22), _windows(902, 9, 22)
    alone = [_pair(m, src, cha, norm) for m in models]
    _same(alone[0], alone[1], "walk 2 against 1")
    streams = [torch.cuda.Stream(device=DEV) for _ in models]
    torch.cuda.synchronize()
    got = [[], []]
    for _ in range(3):
        for k, m in enumerate(models):
            with torch.cuda.stream(streams[k]):
                got[k].append(m.characterize_pair(src, cha, norm[0], norm[1], return_index=True, return_bank=True))
    torch.cuda.synchronize()
    for k in range(2):
        for r in got[k]:
            _same(alone[k], list(r), f"context {k} beside the other")
