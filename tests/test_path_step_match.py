"""mocha_match_path_segmented on the MI355X (run with -m gpu): the online path step against a segmented bank of three characters of 17,
1 030 and 40 rows at the real width D = 23 040 (about 100 MB), with one exact duplicate pair of rows.

* dist_row - every d[j] the step saw - equals mocha_match_dist_matrix over the character's range bit for bit, and nothing past the
  character's rows is written;
* idx, dist and continued of every step equal tests/path_step_ref.py on those distances (streams on different characters, a character
  switch, an id outside the table, a restart word, clip starts from mocha_bank_set_starts);
* the same bank with a bf16 copy gives the same bits (the step reads the fp32 rows whatever the bank's flags);
* planted case: character 1 is two random-walk clips of 515 rows; 80 noisy queries (noise 8.0 per value) follow rows 100..139 of the
  first clip, then jump to rows 600..639 of the second.  In float64 NumPy on the host the hard match finds 48 of the 80 planted rows
  and the online restatement at jump = 6.0 (0.005 x the median nearest distance, 1 214) finds 80, as the whole-clip path does; the
  asserted bounds are <= 60 and >= 78.  On the device idx equals the restatement on the device's own distances exactly, and finds >= 78."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from mocha_sigasia2023_amd import Generator, MultiCharacterBank, weights  # noqa: E402
from path_step_ref import PathStepRef  # noqa: E402

pytestmark = pytest.mark.gpu
D = 90 * 256
SIZES = (17, 1030, 40)
FIRST = (0, 17, 1047)
STARTS = ([], [515], [7])                # local rows that begin a clip
DUP = (10, 11)                           # an exact duplicate pair of rows of character 2
PLANTED = np.r_[100:140, 600:640]
NOISE, JUMP = 8.0, 6.0
STATE_ROWS = 1040
T = 12


def dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return torch.device("cuda:0")


def stream():
    return C.c_void_p(torch.cuda.current_stream(dev()).cuda_stream)


def ptr(t):
    return C.c_void_p(0 if t is None else t.data_ptr())


@pytest.fixture(scope="module")
def model():
    sd = weights.synthetic_state_dict(1777, 1.0, "mixamo")
    return Generator(layout="mixamo", device=dev()).load_state_dict(sd).eval()


@pytest.fixture(scope="module")
def data():
    rng = np.random.default_rng(35)
    clips = [np.cumsum(0.1 * rng.standard_normal((515, D)), 0) for _ in range(2)]
    walk = np.concatenate(clips).astype(np.float32)
    qp = (walk[PLANTED] + NOISE * rng.standard_normal((80, D))).astype(np.float32)
    # the planted case's own precondition, float64 on the host
    b, qq = walk.astype(np.float64), qp.astype(np.float64)
    d = np.sqrt(np.maximum((qq * qq).sum(1)[:, None] + (b * b).sum(1)[None] - 2.0 * qq @ b.T, 0.0))
    hard = int((d.argmin(1) == PLANTED).sum())
    ref = PathStepRef(1, JUMP)
    online = int(sum(ref.step_stream(0, d[t], 1, first=FIRST[1], starts=STARTS[1])[0] == PLANTED[t] for t in range(80)))
    assert hard <= 60 and online >= 78, (hard, online)
    rng = np.random.default_rng(36)
    c0 = rng.standard_normal((SIZES[0], D), dtype=np.float32)
    c2 = rng.standard_normal((SIZES[2], D), dtype=np.float32)
    c2[DUP[1]] = c2[DUP[0]]
    chars = [c0, walk, c2]
    # the scenario of the first two tests: three streams, T steps; the rows the queries sit near advance by one per step
    ids = np.tile(np.array([0, 1, 2], dtype=np.int32), (T, 1))
    ids[6:, 2] = 0                                   # a character switch
    ids[5, 0] = 3                                    # an id outside the table: sits out, then restarts
    ids[9, 1] = -1
    q = np.empty((T, 3, D), dtype=np.float32)
    for t in range(T):
        for s in range(3):
            c = int(ids[t, s]) if 0 <= ids[t, s] < 3 else 0
            base = (2, 510, 5)[s] + t                # stream 1 walks over the clip start at row 515, stream 2 over the duplicate pair
            q[t, s] = chars[c][base % SIZES[c]] + (2.0 if s == 1 else 0.3) * rng.standard_normal(D, dtype=np.float32)
    q[5, 2] = c2[DUP[0]] + 0.01 * rng.standard_normal(D, dtype=np.float32)
    flags = np.zeros((T, 3), dtype=np.int32)
    flags[3, 1] = 1                                  # a restart word
    return chars, qp, q, ids, flags


def make_bank(model, chars, bf16):
    banks = [(torch.from_numpy(c).to(dev()), torch.zeros((len(c), 90, 256), dtype=torch.float32, device=dev())) for c in chars]
    return MultiCharacterBank(model, banks, bf16=bf16, dec_cache=False, starts=list(STARTS))


def run_steps(model, q, ids, flags, lam):
    """mocha_match_path_segmented step by step -> per step (idx, dist, continued, dist_row) as numpy, and the restart words at the end."""
    ctx = model._ctx
    steps, S = ids.shape
    nbytes = int(ctx.lib.mocha_path_state_bytes(ctx.h, S, STATE_ROWS))
    state = torch.zeros((nbytes,), dtype=torch.uint8, device=dev())
    restart = torch.zeros((S,), dtype=torch.int32, device=dev())
    q_dev, ids_dev, flags_dev = torch.from_numpy(q).to(dev()), torch.from_numpy(ids).to(dev()), torch.from_numpy(flags).to(dev())
    idx = torch.full((steps, S), -7, dtype=torch.int32, device=dev())
    dist = torch.full((steps, S), float("nan"), dtype=torch.float32, device=dev())
    cont = torch.full((steps, S), 9, dtype=torch.uint8, device=dev())
    rows = torch.full((steps, S, STATE_ROWS), float("nan"), dtype=torch.float32, device=dev())
    for t in range(steps):
        if flags[t].any():
            restart.copy_(torch.maximum(restart, flags_dev[t]))
        ctx.call("mocha_match_path_segmented", ptr(state), S, STATE_ROWS, ptr(q_dev[t]), ptr(ids_dev[t]), ptr(restart), C.c_double(lam), ptr(idx[t]),
                 ptr(dist[t]), ptr(cont[t]), ptr(rows[t]), C.c_int64(STATE_ROWS), stream())
    torch.cuda.synchronize()
    return idx.cpu().numpy(), dist.cpu().numpy(), cont.cpu().numpy(), rows.cpu().numpy(), restart.cpu().numpy()


def matrix(model, q_dev, c):
    """mocha_match_dist_matrix of the queries against character c's range -> (Q, rows of c) numpy."""
    Q, n = q_dev.shape[0], SIZES[c]
    out = torch.empty((Q, n), dtype=torch.float32, device=dev())
    model._ctx.call("mocha_match_dist_matrix", ptr(q_dev), Q, C.c_int64(FIRST[c]), C.c_int64(n), ptr(out), C.c_int64(n), stream())
    return out.cpu().numpy()


def restate(ids, flags, rows, lam):
    """tests/path_step_ref.py on the device's own distances -> idx, dist, continued (steps, S) and the restart words left."""
    steps, S = ids.shape
    ref = PathStepRef(S, lam)
    words = np.zeros(S, dtype=np.int32)
    ei = np.zeros((steps, S), dtype=np.int32)
    ed = np.zeros((steps, S), dtype=np.float32)
    ec = np.zeros((steps, S), dtype=np.uint8)
    for t in range(steps):
        words = np.maximum(words, flags[t])
        for s in range(S):
            e = int(ids[t, s])
            ok = 0 <= e < 3
            ei[t, s], ed[t, s], ec[t, s], used = ref.step_stream(s, rows[t, s, :SIZES[e]] if ok else None, e if ok else -1, first=FIRST[e] if ok else 0,
                                                                 starts=STARTS[e] if ok else (), restart=bool(words[s]))
            if used:
                words[s] = 0
    return ei, ed, ec, words


@pytest.fixture(scope="module")
def fp32_run(model, data):
    chars, qp, q, ids, flags = data
    bank = make_bank(model, chars, bf16=False)
    out = run_steps(model, q, ids, flags, JUMP)
    # the matrix's entries for every (step, stream), from the existing call
    q_dev = torch.from_numpy(q).to(dev())
    mats = {}
    for t in range(T):
        for c in set(int(e) for e in ids[t] if 0 <= e < 3):
            mats[(t, c)] = matrix(model, q_dev[t], c)
    planted = run_steps(model, qp[:, None, :], np.full((80, 1), 1, dtype=np.int32), np.zeros((80, 1), dtype=np.int32), JUMP)
    hard = bank.query(torch.from_numpy(qp).to(dev()), np.full(80, 1))[1][:, 0].cpu().numpy()
    return out, mats, planted, hard


def test_dist_row_is_the_matrix_bit_for_bit(fp32_run, data):
    (idx, dist, cont, rows, words), mats, _, _ = fp32_run
    _, _, _, ids, _ = data
    for t in range(T):
        for s in range(3):
            e = int(ids[t, s])
            if not 0 <= e < 3:
                assert np.isnan(rows[t, s]).all(), (t, s)                     # a stream that sits out writes no distance
                continue
            n = SIZES[e]
            assert np.array_equal(rows[t, s, :n].view(np.uint32), mats[(t, e)][s].view(np.uint32)), (t, s)
            assert np.isnan(rows[t, s, n:]).all(), "columns past the character's rows were written"
    t, s = 5, 2
    assert rows[t, s, DUP[0]] == rows[t, s, DUP[1]]                            # the duplicate pair: equal distances


def test_rows_equal_the_restatement(fp32_run, data):
    (idx, dist, cont, rows, words), _, _, _ = fp32_run
    _, _, _, ids, flags = data
    ei, ed, ec, ew = restate(ids, flags, rows, JUMP)
    assert np.array_equal(idx, ei), (idx.tolist(), ei.tolist())
    assert np.array_equal(dist.view(np.uint32), ed.view(np.uint32))
    assert np.array_equal(cont, ec)
    assert np.array_equal(words, ew) and not words.any()
    assert idx[5, 0] == -1 and np.isinf(dist[5, 0]) and idx[9, 1] == -1 and idx[6, 0] >= 0
    assert cont.sum() > 0 and cont[6, 2] == 0                                # continuations happen; the switch of stream 2 restarts
    at_start = (idx == STARTS[1][0]) & (np.arange(3)[None] == 1)
    assert at_start.any() and not cont[at_start].any()                       # row 515 starts a clip: reaching it is never a continuation


def test_planted_path(fp32_run, data):
    _, _, (idx, dist, cont, rows, _), hard = fp32_run
    ids = np.full((80, 1), 1, dtype=np.int32)
    ei, ed, ec, _ = restate(ids, np.zeros((80, 1), dtype=np.int32), rows, JUMP)
    assert np.array_equal(idx, ei) and np.array_equal(cont, ec) and np.array_equal(dist.view(np.uint32), ed.view(np.uint32))
    found = int((idx[:, 0] == PLANTED).sum())
    print(f"planted rows found: online {found}, hard (device) {int((hard == PLANTED).sum())}")
    assert found >= 78
    assert int((hard == PLANTED).sum()) <= 60
    assert cont[0, 0] == 0 and cont[40, 0] == 0                              # the first window and the planted jump


def test_bf16_bank_gives_the_same_bits(model, fp32_run, data):
    (idx, dist, cont, rows, words), _, _, _ = fp32_run
    chars, _, q, ids, flags = data
    make_bank(model, chars, bf16=True)
    i2, d2, c2, r2, w2 = run_steps(model, q, ids, flags, JUMP)
    assert np.array_equal(i2, idx) and np.array_equal(c2, cont) and np.array_equal(w2, words)
    assert np.array_equal(d2.view(np.uint32), dist.view(np.uint32))
    assert np.array_equal(r2.view(np.uint32), rows.view(np.uint32))           # (NaN fill included: the same columns were written)


def test_refusals(model, fp32_run, data):
    chars = data[0]
    make_bank(model, chars, bf16=False)
    lib, h = model._ctx.lib, model._ctx.h
    S = 2
    nbytes = int(lib.mocha_path_state_bytes(h, S, STATE_ROWS))
    state = torch.zeros((nbytes,), dtype=torch.uint8, device=dev())
    q = torch.zeros((S, D), dtype=torch.float32, device=dev())
    ids = torch.zeros((S,), dtype=torch.int32, device=dev())
    idx = torch.full((S,), -7, dtype=torch.int32, device=dev())

    def call(state_=state, streams=S, state_rows=STATE_ROWS, q_=q, ids_=ids, lam=1.0, idx_=idx, row=None, ld=0):
        return lib.mocha_match_path_segmented(h, ptr(state_), streams, state_rows, ptr(q_), ptr(ids_), None, lam, ptr(idx_), None, None, ptr(row), ld,
                                              stream())
    for kw in (dict(state_=None), dict(q_=None), dict(ids_=None), dict(idx_=None), dict(streams=0), dict(streams=17), dict(lam=-1.0),
               dict(lam=float("nan")), dict(lam=float("inf")), dict(state_rows=0), dict(state_rows=16385), dict(row=q, ld=STATE_ROWS - 1)):
        assert call(**kw) == -1, kw
    assert call(state_rows=1029) == -3                                        # MOCHA_ERR_STATE: the largest character has 1 030 rows
    torch.cuda.synchronize()
    assert bool((idx == -7).all()) and not bool(state.any())
    # starts: unsorted or out of range
    bad = (C.c_int64 * 2)(5, 5)
    assert lib.mocha_bank_set_starts(h, bad, 2, stream()) == -1
    bad = (C.c_int64 * 1)(sum(SIZES))
    assert lib.mocha_bank_set_starts(h, bad, 1, stream()) == -1
