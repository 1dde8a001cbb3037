"""The restatement of the online path step (tests/path_step_ref.py) against the whole-clip restatement (tests/path_ref.py), no GPU:
the row the step emits at window t is the last row of the whole-clip path over windows 0..t; lambda = 0 is the arg-min; and the restart
rules - id change, extent change, epoch change, the one-shot flag, a sit-out step, reset - each start a new path."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from path_ref import path_ref  # noqa: E402
from path_step_ref import PathStepRef  # noqa: E402


def matrices():
    out = []
    for seed in range(12):
        rng = np.random.default_rng(100 + seed)
        Q, N = int(rng.integers(1, 41)), int(rng.integers(1, 13))
        if seed % 2:
            d = rng.integers(0, 4, (Q, N)).astype(np.float32)              # tie-laden: few distinct values, ties in d and in a == lambda
        else:
            d = rng.uniform(0.5, 2.0, (Q, N)).astype(np.float32)
        starts = sorted(set(int(x) for x in rng.integers(0, N, int(rng.integers(0, 4)))))
        out.append((d, starts))
    return out


@pytest.mark.parametrize("lam", [0.0, 0.25, 1.0, 2.0, 1e6])
def test_row_at_t_is_the_last_row_of_the_path_over_the_prefix(lam):
    for d, starts in matrices():
        ref = PathStepRef(1, lam)
        for t in range(len(d)):
            m, dist, cont, _ = ref.step_stream(0, d[t], 0, starts=starts)
            whole = path_ref(d[:t + 1], lam, bank_starts=starts)[0]
            assert m == whole[-1], (lam, t, starts)
            assert dist == d[t, m]
            if t == 0:
                assert cont == 0


def test_lambda_zero_is_the_argmin():
    for d, starts in matrices():
        ref = PathStepRef(1, 0.0)
        for t in range(len(d)):
            m, _, cont, _ = ref.step_stream(0, d[t], 0, starts=starts)
            assert m == int(np.argmin(d[t]))


def planted(N=10, Q=12):
    """Distances whose coherent row runs 2, 3, 4, ... while a far row 8 is marginally nearer at every other window."""
    d = np.full((Q, N), 5.0, dtype=np.float32)
    for t in range(Q):
        d[t, min(2 + t, N - 1)] = 1.0
        if t % 2:
            d[t, 8 if 2 + t != 8 else 0] = 0.9
    return d


def test_continues_where_the_argmin_flickers():
    d = planted()
    ref = PathStepRef(1, 1.0)
    rows = [ref.step_stream(0, d[t], 0)[0] for t in range(6)]
    assert rows == [2, 3, 4, 5, 6, 7]
    assert [int(np.argmin(d[t])) for t in range(6)] == [2, 8, 4, 8, 6, 8]


@pytest.mark.parametrize("how", ["id", "extent", "epoch", "flag", "sit-out", "reset"])
def test_restart_rules(how):
    d = planted()
    ref = PathStepRef(2, 1.0)
    for t in range(3):
        assert ref.step_stream(0, d[t], 4)[0] == 2 + t
    # window 3 continues when nothing happened: row 5, although row 8 is nearer
    e, first, epoch, flag, dd = 4, 0, 0, False, d[3]
    if how == "id":
        e = 5
    elif how == "extent":
        first = 16
    elif how == "epoch":
        epoch = 1
    elif how == "flag":
        flag = True
    elif how == "sit-out":
        assert ref.step_stream(0, None, -1) == (-1, np.float32(np.inf), 0, False)
        assert ref.st[0].running is False
    elif how == "reset":
        ref.reset([0])
    m, dist, cont, used = ref.step_stream(0, dd, e, first=first, epoch=epoch, restart=flag)
    assert (m, cont) == (8, 0), how                                         # a restart: the arg-min, not a continuation
    assert used == (how == "flag")
    # ... and the path goes on from there
    m, _, cont, _ = ref.step_stream(0, d[4], e, first=first, epoch=epoch)
    assert (m, cont) == (6, 0)                                              # row 6 continues row 5 of the restarted R; the EMITTED row came from 8


def test_a_start_has_no_predecessor():
    d = planted()
    ref = PathStepRef(1, 1.0)
    assert ref.step_stream(0, d[0], 0, starts=[3])[0] == 2
    m, _, cont, _ = ref.step_stream(0, d[1], 0, starts=[3])
    assert (m, cont) == (8, 0)                                              # row 3 starts a clip: 2 -> 3 is a jump, and 8 is nearer


def test_advance_wraps_the_streams():
    rng = np.random.default_rng(5)
    d = rng.uniform(1, 2, (3, 9)).astype(np.float32)
    ref = PathStepRef(3, 0.5)
    restart = np.array([0, 1, 1], dtype=np.int32)
    idx, dist, cont = ref.advance(d, np.array([0, -1, 2]), np.array([9, 9, 4]), restart=restart)
    assert idx[1] == -1 and np.isinf(dist[1]) and restart.tolist() == [0, 1, 0]      # a stream that sits out consumes nothing
    assert idx[0] == int(np.argmin(d[0])) and idx[2] == int(np.argmin(d[2, :4]))
    idx, _, _ = ref.advance(d, np.array([0, 1, 2]), np.array([9, 12, 4]), limit=16)
    assert idx[1] == -1                                                     # more rows than the leading dimension: sits out
