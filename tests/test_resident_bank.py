"""ResidentCharacterBank / mocha_bank_resident_* on the MI355X (run with -m gpu): characters added to and retired from one bank in place,
compared bit for bit with a FRESH MultiCharacterBank(labels=) of the characters that are live, in slot order, on a second model with the
same weights (tests/resident_world.py: characters A .. F of 33, 30, 20, 17, 16 and 1 rows; capacity 160 rows = 10 granules, 6 slots, at
most 48 rows per character).

The sequence: add A, B, C; retire B; add D (B's extent, B's slot); add E, F; retire A; add B (shorter than A: A's extent, A's slot, one
granule left over); add C as a seventh request - refused, MOCHA_ERR_STATE: 32 rows are free, the largest extent is 16.  Every extent is
asserted against the test's own model of first fit, and the generation does not move from the first add on.

After the third, fifth and ninth operation (three, three and five live characters): 6 windows spread over the live characters -
query (k = 1 and k = 3), query(allow=), characterize hard, soft and allow= - every idx, dist, weight, applied and Y equal to the fresh
bank's (torch.equal).  A's own bank rows asked in the slot B now occupies give B's answer from the fresh bank, dist > 0, also under a mask
that names an action A had and B has not: rows, label bytes, granule words and the `any` word A left behind would show there.  An id
naming an empty slot gives -1 / +inf / weights 0 / applied 0.  Then the refusals and every union call.

Mutations run on a scratch copy of the library, and the tests that failed:
  * gran_start = first_row / 16 + 1 in the publish kernel: test_sequence (the first comparison, "A B C": query(allow=)) and
    test_resident_live.py::test_multi_stream_characterizer[True];
  * add leaving the slot's previous `any` word in place (the label kernel OR-ing into it): test_sequence (the comparison after D took
    B's slot, "A D C": D answers constrained where the fresh bank falls back);
  * retire freeing the extent but leaving the row count: test_sequence (the empty-slot check after the retire of B, "A - C") and
    test_resident_live.py::test_multi_stream_characterizer[False], [True] and test_live_session (frame 66: valid stays 1);
  * the add path taking launch_linear_f64's default kernel choice: NOTHING failed on this data.  The two float64 summation orders differ
    in the last bits of a double, and the style MLP's result is rounded to fp32: gamma / beta of E (16 rows) and F (1 row) came out the
    same.  test_small_characters_take_the_tiled_style_mlp and the last comparison of test_sequence are where a difference would show
    (hard characterize of windows matched to E and F, bit for bit); the property itself - a row's result does not depend on the
    launch's row count - is the tiled kernel's by construction (one fma chain over ascending k per output)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import resident_world as RW  # noqa: E402
from mocha_sigasia2023_amd import ContextBank, MultiCharacterBank, MultiStreamCharacterizer, ResidentCharacterBank, action_mask  # noqa: E402

pytestmark = pytest.mark.gpu
A, B, C, D, E, F = range(6)
NAMES = "ABCDEF"
# six masks: constrained for some characters, nothing asked, falling back for others
MASKS = [action_mask([1]), action_mask([0, 1]), action_mask([0, 1, 2]), 0, action_mask([3, 4, 5]), action_mask([6, 7])]


@pytest.fixture(scope="module")
def world():
    w = RW.build(70, 3)
    # six windows: the three streams' windows ending at frames 59 and 66
    w["X"] = torch.cat([RW.windows(w, 59), RW.windows(w, 66)]).contiguous()
    _, _, nm = w["model"].encode(w["X"], w["mean"], w["std"], raw=True)
    w["q"] = nm.reshape(6, -1).contiguous()
    return w


def _add(w, rb, ch, slot=None):
    nm, enc = w["banks"][ch]
    lab = None if ch == F else (torch.from_numpy(RW.LABELS[ch]).to(RW.dev()) if ch == D else RW.LABELS[ch])      # none / device / host labels
    return rb.add(nm, enc, labels=lab, slot=slot)


def _fresh(w, live):
    """The reference: a fresh labelled MultiCharacterBank of the live characters in slot order, and slot -> its id there."""
    slots = sorted(live)
    mb = MultiCharacterBank(w["ref_model"], [w["banks"][live[s]] for s in slots], labels=[RW.LABELS[live[s]] for s in slots])
    return mb, {s: i for i, s in enumerate(slots)}


def _same(a, b, what):
    assert len(a) == len(b), what
    for i, (x, y) in enumerate(zip(a, b)):
        assert x.shape == y.shape and torch.equal(x, y), (what, i, x, y) if x.numel() < 64 else (what, i, float((x - y).abs().max()))


def _compare(w, rb, live, tag):
    """Every segmented call on 6 windows spread over the live characters: the resident bank against the fresh one, bit for bit."""
    mb, rank = _fresh(w, live)
    slots = sorted(live)
    ids = [slots[i % len(slots)] for i in range(6)]
    rids = [rank[s] for s in ids]
    q, X, mean, std = w["q"], w["X"], w["mean"], w["std"]
    for k in (1, 3):
        _same(rb.query(q, ids, k=k), mb.query(q, rids, k=k), (tag, "query", k))
        _same(rb.query(q, ids, k=k, allow=MASKS, return_applied=True), mb.query(q, rids, k=k, allow=MASKS, return_applied=True), (tag, "query allow", k))
    _same(rb.characterize(X, ids, mean, std, return_index=True, raw=True), mb.characterize(X, rids, mean, std, return_index=True, raw=True), (tag, "hard"))
    _same(rb.characterize(X, ids, mean, std, return_index=True, raw=True, soft=RW.SOFT),
          mb.characterize(X, rids, mean, std, return_index=True, raw=True, soft=RW.SOFT), (tag, "soft"))
    got = rb.characterize(X, ids, mean, std, return_index=True, raw=True, allow=MASKS)
    _same(got, mb.characterize(X, rids, mean, std, return_index=True, raw=True, allow=MASKS), (tag, "allow"))
    _same(rb.characterize(X, ids, mean, std, return_index=True, raw=True, allow=MASKS, soft=RW.SOFT),
          mb.characterize(X, rids, mean, std, return_index=True, raw=True, allow=MASKS, soft=RW.SOFT), (tag, "soft allow"))
    torch.cuda.synchronize()
    assert bool((got[1] >= 0).all()), (tag, got[1])
    return got[-1].tolist()


def _empty_slot(w, rb, slot, tag):
    """An id naming an empty slot, next to one naming a live character: -1 / +inf / 0."""
    q, X, mean, std = w["q"][:2], w["X"][:2], w["mean"], w["std"]
    live = next(s for s in range(rb.S) if rb.rows(s)[0] != rb.rows(s)[1])
    ids = [slot, live]
    for k in (1, 3):
        dist, idx = rb.query(q, ids, k=k)
        assert idx[0].tolist() == [-1] * k and bool(torch.isinf(dist[0]).all()) and int(idx[1, 0]) >= 0, (tag, idx, dist)
        dist, idx, ap = rb.query(q, ids, k=k, allow=[MASKS[1]] * 2, return_applied=True)
        assert idx[0].tolist() == [-1] * k and bool(torch.isinf(dist[0]).all()) and int(ap[0]) == 0, (tag, idx, dist, ap)
    _, idx = rb.characterize(X, ids, mean, std, return_index=True, raw=True)
    assert int(idx[0]) == -1 and int(idx[1]) >= 0, (tag, idx)
    _, idx_k, wk = rb.characterize(X, ids, mean, std, return_index=True, raw=True, soft=RW.SOFT)
    assert idx_k[0].tolist() == [-1] * RW.SOFT[0] and wk[0].tolist() == [0.0] * RW.SOFT[0] and abs(float(wk[1].sum()) - 1.0) < 1e-5, (tag, idx_k, wk)


def test_sequence(world):
    w = world
    model = w["model"]
    rb = ResidentCharacterBank(model, RW.CAPACITY, RW.MAX_CHARACTERS, RW.MAX_ROWS)
    assert rb.S == 6 and rb.free_rows == 160 and rb.largest_free == 160 and all(rb.rows(s) == (0, 0) for s in range(6))
    zeros = torch.zeros((6, 60, RW.J, 15), device=RW.dev())
    for kw in (dict(), dict(soft=RW.SOFT)):                 # eager first, on empty slots: the workspaces for 6 windows exist
        rb.characterize(zeros, [0] * 6, w["mean"], w["std"], raw=True, **kw)
    gen = model._ctx.generation()
    free = [True] * (RW.CAPACITY // 16)                     # the test's own first fit, in 16-row units
    live = {}

    def add(ch, want_slot):
        first = RW.first_fit(free, -(-RW.ROWS[ch] // 16))
        assert first is not None
        slot = _add(w, rb, ch)
        assert slot == want_slot and rb.rows(slot) == (16 * first, 16 * first + RW.ROWS[ch]), (NAMES[ch], slot, rb.rows(slot), first)
        live[slot] = ch
        assert rb.free_rows == 16 * sum(free) and model._ctx.generation() == gen, NAMES[ch]

    def retire(slot):
        first, stop = rb.rows(slot)
        rb.retire(slot)
        for u in range(first // 16, -(-stop // 16)):
            free[u] = True
        del live[slot]
        assert rb.rows(slot) == (0, 0) and rb.free_rows == 16 * sum(free) and model._ctx.generation() == gen

    add(A, 0); add(B, 1); add(C, 2)                         # 1
    assert [rb.rows(s) for s in range(3)] == [(0, 33), (48, 78), (80, 100)]
    assert _compare(w, rb, live, "A B C") == [1, 1, -1, 0, -1, -1]
    _empty_slot(w, rb, 4, "A B C")
    retire(1)                                               # 2
    _empty_slot(w, rb, 1, "A - C")
    add(D, 1)                                               # 3: B's extent, B's slot
    assert rb.rows(1) == (48, 65)
    _compare(w, rb, live, "A D C")
    add(E, 3); add(F, 4)                                    # 4
    assert rb.rows(3) == (112, 128) and rb.rows(4) == (128, 129)
    retire(0)                                               # 5
    _empty_slot(w, rb, 0, "- D C E F")
    add(B, 0)                                               # 6: shorter than A: A's extent, A's slot
    assert rb.rows(0) == (0, 30) and rb.free_rows == 32 and rb.largest_free == 16
    ap = _compare(w, rb, live, "B D C E F")
    assert sorted(set(ap)) == [-1, 0, 1], ap
    # A's own rows asked in the slot B now occupies: B's answer, from the fresh bank; nothing of A is left - not its rows (dist > 0), not
    # its label bytes, granule words or `any` word (action 2: A had it, B has not - the fresh bank falls back)
    mb, rank = _fresh(w, live)
    qa = w["banks"][A][0]
    n = qa.shape[0]
    for allow in (None, action_mask([2]), action_mask([1])):
        for k in (1, 3):
            kw = dict(k=k) if allow is None else dict(k=k, allow=[allow] * n, return_applied=True)
            got, ref = rb.query(qa, [0] * n, **kw), mb.query(qa, [rank[0]] * n, **kw)
            _same(got, ref, ("stale", allow, k))
            assert bool((got[0][:, 0] > 0).all()) and bool((got[1][:, 0] >= 0).all()) and bool((got[1] < 30).all())
            if allow is not None:
                assert got[2].tolist() == [-1 if allow == action_mask([2]) else 1] * n
    # 7: a seventh request - C again, 20 rows = 2 granules: the 2 free granules are not adjacent
    with pytest.raises(RuntimeError, match=r"status -3.*no free extent of 20 rows: the largest is 16 rows \(32 rows free"):
        _add(w, rb, C)
    assert rb.free_rows == 32 and rb.largest_free == 16 and rb.rows(5) == (0, 0) and model._ctx.generation() == gen
    assert RW.first_fit(list(free), 2) is None and RW.first_fit(list(free), 1) == 2
    _compare(w, rb, live, "after the refusal")


def test_small_characters_take_the_tiled_style_mlp(world):
    """E (16 rows) and F (1 row) alone in a resident bank: their decoder constants are the tiled float64 kernel's, which rows of a larger
    bank get, so the hard characterize of windows matched to them equals the one on a fresh bank that holds them among A's rows."""
    w = world
    rb = ResidentCharacterBank(w["model"], 64, 2, 16)
    assert _add(w, rb, F) == 0 and _add(w, rb, E) == 1 and rb.rows(0) == (0, 1) and rb.rows(1) == (16, 32)
    mb = MultiCharacterBank(w["ref_model"], [w["banks"][A], w["banks"][F], w["banks"][E]], labels=[RW.LABELS[A], RW.LABELS[F], RW.LABELS[E]])
    ids = [0, 1, 0, 1, 1, 0]
    got = rb.characterize(w["X"], ids, w["mean"], w["std"], return_index=True, raw=True)
    ref = mb.characterize(w["X"], [i + 1 for i in ids], w["mean"], w["std"], return_index=True, raw=True)
    _same(got, ref, "tiled")


def test_refusals_and_union_calls(world):
    w = world
    model, d = w["model"], RW.dev()
    ctx = model._ctx
    with pytest.raises(RuntimeError, match="status -1"):
        ctx.call("mocha_bank_resident_create", 64, 2, 16, 2, None)           # MOCHA_BANK_BF16
    with pytest.raises(RuntimeError, match="status -1"):
        ctx.call("mocha_bank_resident_create", 64, 2, 16, 1, None)           # MOCHA_BANK_BORROW
    with pytest.raises(RuntimeError, match="status -1"):
        ctx.call("mocha_bank_resident_create", 64, 2, 65, 0, None)           # more rows per character than the bank holds
    rb = ResidentCharacterBank(model, 50, 2, 16, dec_cache=False)            # 50 rows -> 64; no decoder cache: the per-call flow
    assert rb.free_rows == 64
    nm, enc = w["banks"][E]
    assert rb.add(nm, enc, labels=RW.LABELS[E]) == 0
    gen = ctx.generation()
    with pytest.raises(RuntimeError, match="status -3.*occupied"):
        rb.add(nm, enc, slot=0)
    with pytest.raises(IndexError):
        rb.add(nm, enc, slot=2)
    with pytest.raises(RuntimeError, match="status -1"):
        ctx.call("mocha_bank_resident_add", 2, nm.data_ptr(), enc.data_ptr(), 16, None, None, None)
    with pytest.raises(RuntimeError, match="status -1.*17 rows"):
        rb.add(torch.zeros((17, 90 * 256), device=d), torch.zeros((17, 90, 256), device=d))
    with pytest.raises(RuntimeError, match="status -1"):
        rb.add(torch.zeros((0, 90 * 256), device=d), torch.zeros((0, 90, 256), device=d))
    with pytest.raises(ValueError, match="0 .. 63"):
        rb.add(nm, enc, labels=np.full(16, 64))
    with pytest.raises(ValueError, match="labels for"):
        rb.add(nm, enc, labels=np.zeros(15, np.int64))
    assert rb.add(nm[:1], enc[:1]) == 1
    with pytest.raises(RuntimeError, match="status -3.*all 2 slots"):
        rb.add(nm[:1], enc[:1])
    with pytest.raises(RuntimeError, match="status -3.*empty"):
        rb.retire(1).retire(1)
    with pytest.raises(IndexError):
        rb.retire(2)
    with pytest.raises(ValueError, match="ids must lie"):
        rb.query(w["q"][:1], [2])
    # the no-cache bank answers as the fresh one does
    mb = MultiCharacterBank(w["ref_model"], [w["banks"][E]], labels=[RW.LABELS[E]], dec_cache=False)
    _same(rb.characterize(w["X"], [0] * 6, w["mean"], w["std"], return_index=True, raw=True),
          mb.characterize(w["X"], [0] * 6, w["mean"], w["std"], return_index=True, raw=True), "no cache")
    # replace: another character under the same id
    assert rb.replace(0, *w["banks"][F]) == 0 and rb.rows(0) == (0, 1) and rb.replace(1, nm, enc, labels=RW.LABELS[E]) == 1
    assert ctx.generation() == gen
    # every call that searches or reads the union
    q1 = w["q"][:1]
    idx, dist = torch.zeros(8, dtype=torch.int32, device=d), torch.zeros(8, device=d)
    out = torch.zeros((1, 90, 256), device=d)
    Y = torch.zeros((1, 60, RW.V, 15), device=d)
    x1 = torch.zeros((1, 60, RW.V, 15), device=d)
    p = lambda t: t.data_ptr()                                                # noqa: E731
    union = {
        "mocha_match": (p(q1), 1, p(idx), p(dist), None),
        "mocha_match_topk": (p(q1), 1, 2, p(idx), p(dist), None),
        "mocha_characterize": (p(x1), 1, p(w["mean"]), p(w["std"]), p(Y), p(idx), None),
        "mocha_step_graph": (p(x1), p(w["mean"]), p(w["std"]), p(Y), p(idx), 0, None),
        "mocha_step_graph_lane": (0, p(x1), p(w["mean"]), p(w["std"]), p(Y), p(idx), 0, None),
        "mocha_bank_gather": (p(idx), 1, p(out), None),
        "mocha_bank_gather_blend": (p(idx), p(dist), 1.0, 1, 1, p(out), None),
        "mocha_bank_export": (p(out), p(out), None),
        "mocha_bank_view": (None, None, None, None, None, None),
    }
    for name, args in union.items():
        with pytest.raises(RuntimeError, match="status -3.*resident bank"):
            ctx.call(name, *args)
    import ctypes
    # mocha_bank_broadcast with the resident bank's context as the root of a one-rank communicator (as tests/test_runtime_gpu.py makes one)
    from mocha_sigasia2023_amd import distributed as Dist
    os.environ.pop("RANK", None); os.environ.pop("WORLD_SIZE", None)
    Dist.init_comm(model)
    with pytest.raises(RuntimeError, match="status -3.*mocha_bank_broadcast.*resident bank"):
        ctx.call("mocha_bank_broadcast", None, 0, 64, 0, None)
    with pytest.raises(RuntimeError, match="status -3.*resident bank takes its labels"):
        ctx.call("mocha_bank_set_labels", (ctypes.c_int32 * 64)(), None)
    assert ctx.generation() == gen
    # constrained steps take a resident bank as they take a labelled MultiCharacterBank
    step = MultiStreamCharacterizer(rb, w["mean"], w["std"], streams=2, raw=True, constrained=True)
    assert step.step(w["X"][:2], [0, 1], allow=[0, 0])[1].tolist()[0] == 0
    # another bank on the model: the resident bank is gone and says so
    ContextBank(model, *w["banks"][A])
    with pytest.raises(RuntimeError, match="cannot be rebuilt"):
        rb.query(q1, [0])
    with pytest.raises(RuntimeError, match="cannot be rebuilt"):
        rb.add(nm[:1], enc[:1])
    with pytest.raises(RuntimeError, match="status -3.*no resident bank"):
        ctx.call("mocha_bank_resident_retire", 0, None)
    # ... and a bank replaced through the C ABI, behind the Python object's back, is a state error, not a slot out of range
    kept, model._bank = model._bank, rb
    with pytest.raises(RuntimeError, match="status -3.*not a resident bank"):
        rb.rows(0)
    with pytest.raises(IndexError):
        rb.rows(2)
    model._bank = kept
