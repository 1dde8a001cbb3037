"""Action-constrained characterize and captured step on the MI355X (run with -m gpu): MultiCharacterBank.characterize(allow=) /
mocha_characterize_segmented_allow and MultiStreamCharacterizer(constrained=True) / mocha_step_graph_segmented_allow.

  * characterize(allow=), hard and soft (k = 3), equals the plain characterize on a bank whose characters are the admissible subsets, bit
    for bit in Y (fp32 bank, the same batch size: the same kernels and launch shapes; only the matcher differs, and a row's distance does
    not depend on the other rows);
  * the captured constrained step equals the eager call bit for bit, new masks written into ``allow`` between steps change idx as the
    float64 restatement says (tests/allow_ref.py; the data rule of test_scan_kernels.py asserted on the CPU), and nothing is captured
    again (mocha_generation does not move)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import allow_ref as ar  # noqa: E402
import allow_world as W  # noqa: E402
import scan_ref as sr  # noqa: E402
from mocha_sigasia2023_amd import MultiCharacterBank, MultiStreamCharacterizer, action_mask  # noqa: E402

pytestmark = pytest.mark.gpu
F = 64


@pytest.fixture(scope="module")
def world():
    return W.build(F)


def restated(w, X, chars, masks, k):
    """(idx [B, k], applied [B]) of the float64 restatement for raw windows X, the data rule asserted."""
    q = W.queries(w, X)
    seg = np.asarray(chars, np.int32)
    gap = ar.gaps_ok(q, w["rows"], seg, w["seg_start"], w["labels"], masks, w["rows"].view(np.uint32), k)
    assert gap is not None and gap >= sr.MIN_GAP, gap
    idx, _, _, applied = ar.search(q, w["rows"], seg, w["seg_start"], w["labels"], masks, k)
    return idx, applied


@pytest.mark.parametrize("mask", [action_mask([1]), action_mask([0, 2]), action_mask([2])])
def test_characterize_allow_is_the_plain_characterize_on_the_subset_bank(world, mask):
    w = world
    mb, mean, std = w["mb"], w["mean"], w["std"]
    X = torch.cat([W.windows(w, 59), W.windows(w, 63)])                       # 6 windows
    chars = [0, 1, 2, 1, 0, 2]
    cands = [ar.candidates(lab, mask) for lab in W.LABELS]                    # character 2 has none of these actions: all its rows
    d = W.dev()
    Yh, ih, ah = mb.characterize(X, chars, mean, std, return_index=True, raw=True, allow=mask)
    Ys, ik, wk, as_ = mb.characterize(X, chars, mean, std, return_index=True, raw=True, soft=W.SOFT, allow=[mask] * 6)
    ridx, rap = restated(w, X, chars, [mask] * 6, 3)
    torch.cuda.synchronize()
    assert np.array_equal(ih.cpu().numpy(), ridx[:, 0]) and np.array_equal(ik.cpu().numpy(), ridx)
    anys = ar.any_table(w["labels"], w["seg_start"])                           # a character without any of these actions falls back
    assert ah.tolist() == rap.tolist() == [(1 if mask & anys[c] else -1) for c in chars] and as_.tolist() == ah.tolist()
    assert -1 in ah.tolist() and 1 in ah.tolist()
    sub = MultiCharacterBank(w["model"], [(nm[torch.from_numpy(c).to(d)], enc[torch.from_numpy(c).to(d)]) for (nm, enc), c in zip(w["banks"], cands)])
    Y0, i0 = sub.characterize(X, chars, mean, std, return_index=True, raw=True)
    Y1, i1, w1 = sub.characterize(X, chars, mean, std, return_index=True, raw=True, soft=W.SOFT)
    torch.cuda.synchronize()
    assert torch.equal(Yh, Y0), float((Yh - Y0).abs().max())
    assert torch.equal(Ys, Y1) and torch.equal(wk, w1), float((Ys - Y1).abs().max())
    for j, c in enumerate(chars):
        assert int(ih[j]) == cands[c][int(i0[j])]
        assert ik[j].tolist() == [int(cands[c][v]) if v >= 0 else -1 for v in i1[j].tolist()]
    Yp, ip = mb.characterize(X, chars, mean, std, return_index=True, raw=True)
    torch.cuda.synchronize()
    assert torch.equal(Yh, Yp) == torch.equal(ih, ip)                         # the constraint changes Y exactly where it changes the match
    if mask == action_mask([1]):
        assert not torch.equal(ih, ip)                                        # ... which this narrow mask does


@pytest.mark.parametrize("soft", [None, W.SOFT])
def test_captured_constrained_step(world, soft):
    w = world
    mb, mean, std, model = w["mb"], w["mean"], w["std"], w["model"]
    st = MultiStreamCharacterizer(mb, mean, std, streams=3, raw=True, soft=soft, constrained=True)
    assert st.allow.dtype == torch.int64 and st.allow.tolist() == [0, 0, 0]
    k = soft[0] if soft else 1
    schedule = [(59, [0, 1, 2], None),                                        # zero masks: the plain step
                (60, None, [action_mask([1]), action_mask([1]), action_mask([1])]),
                (61, None, [action_mask([2]), 0, action_mask([0, 1, 2])]),    # a producer writes the device tensor in place below
                (62, [1, 0, 0], [action_mask([0]), action_mask([0, 2]), action_mask([1])]),
                (63, None, None)]
    gen = None
    seen = []
    chars, masks = None, [0, 0, 0]
    for f, c, m in schedule:
        X = W.windows(w, f)
        chars = c or chars
        if m is not None and f == 61:
            st.allow.copy_(torch.from_numpy(ar.as_int64(m)).to(W.dev()))      # in place, not through step()
            out = st.step(X, c)
        else:
            out = st.step(X, c, allow=m)
        masks = m or masks
        gen = gen or model._ctx.generation()
        assert model._ctx.generation() == gen, f                              # new masks, ids and windows do not capture again
        y, idx, applied = out[0].clone(), out[1].clone(), out[-1].clone()
        wt = out[2].clone() if soft else None
        eager = mb.characterize(X, chars, mean, std, return_index=True, raw=True, soft=soft, allow=masks)
        plain = mb.characterize(X, chars, mean, std, return_index=True, raw=True, soft=soft)
        ridx, rap = restated(w, X, chars, masks, k)
        torch.cuda.synchronize()
        assert torch.equal(y, eager[0]) and torch.equal(idx, eager[1]) and torch.equal(applied, eager[-1]), f
        if soft:
            assert torch.equal(wt, eager[2]), f
        assert np.array_equal(idx.cpu().numpy().reshape(3, -1), ridx[:, :k]) and applied.tolist() == rap.tolist(), (f, idx, ridx)
        if all(v == 0 for v in masks):
            assert torch.equal(y, plain[0]) and torch.equal(idx, plain[1]), f
        seen.append(idx.cpu().numpy().reshape(3, -1)[:, 0].tolist())
    assert len({tuple(s) for s in seen}) >= 3                                 # the masks moved the answers
    with pytest.raises(RuntimeError):
        MultiStreamCharacterizer(mb, mean, std, streams=3, raw=True).step(allow=[1, 1, 1])
