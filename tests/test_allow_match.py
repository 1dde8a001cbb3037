"""Action-constrained matching on the MI355X (run with -m gpu): mocha_bank_set_labels and mocha_match_segmented_allow through the Python
surface and the C ABI at D = 23 040, on one bank of six characters of 1, 15, 16, 17, 33 and 49 rows (12 MB), fp32 and bf16.

What is held
  indices   equal to the float64 restatement (tests/allow_ref.py) - no near-tie allowance: every case asserts on the CPU that any two
            candidate rows an answer must order differ in float64 d2 by exactly 0 (bit-identical copies) or by at least scan_ref.MIN_GAP
            relative.  The operands are the ones the device scans: the fp32 rows and queries, or - bf16 bank - the bits of the device's own
            centred copy and centroid (mocha_bank_view) with fp32-centred queries.
  applied   1 / 0 / -1 per query, as the restatement says.
  distances against float64 with the margins test_scan_kernels.py uses for the segmented matcher (DEFAULT_MARGIN on the fp32 CPU evaluation
            of the same direct form; the arithmetic is the plain matcher's).
  bits      an all-ones mask and a zero mask give mocha_match_segmented / mocha_match_topk_segmented; on the fp32 bank a constrained answer
            is the plain call on a bank whose characters are the admissible subsets (distance bits equal, index through flatnonzero);
            column 0 of the top-k call is the hard call.
The rows of a character sit on shells around the character's anchor (scan_ref._shells: squared distances a factor 1.1 apart); a query is
the anchor plus small noise, or a bit-identical copy of a row (the trap: that row has distance 0 and, where its label is not allowed, must
not win)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import allow_ref as ar  # noqa: E402
import scan_ref as sr  # noqa: E402
from test_allow_ref import fixture_problem  # noqa: E402
from test_scan_kernels import hold_rel  # noqa: E402

from mocha_sigasia2023_amd import Generator, MultiCharacterBank, action_mask, weights  # noqa: E402

pytestmark = pytest.mark.gpu
D = 90 * 256
SIZES = [1, 15, 16, 17, 33, 49]
START = np.concatenate([[0], np.cumsum(SIZES)]).astype(np.int64)
N = int(START[-1])
S = len(SIZES)
COPY_LO, COPY_HI = 20, 40                  # character 5: row 40 is a bit-identical copy of row 20 (another workgroup)
PER_SEGMENT = (1, 2, 3, 4, 5, 8, 9, 17)    # queries per segment: every scan body (1 / 2 / 4 / 8 queries), one and several blocks
ERR_ARG = -1


def dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def model():
    return Generator(layout="mixamo", device=dev()).load_state_dict(weights.synthetic_state_dict(1777, 1.0, "mixamo")).eval()


class World:
    """The rows, the anchors, and per arithmetic the bank on the device with the operands the device scans."""


@pytest.fixture(scope="module")
def world():
    r = sr.rng("allow-match")
    w = World()
    w.anchors = r.standard_normal((S, D), dtype=np.float32)
    rows = np.empty((N, D), np.float32)
    for s in range(S):
        rows[START[s] + r.permutation(SIZES[s])] = sr._shells(r, w.anchors[s], SIZES[s], D, 0.1, 0.01)
    rows[START[5] + COPY_HI] = rows[START[5] + COPY_LO]
    w.rows, w.banks = rows, {}
    w.radius2 = np.concatenate([sr.dist2(w.anchors[s:s + 1], rows[START[s]:START[s + 1]])[0] for s in range(S)])
    w.probe = (w.anchors.astype(np.float64) + 1e-3 * 0.1 * r.standard_normal((S, D))).astype(np.float32)      # one query per character
    return w


def error_samples(world, values, to_scan):
    """(float64, fp32) distances of every character's probe query to every row of the character: 131 samples of the fp32 CPU
    evaluation's error, for cases of a handful of outputs (hold's `extra`)."""
    sq = to_scan(world.probe)
    d64 = np.concatenate([sr.dist2(sq[s:s + 1], values[START[s]:START[s + 1]])[0] for s in range(S)])
    d32 = np.concatenate([sr.dist2(sq[s:s + 1], values[START[s]:START[s + 1]], np.float32)[0] for s in range(S)])
    return np.sqrt(d64), np.sqrt(d32)


def pull(ptr, shape, dt):
    hip = None
    for name in ("libamdhip64.so", "libamdhip64.so.7", "libamdhip64.so.6"):
        try:
            hip = C.CDLL(name)
            break
        except OSError:
            continue
    assert hip is not None, "the HIP runtime library is not loadable"
    a = np.empty(shape, dt)
    torch.cuda.synchronize()
    assert hip.hipMemcpy(a.ctypes.data_as(C.c_void_p), ptr, C.c_size_t(a.nbytes), 2) == 0
    return a


def characters(rows):
    t = torch.from_numpy(rows).to(dev())
    return [(t[START[c]:START[c + 1]], t[START[c]:START[c + 1]].view(-1, 90, 256)) for c in range(S)]


def bank_of(model, world, bf16):
    """(MultiCharacterBank, values [N, D] the scan sees, to_scan(q) the query the scan sees, bits for the copies rule)."""
    if bf16 not in world.banks:
        mb = MultiCharacterBank(model, characters(world.rows), bf16=bf16, dec_cache=False)
        if bf16:
            ptrs = [C.c_void_p() for _ in range(5)]
            model._ctx.call("mocha_bank_view", *[C.byref(p) for p in ptrs], None)
            centre = pull(ptrs[2], (D,), np.float32)
            bits = pull(ptrs[4], (N, D), np.uint16)
            world.banks[bf16] = (mb, sr.bf16_value(bits), lambda q: (q - centre[None, :]).astype(np.float32), bits)
        else:
            world.banks[bf16] = (mb, world.rows, lambda q: q, world.rows.view(np.uint32))
        world.extra = getattr(world, "extra", {})
        world.extra[bf16] = error_samples(world, world.banks[bf16][1], world.banks[bf16][2])
    return world.banks[bf16]


# ------------------------------------------------------------------------------------------------------------------ label layouts
def layout(name):
    """Labels (N,) of the six characters."""
    lab = np.zeros(N, np.int32)
    for s in range(S):
        n, lo = SIZES[s], int(START[s])
        r = np.arange(n)
        if name == "aligned":                          # runs aligned to 16: whole workgroups are skipped
            v = (r // 16) % 3
        elif name == "edges":                          # run edges at rows 15 and 17
            v = np.where(r < 15, 0, np.where(r < 17, 1, 2))
        elif name == "alternate":                      # nothing can be skipped
            v = r % 2
        elif name.startswith("single"):                # one admissible row (label 0) among rows of label 1
            at = {"single-0": 0, "single-15": 15, "single-16": 16, "single-last": n - 1}[name]
            v = np.where(r == min(at, n - 1), 0, 1)
        elif name == "0-63":                           # the two ends of the label range
            v = np.where((r >= 8) & (r < 24), 63, 0)
        else:
            raise KeyError(name)
        lab[lo:lo + n] = v
    return lab


LAYOUTS = ["aligned", "edges", "alternate", "single-0", "single-15", "single-16", "single-last", "0-63"]


def mask_menu(name):
    """Masks a layout is asked with: single labels, a pair, nothing (0), everything, and a label no character has (falls back)."""
    if name == "0-63":
        return [1, 1 << 63, 0, ar.ALL, 1 << 7, (1 << 63) | 1]
    if name.startswith("single") or name == "alternate":
        return [1, 2, 0, ar.ALL, 1 << 7, 3]
    return [1, 2, 4, 0, ar.ALL, 1 << 7, 3, 6]


def make_queries(world, lab, menu, per, seed):
    """`per` queries for every character, shuffled: masks from the menu in turn; every other query is the character's anchor plus noise,
    the others bit-identical copies of a row of the character - preferring a row the mask does NOT allow (the trap)."""
    r = sr.rng(f"allow-q-{seed}-{per}")
    seg, masks, q = [], [], []
    n = 0
    for s in range(S):
        lo, hi = int(START[s]), int(START[s + 1])
        for j in range(per):
            m = menu[n % len(menu)]
            n += 1
            if j % 2 == 0:
                v = (world.anchors[s].astype(np.float64) + 1e-3 * np.sqrt(0.01) * r.standard_normal(D)).astype(np.float32)
            else:
                out = [i for i in range(hi - lo) if not (m >> int(lab[lo + i])) & 1]
                pool = out if out else list(range(hi - lo))
                pool = sorted(pool, key=lambda i: world.radius2[lo + i])[:3]          # near the anchor: the other rows' distances stay well apart
                v = world.rows[lo + pool[int(r.integers(0, len(pool)))]].copy()
            seg.append(s); masks.append(m); q.append(v)
    order = r.permutation(len(seg))
    return np.stack(q)[order], np.array(seg, np.int32)[order], [masks[i] for i in order]


def ask(mb, q, seg, masks, k):
    dist, idx, applied = mb.query(torch.from_numpy(q), torch.from_numpy(np.asarray(seg, np.int32)).to(dev()),
                                  k=k, allow=torch.from_numpy(ar.as_int64(masks)).to(dev()), return_applied=True)
    torch.cuda.synchronize()
    return dist.cpu().numpy(), idx.cpu().numpy().astype(np.int64), applied.cpu().numpy()


def check(case, tag, values, bits, sq, seg, lab, masks, k, got, extra):
    """One constrained call against the restatement; returns the float64 answers."""
    dist, idx, applied = got
    gap = ar.gaps_ok(sq, values, seg, START, lab, masks, bits, k)
    assert gap is not None and gap >= sr.MIN_GAP, (case, gap)
    ridx, _, d64, rap = ar.search(sq, values, seg, START, lab, masks, k)
    _, _, d32, _ = ar.search(sq, values, seg, START, lab, masks, k, np.float32)
    print(f"[allow] {case}: Q {len(seg)} k {k} smallest gap {gap:.3e} constrained {int((rap == 1).sum())} fell back {int((rap == -1).sum())}")
    assert np.array_equal(idx, ridx), (case, np.argwhere(idx != ridx)[:4], idx[idx != ridx][:4], ridx[idx != ridx][:4])
    assert np.array_equal(applied, rap), (case, applied, rap)
    have = ridx >= 0
    assert np.isposinf(dist[~have]).all(), case
    pos = have & (d64 > 0)
    assert (dist[have & (d64 == 0)] == 0).all(), (case, "a copy's distance is exactly 0")
    if pos.any():
        hold_rel(f"allow: segmented {tag} dist", case, dist[pos], np.sqrt(d64[pos]), np.sqrt(d32[pos]), extra=extra)
    return ridx, d64


# ------------------------------------------------------------------------------------------------------------------ the cases
@pytest.mark.parametrize("bf16", [False, True])
@pytest.mark.parametrize("name", LAYOUTS)
def test_layouts_and_queries_per_segment(model, world, name, bf16):
    """Every label layout, 1 .. 17 queries per character (mixed masks inside every block, traps among them), the hard matcher; top-k with
    k = 2, 5, 8 - more than the admissible rows of most masks - at 3 and 9 queries per character, its column 0 the hard call to the bit."""
    mb, values, to_scan, bits = bank_of(model, world, bf16)
    lab = layout(name)
    mb.set_labels([lab[START[c]:START[c + 1]] for c in range(S)])
    tag = "b16" if bf16 else "f32"
    # the bf16 copy of a row is not the row: a "copy" query is then a near-copy, nearest by far (the rounding residual)
    for per in PER_SEGMENT:
        q, seg, masks = make_queries(world, lab, mask_menu(name), per, name)
        sq = to_scan(q)
        hard = ask(mb, q, seg, masks, 1)
        check(f"{name}-{tag}-p{per}-hard", tag, values, bits, sq, seg, lab, masks, 1, hard, world.extra[bf16])
        if per in (3, 9):
            for k in (2, 5, 8):
                soft = ask(mb, q, seg, masks, k)
                check(f"{name}-{tag}-p{per}-k{k}", tag, values, bits, sq, seg, lab, masks, k, soft, world.extra[bf16])
                assert np.array_equal(soft[1][:, 0], hard[1][:, 0]) and np.array_equal(soft[0][:, 0].view(np.uint32), hard[0][:, 0].view(np.uint32))
                assert np.array_equal(soft[2], hard[2])


@pytest.mark.parametrize("bf16", [False, True])
def test_trap_copies_mixed_block_and_invalid_id(model, world, bf16):
    mb, values, to_scan, bits = bank_of(model, world, bf16)
    lab = layout("edges")
    lab[START[5] + COPY_LO], lab[START[5] + COPY_HI] = 5, 6          # the two copies carry labels of their own
    mb.set_labels([lab[START[c]:START[c + 1]] for c in range(S)])
    tag = "b16" if bf16 else "f32"
    row = world.rows[START[5] + COPY_LO]
    # copies of the winner: the lower one inadmissible -> the higher one; both admissible -> the lower one; neither -> some other row
    q = np.stack([row, row, row, row])
    seg = np.array([5, 5, 5, 5], np.int32)
    masks = [action_mask([6]), action_mask([5, 6]), action_mask([0, 1]), 0]
    got = ask(mb, q, seg, masks, 1)
    ridx, _ = check(f"copies-{tag}", tag, values, bits, to_scan(q), seg, lab, masks, 1, got, world.extra[bf16])
    assert got[1][:, 0].tolist()[:2] == [COPY_HI, COPY_LO] and got[1][3, 0] == COPY_LO and got[1][2, 0] not in (COPY_LO, COPY_HI)
    for k in (2, 8):
        gk = ask(mb, q, seg, masks, k)
        check(f"copies-{tag}-k{k}", tag, values, bits, to_scan(q), seg, lab, masks, k, gk, world.extra[bf16])
        assert gk[1][1, :2].tolist() == [COPY_LO, COPY_HI] and gk[1][0].tolist() == [COPY_HI] + [-1] * (k - 1)
    # a block of 8 queries of one character with 8 different masks, a zero mask and a falling-back one among them: each its own answer
    r = sr.rng("allow-mixed")
    q8 = np.stack([(world.anchors[5].astype(np.float64) + 1e-3 * 0.1 * r.standard_normal(D)).astype(np.float32) for _ in range(8)])
    q8[1], q8[5] = world.rows[START[5] + 3], world.rows[START[5] + 30]        # traps: rows of label 0 and of label 2
    m8 = [1, 2, 4, 0, 1 << 9, 3, 1 << 5, ar.ALL]
    s8 = np.full(8, 5, np.int32)
    g8 = ask(mb, q8, s8, m8, 1)
    check(f"mixed-{tag}", tag, values, bits, to_scan(q8), s8, lab, m8, 1, g8, world.extra[bf16])
    assert g8[2].tolist() == [1, 1, 1, 0, -1, 1, 1, 1] and len(set(g8[1][:, 0].tolist())) >= 4
    for i in range(8):                                                        # ... which is the answer it gets alone, to the bit
        one = ask(mb, q8[i:i + 1], s8[i:i + 1], m8[i:i + 1], 1)
        assert one[1][0, 0] == g8[1][i, 0] and one[0].view(np.uint32)[0, 0] == g8[0].view(np.uint32)[i, 0] and one[2][0] == g8[2][i]
    # ids outside [0, S) with a mask: idx -1, dist +inf, applied 0; the others' bits are those of the call without them
    sx = np.array([5, -1, 5, S, 5, 5, 1 << 20, 5], np.int32)
    gx = ask(mb, q8, sx, m8, 1)
    bad = (sx < 0) | (sx >= S)
    assert (gx[1][bad, 0] == -1).all() and np.isposinf(gx[0][bad, 0]).all() and (gx[2][bad] == 0).all()
    assert np.array_equal(gx[1][~bad], g8[1][~bad]) and np.array_equal(gx[0][~bad].view(np.uint32), g8[0][~bad].view(np.uint32))
    gk = ask(mb, q8, sx, m8, 5)
    assert (gk[1][bad] == -1).all() and np.isposinf(gk[0][bad]).all() and (gk[2][bad] == 0).all()


@pytest.mark.parametrize("bf16", [False, True])
def test_unconstrained_masks_give_the_plain_calls_bits(model, world, bf16):
    mb, values, to_scan, bits = bank_of(model, world, bf16)
    lab = layout("aligned")
    mb.set_labels([lab[START[c]:START[c + 1]] for c in range(S)])
    q, seg, _ = make_queries(world, lab, [0], 5, "plain")
    ids = torch.from_numpy(seg).to(dev())
    for k in (1, 2, 8):
        pd, pi = mb.query(torch.from_numpy(q), ids, k=k)
        torch.cuda.synchronize()
        for masks, want in (([0] * len(seg), 0), ([ar.ALL] * len(seg), 1), ([1 << 40] * len(seg), -1)):
            d, i, ap = ask(mb, q, seg, masks, k)
            assert np.array_equal(i, pi.cpu().numpy()) and np.array_equal(d.view(np.uint32), pd.cpu().numpy().view(np.uint32)), (k, want)
            assert (ap == want).all()


def test_constrained_answer_is_the_plain_answer_on_the_subset_bank(model, world):
    """fp32: a row's squared distance does not depend on the other rows, so the constrained answer has the bits of the plain call on a
    bank whose characters are the admissible subsets; the index maps through flatnonzero."""
    mb, values, to_scan, bits = bank_of(model, world, False)
    for name, mask in (("edges", 2), ("edges", 5), ("aligned", 4), ("alternate", 1), ("0-63", 1 << 63)):
        lab = layout(name)
        mb.set_labels([lab[START[c]:START[c + 1]] for c in range(S)])
        q, seg, masks = make_queries(world, lab, [mask], 3, f"subset-{name}")
        cands = [ar.candidates(lab[START[c]:START[c + 1]], mask) for c in range(S)]
        for k in (1, 5):
            d, i, ap = ask(mb, q, seg, masks, k)
            t = torch.from_numpy(world.rows).to(dev())
            picked = [t[START[c] + torch.from_numpy(cands[c]).to(dev())] for c in range(S)]
            sub = MultiCharacterBank(model, [(x, x.view(-1, 90, 256)) for x in picked], dec_cache=False)
            sd, si = sub.query(torch.from_numpy(q), torch.from_numpy(seg).to(dev()), k=k)
            torch.cuda.synchronize()
            sd, si = sd.cpu().numpy(), si.cpu().numpy()
            assert np.array_equal(d.view(np.uint32), sd.view(np.uint32)), (name, mask, k)
            for j in range(len(seg)):
                mapped = np.where(si[j] >= 0, cands[seg[j]][np.maximum(si[j], 0)], -1)
                assert np.array_equal(i[j], mapped), (name, mask, k, j)


def test_nan_rows_in_skipped_workgroups_change_nothing(model, world):
    """fp32: the rows of workgroups wholly inadmissible for the call's masks are NaN in a second bank: the same answers, bit for bit - the
    workgroups were skipped, not scanned and masked (a NaN row in a scanned workgroup is masked at key time just the same)."""
    mb, values, to_scan, bits = bank_of(model, world, False)
    lab = layout("aligned")                                  # character 5: rows 16 .. 31 carry label 1, the other three workgroups do not
    q, seg, masks = make_queries(world, lab, [2], 8, "nan")
    keep = seg >= 3                                          # characters with more than one workgroup
    q, seg, masks = q[keep], seg[keep], [2] * int(keep.sum())
    mb.set_labels([lab[START[c]:START[c + 1]] for c in range(S)])
    clean = [ask(mb, q, seg, masks, k) for k in (1, 5)]
    rows = world.rows.copy()
    for s in (3, 4, 5):
        for x in range(0, SIZES[s], 16):
            if not (lab[START[s] + x:START[s] + min(x + 16, SIZES[s])] == 1).any():
                rows[START[s] + x:START[s] + min(x + 16, SIZES[s])] = np.nan
    assert np.isnan(rows).any(1).sum() >= 16 + 17 + 1
    nb = MultiCharacterBank(model, characters(rows), dec_cache=False, labels=[lab[START[c]:START[c + 1]] for c in range(S)])
    for (d, i, ap), k in zip(clean, (1, 5)):
        nd, ni, nap = ask(nb, q, seg, masks, k)
        assert np.array_equal(ni, i) and np.array_equal(nd.view(np.uint32), d.view(np.uint32)) and np.array_equal(nap, ap)
        assert (ap == 1).all() and not np.isnan(nd).any()


def test_optional_outputs_and_refusals(model, world):
    mb, values, to_scan, bits = bank_of(model, world, False)
    lab = layout("edges")
    mb.set_labels([lab[START[c]:START[c + 1]] for c in range(S)])
    q, seg, masks = make_queries(world, lab, mask_menu("edges"), 2, "optional")
    Q = len(seg)
    full = {k: ask(mb, q, seg, masks, k) for k in (1, 5)}
    lib, h = model._ctx.lib, model._ctx.h
    dq, ds = torch.from_numpy(q).to(dev()), torch.from_numpy(seg).to(dev())
    da = torch.from_numpy(ar.as_int64(masks)).to(dev())
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())              # noqa: E731
    GUARD = -12345

    def outs(k):
        return (torch.full((Q, k), GUARD, dtype=torch.int32, device=dev()), torch.full((Q, k), float(GUARD), device=dev()),
                torch.full((Q,), GUARD, dtype=torch.int32, device=dev()))
    for k in (1, 5):
        for null in ("dist", "applied", "both"):
            idx, dist, applied = outs(k)
            rc = lib.mocha_match_segmented_allow(h, p(dq), Q, p(ds), p(da), k, p(idx), None if null in ("dist", "both") else p(dist),
                                                 None if null in ("applied", "both") else p(applied), None)
            torch.cuda.synchronize()
            assert rc == 0 and np.array_equal(idx.cpu().numpy(), full[k][1])
            if null in ("dist", "both"):
                assert (dist == GUARD).all()
            else:
                assert np.array_equal(dist.cpu().numpy().view(np.uint32), full[k][0].view(np.uint32))
            if null in ("applied", "both"):
                assert (applied == GUARD).all()
            else:
                assert np.array_equal(applied.cpu().numpy(), full[k][2])
    # refusals leave the guard pattern: k out of range, a required pointer missing
    idx, dist, applied = outs(1)
    for k in (0, 9, -1):
        assert lib.mocha_match_segmented_allow(h, p(dq), Q, p(ds), p(da), k, p(idx), p(dist), p(applied), None) == ERR_ARG
    assert lib.mocha_match_segmented_allow(h, p(dq), Q, p(ds), None, 1, p(idx), p(dist), p(applied), None) == ERR_ARG
    assert lib.mocha_match_segmented_allow(h, p(dq), Q, p(ds), p(da), 1, None, p(dist), p(applied), None) == ERR_ARG
    torch.cuda.synchronize()
    assert (idx == GUARD).all() and (dist == GUARD).all() and (applied == GUARD).all()
    # the Python surface: labels outside 0 .. 63, masks and labels checked on the host, allow= without labels
    with pytest.raises(ValueError):
        mb.set_labels([np.full(n, 64) for n in SIZES])
    with pytest.raises(ValueError):
        mb.set_labels([np.zeros(n + 1, np.int64) for n in SIZES])
    with pytest.raises(ValueError):
        mb.query(dq, ds, allow=[[64]] * Q)
    with pytest.raises(ValueError):
        mb.query(dq, ds, allow=[1] * (Q - 1))
    d2, i2 = mb.query(dq, ds, allow=[[0, 1] if m == 3 else m for m in masks])          # labels and int masks mixed, from the host
    torch.cuda.synchronize()
    assert np.array_equal(i2.cpu().numpy(), full[1][1])
    gen0 = lib.mocha_generation(h)
    mb.set_labels(None)
    assert lib.mocha_generation(h) > gen0
    with pytest.raises(RuntimeError):
        mb.query(dq, ds, allow=1)
    idx, dist, applied = outs(1)
    assert lib.mocha_match_segmented_allow(h, p(dq), Q, p(ds), p(da), 1, p(idx), p(dist), p(applied), None) == -3          # MOCHA_ERR_STATE
    torch.cuda.synchronize()
    assert (idx == GUARD).all() and (applied == GUARD).all()


def test_reference_pin_on_the_device(model):
    """The GPU's answers on the fixture of tests/golden/action_match.npz (BallTree over the picked action's subset) equal the fixture."""
    z, rows, seg_start, labels, q, cha, masks = fixture_problem()
    t = torch.from_numpy(rows).to(dev())
    chars = [(t[seg_start[c]:seg_start[c + 1]], t[seg_start[c]:seg_start[c + 1]].view(-1, 90, 256)) for c in range(2)]
    mb = MultiCharacterBank(model, chars, dec_cache=False, labels=[labels[seg_start[c]:seg_start[c + 1]] for c in range(2)])
    dist, idx, applied = mb.query(torch.from_numpy(q), cha.tolist(), allow=[[int(a)] for a in z["action"]], return_applied=True)
    pd, pi = mb.query(torch.from_numpy(q), cha.tolist())
    torch.cuda.synchronize()
    assert np.array_equal(idx[:, 0].cpu().numpy(), z["idx"]) and (applied == 1).all()
    assert np.array_equal(pi[:, 0].cpu().numpy(), z["plain_idx"])
    # fp32 direct form over 23 040 terms against BallTree's float64: the fp32 CPU evaluation of the same sums is within 2e-6 relative
    assert np.allclose(dist[:, 0].cpu().numpy(), z["dist"], rtol=1e-5, atol=0)
