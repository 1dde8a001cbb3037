"""The live Ours step with ONE CVAE PER CHARACTER (LiveOursSession(cvaes=CVAEBank) / mocha_live_step_ours_grouped) on the data recipe,
plans and bounds of tests/test_live_ours.py: `mixamo`, 23 bones, three characters of 40 bank rows, its S3 plans (characters 2, 0, 1), its
noise.  The reference is ONE OursOracle PER STREAM (tests/live_ours_ref.py), constructed with the state dict and the statistics of the
slot of that stream's character; Switching (below) wraps it for a change in mid-run.

CVAEs: weights.synthetic_cvae_state_dict(seed, 1.0) for seeds 99 / 100 / 101 in slots 0 / 1 / 2, statistics seeded per slot as
tests/test_hip_cvae.py makes its four (slot 0: exactly those).  tests/test_cvae_grouped.py asserts on the CPU that a wrong slot misses
the sampler's bound by more than 100 x.

(a) S = 3, 60 + 5 pushes, characters 2 / 0 / 1 on slots 0 / 1 / 2: stage by stage - cond, vae / mu / logvar, prev, Y, idx - and end to
    end at the bounds of tests/test_live_ours.py (its docstring), E2E_BOUND included.
(b) the same with stream 1's character mapped to -1: seeded on every valid frame, its cond / vae rows zeros, and its Y staging and
    outputs are a LiveSession's, bit for bit, on every valid frame (as test_live_ours.py holds its seed frame); streams 0 and 2 keep
    the bits of (a).
(c) 60 + 9 pushes with, in mid-run and with no new capture (mocha_generation() unchanged): set_cvae (stream 0's character to slot 2 before
    push 61), a store of another CVAE into the slot stream 1 is sampling with (before push 63), a clear of stream 2's slot (before push
    65).  Every frame follows the reference that switches at that push; the cleared slot's stream seeds on every frame from then on.
(d) every character on one slot that holds the CVAE a plain LiveOursSession on a SECOND model uses: pos / rot within E2E_BOUND, idx and
    seeded equal.
(e) a resident bank: a character is added, its CVAE stored and set_cvae called with no new capture; its stream warms, seeds, chains.
(f) S = 1 and S = 16 construct and step.     (g) the refusals.

Mutation (scratch build, run once against this file): the statistics of slot 0 for every stream in mocha_live_ours_condition -> (a) fails
on the cond stage of streams 1 and 2 (recorded in the pull request's summary)."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import live_ours_ref as R                                                   # noqa: E402
import test_live_oracle as TLO                                              # noqa: E402  (the shared data recipe; its tests are not re-collected)
import test_live_ours as TL                                                 # noqa: E402  (plans, noise, staging views, bounds)
from mocha_sigasia2023_amd import _C, synthetic, weights                    # noqa: E402
from oracle import live_oracle as LO                                        # noqa: E402

pytestmark = pytest.mark.gpu

LAYOUT, TOES, KEYS, E2E_BOUND = TLO.LAYOUT, TLO.TOES, TL.KEYS, TL.E2E_BOUND
SEEDS = (99, 100, 101)
F = TL.F
PLANS = TL.RUNS["S3"]                                                       # streams 0, 1, 2 on characters 2, 0, 1
CHARS = (2, 0, 1)
CVAE_OF = (1, 2, 0)                                                         # character -> slot: streams 0, 1, 2 sample with slots 0, 1, 2
ERR_ARG, ERR_STATE = -1, -3


def _stats(slot):
    rng = np.random.Generator(np.random.PCG64(3 + slot))                    # slot 0: the statistics of tests/test_hip_cvae.py
    return ((0.1 * rng.standard_normal((90, 256))).astype(np.float32), rng.uniform(0.5, 1.5, (90, 256)).astype(np.float32),
            (0.1 * rng.standard_normal((90, 256))).astype(np.float32), rng.uniform(0.5, 1.5, (90, 256)).astype(np.float32))


@functools.lru_cache(maxsize=None)
def _sd(slot):
    return weights.synthetic_cvae_state_dict(SEEDS[slot], 1.0)


class Switching:
    """One stream's reference: an OursOracle whose CVAE (state dict + statistics of a slot) changes at given pushes.  schedule: {push:
    slot or None}; the entry of push 0 is the initial one.  None = the character has no CVAE: every valid frame is a seed frame.  A
    change does not reseed: prev stays in de-normalised feature units and meets the new statistics."""

    def __init__(self, schedule):
        w = TLO._inputs()
        self.schedule = dict(schedule)
        s0 = self.schedule[0]
        self.o = R.OursOracle(w["sd"], LAYOUT, w["pose_norm"], w["mean"], w["std"], TLO._oracle_banks(), TOES, _sd(s0 or 0), _stats(s0 or 0))
        self.slot = s0

    def run(self, plan, s, eps):
        out, slots = [], []
        for k, (clip, f, char, reset) in enumerate(plan):
            if k in self.schedule and k > 0:
                self.slot = self.schedule[k]
                if self.slot is not None:
                    self.o.csd = R.cvae_state(_sd(self.slot))
                    self.o.stats = tuple(np.asarray(a, np.float32) for a in _stats(self.slot))
            if reset:
                self.o.reset()
            if self.slot is None:
                self.o.prev = None                                          # no CVAE: plain context matching, a seed frame
            out.append(self.o.push(*TLO._push_args(clip, f), char, eps=eps[k, s]))
            slots.append(self.slot)
        return out, slots


@functools.lru_cache(maxsize=None)
def _reference(s, schedule, pushes):
    """(push results, slot per push) of stream s of PLANS under `schedule` (a tuple of (push, slot) pairs); computed once."""
    plan = TL._plan(PLANS[s][0][0], pushes, PLANS[s][0][2])
    return Switching(dict(schedule)).run(plan, s, TL._eps())


# ------------------------------------------------------------------------------------------------ device side
def _make_world(d):
    from mocha_sigasia2023_amd import Generator, MultiCharacterBank, PostProcessor, build_bank
    w = TLO._inputs()
    model = Generator(layout=LAYOUT, device=d).load_state_dict(w["sd"]).eval()
    model.set_pose_norm(*w["pose_norm"])
    mean, std = torch.from_numpy(w["mean"]).to(d), torch.from_numpy(w["std"]).to(d)
    banks = []
    for clip in w["bank_clips"]:
        b = build_bank(model, model.featurize(*[torch.from_numpy(synthetic.slide_windows(a)) for a in clip]), raw=True)
        banks.append((((b["cnt"] - mean) / std).reshape(-1, 90 * 256), b["encoded"]))
    return dict(model=model, mean=mean, std=std, banks=banks, mb=MultiCharacterBank(model, banks), post=PostProcessor(model, contact_bones=list(TOES)))


@pytest.fixture(scope="module")
def world():
    from mocha_sigasia2023_amd import CVAEBank
    w = _make_world(TLO.dev())
    w["cvaes"] = CVAEBank(w["model"], 4)
    for slot in range(3):
        w["cvaes"].store(slot, _sd(slot), *_stats(slot))
    return w


def _session(world, S, cvae_of=CVAE_OF, noise="given", bank=None):
    from mocha_sigasia2023_amd import LiveOursSession
    return LiveOursSession(bank or world["mb"], world["mean"], world["std"], None, None, None, None, None, streams=S, post=world["post"], noise=noise,
                           cvaes=world["cvaes"], cvae_of=cvae_of)


def _push(sess, plans, k, S):
    sess.eps.copy_(torch.from_numpy(TL._eps()[k, :S]))
    args = [np.stack([TLO._push_args(plans[s][k][0], plans[s][k][1])[i] for s in range(S)]) for i in range(8)]
    return sess.push(*[torch.from_numpy(np.ascontiguousarray(a)) for a in args], characters=[plans[s][k][2] for s in range(S)])


def _run_device(world, sess, plans, pushes, events=None):
    """The session over the plans -> per push a dict of NumPy arrays (all streams): outputs and the staging of both buffers.  events:
    {push: callable} run before that push."""
    S = len(plans)
    stage = dict(TL._ours_staging(sess), Y=TLO._staging(sess)["Y"])
    for n in KEYS:
        sess.out[n].fill_(-12345.0)
    rec = []
    for k in range(pushes):
        if events and k in events:
            events[k]()
        o = _push(sess, plans, k, S)
        torch.cuda.synchronize()
        r = {n: o[n].cpu().numpy().copy() for n in KEYS + ("idx", "valid", "seeded")}
        r.update({n: t.cpu().numpy().copy() for n, t in stage.items()})
        r["generation"] = sess.model._ctx.generation()
        rec.append(r)
    return rec


def _check_stream(world, rec, s, ref, slots, errs):
    """Stream s of a recorded run against its reference (push results and the slot in force per push), stage by stage - each stage
    against the reference fed the device's own previous stage - and end to end (tests/test_live_ours.py::_check_stream, per slot)."""
    w = TLO._inputs()
    sd = LO.torch_state(w["sd"])
    char = CHARS[s]

    def worst(name, e, bound=1.0):
        errs[name] = max(errs.get(name, 0.0), float(e))
        assert e <= bound, (name, s, k, float(e), bound)
    for k, o in enumerate(ref):
        r, slot = rec[k], slots[k]
        assert int(r["valid"][s]) == o["valid"], (s, k)
        if not o["valid"]:
            assert int(r["idx"][s]) == -1 and int(r["seeded"][s]) == 0 and not r["counters"][s].any() and not r["prev"][s].any(), (s, k)
            assert all((r[n][s] == -12345.0).all() for n in KEYS), (s, k)
            continue
        seeded = bool(o["seeded"])
        assert seeded == (slot is None or k == 59), (s, k)
        assert int(r["idx"][s]) == o["idx"], (s, k, int(r["idx"][s]), o["idx"])
        assert int(r["seeded"][s]) == int(seeded), (s, k, "seeded")
        assert r["counters"][s].tolist() == [k - 58, char, 1 if seeded else 2], (s, k, r["counters"][s])
        if slot is None:                                                    # no CVAE: no statistics, no weights - zeros
            assert not r["cond"][s].any() and not r["vae"][s].any() and not r["mu"][s].any() and not r["logvar"][s].any(), (s, k)
        else:
            sm, ss, cm, cs = (a.astype(np.float64) for a in _stats(slot))
            zc = (r["cnt"][s].astype(np.float64) - sm) / ss
            want = np.concatenate([zc, np.zeros_like(zc) if seeded else (rec[k - 1]["prev"][s].astype(np.float64) - cm) / cs])
            worst("cond / (1e-6 max(1, |ref|))", (np.abs(r["cond"][s] - want) / (1e-6 * np.maximum(1.0, np.abs(want)))).max())
            with torch.no_grad():
                vae, mu, lv = R.cvae_sample(R.cvae_state(_sd(slot)), torch.from_numpy(r["cond"][s][None]), torch.from_numpy(r["eps"][s][None]))
            for n, t in (("vae", vae), ("mu", mu), ("logvar", lv)):
                worst(n, np.abs(r[n][s] - t.numpy()[0]).max(), 1e-4 * max(1.0, float(t.abs().max())))
        assert np.array_equal(r["eps"][s], TL._eps()[k, s]), (s, k)
        if seeded:
            g0, _ = world["mb"].rows(char)
            assert np.array_equal(r["prev"][s], world["mb"].encoded[g0 + int(r["idx"][s])].cpu().numpy()), (s, k)
        else:
            want = r["vae"][s].astype(np.float64) * cs + cm
            worst("prev, relative", (np.abs(r["prev"][s] - want) / np.maximum(np.abs(want), 1e-30)).max(), 1e-6)
        worst("Y", np.abs(r["Y"][s] - LO.decode(sd, o["enc"], r["prev"][s], w["pose_norm"])).max(), 1e-4)
        for n in ("pos", "rot"):
            worst("end to end " + n, np.abs(r[n][s] - o[n]).max(), E2E_BOUND)


@pytest.fixture(scope="module")
def run_a(world):
    return _run_device(world, _session(world, 3), PLANS, F)


def test_a_three_characters_on_three_slots(world, run_a):
    errs = {}
    try:
        for s in range(3):
            ref, slots = _reference(s, ((0, s),), F)
            _check_stream(world, run_a, s, ref, slots, errs)
    finally:
        for k, v in errs.items():
            print(f"(a): max error {k}: {v:.3e}")
    assert all(int(r["valid"].sum()) == (3 if k >= 59 else 0) for k, r in enumerate(run_a))


def test_b_a_character_without_a_cvae_falls_back_to_context_matching(world, run_a):
    from mocha_sigasia2023_amd import LiveSession
    cvae_of = list(CVAE_OF)
    cvae_of[CHARS[1]] = -1
    rec = _run_device(world, _session(world, 3, cvae_of), PLANS, F)
    plain = LiveSession(world["mb"], world["mean"], world["std"], streams=3, post=world["post"])
    stage = TLO._staging(plain)
    for k in range(F):
        args = [np.stack([TLO._push_args(p[k][0], p[k][1])[i] for p in PLANS]) for i in range(8)]
        o = plain.push(*[torch.from_numpy(np.ascontiguousarray(a)) for a in args], characters=[p[k][2] for p in PLANS])
        torch.cuda.synchronize()
        r = rec[k]
        if k < 59:
            assert not r["valid"].any() and not r["seeded"].any()
            continue
        assert r["seeded"].tolist() == [1 if k == 59 else 0, 1, 1 if k == 59 else 0], k
        assert int(r["idx"][1]) == int(o["idx"][1]) and not r["cond"][1].any() and not r["vae"][1].any(), k
        assert r["counters"][1].tolist() == [k - 58, CHARS[1], 1], k
        assert np.array_equal(stage["Y"][1].cpu().numpy(), r["Y"][1]), (k, "Y staging")
        for n in KEYS:
            assert np.array_equal(o[n][1].cpu().numpy(), r[n][1]), (k, n)
        for s in (0, 2):                                                    # the neighbours: the bits of (a)
            for n in KEYS + ("idx", "seeded", "prev", "vae", "cond", "Y"):
                assert np.array_equal(r[n][s], run_a[k][n][s]), (s, k, n)


def test_c_set_cvae_store_and_clear_in_mid_run_without_a_new_capture(world):
    pushes = 60 + 9
    plans = tuple(TL._plan(p[0][0], pushes, p[0][2]) for p in PLANS)
    sess = _session(world, 3)
    cv = world["cvaes"]
    events = {61: lambda: sess.set_cvae(CHARS[0], 2),                       # stream 0: slot 0 -> slot 2
              63: lambda: cv.store(1, _sd(0), *_stats(2)),                  # stream 1's slot gets slot 0's weights with slot 2's statistics
              65: lambda: cv.clear(2)}                                      # streams 0 and 2 lose their CVAE
    try:
        rec = _run_device(world, sess, plans, pushes, events)
    finally:
        cv.store(1, _sd(1), *_stats(1))
        cv.store(2, _sd(2), *_stats(2))
    assert len({r["generation"] for r in rec[1:]}) == 1, "the generation moved: a captured step would capture again"
    assert cv.stored[:3] == [True, True, True]
    # the references: per stream the slot in force per push (stream 1 after push 63: a CVAE that is in no slot of _sd / _stats - checked
    # on stages through its own pair below)
    errs = {}
    try:
        ref0, slots0 = _reference(0, ((0, 0), (61, 2), (65, None)), pushes)
        _check_stream(world, rec, 0, ref0, slots0, errs)
        ref2, slots2 = _reference(2, ((0, 2), (65, None)), pushes)
        _check_stream(world, rec, 2, ref2, slots2, errs)
    finally:
        for k, v in errs.items():
            print(f"(c): max error {k}: {v:.3e}")
    assert [int(r["seeded"][2]) for r in rec[59:]] == [1, 0, 0, 0, 0, 0, 1, 1, 1, 1]
    assert [int(r["seeded"][0]) for r in rec[59:]] == [1, 0, 0, 0, 0, 0, 1, 1, 1, 1]
    assert [int(r["seeded"][1]) for r in rec[59:]] == [1] + [0] * 9          # a store into a slot in use does not reseed
    # stream 1: slot 1's CVAE and statistics up to push 62, then the stored pair - the sampler and the condition stage by stage
    sm, ss, cm, cs = (a.astype(np.float64) for a in _stats(2))
    for k in range(60, pushes):
        r = rec[k]
        if k < 63:
            continue
        zc = (r["cnt"][1].astype(np.float64) - sm) / ss
        want = np.concatenate([zc, (rec[k - 1]["prev"][1].astype(np.float64) - cm) / cs])
        assert (np.abs(r["cond"][1] - want) / (1e-6 * np.maximum(1.0, np.abs(want)))).max() <= 1.0, k
        with torch.no_grad():
            vae, _, _ = R.cvae_sample(R.cvae_state(_sd(0)), torch.from_numpy(r["cond"][1][None]), torch.from_numpy(r["eps"][1][None]))
        assert np.abs(r["vae"][1] - vae.numpy()[0]).max() <= 1e-4 * max(1.0, float(vae.abs().max())), k
        want = r["vae"][1].astype(np.float64) * cs + cm
        assert (np.abs(r["prev"][1] - want) / np.maximum(np.abs(want), 1e-30)).max() <= 1e-6, k
    ref1, slots1 = _reference(1, ((0, 1),), 63)
    _check_stream(world, rec[:63], 1, ref1, slots1, {})


def test_d_one_slot_for_every_character_against_the_single_cvae_session(world, run_a):
    from mocha_sigasia2023_amd import LiveOursSession
    other = _make_world(TLO.dev())
    plain = LiveOursSession(other["mb"], other["mean"], other["std"], _sd(0), *_stats(0), streams=3, post=other["post"], noise="given")
    grouped = _session(world, 3, (0, 0, 0))
    worst = 0.0
    for k in range(F):
        a = _push(plain, PLANS, k, 3)
        b = _push(grouped, PLANS, k, 3)
        torch.cuda.synchronize()
        assert torch.equal(a["valid"], b["valid"]) and torch.equal(a["idx"], b["idx"]) and torch.equal(a["seeded"], b["seeded"]), k
        if k >= 59:
            worst = max(worst, max(float((a[n] - b[n]).abs().max()) for n in ("pos", "rot")))
    print(f"(d): grouped on one slot vs the single-CVAE session: max |pos|, |rot| difference {worst:.3e}")
    assert worst <= E2E_BOUND
    # (g) on a model WITHOUT a weight bank the grouped step refuses; so does a NULL cvae_of on a model with one
    lib = other["model"]._ctx.lib
    o = plain.out
    p = lambda t: C.c_void_p(t.data_ptr())                                   # noqa: E731

    def args(sess, cvae_of):
        o = sess.out
        return [C.byref(sess.post.cfg), p(sess.live), sess.streams, p(sess.rot), p(sess.pos), p(sess.vel), p(sess.ang), p(sess.rvel), p(sess.rang),
                p(sess.speed), p(sess.contact), p(sess.ids), p(sess.mean), p(sess.std), p(sess.ours), C.byref(sess.ocfg), cvae_of, p(o["pos"]), p(o["rot"]),
                p(o["ik_rot"]), p(o["bvh_pos"]), p(o["bvh_euler"]), p(o["idx"]), p(o["valid"]), p(o["seeded"]),
                C.c_void_p(torch.cuda.current_stream().cuda_stream)]
    torch.cuda.synchronize()
    live0, ours0 = plain.live.clone(), plain.ours.clone()
    of = torch.zeros(3, dtype=torch.int32, device=plain.live.device)
    assert lib.mocha_live_step_ours_grouped(other["model"]._ctx.h, *args(plain, p(of))) == ERR_STATE
    assert b"weight bank" in lib.mocha_last_error(other["model"]._ctx.h)
    glive0, gours0 = grouped.live.clone(), grouped.ours.clone()
    h = world["model"]._ctx.h
    assert lib.mocha_live_step_ours_grouped(h, *args(grouped, None)) == ERR_ARG and b"cvae_of" in lib.mocha_last_error(h)
    a = args(grouped, p(grouped.cvae_of)); a[14] = None
    assert lib.mocha_live_step_ours_grouped(h, *a) == ERR_ARG
    a = args(grouped, p(grouped.cvae_of)); a[2] = 17
    assert lib.mocha_live_step_ours_grouped(h, *a) == ERR_ARG
    torch.cuda.synchronize()
    assert torch.equal(plain.live, live0) and torch.equal(plain.ours, ours0) and torch.equal(grouped.live, glive0) and torch.equal(grouped.ours, gours0)
    assert lib.mocha_live_step_ours_grouped(h, *args(grouped, p(grouped.cvae_of))) == 0      # statistics pointers NULL: ignored
    with pytest.raises(ValueError, match="cvaes"):
        LiveOursSession(world["mb"], world["mean"], world["std"], _sd(0), *_stats(0), streams=1, post=world["post"], cvaes=world["cvaes"])
    with pytest.raises(ValueError, match="cvae_of"):
        LiveOursSession(world["mb"], world["mean"], world["std"], _sd(0), *_stats(0), streams=1, post=world["post"], cvae_of=[0, 0, 0])
    with pytest.raises(ValueError, match="entries"):
        _session(world, 1, (0, 0))
    with pytest.raises(RuntimeError, match="cvaes"):
        plain.set_cvae(0, 0)
    with pytest.raises(ValueError, match="out of range"):
        grouped.set_cvae(3, 0)


def test_f_one_and_sixteen_streams_construct_and_step(world):
    for S in (1, 16):
        sess = _session(world, S)
        plans = tuple(PLANS[s % 3] for s in range(S))
        sess.eps.zero_()
        for k in range(2):
            args = [np.stack([TLO._push_args(plans[s][k][0], plans[s][k][1])[i] for s in range(S)]) for i in range(8)]
            o = sess.push(*[torch.from_numpy(np.ascontiguousarray(a)) for a in args], characters=[plans[s][k][2] for s in range(S)])
        torch.cuda.synchronize()
        assert o["valid"].tolist() == [0] * S and o["seeded"].tolist() == [0] * S and o["idx"].tolist() == [-1] * S


def test_e_resident_bank_add_store_set_cvae_without_a_new_capture(world):
    """Last in the file: the resident bank replaces the model's current bank."""
    from mocha_sigasia2023_amd import ResidentCharacterBank
    rb = ResidentCharacterBank(world["model"], 3 * 48, 3, 48)
    for c in (0, 1):
        assert rb.add(*world["banks"][c]) == c
    sess = _session(world, 2, (1, 2, -1), bank=rb)                           # characters 0, 1 on slots 1, 2; slot 2 of the bank is empty
    plans = (TL._plan(1, 64, 0), TL._plan(0, 64, 2))                         # stream 1 names the empty slot: it sits the steps out
    seen = []
    gen = None
    for k in range(64):
        if k == 61:
            assert rb.add(*world["banks"][2]) == 2
            world["cvaes"].store(3, _sd(0), *_stats(0))
            sess.set_cvae(2, 3)
        o = _push(sess, plans, k, 2)
        torch.cuda.synchronize()
        seen.append((o["valid"].tolist(), o["seeded"].tolist()))
        gen = gen if k != 1 else sess.model._ctx.generation()
        assert gen is None or sess.model._ctx.generation() == gen, (k, "the generation moved")
    assert all(v == [0, 0] for v, _ in seen[:59])
    assert seen[59] == ([1, 0], [1, 0]) and seen[60] == ([1, 0], [0, 0])
    assert seen[61] == ([1, 1], [0, 1]) and seen[62] == ([1, 1], [0, 0]) and seen[63] == ([1, 1], [0, 0])
    # stream 1's chain frames are sampled: vae is not zeros, prev is vae de-normalised with slot 3's (= slot 0's) statistics
    st = TL._ours_staging(sess)
    cm, cs = (torch.from_numpy(a).double() for a in _stats(0)[2:])
    vae, prev = st["vae"][1].cpu().double(), st["prev"][1].cpu().double()
    assert float(vae.abs().max()) > 0.1
    assert float(((prev - (vae * cs + cm)).abs() / (vae * cs + cm).abs().clamp_min(1e-30)).max()) <= 1e-6
    world["cvaes"].clear(3)
