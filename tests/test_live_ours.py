"""The CVAE ("Ours") branch inside the live step (LiveOursSession / mocha_live_step_ours) against an independent reference of one
stream (tests/live_ours_ref.py: oracle parts only), on the layout and data of tests/test_live_oracle.py: `mixamo`, 23 bones, three
characters of 40 bank rows, synthetic.smooth_bone_clip sources, weights.synthetic_cvae_state_dict(99, 1.0) and four seeded (90,256)
statistics as in tests/test_hip_cvae.py.

CPU part (-m "not gpu"): Philox4x32-10 restated in NumPy against Random123's known-answer vectors; the frame-at-a-time reference
against the clip-at-once composition of the same oracle parts; the conditions the GPU tests' inputs must meet; the end-to-end bound.

GPU part (-m gpu): S = 1 and S = 3 over 60 + 5 pushes (six valid frames per stream: one seed frame, five chain frames), stage by
stage and end to end; the seed frame against LiveSession's frame; an events run (S = 3, 60 + 66 pushes, no CPU reference: a stream
reset before push 65 needs 59 more pushes to seed again, so the run is longer than the others); the device's noise.

Bounds.  cond: 1e-6 * max(1, |ref|) per element against the formula, in double, on the device's own cnt and previous prev.  vae, mu,
logvar: 1e-4 * max(1, max|ref|) against cvae_oracle.sample on the device's own cond and eps
(tests/test_hip_cvae.py::test_sample_with_noise_matches_oracle).  prev: 1e-6 relative against vae * std + mean on the device's vae; on
a seed frame the bank row itself.  Y: 1e-4 against the oracle's decode of the device's prev.  idx: the float64 search, no near-tie
accepted (the inputs have gaps >= 1e-4).  End to end (pos, rot of the fully independent fp32 reference run, same noise): E2E_BOUND.

End-to-end bound.  Spread between the reference chain with both networks in fp32 and in float64 (same frames, same noise), measured on
the CPU over every valid frame of the three streams of the S = 3 run (18 frames; the S = 1 run is its stream 0): max |pos| difference
2.0e-8, max |rot| difference 5.4e-7 -> spread 5.4e-7.  4 x spread = 2.2e-6 is below the floor, so the bound max(1e-4, 4 x spread) is
1e-4 (the rule of tests/test_live_oracle.py::E2E_BOUND).  test_end_to_end_bound_covers_the_reference_spread repeats the measurement on
one stream."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import live_ours_ref as R                                                   # noqa: E402
import test_live_oracle as TLO                                              # noqa: E402  (the shared data recipe; its tests are not re-collected)
from mocha_sigasia2023_amd import synthetic, weights                        # noqa: E402
from oracle import live_oracle as LO                                        # noqa: E402
from oracle import postprocess_oracle as P                                  # noqa: E402

LAYOUT, V, J, TOES, PARENTS = TLO.LAYOUT, TLO.V, TLO.J, TLO.TOES, TLO.PARENTS
F = 60 + 5                                                                  # pushes of the two main runs: six valid frames
EVENTS = 60 + 66                                                            # pushes of the events run
RESET_AT, CHANGE_AT = 65, 70
KEYS = ("pos", "rot", "ik_rot", "bvh_pos", "bvh_euler")
SPREAD = 5.4e-7
E2E_BOUND = max(1e-4, 4 * SPREAD)

_plan = TLO._plan
# stream plans: (clip, character) pairs of test_live_oracle's S4 run, whose matches are known to be clear
RUNS = {
    "S1": (_plan(0, F, 2),),
    "S3": (_plan(0, F, 2), _plan(1, F, 0), _plan(2, F, 1)),
    "events": (_plan(0, EVENTS, 0), _plan(2, EVENTS, 1, reset_at=RESET_AT), _plan(1, EVENTS, 1, char_at=(CHANGE_AT, 0))),
    "events_no_reset": (_plan(0, EVENTS, 0), _plan(2, EVENTS, 1), _plan(1, EVENTS, 1, char_at=(CHANGE_AT, 0))),
}


@functools.lru_cache(maxsize=None)
def _cvae():
    csd = weights.synthetic_cvae_state_dict(99, 1.0)
    rng = np.random.Generator(np.random.PCG64(3))                           # the statistics of tests/test_hip_cvae.py
    stats = ((0.1 * rng.standard_normal((90, 256))).astype(np.float32), rng.uniform(0.5, 1.5, (90, 256)).astype(np.float32),
             (0.1 * rng.standard_normal((90, 256))).astype(np.float32), rng.uniform(0.5, 1.5, (90, 256)).astype(np.float32))
    return csd, stats


@functools.lru_cache(maxsize=None)
def _eps():
    """The sampler's noise of the noise="given" runs: (push, stream, 256)."""
    return np.ascontiguousarray(synthetic.token_features(4242, EVENTS)[:, :3])


def _reference(float64=False):
    w = TLO._inputs()
    csd, stats = _cvae()
    return R.OursOracle(w["sd"], LAYOUT, w["pose_norm"], w["mean"], w["std"], TLO._oracle_banks(float64), TOES, csd, stats, float64=float64)


def _reference_run(plan, s, float64=False):
    o = _reference(float64)
    out = []
    for k, (clip, f, char, reset) in enumerate(plan):
        if reset:
            o.reset()
        out.append(o.push(*TLO._push_args(clip, f), char, eps=_eps()[k, s]))
    return out


_reference_run_cached = functools.lru_cache(maxsize=None)(lambda plan, s: _reference_run(plan, s))


# ------------------------------------------------------------------------------------------------ CPU
def test_philox4x32_10_known_answers():
    """Random123's kat_vectors for philox4x32-10: counter, key -> output.  (Third word of the all-ones vector: a20bc7c6, as Random123's
    file has it.  A bijection of ten mixing rounds cannot miss one word by three units and hit the other eleven of these twelve.)"""
    kat = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
           ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
           ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]
    for ctr, key, want in kat:
        got = R.philox4x32_10(np.array(ctr, np.uint32), np.array(key, np.uint32))
        assert tuple(int(x) for x in got) == want, (ctr, key, [hex(int(x)) for x in got])
    # vectorised over leading axes, as device_noise uses it
    got = R.philox4x32_10(np.array([k[0] for k in kat], np.uint32), np.array([k[1] for k in kat], np.uint32))
    assert [tuple(int(x) for x in row) for row in got] == [k[2] for k in kat]
    e = R.device_noise(7, 1, 3)
    assert e.shape == (256,) and np.isfinite(e).all() and not np.array_equal(e, R.device_noise(7, 2, 3)) and not np.array_equal(e, R.device_noise(7, 1, 4))
    assert not np.array_equal(e, R.device_noise(7 << 32, 1, 3))              # both words of the seed are key


def test_reference_equals_the_clip_at_once_composition():
    """The frame-at-a-time reference against the clip at once from the same oracle parts: windows -> featurize -> encode -> search ->
    the loop of tests/test_hip_cvae.py::test_ours_branch_frames_match_oracle (frame 0 on the matched row, then condition -> sample ->
    de-normalise -> decode, feeding the feature back) -> pose heads -> run_clip."""
    w = TLO._inputs()
    csd, stats = _cvae()
    clip, char, frames = 1, 0, F
    got = _reference_run_cached(RUNS["S3"][1], 1)
    assert [g["valid"] for g in got] == [0] * 59 + [1] * 6 and all(set(g) == {"valid"} for g in got[:59])
    assert [g["seeded"] for g in got[59:]] == [1, 0, 0, 0, 0, 0]
    sd, tc = LO.torch_state(w["sd"]), R.cvae_state(csd)
    X = TLO.FO.featurize(*[synthetic.slide_windows(a[:frames]) for a in w["clips"][clip]], PARENTS)
    enc, cnt = LO.encode_windows(sd, X, w["pose_norm"])
    nm, encoded = TLO._oracle_banks()[char]
    q = LO.O.znorm(cnt.numpy(), w["mean"], w["std"])
    idx = [int(LO.search(q[i], nm)[0][0]) for i in range(len(q))]
    sm, ss, cm, cs = (torch.from_numpy(a) for a in stats)
    prev = torch.from_numpy(encoded[idx[0]])[None]
    Y = [LO.decode(sd, enc[:1], prev[0].numpy(), w["pose_norm"])]
    for i in range(1, len(q)):
        with torch.no_grad():
            cond = torch.cat([(cnt[i:i + 1] - sm) / ss, (prev - cm) / cs], dim=1)
            vae, _, _ = R.CO.sample(tc, cond, torch.from_numpy(_eps()[59 + i, 1])[None])
            prev = vae * cs + cm
        assert np.array_equal(got[59 + i]["cond"], cond.numpy()[0]) and np.array_equal(got[59 + i]["prev"], prev.numpy()[0]), i
        Y.append(LO.decode(sd, enc[i:i + 1], prev[0].numpy(), w["pose_norm"]))
    Y = np.stack(Y)
    heads, speed = P.pose_heads(Y)
    pos, rot, ik = P.run_clip(heads, speed, *[a[59:frames] for a in w["per"][clip]], PARENTS, contact_bones=TOES)
    bp, be = P.bvh_channels(pos, ik)
    ref = dict(idx=np.array(idx), Y=Y, pos=pos, rot=rot, ik_rot=ik, bvh_pos=bp, bvh_euler=be)
    for k, r in ref.items():
        a = np.stack([np.asarray(g[k]) for g in got[59:]])
        assert a.shape == r.shape and np.array_equal(a, r), k
    # a seed frame IS the nearest-neighbour frame of the live oracle
    nn = TLO._oracle_run(RUNS["S3"][1][:60])[59]
    assert all(np.array_equal(nn[k], got[59][k]) for k in ("Y",) + KEYS)
    assert not np.array_equal(TLO._oracle_run(RUNS["S3"][1][:61])[60]["Y"], got[60]["Y"])


def test_inputs_have_clear_matches():
    """Every valid frame of the S = 1 / S = 3 runs (idx is asserted on each of them) and every seed frame of the events run: the float64
    gap between the best and the second-best row of the stream's own character is at least 1e-4 relative, so the GPU tests accept no
    near-tie at all."""
    gaps = []
    for s, plan in enumerate(RUNS["S3"]):
        gaps += [((g["dist2"] - g["dist"]) / g["dist"], "S3", s, k) for k, g in enumerate(_reference_run_cached(plan, s)) if g["valid"]]
    for s, plan in enumerate(RUNS["events"]):                              # seed frames: push 59 of every stream (a reset stream sees its
        run = TLO._oracle_run(plan[:CHANGE_AT + 1 if s == 2 else 60])      # clip from frame 0 again), push 70 of the stream that changes
        gaps += [((run[k]["dist2"] - run[k]["dist"]) / run[k]["dist"], "events", s, k) for k in ([59, CHANGE_AT] if s == 2 else [59])]
    print("min relative gap", min(gaps))
    assert min(g[0] for g in gaps) >= 1e-4, min(gaps)
    assert RUNS["S1"][0] == RUNS["S3"][0]


def test_end_to_end_bound_covers_the_reference_spread():
    """The measurement behind E2E_BOUND, repeated on one stream: the reference chain in float64 against fp32, same noise."""
    plan = RUNS["S1"][0]
    a, b = _reference_run_cached(plan, 0), _reference_run(plan, 0, float64=True)
    assert [x.get("idx") for x in a] == [y.get("idx") for y in b]
    spread = max(max(np.abs(x[k] - y[k]).max() for k in ("pos", "rot")) for x, y in zip(a, b) if x["valid"])
    print(f"fp32 / float64 reference spread on pos, rot: {spread:.3e}")
    assert b[-1]["Y"].dtype == np.float64 and b[-1]["vae"].dtype == np.float64 and a[-1]["vae"].dtype == np.float32
    assert 0 < spread and 4 * spread <= E2E_BOUND and 4 * SPREAD <= E2E_BOUND


# ------------------------------------------------------------------------------------------------ GPU
@pytest.fixture(scope="module")
def world():
    from mocha_sigasia2023_amd import Generator, MultiCharacterBank, PostProcessor, build_bank
    d, w = TLO.dev(), TLO._inputs()
    model = Generator(layout=LAYOUT, device=d).load_state_dict(w["sd"]).eval()
    model.set_pose_norm(*w["pose_norm"])
    mean, std = torch.from_numpy(w["mean"]).to(d), torch.from_numpy(w["std"]).to(d)
    banks = []
    for clip in w["bank_clips"]:
        b = build_bank(model, model.featurize(*[torch.from_numpy(synthetic.slide_windows(a)) for a in clip]), raw=True)
        banks.append((((b["cnt"] - mean) / std).reshape(-1, 90 * 256), b["encoded"]))
    mb = MultiCharacterBank(model, banks)
    post = PostProcessor(model, contact_bones=list(TOES))
    return dict(model=model, mean=mean, std=std, mb=mb, post=post)


def _session(world, S, noise="given", seed=0):
    from mocha_sigasia2023_amd import LiveOursSession
    csd, stats = _cvae()
    return LiveOursSession(world["mb"], world["mean"], world["std"], csd, *stats, streams=S, post=world["post"], noise=noise, seed=seed)


def _ours_staging(sess):
    """Views of the sections of `ours` (include/mocha_hip.h: every section on a 256-byte boundary), checked against
    mocha_live_ours_state_bytes."""
    S = sess.streams
    lib, h = sess.model._ctx.lib, sess.model._ctx.h
    T = 90 * 256 * 4
    sections = [("counters", S * 12, torch.int32, (S, 3)), ("prev", S * T, torch.float32, (S, 90, 256)), ("cnt", S * T, torch.float32, (S, 90, 256)),
                ("cond", S * 2 * T, torch.float32, (S, 180, 256)), ("vae", S * T, torch.float32, (S, 90, 256)),
                ("eps", S * 1024, torch.float32, (S, 256)), ("mu", S * 1024, torch.float32, (S, 256)), ("logvar", S * 1024, torch.float32, (S, 256))]
    out, at = {}, 0
    for name, n, dt, shape in sections:
        out[name] = sess.ours[at: at + n].view(dt).reshape(shape)
        at += (n + 255) // 256 * 256
    assert at == int(lib.mocha_live_ours_state_bytes(h, S)) == sess.ours.numel()
    assert out["prev"].data_ptr() == sess.cha_encoded.data_ptr() and out["prev"].shape == sess.cha_encoded.shape
    return out


def _run_device(world, plans, sess=None, noise="given", seed=0, pushes=None):
    """A session over the streams' plans -> per push a dict of NumPy arrays (all streams): outputs, the staging of both buffers."""
    S = len(plans)
    sess = sess or _session(world, S, noise, seed)
    stage = dict(_ours_staging(sess), Y=TLO._staging(sess)["Y"])
    for k in KEYS:
        sess.out[k].fill_(-12345.0)
    rec = []
    for k in range(pushes or len(plans[0])):
        resets = [s for s in range(S) if plans[s][k][3]]
        if resets:
            sess.reset(resets)
        if noise == "given":
            sess.eps.copy_(torch.from_numpy(_eps()[k, :S]))
        args = [np.stack([TLO._push_args(plans[s][k][0], plans[s][k][1])[i] for s in range(S)]) for i in range(8)]
        o = sess.push(*[torch.from_numpy(np.ascontiguousarray(a)) for a in args], characters=[plans[s][k][2] for s in range(S)])
        torch.cuda.synchronize()
        r = {n: o[n].cpu().numpy().copy() for n in KEYS + ("idx", "valid", "seeded")}
        r.update({n: t.cpu().numpy().copy() for n, t in stage.items()})
        rec.append(r)
    return rec


def _check_stream(world, rec, s, plan, errs):
    """Stream s of a recorded noise="given" run, stage by stage (each stage against the reference fed the device's own previous stage)
    and end to end against the independent reference run (module docstring)."""
    w = TLO._inputs()
    csd, stats = _cvae()
    sm, ss, cm, cs = (a.astype(np.float64) for a in stats)
    sd, tc = LO.torch_state(w["sd"]), R.cvae_state(csd)
    ref = _reference_run_cached(plan, s)
    first = True

    def worst(name, e, bound=1.0):
        errs[name] = max(errs.get(name, 0.0), float(e))
        assert e <= bound, (name, s, k, float(e), bound)
    for k, (clip, f, char, reset) in enumerate(plan):
        r, o = rec[k], ref[k]
        assert int(r["valid"][s]) == o["valid"], (s, k)
        if not o["valid"]:
            assert int(r["idx"][s]) == -1 and int(r["seeded"][s]) == 0 and not r["counters"][s].any() and not r["prev"][s].any(), (s, k)
            assert all((r[n][s] == -12345.0).all() for n in KEYS), (s, k)
            continue
        assert int(r["idx"][s]) == o["idx"], (s, k, int(r["idx"][s]), o["idx"])
        assert int(r["seeded"][s]) == (1 if first else 0) == o["seeded"], (s, k)
        assert r["counters"][s].tolist() == [k - 58, char, 1 if first else 2], (s, k, r["counters"][s])
        cnt = r["cnt"][s].astype(np.float64)
        worst("cnt vs reference (reported, not bounded here)", np.abs(cnt - o["cnt"]).max(), np.inf)
        zc = (cnt - sm) / ss
        want = np.concatenate([zc, np.zeros_like(zc) if first else (rec[k - 1]["prev"][s].astype(np.float64) - cm) / cs])
        worst("cond / (1e-6 max(1, |ref|))", (np.abs(r["cond"][s] - want) / (1e-6 * np.maximum(1.0, np.abs(want)))).max())
        if first:
            assert not r["cond"][s][90:].any(), (s, k)
        with torch.no_grad():
            vae, mu, lv = R.cvae_sample(tc, torch.from_numpy(r["cond"][s][None]), torch.from_numpy(r["eps"][s][None]))
        assert np.array_equal(r["eps"][s], _eps()[k, s]), (s, k)
        for n, t in (("vae", vae), ("mu", mu), ("logvar", lv)):
            worst(n, np.abs(r[n][s] - t.numpy()[0]).max(), 1e-4 * max(1.0, float(t.abs().max())))
        if first:
            g0, _ = world["mb"].rows(char)
            assert np.array_equal(r["prev"][s], world["mb"].encoded[g0 + int(r["idx"][s])].cpu().numpy()), (s, k)
        else:
            want = r["vae"][s].astype(np.float64) * cs + cm
            worst("prev, relative", (np.abs(r["prev"][s] - want) / np.maximum(np.abs(want), 1e-30)).max(), 1e-6)
        worst("Y", np.abs(r["Y"][s] - LO.decode(sd, o["enc"], r["prev"][s], w["pose_norm"])).max(), 1e-4)
        for n in ("pos", "rot"):
            worst("end to end " + n, np.abs(r[n][s] - o[n]).max(), E2E_BOUND)
        first = False


@pytest.mark.gpu
@pytest.mark.parametrize("run", ["S1", "S3"])
def test_live_ours_session_against_the_reference(world, run):
    """S = 1 and S = 3 (characters 2, 0, 1), 60 + 5 pushes, noise given: every valid frame of every stream, stage by stage and end to
    end, at the bounds of the module docstring."""
    plans = RUNS[run]
    rec = _run_device(world, plans)
    errs = {}
    try:
        for s, plan in enumerate(plans):
            _check_stream(world, rec, s, plan, errs)
    finally:
        for k, v in errs.items():
            print(f"{run}: max error {k}: {v:.3e}")
    assert all(int(r["valid"].sum()) == (len(plans) if k >= 59 else 0) for k, r in enumerate(rec))


@pytest.mark.gpu
def test_seed_frame_is_the_nearest_neighbour_frame(world):
    """The first valid frame of LiveOursSession is that of a LiveSession on the same inputs, bit for bit in the Y staging and in every
    output: the literal decoder flow on the seeded feature against the cached flow on the matched row."""
    from mocha_sigasia2023_amd import LiveSession
    plans = RUNS["S3"]
    ours = _run_device(world, plans, pushes=60)[59]
    sess = LiveSession(world["mb"], world["mean"], world["std"], streams=3, post=world["post"])
    stage = TLO._staging(sess)
    for k in range(60):
        args = [np.stack([TLO._push_args(p[k][0], p[k][1])[i] for p in plans]) for i in range(8)]
        o = sess.push(*[torch.from_numpy(np.ascontiguousarray(a)) for a in args], characters=[p[k][2] for p in plans])
    torch.cuda.synchronize()
    assert o["valid"].tolist() == [1, 1, 1] and ours["seeded"].tolist() == [1, 1, 1]
    assert np.array_equal(o["idx"].cpu().numpy(), ours["idx"])
    dY = np.abs(stage["Y"].cpu().numpy() - ours["Y"]).max()
    print(f"seed frame vs LiveSession: max |Y| difference {dY:.3e}")
    assert dY == 0.0
    for n in KEYS:
        assert np.array_equal(o[n].cpu().numpy(), ours[n]), n


@pytest.fixture(scope="module")
def events(world):
    return _run_device(world, RUNS["events"]), _run_device(world, RUNS["events_no_reset"])


@pytest.mark.gpu
def test_events_reset_stream_seeds_again_and_disturbs_no_other(events):
    """Stream 1 is reset before push 65: it warms up for 59 pushes - its counters, prev and (zero) cond do not change meanwhile, no
    output row is written - and seeds again on push 124; streams 0 and 2 are bit for bit what they are in the same run without the
    reset."""
    a, b = events
    assert [int(r["valid"][1]) for r in a] == [0] * 59 + [1] * 6 + [0] * 59 + [1] * (EVENTS - 124)
    assert [k for k, r in enumerate(a) if r["seeded"][1]] == [59, 124]
    assert [r["counters"][1].tolist() for r in a[59:65]] == [[i + 1, 1, 1 if i == 0 else 2] for i in range(6)]
    for k in range(RESET_AT, 124):
        assert a[k]["counters"][1].tolist() == [0, 0, 0], k
        assert np.array_equal(a[k]["prev"][1], a[RESET_AT - 1]["prev"][1]) and not a[k]["cond"][1].any(), k
        assert all(np.array_equal(a[k][n][1], a[RESET_AT - 1][n][1]) for n in KEYS), k
    assert a[124]["counters"][1].tolist() == [1, 1, 1] and a[125]["counters"][1].tolist() == [2, 1, 2]
    # the reset stream sees its clip from frame 0 again: its second seed frame is its first one (same window, fresh post state)
    assert all(np.array_equal(a[124][n][1], a[59][n][1]) for n in KEYS + ("prev", "Y"))
    assert not np.array_equal(a[125]["prev"][1], a[60]["prev"][1])          # other noise on the chain frame that follows
    for s in (0, 2):
        for k in range(EVENTS):
            for n in KEYS + ("idx", "valid", "seeded", "prev", "vae", "cond", "Y"):
                assert np.array_equal(a[k][n][s], b[k][n][s]), (s, k, n)
    assert any(not np.array_equal(a[k]["pos"][1], b[k]["pos"][1]) for k in range(RESET_AT, EVENTS))


@pytest.mark.gpu
def test_events_character_change_seeds_from_the_new_character(world, events):
    """Stream 2 goes from character 1 to character 0 before push 70: that push is a seed frame and its prev is the matched row of
    character 0; the stream's ring and post state go on."""
    a, _ = events
    assert [k for k, r in enumerate(a) if r["seeded"][2]] == [59, CHANGE_AT]
    assert [int(r["valid"][2]) for r in a] == [0] * 59 + [1] * (EVENTS - 59)
    r = a[CHANGE_AT]
    g0, g1 = world["mb"].rows(0)
    assert 0 <= int(r["idx"][2]) < g1 - g0
    assert np.array_equal(r["prev"][2], world["mb"].encoded[g0 + int(r["idx"][2])].cpu().numpy())
    assert r["counters"][2].tolist() == [CHANGE_AT - 58, 0, 1] and a[CHANGE_AT - 1]["counters"][2].tolist() == [CHANGE_AT - 59, 1, 2]
    assert a[CHANGE_AT + 1]["counters"][2].tolist() == [CHANGE_AT - 57, 0, 2]
    ref = TLO._oracle_run(RUNS["events"][2][:CHANGE_AT + 1])
    assert int(r["idx"][2]) == ref[CHANGE_AT]["idx"] and int(a[59]["idx"][2]) == ref[59]["idx"]
    assert not np.array_equal(r["ik_rot"][2], r["rot"][2])                  # not a first frame of the post state
    assert [k for k, x in enumerate(a) if x["seeded"][0]] == [59]


@pytest.mark.gpu
def test_device_noise(world):
    """noise="device": eps after every step against the NumPy restatement (Philox4x32-10 + Box-Muller in double) within 1e-5 absolute -
    the inputs u are the same float32 numbers on both sides, r <= 5.9, a few ulp from each of logf, sqrtf, sinf / cosf, and about 2e-6
    from the angle's float32 product; the same seed repeats a session bit for bit, another seed and another stream do not; mean and
    variance over 20 frames x 3 streams x 256 values."""
    plans, n = RUNS["S3"], 60 + 19
    plans = tuple(_plan(p[0][0], n, p[0][2]) for p in plans)
    a = _run_device(world, plans, noise="device", seed=(5 << 32) | 7)
    worst, vals = 0.0, []
    for k, r in enumerate(a):
        for s in range(3):
            chain = int(r["counters"][s][0]) - int(r["valid"][s])           # the counter the step drew with: before its increment
            assert chain == max(k - 59, 0)
            worst = max(worst, float(np.abs(r["eps"][s] - R.device_noise((5 << 32) | 7, s, chain)).max()))
            if r["valid"][s]:
                vals.append(r["eps"][s])
    print(f"device noise vs restatement: max error {worst:.3e}")
    assert worst <= 1e-5
    vals = np.concatenate(vals).astype(np.float64)
    assert vals.size == 20 * 3 * 256
    print(f"device noise: mean {vals.mean():.4f}, var {vals.var():.4f} over {vals.size} values")
    assert abs(vals.mean()) < 5 / np.sqrt(vals.size) and abs(vals.var() - 1) < 0.1
    assert not np.array_equal(a[70]["eps"][0], a[70]["eps"][1]) and not np.array_equal(a[70]["eps"][0], a[71]["eps"][0])
    b = _run_device(world, plans, noise="device", seed=(5 << 32) | 7)
    for k in range(n):
        for key in KEYS + ("eps", "prev", "idx", "seeded"):
            assert np.array_equal(a[k][key], b[k][key]), (k, key)
    c = _run_device(world, plans, noise="device", seed=(5 << 32) | 8, pushes=62)
    assert not np.array_equal(a[61]["eps"], c[61]["eps"]) and not np.array_equal(a[61]["pos"], c[61]["pos"])
    assert np.array_equal(a[59]["pos"], c[59]["pos"])                        # the seed frame does not depend on the noise
    d = _run_device(world, plans, noise="none", pushes=62)
    assert np.array_equal(d[61]["vae"].shape, (3, 90, 256)) and not np.array_equal(d[61]["pos"], a[61]["pos"])
