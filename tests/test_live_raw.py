"""Raw mocap frames into a live session on the MI355X (run with -m gpu): LiveSession(raw=...) / push_raw / mocha_live_step_raw.

The world is the one of tests/test_live_inertial.py (mixamo layout, 3 characters of 40 rows, 2 streams); the raw clips are
ingest_ref.walk_clip on the mixamo skeleton, Euler degrees and centimetres.  The reference composition is the staged route on the SAME
context: Ingestor.step -> LiveSession.push of the emitted frames.  Same kernels, same launch shapes: every comparison is exact."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ingest_ref as R  # noqa: E402
from mocha_sigasia2023_amd import (Generator, IngestConfig, Ingestor, LiveSession, MultiCharacterBank, PostProcessor, build_bank,  # noqa: E402
                                   synthetic, weights)
from mocha_sigasia2023_amd.skeleton import LAYOUTS  # noqa: E402

pytestmark = pytest.mark.gpu
V, J = 22, 23
F, LONG = 100, 190
L = 2
SOFT, HALFLIFE = (4, 2.0), 0.1
CHARS, AFTER, SWITCH = [2, 0], [1, 0], 95           # stream 0 names character 2, from push 96 (index 95) on character 1
KINDS = {"hard": dict(), "soft": dict(soft=SOFT), "inertial": dict(inertial=HALFLIFE)}


def dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def world():
    d = dev()
    model = Generator(layout="mixamo", device=d).load_state_dict(weights.synthetic_state_dict(1777, 1.0, "mixamo")).eval()
    rng = np.random.Generator(np.random.PCG64(0))
    X_mean = (0.05 * rng.standard_normal((J, 15))).astype(np.float32); X_std = rng.uniform(0.5, 1.5, (J, 15)).astype(np.float32)
    Y_mean = (0.05 * rng.standard_normal((J, 15))).astype(np.float32); Y_std = rng.uniform(0.2, 0.6, (J, 15)).astype(np.float32)
    model.set_pose_norm(X_mean, X_std, Y_mean, Y_std)
    mean_, std_ = synthetic.cnt_norm(7)
    mean, std = torch.from_numpy(mean_).to(d), torch.from_numpy(std_).to(d)
    banks = []
    for seed in (101, 102, 103):
        clip = synthetic.smooth_bone_clip(seed, 60 + 40 - 1, J)
        X = model.featurize(*[torch.from_numpy(synthetic.slide_windows(a)) for a in clip])
        b = build_bank(model, X, raw=True)
        banks.append((((b["cnt"] - mean) / std).reshape(-1, 90 * 256), b["encoded"]))
    mb = MultiCharacterBank(model, banks)
    par = LAYOUTS["mixamo"]["parents"]
    clips = [R.walk_clip(par, LONG, seed=300 + s, legs=((18, 19, 20, 21), (14, 15, 16, 17)), shoulders=(6, 10), spine=(1, 2, 3), flip_bone=9)
             for s in range(2)]
    rot = torch.from_numpy(np.stack([c[0] for c in clips])).to(d)             # (2, LONG, V, 3) degrees
    pos = torch.from_numpy(np.stack([c[1] for c in clips])).to(d)             # (2, LONG, V, 3) centimetres
    post = PostProcessor(model, contact_bones=[22, 18])                       # the two toes of the mixamo layout, root bone in front
    zeros = torch.zeros((2, 60, J, 15), device=d)
    mb.characterize(zeros, [0, 0], mean, std, raw=True)                       # eager first: everything made on first use exists
    mb.characterize(zeros, [0, 0], mean, std, raw=True, soft=SOFT)
    return dict(model=model, mean=mean, std=std, mb=mb, rot=rot, pos=pos, post=post)


def _session(w, raw=None, **kind):
    return LiveSession(w["mb"], w["mean"], w["std"], streams=2, post=w["post"], raw=raw, **kind)


def _chars(f):
    return CHARS if f == 0 else (AFTER if f == SWITCH else None)


def _run_raw(w, sess, frames=F, check_generation=False):
    got = {k: [] for k in sess.out}
    gen = None
    for f in range(frames):
        o = sess.push_raw(w["rot"][:, f], w["pos"][:, f], characters=_chars(f))
        if check_generation:
            gen = gen or w["model"]._ctx.generation()
            assert w["model"]._ctx.generation() == gen, f                       # captured once: frames and ids are device data
        for k in got:
            got[k].append(o[k].clone())
    return {k: torch.stack(v, 1) for k, v in got.items()}


def _run_staged(w, kind):
    """Ingestor.step, then push of the emitted frame into a session without a front end: outputs after every raw frame."""
    ing = Ingestor(w["model"], L, streams=2, post=w["post"])
    sess = _session(w, **kind)
    got = {k: [] for k in sess.out}
    for f in range(F):
        e = ing.step(w["rot"][:, f], w["pos"][:, f])
        if f == 0:
            sess.characters.copy_(torch.tensor(CHARS, dtype=torch.int32))
        if f == SWITCH:
            sess.characters.copy_(torch.tensor(AFTER, dtype=torch.int32))
        if f >= R.FIRST - 1:                                                    # both streams emit from push 31 on
            sess.push(e["Yrot"], e["Ypos"], e["Yvel"], e["Yang"], e["src_rvel"], e["src_rang"], e["src_speed"], e["contact"])
        for k in got:
            got[k].append(sess.out[k].clone())
    assert ing.out["have"].tolist() == [1, 1]
    return {k: torch.stack(v, 1) for k, v in got.items()}


@pytest.fixture(scope="module")
def raw_runs(world):
    r = {name: _run_raw(world, _session(world, raw=L, **kind), check_generation=(name == "hard")) for name, kind in KINDS.items()}
    torch.cuda.synchronize()
    return r


@pytest.mark.parametrize("name", list(KINDS))
def test_push_raw_equals_the_staged_route(world, raw_runs, name):
    got, ref = raw_runs[name], _run_staged(world, KINDS[name])
    torch.cuda.synchronize()
    assert set(got) == set(ref)
    assert got["valid"][:, :89].eq(0).all() and got["valid"][:, 89:].eq(1).all()
    for k in got:
        assert torch.equal(got[k], ref[k]), (k, name)
    assert not torch.equal(got["pos"][:, 89], got["pos"][:, 99])             # the session produced something


def test_valid_first_on_push_90_for_every_lookahead(world):
    w = world
    for look in range(R.MAX_LOOKAHEAD + 1):
        sess = _session(w, raw=IngestConfig(lookahead=look))
        valid = []
        for f in range(91):
            valid.append(sess.push_raw(w["rot"][:, f], w["pos"][:, f], characters=CHARS if f == 0 else None)["valid"].clone())
        torch.cuda.synchronize()
        v = torch.stack(valid, 1).cpu()
        assert v[:, :89].eq(0).all() and v[:, 89:].eq(1).all(), look


def _run_schedule(w, sess, reset_at=None):
    """LONG - 1 pushes: stream 1 walks its clip; stream 0 too, starting it over at `reset_at`; stream 1 names character 1 from push 121."""
    got = {k: [] for k in sess.out}
    gen = None
    for f in range(LONG - 1):
        if f == reset_at:
            sess.reset([0])
        f0 = f - reset_at if reset_at is not None and f >= reset_at else f
        o = sess.push_raw(torch.stack([w["rot"][0, f0], w["rot"][1, f]]), torch.stack([w["pos"][0, f0], w["pos"][1, f]]),
                          characters=CHARS if f == 0 else ([CHARS[0], 1] if f == 120 else None))
        gen = gen or w["model"]._ctx.generation()
        assert w["model"]._ctx.generation() == gen, f                           # a reset and a new id are device data: no new capture
        for k in got:
            got[k].append(o[k].clone())
    torch.cuda.synchronize()
    return {k: torch.stack(v, 1) for k, v in got.items()}


def test_a_mid_clip_reset_starts_that_stream_over(world, raw_runs):
    """reset([0]) before push 97: stream 0 warms for 89 pushes of its clip from frame 0 and its push 90 is a fresh session's; stream 1 keeps
    the bits of a run without the reset; nothing is captured again."""
    w, at = world, 96
    plain = _run_schedule(w, _session(w, raw=L))
    got = _run_schedule(w, _session(w, raw=L), reset_at=at)
    assert got["valid"][0].tolist() == [0] * 89 + [1] * (at - 89) + [0] * 89 + [1] * (LONG - 1 - at - 89)
    assert got["valid"][1].tolist() == [0] * 89 + [1] * (LONG - 1 - 89)
    fresh = raw_runs["hard"]
    for k in got:
        assert torch.equal(got[k][0, :at], plain[k][0, :at]), k
        assert torch.equal(got[k][0, at + 89], fresh[k][0, 89]), k              # the stream's first valid frame after the reset
        assert torch.equal(got[k][1], plain[k][1]), k                           # the other stream never notices
    assert not torch.equal(plain["idx"][1, 119], plain["idx"][1, 121]) or not torch.equal(plain["pos"][1, 119], plain["pos"][1, 121])


def test_profiling_runs_the_step_eagerly_and_names_the_launch(world):
    w = world
    sess = _session(w, raw=L)
    sess.push_raw(w["rot"][:, 0], w["pos"][:, 0], characters=CHARS)
    w["model"].profile_start()
    sess.replay_raw()
    prof = w["model"].profile_stop()
    assert prof["kernels"]["mocha_live_ingest"]["launches"] == 1
    assert [k for k in prof["sites"] if k.split("|")[0] == "live.ingest"] == ["live.ingest|mocha_live_ingest"], list(prof["sites"])


def test_a_session_without_raw_refuses_push_raw(world):
    with pytest.raises(RuntimeError, match="raw="):
        _session(world).push_raw(world["rot"][:, 0], world["pos"][:, 0])
