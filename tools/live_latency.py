#!/usr/bin/env python3
"""Latency of the live step (LiveSession.push = mocha_live_step: ring push + featurize -> segmented characterize -> pose heads -> one
post-processing frame, one captured graph) on one MI355X, next to the step it is built on (MultiStreamCharacterizer.step =
mocha_step_graph_segmented alone), for S = 1 and S = 8 streams against an 8 x 2 048-row fp32 segmented bank.

Both steps are timed in ONE process with HIP events around single replays, alternating live / baseline replay by replay after a
warm-up, so that both see the same clocks and the same neighbours; p50 and p99 over --reps replays each.  Clocks are not touched.
The three launches the live step adds (mocha_live_push, mocha_pose_heads, the post-processing frame = mocha_post_clip + mocha_post_bvh on one
frame) are then timed one launch at a time with
mocha_profile_start / stop, during which the step runs eagerly.

    python tools/live_latency.py [--reps 1000] [--out profiles/r08/live_step.json]
    python tools/live_latency.py --baseline-only      only the segmented step (runs on a build without the live step, too)
    python tools/live_latency.py --ours [--out profiles/r09/live_ours_step.json]
        the CVAE ("Ours") branch: (a) LiveSession.replay, (b) LiveOursSession.replay with device noise, (c) the same frame without the
        live step - featurize + encode + segmented match + OursSession.step + pose heads + PostProcessor.step on a window the caller
        keeps (its upkeep is not timed) - alternating replay by replay in one process, S = 1 and S = 8
    python tools/live_latency.py --ours --grouped [--out profiles/r19/live_ours_grouped_step.json]
        one CVAE per character: (a) LiveOursSession.replay (mocha_live_step_ours, one CVAE), (b) the grouped step
        (LiveOursSession(cvaes=CVAEBank) = mocha_live_step_ours_grouped) with every character on ONE slot, (c) the grouped step with S
        distinct slots - (b) and (c) are one session whose cvae_of is rewritten in place, so nothing captures again - alternating replay
        by replay in one process, S = 1 and S = 8, p50 / p10 / p90; then the sampler's launches one at a time (profile hooks, eager)
    python tools/live_latency.py --inertial 0.1 [--out profiles/r12/live_inert_step.json]
        the plain live step and the inertialized one (LiveSession(inertial=H) = mocha_live_step_inert: one more launch, mocha_inertialize,
        between the pose heads and the post frame), alternating replay by replay in one process, S = 1 and S = 8; stream 0 switches
        character half-way through the warm-up, so the timed inertialized steps take the kernel's arithmetic path
    python tools/live_latency.py --raw 2 [--out profiles/r13/live_raw_step.json]
        the plain live step and the raw step (LiveSession(raw=L) = mocha_live_step_raw: one more launch, mocha_live_ingest, in front of
        the ring push), alternating replay by replay in one process, S = 1 and S = 8, both past their warm-up
    python tools/live_latency.py --world [--out profiles/r22/live_world_step.json]
        the plain live step and the one with world=SkinBind (one more launch, mocha_world_pose, behind the captured graph): both p50 in one
        file, from one run of one tree
    python tools/live_latency.py --mix 1,2,4 [--out profiles/r20/live_mix_step.json]
        character mixing: the plain live step, the soft live step at k = J and the mix step (LiveSession(mix=J) = mocha_live_step_mix)
        with every stream's J components on J different characters, alternating replay by replay in one process, S = 1, 8 and 16, for
        every listed J; then the mix step's own launches one at a time (profile hooks, eager)
    python tools/live_latency.py --coherent L [--out profiles/r24/live_path_step.json]
        coherent matching: the plain live step, the soft live step at k = 1 (the same all-keys scan plus a selection launch: the
        yardstick) and the coherent step (LiveSession(coherent=L) = mocha_live_step_path: the all-keys scan plus the path step),
        alternating replay by replay in one process, S = 1, 8 and 16; then the coherent step's matcher launches one at a time (profile
        hooks, eager)
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from mocha_sigasia2023_amd import Generator, MultiCharacterBank, MultiStreamCharacterizer, synthetic, synthetic_state_dict  # noqa: E402

D = 90 * 256
ADDED = ("live.push", "live.heads", "live.post")       # profiling sites of the launches the live step adds to the segmented step


def event_ms(fn, reps):
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1))
    return np.asarray(out)


def pct(a):
    return {"p50_ms": float(np.percentile(a, 50)), "p99_ms": float(np.percentile(a, 99)), "replays": int(len(a))}


def ours(a, dev, model, mb, mean, std, clip, per, J):
    """--ours: the three routes to a posed frame of the CVAE branch, alternating in one process."""
    from mocha_sigasia2023_amd import CVAE, LiveOursSession, LiveSession, OursSession, PostProcessor, pose_heads
    from mocha_sigasia2023_amd.weights import synthetic_cvae_state_dict
    csd = synthetic_cvae_state_dict(99, 1.0)
    rng = np.random.Generator(np.random.PCG64(3))
    stats = [(0.1 * rng.standard_normal((90, 256))).astype(np.float32), rng.uniform(0.5, 1.5, (90, 256)).astype(np.float32),
             (0.1 * rng.standard_normal((90, 256))).astype(np.float32), rng.uniform(0.5, 1.5, (90, 256)).astype(np.float32)]
    cvae = CVAE(device=dev).load_state_dict(csd).eval()
    res = {"bank": "8 characters x 2048 rows, fp32, segmented", "layout": "mocha (24 joints)",
           "timing": "HIP events around single steps; (a) live step, (b) live step with the CVAE branch and device noise, (c) featurize + encode + "
                     "match + OursSession.step + pose_heads + PostProcessor.step, alternating", "streams": {}}
    for S in (1, 8):
        ids = torch.tensor([(k * 3) % 8 for k in range(S)], dtype=torch.int32)
        live = LiveSession(mb, mean, std, streams=S)
        lo = LiveOursSession(mb, mean, std, csd, *stats, streams=S, noise="device", seed=11)
        old = OursSession(model, cvae, *stats)
        post = PostProcessor(model)
        state = post.state(S)
        frame = [0]

        def push():
            f = frame[0] % 644; frame[0] += 1
            for sess in (live, lo):
                sess.rot.copy_(clip[0][f]); sess.pos.copy_(clip[1][f]); sess.vel.copy_(clip[2][f]); sess.ang.copy_(clip[3][f])
                sess.rvel.copy_(per[0][f]); sess.rang.copy_(per[1][f]); sess.speed.copy_(per[2][f]); sess.contact.copy_(per[3][f])
            return f
        window = [x[:60][None].expand(S, -1, -1, -1).contiguous() for x in clip]     # (c)'s window: kept by the caller, not timed
        ids_d = ids.to(dev)
        f_now = [0]

        def parent_way():
            f = f_now[0]
            enc, cnt, nm = model.encode(model.featurize(*window), mean, std, raw=True)
            _, idx = mb.query(nm, ids_d)
            if old.prev is None:
                # any (S,90,256) feature starts the chain: every timed step is a chain step, whose cost does not depend on the values
                # (the demo seeds with the matched row)
                old.reset(enc)
            Y, _ = old.step(enc, cnt)
            heads, speed = pose_heads(model, Y)
            return post.step(state, heads, speed, per[0][f].expand(S, 3), per[1][f].expand(S, 3), per[2][f].expand(S), per[3][f].expand(S, -1))
        for sess in (live, lo):
            sess.characters.copy_(ids)
        for _ in range(max(a.warmup, 70)):
            f_now[0] = push(); live.replay(); lo.replay(); parent_way()
        torch.cuda.synchronize()
        assert bool((lo.out["valid"] == 1).all()) and not bool(lo.out["seeded"].any())
        ta, tb, tc = [], [], []
        for _ in range(a.reps):
            f_now[0] = push(); torch.cuda.synchronize()
            ta.append(event_ms(live.replay, 1)[0]); tb.append(event_ms(lo.replay, 1)[0]); tc.append(event_ms(parent_way, 1)[0])
        e = {"a_live_step": pct(np.asarray(ta)), "b_live_step_ours": pct(np.asarray(tb)), "c_parent_route": pct(np.asarray(tc))}
        e["b_minus_a_p50_ms"] = e["b_live_step_ours"]["p50_ms"] - e["a_live_step"]["p50_ms"]
        e["c_minus_b_p50_ms"] = e["c_parent_route"]["p50_ms"] - e["b_live_step_ours"]["p50_ms"]
        assert bool(torch.isfinite(lo.out["pos"]).all())
        res["streams"][str(S)] = e
        del live, lo, old
    return res


def ours_grouped(a, dev, model, mb, mean, std, clip, per, J):
    """--ours --grouped: the single-CVAE live step against the grouped one (one slot for all / S distinct slots), alternating."""
    from mocha_sigasia2023_amd import CVAEBank, LiveOursSession
    from mocha_sigasia2023_amd.weights import synthetic_cvae_state_dict

    def stats(slot):
        rng = np.random.Generator(np.random.PCG64(3 + slot))
        return [(0.1 * rng.standard_normal((90, 256))).astype(np.float32), rng.uniform(0.5, 1.5, (90, 256)).astype(np.float32),
                (0.1 * rng.standard_normal((90, 256))).astype(np.float32), rng.uniform(0.5, 1.5, (90, 256)).astype(np.float32)]

    def pct3(t):
        t = np.asarray(t)
        return {"p50_ms": float(np.percentile(t, 50)), "p10_ms": float(np.percentile(t, 10)), "p90_ms": float(np.percentile(t, 90)), "replays": int(len(t))}
    cvaes = CVAEBank(model, 8)
    for slot in range(8):
        cvaes.store(slot, synthetic_cvae_state_dict(99 + slot, 1.0), *stats(slot))
    model.load_cvae(synthetic_cvae_state_dict(99, 1.0))          # the model's own CVAE, after the stores (they stage through the same host copy)
    res = {"bank": "8 characters x 2048 rows, fp32, segmented", "layout": "mocha (24 joints)", "cvae_bank": "8 slots, synthetic CVAEs 99 .. 106",
           "timing": "HIP events around single graph replays; (a) mocha_live_step_ours, (b) mocha_live_step_ours_grouped with every character on "
                     "slot 0, (c) the same session with character c on slot c, alternating; device noise; clocks untouched", "streams": {}}
    one, distinct = torch.zeros(8, dtype=torch.int32, device=dev), torch.arange(8, dtype=torch.int32, device=dev)
    for S in (1, 8):
        ids = torch.tensor([(k * 3) % 8 for k in range(S)], dtype=torch.int32)
        plain = LiveOursSession(mb, mean, std, None, *stats(0), streams=S, noise="device", seed=11)
        grp = LiveOursSession(mb, mean, std, None, None, None, None, None, streams=S, noise="device", seed=11, cvaes=cvaes, cvae_of=distinct)
        frame = [0]

        def push():
            f = frame[0] % 644; frame[0] += 1
            for sess in (plain, grp):
                sess.rot.copy_(clip[0][f]); sess.pos.copy_(clip[1][f]); sess.vel.copy_(clip[2][f]); sess.ang.copy_(clip[3][f])
                sess.rvel.copy_(per[0][f]); sess.rang.copy_(per[1][f]); sess.speed.copy_(per[2][f]); sess.contact.copy_(per[3][f])
        for sess in (plain, grp):
            sess.characters.copy_(ids)
        gen = None
        for i in range(max(a.warmup, 70)):
            push(); plain.replay(); grp.replay()
            gen = model._ctx.generation() if i == 1 else gen
        torch.cuda.synchronize()
        assert bool((grp.out["valid"] == 1).all()) and not bool(grp.out["seeded"].any()) and not bool(plain.out["seeded"].any())
        ta, tb, tc = [], [], []
        for _ in range(a.reps):
            push(); torch.cuda.synchronize()
            ta.append(event_ms(plain.replay, 1)[0])
            grp.cvae_of.copy_(one); torch.cuda.synchronize()
            tb.append(event_ms(grp.replay, 1)[0])
            grp.cvae_of.copy_(distinct); torch.cuda.synchronize()
            tc.append(event_ms(grp.replay, 1)[0])
        assert model._ctx.generation() == gen and not bool(grp.out["seeded"].any())      # nothing captured again, nothing reseeded
        e = {"a_live_step_ours": pct3(ta), "b_grouped_one_slot": pct3(tb), "c_grouped_distinct_slots": pct3(tc)}
        e["b_over_a_p50"] = e["b_grouped_one_slot"]["p50_ms"] / e["a_live_step_ours"]["p50_ms"]
        e["c_over_a_p50"] = e["c_grouped_distinct_slots"]["p50_ms"] / e["a_live_step_ours"]["p50_ms"]
        n = 50                                           # the sampler's launches, one at a time (the steps run eagerly while profiling)
        for name, sess in (("a", plain), ("c", grp)):
            model.profile_start()
            for _ in range(n):
                sess.replay()
            prof = model.profile_stop()
            e[name + "_cvae_sites_us_per_launch"] = {k: 1e3 * v["ms"] / v["launches"] for k, v in prof["sites"].items() if k.startswith("cvae.")}
            e[name + "_cvae_launches_per_step"] = int(sum(v["launches"] for k, v in prof["sites"].items() if k.startswith("cvae.")) // n)
            e[name + "_cvae_sum_us_per_step"] = float(sum(1e3 * v["ms"] for k, v in prof["sites"].items() if k.startswith("cvae.")) / n)
        assert bool(torch.isfinite(grp.out["pos"]).all())
        res["streams"][str(S)] = e
        del plain, grp
    return res


def soft(a, dev, model, mb, mean, std, clip, per, J):
    """--soft K: the hard live step and the soft live step (K neighbours, temperature 2), alternating in one process."""
    from mocha_sigasia2023_amd import LiveSession
    res = {"bank": "8 characters x 2048 rows, fp32, segmented", "layout": "mocha (24 joints)", "soft": [a.soft, 2.0],
           "timing": "HIP events around single graph replays; (a) live step, (b) soft live step, alternating", "streams": {}}
    for S in (1, 8):
        ids = torch.tensor([(k * 3) % 8 for k in range(S)], dtype=torch.int32)
        hard, sft = LiveSession(mb, mean, std, streams=S), LiveSession(mb, mean, std, streams=S, soft=(a.soft, 2.0))
        frame = [0]

        def push():
            f = frame[0] % 644; frame[0] += 1
            for sess in (hard, sft):
                sess.rot.copy_(clip[0][f]); sess.pos.copy_(clip[1][f]); sess.vel.copy_(clip[2][f]); sess.ang.copy_(clip[3][f])
                sess.rvel.copy_(per[0][f]); sess.rang.copy_(per[1][f]); sess.speed.copy_(per[2][f]); sess.contact.copy_(per[3][f])
        for sess in (hard, sft):
            sess.characters.copy_(ids)
        for _ in range(max(a.warmup, 70)):
            push(); hard.replay(); sft.replay()
        torch.cuda.synchronize()
        assert bool((sft.out["valid"] == 1).all()) and bool((sft.out["idx_k"] >= 0).all())
        ta, tb = [], []
        for _ in range(a.reps):
            push(); torch.cuda.synchronize()
            ta.append(event_ms(hard.replay, 1)[0]); tb.append(event_ms(sft.replay, 1)[0])
        e = {"a_live_step": pct(np.asarray(ta)), "b_live_step_soft": pct(np.asarray(tb))}
        e["b_minus_a_p50_ms"] = e["b_live_step_soft"]["p50_ms"] - e["a_live_step"]["p50_ms"]
        n = 100                                         # the soft step's kernels, one launch at a time (eager while profiling)
        model.profile_start()
        for _ in range(n):
            sft.replay()
        prof = model.profile_stop()
        e["soft_sites_us"] = {k: 1e3 * v["ms"] / n for k, v in prof["sites"].items() if k.split("|")[0] in ("match.soft", "dec.in_cha", "dec.style")}
        assert bool(torch.isfinite(sft.out["pos"]).all())
        res["streams"][str(S)] = e
        del hard, sft
    return res


def mix(a, dev, model, mb, mean, std, clip, per, J):
    """--mix J[,J..]: the plain live step, the soft live step at k = J (temperature 2) and the mix step with J components per stream on J
    different characters, alternating in one process.  The soft step has the same literal decoder and a J-row blend; the mix step adds
    the scans of J - 1 further characters and one prep launch."""
    from mocha_sigasia2023_amd import LiveSession
    res = {"bank": "8 characters x 2048 rows, fp32, segmented", "layout": "mocha (24 joints)",
           "timing": "HIP events around single graph replays; (a) live step, (b) soft live step with k = J, temperature 2, (c) mix live step "
                     "with J components per stream on J different characters, alternating; clocks untouched", "streams": {}}
    for S in (1, 8, 16):
        ids = torch.tensor([(k * 3) % 8 for k in range(S)], dtype=torch.int32)
        res["streams"][str(S)] = {}
        for Jm in a.mix:
            hard = LiveSession(mb, mean, std, streams=S)
            sft = LiveSession(mb, mean, std, streams=S, soft=(Jm, 2.0))
            mx = LiveSession(mb, mean, std, streams=S, mix=Jm)
            mx.set_mix((np.array([[(k * 3 + 2 * j) % 8 for j in range(Jm)] for k in range(S)], np.int32),
                        np.array([[(j + 1.0) for j in range(Jm)]] * S, np.float32)))
            frame = [0]

            def push():
                f = frame[0] % 644; frame[0] += 1
                for sess in (hard, sft, mx):
                    sess.rot.copy_(clip[0][f]); sess.pos.copy_(clip[1][f]); sess.vel.copy_(clip[2][f]); sess.ang.copy_(clip[3][f])
                    sess.rvel.copy_(per[0][f]); sess.rang.copy_(per[1][f]); sess.speed.copy_(per[2][f]); sess.contact.copy_(per[3][f])
            for sess in (hard, sft):
                sess.characters.copy_(ids)
            for _ in range(max(a.warmup, 70)):
                push(); hard.replay(); sft.replay(); mx.replay()
            torch.cuda.synchronize()
            assert bool((mx.out["valid"] == 1).all()) and bool((mx.out["idx"] >= 0).all()) and bool((sft.out["idx_k"] >= 0).all())
            ta, tb, tc = [], [], []
            for _ in range(a.reps):
                push(); torch.cuda.synchronize()
                ta.append(event_ms(hard.replay, 1)[0]); tb.append(event_ms(sft.replay, 1)[0]); tc.append(event_ms(mx.replay, 1)[0])
            e = {"a_live_step": pct(np.asarray(ta)), "b_live_step_soft": pct(np.asarray(tb)), "c_live_step_mix": pct(np.asarray(tc))}
            e["c_minus_a_p50_ms"] = e["c_live_step_mix"]["p50_ms"] - e["a_live_step"]["p50_ms"]
            e["c_minus_b_p50_ms"] = e["c_live_step_mix"]["p50_ms"] - e["b_live_step_soft"]["p50_ms"]
            n = 100                                         # the mix step's kernels, one launch at a time (eager while profiling)
            model.profile_start()
            for _ in range(n):
                mx.replay()
            prof = model.profile_stop()
            e["mix_sites_us"] = {k: 1e3 * v["ms"] / n for k, v in prof["sites"].items() if k.split("|")[0] in ("match.mix", "dec.in_cha", "dec.style")}
            assert bool(torch.isfinite(mx.out["pos"]).all())
            res["streams"][str(S)]["J=%d" % Jm] = e
            del hard, sft, mx
    return res


def coherent(a, dev, model, mb, mean, std, clip, per, J):
    """--coherent L: the plain live step, the soft live step at k = 1 and the coherent live step with jump penalty L, alternating in one
    process.  The soft step at k = 1 runs the same plan and all-keys scan and one selection / blend launch where the coherent step runs
    the path step; its decoder is the literal one, the coherent step's the hard one through the bank's per-entry constants."""
    from mocha_sigasia2023_amd import LiveSession
    res = {"bank": "8 characters x 2048 rows, fp32, segmented", "layout": "mocha (24 joints)", "coherent_jump": a.coherent,
           "timing": "HIP events around single graph replays; (a) live step, (b) soft live step with k = 1, temperature 2, (c) coherent live "
                     "step, alternating; clocks untouched", "streams": {}}
    for S in (1, 8, 16):
        ids = torch.tensor([(k * 3) % 8 for k in range(S)], dtype=torch.int32)
        hard = LiveSession(mb, mean, std, streams=S)
        sft = LiveSession(mb, mean, std, streams=S, soft=(1, 2.0))
        co = LiveSession(mb, mean, std, streams=S, coherent=a.coherent)
        frame = [0]

        def push():
            f = frame[0] % 644; frame[0] += 1
            for sess in (hard, sft, co):
                sess.rot.copy_(clip[0][f]); sess.pos.copy_(clip[1][f]); sess.vel.copy_(clip[2][f]); sess.ang.copy_(clip[3][f])
                sess.rvel.copy_(per[0][f]); sess.rang.copy_(per[1][f]); sess.speed.copy_(per[2][f]); sess.contact.copy_(per[3][f])
        for sess in (hard, sft, co):
            sess.characters.copy_(ids)
        gen = None
        for i in range(max(a.warmup, 70)):
            push(); hard.replay(); sft.replay(); co.replay()
            gen = model._ctx.generation() if i == 1 else gen
        torch.cuda.synchronize()
        assert bool((co.out["valid"] == 1).all()) and bool((co.out["idx"] >= 0).all()) and bool(torch.isfinite(co.out["dist"]).all())
        ta, tb, tc = [], [], []
        for _ in range(a.reps):
            push(); torch.cuda.synchronize()
            ta.append(event_ms(hard.replay, 1)[0]); tb.append(event_ms(sft.replay, 1)[0]); tc.append(event_ms(co.replay, 1)[0])
        assert model._ctx.generation() == gen                                     # nothing captured again
        e = {"a_live_step": pct(np.asarray(ta)), "b_live_step_soft_k1": pct(np.asarray(tb)), "c_live_step_path": pct(np.asarray(tc))}
        e["c_minus_a_p50_ms"] = e["c_live_step_path"]["p50_ms"] - e["a_live_step"]["p50_ms"]
        e["c_minus_b_p50_ms"] = e["c_live_step_path"]["p50_ms"] - e["b_live_step_soft_k1"]["p50_ms"]
        e["continued_fraction_last_step"] = float(co.out["continued"].float().mean())
        n = 100                                         # the coherent step's matcher, one launch at a time (eager while profiling)
        model.profile_start()
        for _ in range(n):
            co.replay()
        prof = model.profile_stop()
        e["path_sites_us"] = {k: 1e3 * v["ms"] / n for k, v in prof["sites"].items() if k.split("|")[0] in ("match.path_keys", "match.path_step")}
        model.profile_start()
        for _ in range(n):
            sft.replay()
        prof = model.profile_stop()
        e["soft_sites_us"] = {k: 1e3 * v["ms"] / n for k, v in prof["sites"].items() if k.split("|")[0] in ("match.soft", "dec.in_cha", "dec.style")}
        assert bool(torch.isfinite(co.out["pos"]).all())
        res["streams"][str(S)] = e
        del hard, sft, co
    return res


def constrained(a, dev, model, mb, mean, std, clip, per, J):
    """--constrained: the plain live step and the action-constrained one with zero masks (LiveSession(constrained=True) =
    mocha_live_step_allow: the same launches, the scan reads the masks and one granule word), alternating in one process; then the same
    with every stream allowing one action of 16 (labels in runs of 128 rows)."""
    from mocha_sigasia2023_amd import LiveSession
    mb.set_labels([(np.arange(2048) // 128).astype(np.int32)] * 8)
    res = {"bank": "8 characters x 2048 rows, fp32, segmented, labels in runs of 128 rows (16 actions)", "layout": "mocha (24 joints)",
           "timing": "HIP events around single graph replays; (a) live step, (b) constrained live step with zero masks, (c) constrained live "
                     "step with one action of 16 allowed per stream, alternating", "streams": {}}
    for S in (1, 8):
        ids = torch.tensor([(k * 3) % 8 for k in range(S)], dtype=torch.int32)
        plain = LiveSession(mb, mean, std, streams=S)
        zero = LiveSession(mb, mean, std, streams=S, constrained=True)
        one = LiveSession(mb, mean, std, streams=S, constrained=True)
        one.allow.copy_(torch.tensor([1 << (k % 16) for k in range(S)], dtype=torch.int64))
        frame = [0]

        def push():
            f = frame[0] % 644; frame[0] += 1
            for sess in (plain, zero, one):
                sess.rot.copy_(clip[0][f]); sess.pos.copy_(clip[1][f]); sess.vel.copy_(clip[2][f]); sess.ang.copy_(clip[3][f])
                sess.rvel.copy_(per[0][f]); sess.rang.copy_(per[1][f]); sess.speed.copy_(per[2][f]); sess.contact.copy_(per[3][f])
        for sess in (plain, zero, one):
            sess.characters.copy_(ids)
        for _ in range(max(a.warmup, 70)):
            push(); plain.replay(); zero.replay(); one.replay()
        torch.cuda.synchronize()
        assert bool((zero.out["valid"] == 1).all()) and torch.equal(zero.out["idx"], plain.out["idx"]) and bool((one.out["applied"] == 1).all())
        # the two constrained sessions share ONE captured graph slot of the context (keyed on the session's buffers): alternating them
        # would capture again at every replay, so each is measured in its own pass, alternating with the plain step
        ta, tb, tc = [], [], []
        for sess, t in ((zero, tb), (one, tc)):
            for _ in range(10):
                push(); sess.replay()
            for _ in range(a.reps):
                push(); torch.cuda.synchronize()
                ta.append(event_ms(plain.replay, 1)[0]); t.append(event_ms(sess.replay, 1)[0])
        e = {"a_live_step": pct(np.asarray(ta)), "b_live_step_allow_zero_masks": pct(np.asarray(tb)), "c_live_step_allow_one_of_16": pct(np.asarray(tc))}
        e["b_minus_a_p50_ms"] = e["b_live_step_allow_zero_masks"]["p50_ms"] - e["a_live_step"]["p50_ms"]
        e["c_minus_a_p50_ms"] = e["c_live_step_allow_one_of_16"]["p50_ms"] - e["a_live_step"]["p50_ms"]
        res["streams"][str(S)] = e
        del plain, zero, one
    return res


def inertial(a, dev, model, mb, mean, std, clip, per, J):
    """--inertial H: the plain live step and the inertialized one (half-life H seconds), alternating in one process."""
    from mocha_sigasia2023_amd import LiveSession
    res = {"bank": "8 characters x 2048 rows, fp32, segmented", "layout": "mocha (24 joints)", "inertial_halflife_s": a.inertial,
           "timing": "HIP events around single graph replays; (a) live step, (b) inertialized live step, alternating; every stream of (b) has "
                     "switched character once and is decaying its offsets", "streams": {}}
    for S in (1, 8):
        ids = torch.tensor([(k * 3) % 8 for k in range(S)], dtype=torch.int32)
        plain, inert = LiveSession(mb, mean, std, streams=S), LiveSession(mb, mean, std, streams=S, inertial=a.inertial)
        frame = [0]

        def push():
            f = frame[0] % 644; frame[0] += 1
            for sess in (plain, inert):
                sess.rot.copy_(clip[0][f]); sess.pos.copy_(clip[1][f]); sess.vel.copy_(clip[2][f]); sess.ang.copy_(clip[3][f])
                sess.rvel.copy_(per[0][f]); sess.rang.copy_(per[1][f]); sess.speed.copy_(per[2][f]); sess.contact.copy_(per[3][f])
        for sess in (plain, inert):
            sess.characters.copy_((ids + 1) % 8)
        warm = max(a.warmup, 70)
        for i in range(warm):
            if i == 65:                                  # every stream is running: all of them switch, the offsets start to decay
                for sess in (plain, inert):
                    sess.characters.copy_(ids)
            push(); plain.replay(); inert.replay()
        torch.cuda.synchronize()
        assert bool((inert.out["valid"] == 1).all()) and torch.equal(inert.out["idx"], plain.out["idx"])
        ta, tb = [], []
        for _ in range(a.reps):
            push(); torch.cuda.synchronize()
            ta.append(event_ms(plain.replay, 1)[0]); tb.append(event_ms(inert.replay, 1)[0])
        e = {"a_live_step": pct(np.asarray(ta)), "b_live_step_inert": pct(np.asarray(tb))}
        e["b_minus_a_p50_ms"] = e["b_live_step_inert"]["p50_ms"] - e["a_live_step"]["p50_ms"]
        n = 200                                          # the step's own launches, one at a time (eager while profiling)
        model.profile_start()
        for _ in range(n):
            inert.replay()
        prof = model.profile_stop()
        e["sites_us"] = {k: 1e3 * v["ms"] / v["launches"] for k, v in prof["sites"].items() if k.split("|")[0] in ADDED + ("live.inert",)}
        assert bool(torch.isfinite(inert.out["pos"]).all())
        res["streams"][str(S)] = e
        del plain, inert
    return res


def raw(a, dev, model, mb, mean, std, clip, per, J):
    """--raw L: the plain live step and the raw step (the mocap front end in the graph, L frames of lookahead), alternating in one process."""
    from mocha_sigasia2023_amd import LiveSession
    from mocha_sigasia2023_amd.skeleton import LAYOUTS
    res = {"bank": "8 characters x 2048 rows, fp32, segmented", "layout": "mocha (24 joints)", "lookahead": a.raw,
           "timing": "HIP events around single graph replays; (a) live step, (b) raw live step (mocap front end + live step), alternating",
           "streams": {}}
    walk = synthetic.raw_walk_clip(LAYOUTS["mocha"]["parents"], 644, seed=9)
    wrot, wpos = torch.from_numpy(walk[0]).to(dev), torch.from_numpy(walk[1]).to(dev)
    for S in (1, 8):
        ids = torch.tensor([(k * 3) % 8 for k in range(S)], dtype=torch.int32)
        plain, rs = LiveSession(mb, mean, std, streams=S), LiveSession(mb, mean, std, streams=S, raw=a.raw)
        frame = [0]

        def push():
            f = frame[0] % 644; frame[0] += 1
            plain.rot.copy_(clip[0][f]); plain.pos.copy_(clip[1][f]); plain.vel.copy_(clip[2][f]); plain.ang.copy_(clip[3][f])
            plain.rvel.copy_(per[0][f]); plain.rang.copy_(per[1][f]); plain.speed.copy_(per[2][f]); plain.contact.copy_(per[3][f])
            rs.raw_rot.copy_(wrot[f]); rs.raw_pos.copy_(wpos[f])
        for sess in (plain, rs):
            sess.characters.copy_(ids)
        for _ in range(max(a.warmup, 100)):                                        # past both warm-ups: 60 and 90 pushes
            push(); plain.replay(); rs.replay_raw()
        torch.cuda.synchronize()
        assert bool((rs.out["valid"] == 1).all()) and bool((plain.out["valid"] == 1).all())
        ta, tb = [], []
        for _ in range(a.reps):
            push(); torch.cuda.synchronize()
            ta.append(event_ms(plain.replay, 1)[0]); tb.append(event_ms(rs.replay_raw, 1)[0])
        e = {"a_live_step": pct(np.asarray(ta)), "b_live_step_raw": pct(np.asarray(tb))}
        e["b_minus_a_p50_ms"] = e["b_live_step_raw"]["p50_ms"] - e["a_live_step"]["p50_ms"]
        n = 200                                          # the step's own launches, one at a time (eager while profiling)
        model.profile_start()
        for _ in range(n):
            rs.replay_raw()
        prof = model.profile_stop()
        e["sites_us"] = {k: 1e3 * v["ms"] / v["launches"] for k, v in prof["sites"].items() if k.split("|")[0] in ADDED + ("live.ingest",)}
        assert bool(torch.isfinite(rs.out["pos"]).all())
        res["streams"][str(S)] = e
        del plain, rs
    return res


def world(a, dev, model, mb, mean, std, clip, per, J):
    """--world: the plain live step and the one with world= (one more launch, mocha_world_pose, BEHIND the captured graph on the same
    stream: global poses and the skinning palette), alternating in one process."""
    from mocha_sigasia2023_amd import LiveSession, SkinBind
    res = {"bank": "8 characters x 2048 rows, fp32, segmented", "layout": "mocha (24 joints)",
           "timing": "HIP events around single pushes' device work; (a) live step = one graph replay, (b) live step with world=SkinBind = the "
                     "replay and one mocha_world_pose launch behind it, alternating", "streams": {}}
    rng = np.random.Generator(np.random.PCG64(22))
    bind = SkinBind(model, rng.uniform(-0.3, 0.3, (J, 3)), rng.standard_normal((J, 4)), [[100.0, 0, 0, 0], [0, 0, 100.0, 0], [0, 100.0, 0, 0]])
    for S in (1, 8, 16):
        ids = torch.tensor([(k * 3) % 8 for k in range(S)], dtype=torch.int32)
        plain, wd = LiveSession(mb, mean, std, streams=S), LiveSession(mb, mean, std, streams=S, world=bind)
        frame = [0]

        def push():
            f = frame[0] % 644; frame[0] += 1
            for sess in (plain, wd):
                sess.rot.copy_(clip[0][f]); sess.pos.copy_(clip[1][f]); sess.vel.copy_(clip[2][f]); sess.ang.copy_(clip[3][f])
                sess.rvel.copy_(per[0][f]); sess.rang.copy_(per[1][f]); sess.speed.copy_(per[2][f]); sess.contact.copy_(per[3][f])
        for sess in (plain, wd):
            sess.characters.copy_(ids)
        for _ in range(max(a.warmup, 70)):
            push(); plain.replay(); wd.replay()
        torch.cuda.synchronize()
        assert bool((wd.out["valid"] == 1).all()) and all(torch.equal(wd.out[k], plain.out[k]) for k in plain.out)
        ta, tb = [], []
        for _ in range(a.reps):
            push(); torch.cuda.synchronize()
            ta.append(event_ms(plain.replay, 1)[0]); tb.append(event_ms(wd.replay, 1)[0])
        e = {"a_live_step": pct(np.asarray(ta)), "b_live_step_world": pct(np.asarray(tb))}
        e["b_minus_a_p50_ms"] = e["b_live_step_world"]["p50_ms"] - e["a_live_step"]["p50_ms"]
        n = 200                                          # the added launch on its own (eager while profiling)
        model.profile_start()
        for _ in range(n):
            wd.replay()
        prof = model.profile_stop()
        e["sites_us"] = {k: 1e3 * v["ms"] / v["launches"] for k, v in prof["sites"].items() if k.split("|")[0] == "world.pose"}
        assert bool(torch.isfinite(wd.out["palette"]).all()) and bool(torch.isfinite(wd.out["gpos"]).all())
        res["streams"][str(S)] = e
        del plain, wd
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=1000)
    ap.add_argument("--warmup", type=int, default=100)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r08", "live_step.json"))
    ap.add_argument("--baseline-only", action="store_true")
    ap.add_argument("--ours", action="store_true", help="the CVAE branch: live step / live step with the branch / the route without the live step")
    ap.add_argument("--grouped", action="store_true", help="with --ours: the single-CVAE step / the grouped step on one slot / on S distinct slots")
    ap.add_argument("--soft", type=int, default=0, metavar="K", help="soft matching: live step / soft live step with K neighbours, temperature 2")
    ap.add_argument("--inertial", type=float, default=None, metavar="H", help="inertialized switches: live step / live step with half-life H seconds")
    ap.add_argument("--raw", type=int, default=None, metavar="L", help="raw mocap input: live step / raw live step with L frames of lookahead")
    ap.add_argument("--constrained", action="store_true", help="action-constrained matching: live step / constrained live step with zero masks / one action of 16")
    ap.add_argument("--mix", default=None, metavar="J[,J..]", help="character mixing: live step / soft live step at k = J / mix live step with J components, S = 1, 8, 16")
    ap.add_argument("--world", action="store_true", help="world-space poses: live step / live step with world=SkinBind (one mocha_world_pose launch behind the graph), S = 1, 8, 16")
    ap.add_argument("--coherent", type=float, default=None, metavar="L", help="coherent matching: live step / soft live step at k = 1 / coherent live step with jump penalty L, S = 1, 8, 16")
    a = ap.parse_args()
    if a.coherent is not None and a.out == ap.get_default("out"):
        a.out = os.path.join(ROOT, "profiles", "r24", "live_path_step.json")
    if a.world and a.out == ap.get_default("out"):
        a.out = os.path.join(ROOT, "profiles", "r22", "live_world_step.json")
    if a.mix is not None:
        a.mix = [int(x) for x in a.mix.split(",")]
        if not a.mix or any(not 1 <= j <= 4 for j in a.mix):
            raise SystemExit("--mix takes component counts in 1 .. 4, comma-separated")
        if a.out == ap.get_default("out"):
            a.out = os.path.join(ROOT, "profiles", "r20", "live_mix_step.json")
    if a.constrained and a.out == ap.get_default("out"):
        a.out = os.path.join(ROOT, "profiles", "r15", "live_allow_step.json")
    if a.raw is not None and a.out == ap.get_default("out"):
        a.out = os.path.join(ROOT, "profiles", "r13", "live_raw_step.json")
    if a.inertial is not None and a.out == ap.get_default("out"):
        a.out = os.path.join(ROOT, "profiles", "r12", "live_inert_step.json")
    if a.soft and a.out == ap.get_default("out"):
        a.out = os.path.join(ROOT, "profiles", "r10", "live_soft_step.json")
    if a.grouped and not a.ours:
        raise SystemExit("--grouped goes with --ours")
    if a.ours and a.grouped and a.out == ap.get_default("out"):
        a.out = os.path.join(ROOT, "profiles", "r19", "live_ours_grouped_step.json")
    if a.ours and a.out == ap.get_default("out"):
        a.out = os.path.join(ROOT, "profiles", "r09", "live_ours_step.json")
    if not torch.cuda.is_available():
        raise SystemExit("live_latency.py measures on the GPU: no ROCm device found")
    dev = torch.device("cuda:0")
    J = 25
    model = Generator(device=dev).load_state_dict(synthetic_state_dict(1777, 1.0)).eval()
    rng = np.random.Generator(np.random.PCG64(0))
    model.set_pose_norm((0.05 * rng.standard_normal((J, 15))).astype(np.float32), rng.uniform(0.5, 1.5, (J, 15)).astype(np.float32),
                        (0.05 * rng.standard_normal((J, 15))).astype(np.float32), rng.uniform(0.2, 0.6, (J, 15)).astype(np.float32))
    g = torch.Generator(device=dev); g.manual_seed(3)
    nm = torch.randn((8 * 2048, D), device=dev, generator=g)
    enc = torch.randn((8 * 2048, 90, 256), device=dev, generator=g)
    mb = MultiCharacterBank(model, [(nm[c * 2048:(c + 1) * 2048], enc[c * 2048:(c + 1) * 2048]) for c in range(8)])
    m_, s_ = synthetic.cnt_norm(7)
    mean, std = torch.from_numpy(m_).to(dev), torch.from_numpy(s_).to(dev)
    clip = [torch.from_numpy(x).to(dev) for x in synthetic.smooth_bone_clip(21, 644, J)]
    _, rvel, rang, hipvel, contact = synthetic.postprocess_inputs(5, 644)
    per = [torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in (rvel, rang, np.linalg.norm(hipvel, axis=-1).mean(-1).astype(np.float32), contact)]
    res = {"bank": "8 characters x 2048 rows, fp32, segmented", "layout": "mocha (24 joints)", "timing": "HIP events around single graph replays, live and baseline alternating",
           "streams": {}}
    if a.coherent is not None:
        return write_out(a, coherent(a, dev, model, mb, mean, std, clip, per, J))
    if a.world:
        return write_out(a, world(a, dev, model, mb, mean, std, clip, per, J))
    if a.mix is not None:
        return write_out(a, mix(a, dev, model, mb, mean, std, clip, per, J))
    if a.constrained:
        return write_out(a, constrained(a, dev, model, mb, mean, std, clip, per, J))
    if a.raw is not None:
        return write_out(a, raw(a, dev, model, mb, mean, std, clip, per, J))
    if a.inertial is not None:
        return write_out(a, inertial(a, dev, model, mb, mean, std, clip, per, J))
    if a.soft:
        return write_out(a, soft(a, dev, model, mb, mean, std, clip, per, J))
    if a.ours and a.grouped:
        return write_out(a, ours_grouped(a, dev, model, mb, mean, std, clip, per, J))
    if a.ours:
        return write_out(a, ours(a, dev, model, mb, mean, std, clip, per, J))
    for S in (1, 8):
        ids = [(k * 3) % 8 for k in range(S)]
        mb.characterize(torch.zeros((S, 60, J, 15), device=dev), ids, mean, std, raw=True)      # eager first: everything made on first use exists
        ms = MultiStreamCharacterizer(mb, mean, std, streams=S, raw=True)
        ms.characters.copy_(torch.tensor(ids, dtype=torch.int32))
        ms.input.copy_(model.featurize(*[x[:60][None].expand(S, -1, -1, -1).contiguous() for x in clip]))
        base = lambda: ms.step()                                                   # noqa: E731
        entry = {}
        if a.baseline_only:
            event_ms(base, a.warmup)
            entry["segmented_step"] = pct(event_ms(base, a.reps))
        else:
            from mocha_sigasia2023_amd import LiveSession
            sess = LiveSession(mb, mean, std, streams=S)
            frame = [0]

            def push():
                f = frame[0] % 644; frame[0] += 1
                sess.rot.copy_(clip[0][f]); sess.pos.copy_(clip[1][f]); sess.vel.copy_(clip[2][f]); sess.ang.copy_(clip[3][f])
                sess.rvel.copy_(per[0][f]); sess.rang.copy_(per[1][f]); sess.speed.copy_(per[2][f]); sess.contact.copy_(per[3][f])
            sess.characters.copy_(torch.tensor(ids, dtype=torch.int32))
            for _ in range(max(a.warmup, 70)):                                     # past the ring's warm-up: every stream is running
                push(); sess.replay(); base()
            torch.cuda.synchronize()
            assert bool((sess.out["valid"] == 1).all())
            live_t, base_t = [], []
            for _ in range(a.reps):                                                # alternating, inputs staged outside the timed region
                push(); torch.cuda.synchronize()
                live_t.append(event_ms(sess.replay, 1)[0])
                base_t.append(event_ms(base, 1)[0])
            entry["live_step"], entry["segmented_step"] = pct(np.asarray(live_t)), pct(np.asarray(base_t))
            entry["live_minus_segmented_p50_ms"] = entry["live_step"]["p50_ms"] - entry["segmented_step"]["p50_ms"]
            # the added kernels, one launch at a time (the step runs eagerly while profiling is on)
            n = 200
            model.profile_start()
            for _ in range(n):
                sess.replay()
            prof = model.profile_stop()
            entry["added_kernels_us"] = {k: 1e3 * v["ms"] / v["launches"] for k, v in prof["sites"].items() if k.split("|")[0] in ADDED}
            entry["added_kernels_sum_us"] = float(sum(entry["added_kernels_us"].values()))
            entry["eager_step_launches"] = int(sum(v["launches"] for v in prof["kernels"].values()) // n)
            assert bool(torch.isfinite(sess.out["pos"]).all())
            del sess
        res["streams"][str(S)] = entry
        del ms
    write_out(a, res)


def write_out(a, res):
    print(json.dumps(res, indent=1))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
