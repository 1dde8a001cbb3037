"""What a resident bank costs and saves, on the shape of DESIGN.md 8.9: 8 characters x 2 048 rows at D = 23 040, fp32, a LiveSession of 16
streams (stream s on character s % 8).  Three measurements, none of them a threshold (DESIGN.md 8.17 says what is expected and records
what was measured):

 1. the stream time (HIP events) and the host time of one ResidentCharacterBank.add of 2 048 rows, and of retire - the eighth character
    leaving and coming back, alternating;
 2. the route it replaces, in the same tree: a MultiCharacterBank rebuilt from seven to eight characters (torch.cat, mocha_bank_set_segments,
    labels) plus the first live step after it, with its re-capture - host time from before the rebuild to the step's completion;
 3. the live step's p50 on the resident bank against the same content as a plain segmented bank, alternating in one process, with
    max_rows_per_character at 2 048 and at 16 384: the scan grid is sized by that maximum, not by the largest character, so the second
    figure is the cost of the idle workgroups.

    python tools/resident_bank_bench.py [--reps 200] [--out profiles/r17/resident_bank.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from mocha_sigasia2023_amd import (Generator, LiveSession, MultiCharacterBank, PostProcessor, ResidentCharacterBank, synthetic,  # noqa: E402
                                   synthetic_state_dict)

D = 90 * 256
CHARS, ROWS, STREAMS, J = 8, 2048, 16, 25


def stats(a):
    a = np.asarray(a, np.float64)
    return {"p50_us": float(np.percentile(a, 50)), "p10_us": float(np.percentile(a, 10)), "p90_us": float(np.percentile(a, 90)), "n": int(len(a))}


def timed(fn):
    """(stream time, host time until the stream has finished) of one call, in microseconds."""
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    e0.record(); fn(); e1.record()
    e1.synchronize()
    return 1e3 * e0.elapsed_time(e1), 1e6 * (time.perf_counter() - t0)


def make_model(dev):
    model = Generator(device=dev).load_state_dict(synthetic_state_dict(1777, 1.0)).eval()
    rng = np.random.Generator(np.random.PCG64(0))
    model.set_pose_norm((0.05 * rng.standard_normal((J, 15))).astype(np.float32), rng.uniform(0.5, 1.5, (J, 15)).astype(np.float32),
                        (0.05 * rng.standard_normal((J, 15))).astype(np.float32), rng.uniform(0.2, 0.6, (J, 15)).astype(np.float32))
    return model


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--rebuilds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r17", "resident_bank.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("resident_bank_bench.py measures on the GPU: no ROCm device found")
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev); g.manual_seed(3)
    nm = torch.randn((CHARS * ROWS, D), device=dev, generator=g)
    banks = [(nm[c * ROWS:(c + 1) * ROWS], nm[c * ROWS:(c + 1) * ROWS].view(-1, 90, 256)) for c in range(CHARS)]
    labels = [(np.arange(ROWS) // 128).astype(np.int32)] * CHARS
    mean, std = (torch.from_numpy(x).to(dev) for x in synthetic.cnt_norm(7))
    clip = [torch.from_numpy(x).to(dev) for x in synthetic.smooth_bone_clip(30, 64)]
    _, rvel, rang, hipvel, contact = synthetic.postprocess_inputs(5, 64)
    per = [torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in (rvel, rang, np.linalg.norm(hipvel, axis=-1).mean(-1).astype(np.float32), contact)]
    ids = [s % CHARS for s in range(STREAMS)]

    def rep(x):                                               # every stream pushes the same frame
        return x.expand(STREAMS, *x.shape).contiguous()

    def session(bank):
        sess = LiveSession(bank, mean, std, streams=STREAMS, post=PostProcessor(bank.model), bvh=False)
        for f in range(62):                                   # the rings fill; from push 60 on every stream is valid
            o = sess.push(*[rep(x[f]) for x in clip], *[rep(x[f]) for x in per], characters=ids if f == 0 else None)
        torch.cuda.synchronize()
        assert o["valid"].tolist() == [1] * STREAMS
        return sess

    res = {"shape": f"{CHARS} characters x {ROWS} rows, D = {D}, fp32, {STREAMS} live streams",
           "timing": "stream: HIP events around one call; host: perf_counter from before the call until the stream has finished"}

    # ---- 3 (and 1): the live step on a resident bank against the plain segmented bank of the same content
    plain_model = make_model(dev)
    plain_bank = MultiCharacterBank(plain_model, banks, labels=labels)
    res["live_step"] = []
    for max_rows in (ROWS, 16384):
        plain = session(plain_bank)                           # a fresh session each time: both sides have seen the same 62 pushes
        model = make_model(dev)
        rb = ResidentCharacterBank(model, max(CHARS * ROWS, max_rows), CHARS, max_rows)
        for c in range(CHARS):
            rb.add(*banks[c], labels=labels[c])
        sess = session(rb)
        same = all(torch.equal(sess.out[k], plain.out[k]) for k in ("pos", "rot", "ik_rot", "idx"))
        tr, tp = [], []
        for _ in range(a.reps):
            tr.append(timed(sess.replay)[0]); tp.append(timed(plain.replay)[0])
        e = {"max_rows_per_character": max_rows, "resident": stats(tr), "plain": stats(tp),
             "resident_over_plain_p50": float(np.percentile(tr, 50) / np.percentile(tp, 50)), "outputs_equal_plain": bool(same)}
        res["live_step"].append(e); print(json.dumps(e))
        if max_rows == ROWS:
            # ---- 1: the eighth character leaves and comes back; the captured step replays in between
            gen = model._ctx.generation()
            add, ret, step = [], [], []
            for _ in range(max(a.reps // 4, 10)):
                ret.append(timed(lambda: rb.retire(CHARS - 1)))
                step.append(timed(sess.replay)[0])
                add.append(timed(lambda: rb.add(*banks[CHARS - 1], labels=labels[CHARS - 1], slot=CHARS - 1)))
                step.append(timed(sess.replay)[0])
            assert model._ctx.generation() == gen
            res["add_2048_rows"] = {"stream": stats([x[0] for x in add]), "host": stats([x[1] for x in add]),
                                    "bytes_copied": 2 * ROWS * D * 4, "bytes_written_decoder_constants": ROWS * (D + 512 * model.cfg["decoder_depth"]) * 4}
            res["retire"] = {"stream": stats([x[0] for x in ret]), "host": stats([x[1] for x in ret])}
            res["live_step_between_add_and_retire"] = stats(step)
            res["generation_moved_by_add_retire"] = False
            print(json.dumps({k: res[k] for k in ("add_2048_rows", "retire", "live_step_between_add_and_retire")}))
        del sess, rb, model

    # ---- 2: the route it replaces: rebuild the union with one more character, then the first live step (re-capture included)
    seven = MultiCharacterBank(plain_model, banks[:7], labels=labels[:7])
    plain.bank = seven
    plain.characters.copy_(torch.tensor([s % 7 for s in range(STREAMS)], dtype=torch.int32))
    plain.replay(); torch.cuda.synchronize()
    rebuild = []
    for _ in range(a.rebuilds):
        def route():
            plain.bank = MultiCharacterBank(plain_model, banks, labels=labels)
            plain.replay()
        rebuild.append(timed(route))
        plain.bank = seven; plain.replay(); torch.cuda.synchronize()
    res["rebuild_and_first_step"] = {"stream": stats([x[0] for x in rebuild]), "host": stats([x[1] for x in rebuild])}
    print(json.dumps({"rebuild_and_first_step": res["rebuild_and_first_step"]}))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
