#!/usr/bin/env python3
"""What the host layer's segmented and live entry points launch: for each of them ONE profiled call (mocha_profile_start / stop, during
which the steps run eagerly) at the smallest meaningful shape, written as {entry: {"site|kernel": [launches, flops, bytes]}} with the
timing fields dropped.  Launch counts and the host-computed flops / bytes are integers and host arithmetic, not measurements: two builds
of the host layer that enqueue the same work give the same file, so a refactor of mocha_api.cpp is checked by running this before and
after and comparing the two files key for key.

Shape: a bank of 3 characters with 40, 17 and 33 rows (labelled), once fp32 and once bf16; B = S_w = streams = 2.  In the live calls
stream 0 has a full ring and stream 1 is still warming (it was reset a few frames before the profiled step).

    python tools/launch_ledger.py --out profiles/r21/ledger_branch.json
    python tools/launch_ledger.py --compare profiles/r21/ledger_parent.json profiles/r21/ledger_branch.json
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

D = 90 * 256
ROWS = (40, 17, 33)
S = 2


def compare(a_path, b_path):
    with open(a_path) as f:
        a = json.load(f)
    with open(b_path) as f:
        b = json.load(f)
    bad = 0
    for entry in sorted(set(a) | set(b)):
        ea, eb = a.get(entry), b.get(entry)
        if ea is None or eb is None:
            print(f"{entry}: only in {'the first' if eb is None else 'the second'} file"); bad += 1
            continue
        for key in sorted(set(ea) | set(eb)):
            if ea.get(key) != eb.get(key):
                print(f"{entry}: {key}: {ea.get(key)} != {eb.get(key)}"); bad += 1
    print(f"{len(a)} / {len(b)} entries, {bad} difference(s)")
    return 1 if bad else 0


def ledger(model, call):
    """One profiled call -> {site|kernel: [launches, flops, bytes]}."""
    model.profile_start()
    try:
        call()
    finally:
        prof = model.profile_stop()
    return {k: [int(v["launches"]), float(v["flops"]), float(v["bytes"])] for k, v in sorted(prof["sites"].items())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--compare", nargs=2, metavar=("A", "B"), help="compare two ledgers (no GPU needed); exit status 1 when they differ")
    a = ap.parse_args()
    if a.compare:
        raise SystemExit(compare(*a.compare))
    if not torch.cuda.is_available():
        raise SystemExit("launch_ledger.py profiles on the GPU: no ROCm device found")
    from mocha_sigasia2023_amd import (CVAEBank, Generator, LiveOursSession, LiveSession, MultiCharacterBank, synthetic,
                                       synthetic_state_dict)
    from mocha_sigasia2023_amd.skeleton import LAYOUTS
    from mocha_sigasia2023_amd.weights import synthetic_cvae_state_dict
    dev = torch.device("cuda:0")
    J = 25
    model = Generator(device=dev).load_state_dict(synthetic_state_dict(1777, 1.0)).eval()
    rng = np.random.Generator(np.random.PCG64(0))
    model.set_pose_norm((0.05 * rng.standard_normal((J, 15))).astype(np.float32), rng.uniform(0.5, 1.5, (J, 15)).astype(np.float32),
                        (0.05 * rng.standard_normal((J, 15))).astype(np.float32), rng.uniform(0.2, 0.6, (J, 15)).astype(np.float32))
    g = torch.Generator(device=dev); g.manual_seed(3)
    N = sum(ROWS)
    nm = torch.randn((N, D), device=dev, generator=g)
    enc = torch.randn((N, 90, 256), device=dev, generator=g)
    m_, s_ = synthetic.cnt_norm(7)
    mean, std = torch.from_numpy(m_).to(dev), torch.from_numpy(s_).to(dev)
    F = 100
    clip = [torch.from_numpy(x).to(dev) for x in synthetic.smooth_bone_clip(21, F, J)]
    _, rvel, rang, hipvel, contact = synthetic.postprocess_inputs(5, F)
    per = [torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in (rvel, rang, np.linalg.norm(hipvel, axis=-1).mean(-1).astype(np.float32), contact)]
    walk = synthetic.raw_walk_clip(LAYOUTS["mocha"]["parents"], F, seed=9)
    wrot, wpos = torch.from_numpy(walk[0]).to(dev), torch.from_numpy(walk[1]).to(dev)
    X = model.featurize(*[x[:60][None].expand(S, -1, -1, -1).contiguous() for x in clip])
    ids = torch.tensor([2, 1], dtype=torch.int32)
    mix = (np.array([[2, 0], [1, 2]], np.int32), np.array([[1.0, 2.0]] * S, np.float32))
    allow = [1 << 1, 0]
    stats = [(0.1 * rng.standard_normal((90, 256))).astype(np.float32), rng.uniform(0.5, 1.5, (90, 256)).astype(np.float32),
             (0.1 * rng.standard_normal((90, 256))).astype(np.float32), rng.uniform(0.5, 1.5, (90, 256)).astype(np.float32)]
    cvaes = CVAEBank(model, 2)
    for slot in range(2):
        cvaes.store(slot, synthetic_cvae_state_dict(99 + slot, 1.0), *stats)
    model.load_cvae(synthetic_cvae_state_dict(99, 1.0))

    res = {}
    for bf16 in (False, True):
        tag = "bf16" if bf16 else "fp32"
        at, banks = 0, []
        for n in ROWS:
            banks.append((nm[at:at + n], enc[at:at + n])); at += n
        mb = MultiCharacterBank(model, banks, bf16=bf16, labels=[(np.arange(n) % 3).astype(np.int32) for n in ROWS])

        def seg(name, **kw):
            chars = None if "mix" in kw else ids
            mb.characterize(X, chars, mean, std, raw=True, **kw)           # eager first: everything made on first use exists
            res[f"{tag}.{name}"] = ledger(model, lambda: mb.characterize(X, chars, mean, std, raw=True, **kw))
        seg("characterize_segmented")
        seg("characterize_soft_segmented.k3", soft=(3, 2.0))
        seg("characterize_mix_segmented.J2", mix=mix)
        seg("characterize_segmented_allow.k0", allow=allow)
        seg("characterize_segmented_allow.k3", allow=allow, soft=(3, 2.0))

        def live(name, sess, raw_in=False, warm=60):
            """`warm` graph replays fill both rings; stream 1 then starts over and is three frames in when the profiled step runs."""
            def push(f):
                if raw_in:
                    sess.raw_rot.copy_(wrot[f]); sess.raw_pos.copy_(wpos[f])
                    return sess.replay_raw()
                sess.rot.copy_(clip[0][f]); sess.pos.copy_(clip[1][f]); sess.vel.copy_(clip[2][f]); sess.ang.copy_(clip[3][f])
                sess.rvel.copy_(per[0][f]); sess.rang.copy_(per[1][f]); sess.speed.copy_(per[2][f]); sess.contact.copy_(per[3][f])
                return sess.replay()
            if sess.mix is not None:
                sess.set_mix(mix)
            else:
                sess.characters.copy_(ids)
            if sess.constrained:
                sess.set_allow(allow)
            for f in range(warm):
                push(f)
            sess.reset([1])
            for f in range(warm, warm + 3):
                push(f)
            torch.cuda.synchronize()
            assert sess.out["valid"].tolist() == [1, 0], (name, sess.out["valid"].tolist())
            res[f"{tag}.{name}"] = ledger(model, lambda: push(warm + 3))
            torch.cuda.synchronize()
            assert sess.out["valid"].tolist() == [1, 0] and bool(torch.isfinite(sess.out["pos"][0]).all()), name
        live("live_step", LiveSession(mb, mean, std, streams=S))
        live("live_step_soft.k3", LiveSession(mb, mean, std, streams=S, soft=(3, 2.0)))
        live("live_step_inert", LiveSession(mb, mean, std, streams=S, inertial=0.1))
        live("live_step_allow", LiveSession(mb, mean, std, streams=S, constrained=True))
        live("live_step_raw", LiveSession(mb, mean, std, streams=S, raw=2), raw_in=True, warm=96)
        live("live_step_raw_allow", LiveSession(mb, mean, std, streams=S, raw=2, constrained=True), raw_in=True, warm=96)
        live("live_step_mix.J2", LiveSession(mb, mean, std, streams=S, mix=2))
        live("live_step_raw_mix.J2", LiveSession(mb, mean, std, streams=S, raw=2, mix=2), raw_in=True, warm=96)
        live("live_step_ours", LiveOursSession(mb, mean, std, None, *stats, streams=S, noise="device", seed=11))
        live("live_step_ours_grouped", LiveOursSession(mb, mean, std, None, None, None, None, None, streams=S, noise="device", seed=11, cvaes=cvaes,
                                                       cvae_of=torch.tensor([0, 1, 0], dtype=torch.int32)))
        del mb
    print(json.dumps({k: sum(v[0] for v in e.values()) for k, e in res.items()}, indent=1))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:                     # one line per site|kernel
            f.write("{\n" + ",\n".join(" %s: {\n%s\n }" % (json.dumps(k), ",\n".join("  %s: %s" % (json.dumps(s), json.dumps(v)) for s, v in sorted(e.items())))
                                       for k, e in sorted(res.items())) + "\n}\n")


if __name__ == "__main__":
    main()
