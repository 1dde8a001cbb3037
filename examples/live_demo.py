#!/usr/bin/env python3
"""The synthetic demo of examples/demo_pair.py driven frame by frame: two live streams, each against its own character, pushed one
mocap frame at a time through ``LiveSession`` - ring push + featurize, segmented characterize, pose heads and one post-processing
frame per push, one captured graph - and written as two BVH files.

    python examples/live_demo.py [--frames 180] [--out bench_outputs/live_demo] [--ours [--seed 7]] [--switch 120 [--inertial 0.1]] [--raw L [--source-fps R]] [--coherent L]
                                 [--actions A,B[:F]] [--load-at F] [--ours-per-character] [--mix a:b:FRAMES | --mix-parts a:b:MASK]

``--ours`` runs the CVAE ("Ours") branch inside the same graph (``LiveOursSession``): each stream's character feature is seeded with
its matched bank row on the first pose and sampled from the previous one afterwards, the noise drawn on the device; the files are then
named ``Ours_stream<s>.bvh`` as the reference names its result ``Ours.bvh``.

``--ours-per-character`` (implies ``--ours``): ONE CVAE PER CHARACTER from a resident ``CVAEBank`` (synthetic CVAEs 99, 100 with their own
statistics): stream s is sampled with the CVAE of its character, chosen inside the captured graph (``LiveOursSession(cvaes=, cvae_of=)``).
With ``--load-at F`` the new character arrives without a CVAE - it falls back to plain context matching - until, ten frames later, its
CVAE is stored and ``set_cvae`` names it: no new capture.

``--switch FRAME``: stream 0 names character 1 from that frame on - the new id is device data, the graph is not captured again.
``--inertial HALFLIFE`` (seconds): the switch does not pop; the jump of the pose heads decays as an offset (``LiveSession(inertial=...)``,
the reference's per-bone inertializers on the device).  The size of the largest bone-position step at the switch frame is printed.

``--raw L``: the streams push RAW mocap frames - local Euler rotations in degrees and local positions in centimetres of the 24 joints, as
a BVH file holds them (a synthetic walk) - and the mocap front end inside the same graph makes the root bone, the velocities and the foot
contacts (``LiveSession(raw=L)``, ``push_raw``), L = 0..18 frames of lookahead.  The first pose then comes with push 90.
``--source-fps R`` (with ``--raw``): the producer runs at R frames per second (90, 100, 120, 30 ...) while the model, its window and the
root fits stay at 60.  A ``StreamResampler`` in front of a quaternion-input session takes one source frame per push and hands over the 0..4
frames at 60 fps that it completes - one launch in front of the captured step, not inside it; ``--frames`` still counts pushes at 60 fps.

``--actions A,B[:F]``: the bank's entries carry action labels in runs of 25 (a synthetic stand-in for ``load_bank(path)["action_label"]``:
200 entries, actions 0 .. 7) and, from frame F on (default: from the start), every stream is matched among its character's entries of the
listed actions only (``LiveSession(constrained=True)``, ``push(..., allow=)``).  The new masks are device data: nothing is captured again.
How many posed frames were constrained is printed.

``--load-at F``: the run starts on a ``ResidentCharacterBank`` that holds the two characters; at frame F a third character is added to it
in place - its own rows and decoder constants, enqueued on the stream - and stream 1 switches to it.  The captured step keeps replaying:
the model's generation before and after is printed.

``--world``: every push also returns the pose in world space and the fp32 skinning palette (``LiveSession(world=SkinBind(...))``, one more
launch behind the captured step); prints the palette's shape and one bone's world position per frame.

``--mix a:b:FRAMES``: both streams are characterized by a MIX of characters a and b (``LiveSession(mix=2)``): a linear cross-fade from a
to b over FRAMES frames, starting with the first posed frame - a weight ramp written into the session's device weights, in feature
space; nothing is captured again.  ``--mix-parts a:b:MASK``: a splice by body part - MASK is six 0/1 characters, one per body part in the
order of ``PART_NAMES`` (Spine, LeftLeg, LeftArm, Neck, RightArm, RightLeg for this layout): 1 takes the part from a, 0 from b.  Neither
combines with ``--soft``, ``--inertial``, ``--actions``, ``--switch`` or ``--ours``.

``--coherent L``: coherent matching (``LiveSession(coherent=L)``): a stream keeps to the run of consecutive bank rows it is on unless
leaving it is cheaper by more than L, in the matcher's distance units (the bank here is stride-1 windows of one clip per character).  The
number of continued frames and of transitions that are not "next row" is printed.  Combines with ``--raw``, ``--switch``, ``--load-at``
and ``--world``.

Weights, norms and motions are synthetic (see demo_pair.py for what to replace with real assets).
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mocha_sigasia2023_amd import (Generator, IngestConfig, LiveOursSession, LiveSession, MultiCharacterBank, PostProcessor,  # noqa: E402
                                   ResidentCharacterBank, StreamResampler, build_bank, resample_clips, synthetic, synthetic_state_dict, write_bvh)
from mocha_sigasia2023_amd.ingest import resample_ratio  # noqa: E402
from mocha_sigasia2023_amd.skeleton import LAYOUTS  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--frames", type=int, default=180, help="mocap frames pushed per stream (the first 59 fill the window)")
ap.add_argument("--out", default="bench_outputs/live_demo")
ap.add_argument("--ours", action="store_true", help="the CVAE branch inside the live step (synthetic CVAE weights and statistics)")
ap.add_argument("--seed", type=int, default=7, help="--ours: seed of the device's noise")
ap.add_argument("--soft", nargs=2, metavar=("K", "T"), help="soft matching: the decoder reads the softmax(-dist / T) blend of each stream's K nearest "
                "entries (1..8) instead of the nearest one")
ap.add_argument("--switch", type=int, default=None, metavar="FRAME", help="stream 0 takes character 1 from that frame on")
ap.add_argument("--inertial", type=float, default=None, metavar="HALFLIFE", help="inertialize character switches with that half-life in seconds")
ap.add_argument("--raw", type=int, default=None, metavar="L", help="push raw mocap frames; the front end runs in the graph with L frames of lookahead")
ap.add_argument("--source-fps", type=float, default=None, metavar="R", help="with --raw: the mocap producer runs at R frames per second; a "
                "StreamResampler in front of the session brings its frames to the model's 60")
ap.add_argument("--actions", default=None, metavar="A,B[:F]", help="allow only these action labels (0..7 here), from frame F on")
ap.add_argument("--load-at", type=int, default=None, metavar="FRAME", help="start on a resident bank; at that frame a third character is added in "
                "place and stream 1 switches to it")
ap.add_argument("--ours-per-character", action="store_true", help="--ours with one CVAE per character from a CVAEBank (synthetic CVAEs)")
ap.add_argument("--mix", default=None, metavar="a:b:FRAMES", help="cross-fade both streams from character a to b over FRAMES frames")
ap.add_argument("--mix-parts", default=None, metavar="a:b:MASK", help="splice: body parts with 1 in the six-character MASK from a, the others from b")
ap.add_argument("--coherent", type=float, default=None, metavar="L", help="coherent matching: every transition that is not 'next row of the same clip' "
                "costs L (in the matcher's distance units); LiveSession(coherent=L)")
ap.add_argument("--world", action="store_true", help="also produce world-space poses and the skinning palette (LiveSession(world=SkinBind))")
a = ap.parse_args()
a.ours = a.ours or a.ours_per_character
mix_ids = mix_ramp = mix_mask = None
if a.mix or a.mix_parts:
    if a.mix and a.mix_parts:
        raise SystemExit("--mix and --mix-parts are two forms of one thing: give one")
    if a.ours or a.soft or a.inertial is not None or a.actions or a.switch is not None:
        raise SystemExit("--mix / --mix-parts do not combine with --ours, --soft, --inertial, --actions or --switch: mix is hard matching per "
                         "component, and its weights are what changes a stream's character")
    ca, cb, last = (a.mix or a.mix_parts).split(":")
    mix_ids = [int(ca), int(cb)]
    if a.mix:
        mix_ramp = int(last)
        if mix_ramp < 1:
            raise SystemExit("--mix a:b:FRAMES: FRAMES must be at least 1")
    else:
        if len(last) != 6 or set(last) - {"0", "1"}:
            raise SystemExit("--mix-parts a:b:MASK: MASK is six 0/1 characters, one per body part")
        mix_mask = np.array([float(ch) for ch in last], np.float32)
if a.coherent is not None and (a.ours or a.soft or a.inertial is not None or a.actions or a.mix or a.mix_parts):
    raise SystemExit("--coherent does not combine with --ours, --soft, --inertial, --actions or --mix: it takes the hard matcher's place, alone")
if a.ours and a.actions:
    raise SystemExit("--actions does not apply to --ours: the branch's seed match searches the whole character")
allow_from, allow_mask = 0, None
if a.actions:
    from mocha_sigasia2023_amd import action_mask
    spec, _, at = a.actions.partition(":")
    allow_mask, allow_from = action_mask([int(v) for v in spec.split(",")]), int(at) if at else 0
if a.ours and a.raw is not None:
    raise SystemExit("--raw does not apply to --ours: the CVAE session has no mocap front end")
if a.source_fps is not None and a.raw is None:
    raise SystemExit("--source-fps needs --raw: it is the raw mocap producer that runs at another rate")
if a.ours and a.inertial is not None:
    raise SystemExit("--inertial does not apply to --ours: that branch seeds again on a switch and keeps its own chain state")
if a.ours and a.soft:
    raise SystemExit("--soft does not apply to --ours: its decoder already reads a sampled character feature")
soft = (int(a.soft[0]), float(a.soft[1])) if a.soft else None
first = 59 if a.raw is None else 89                                   # index of the push that brings the first pose
if a.frames <= first:
    raise SystemExit(f"--frames must be at least {first + 1}: a stream's first pose comes with that push")
os.makedirs(a.out, exist_ok=True)
dev = torch.device("cuda:0")
F, J, C, S = a.frames, 25, 15, 2

# ---- model and (synthetic) statistics                                                        test_fullframework.py:40-98
model = Generator(device=dev).load_state_dict(synthetic_state_dict(1777, 1.0)).eval()
rng = np.random.Generator(np.random.PCG64(0))
X_mean = (0.05 * rng.standard_normal((J, C))).astype(np.float32); X_std = rng.uniform(0.5, 1.5, (J, C)).astype(np.float32)
Y_mean = (0.05 * rng.standard_normal((J, C))).astype(np.float32); Y_std = rng.uniform(0.2, 0.6, (J, C)).astype(np.float32)
model.set_pose_norm(X_mean, X_std, Y_mean, Y_std)
cnt_mean, cnt_std = (torch.from_numpy(x).to(dev) for x in synthetic.cnt_norm(7))

# ---- two characters' banks from two clips, one multi-character bank                          :203-222, 271-277
banks = []
for seed in (12, 13) + ((14,) if a.load_at is not None else ()):
    clip = synthetic.smooth_bone_clip(seed, 60 + 200 - 1)
    b = build_bank(model, model.featurize(*[synthetic.slide_windows(x) for x in clip]), raw=True)
    banks.append((((b["cnt"] - cnt_mean) / cnt_std).reshape(-1, 90 * 256), b["encoded"]))
labels = [(np.arange(b[0].shape[0]) // 25).astype(np.int32) for b in banks] if a.actions else None      # actions in runs, one per clip range
if a.load_at is not None:                                             # storage for three characters reserved once; two loaded now
    bank = ResidentCharacterBank(model, capacity_rows=3 * 208, max_characters=3, max_rows_per_character=208)
    for c in range(2):
        bank.add(*banks[c], labels=labels[c] if labels else None)
else:
    bank = MultiCharacterBank(model, banks, labels=labels)

# ---- two source clips arriving frame by frame, stream s retargeted to character s
src = [[torch.from_numpy(x).to(dev) for x in synthetic.smooth_bone_clip(30 + s, F, phase=0.4 * s)] for s in range(S)]
per = []
for s in range(S):
    _, rvel, rang, hipvel, contact = synthetic.postprocess_inputs(5 + s, F)
    per.append([torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in
                (rvel, rang, np.linalg.norm(hipvel, axis=-1).mean(-1).astype(np.float32), contact)])
# --world: the mesh is bound in the first source frame's bone offsets, rotations identity; the engine works in centimetres, z up
world = None
if a.world:
    from mocha_sigasia2023_amd import SkinBind
    world = SkinBind(model, src[0][1][0].double(), None, [[100.0, 0, 0, 0], [0, 0, 100.0, 0], [0, 100.0, 0, 0]])


def cvae_stats(seed):
    r = np.random.Generator(np.random.PCG64(seed))
    return [(0.1 * r.standard_normal((90, 256))).astype(np.float32), r.uniform(0.5, 1.5, (90, 256)).astype(np.float32),
            (0.1 * r.standard_normal((90, 256))).astype(np.float32), r.uniform(0.5, 1.5, (90, 256)).astype(np.float32)]


if a.ours_per_character:                                              # train_CVAE.py: one CVAE and one cvae_norm.npz per target character
    from mocha_sigasia2023_amd import CVAEBank
    from mocha_sigasia2023_amd.weights import synthetic_cvae_state_dict
    cvaes = CVAEBank(model, 3)
    for c in range(2):
        cvaes.store(c, synthetic_cvae_state_dict(99 + c, 1.0), *cvae_stats(3 + c))
    sess = LiveOursSession(bank, cnt_mean, cnt_std, None, None, None, None, None, streams=S, post=PostProcessor(model), noise="device",
                           seed=a.seed, cvaes=cvaes, cvae_of=[0, 1, -1][:bank.S], world=world)
elif a.ours:                                                          # test_fullframework.py:52-58, 80-87: the CVAE and its statistics
    from mocha_sigasia2023_amd.weights import synthetic_cvae_state_dict
    r3 = np.random.Generator(np.random.PCG64(3))
    stats = [(0.1 * r3.standard_normal((90, 256))).astype(np.float32), r3.uniform(0.5, 1.5, (90, 256)).astype(np.float32),
             (0.1 * r3.standard_normal((90, 256))).astype(np.float32), r3.uniform(0.5, 1.5, (90, 256)).astype(np.float32)]
    sess = LiveOursSession(bank, cnt_mean, cnt_std, synthetic_cvae_state_dict(99, 1.0), *stats, streams=S, post=PostProcessor(model),
                           noise="device", seed=a.seed, world=world)
else:
    raw_cfg = a.raw if a.source_fps is None else IngestConfig(lookahead=a.raw, order=None)      # the resampler hands over quaternions
    sess = LiveSession(bank, cnt_mean, cnt_std, streams=S, post=PostProcessor(model), soft=soft, inertial=a.inertial, raw=raw_cfg,
                       constrained=bool(a.actions), mix=2 if mix_ids else None, world=world, coherent=a.coherent)
if mix_ids:
    sess.set_mix((mix_ids, np.stack([mix_mask, 1 - mix_mask]) if mix_mask is not None else [1.0, 0.0]))
if a.raw is not None:
    raw = [synthetic.raw_walk_clip(LAYOUTS["mocha"]["parents"], F, seed=40 + s) for s in range(S)]
    raw_rot = torch.from_numpy(np.stack([r[0] for r in raw])).to(dev)  # (S, F, 24, 3) degrees, 'zyx'
    raw_pos = torch.from_numpy(np.stack([r[1] for r in raw])).to(dev)  # (S, F, 24, 3) centimetres
if a.source_fps is not None:
    # The producer at R frames per second: the same walks sampled at R (whole clips, 60 -> R), then pushed one source frame at a time through
    # a StreamResampler (R -> 60) in front of the session.  Its outputs are quaternions and positions at 60 fps: F of them per stream.
    num, den = resample_ratio(a.source_fps, 60)
    n_src = -(-(F - 1) * num // den) + 1                              # source frames that give at least F outputs
    need = -(-(n_src - 1) * den // num) + 1                           # 60 fps frames that give n_src source frames
    raw = [synthetic.raw_walk_clip(LAYOUTS["mocha"]["parents"], max(need, F), seed=40 + s) for s in range(S)]
    prod_rot, prod_pos, prod_len = resample_clips(model, np.concatenate([r[0] for r in raw]), np.concatenate([r[1] for r in raw]),
                                                  [len(r[0]) for r in raw], 60, a.source_fps)
    prod_rot = prod_rot.view(S, prod_len[0], 24, 4)[:, :n_src].contiguous()
    prod_pos = prod_pos.view(S, prod_len[0], 24, 3)[:, :n_src].contiguous()
    resampler = StreamResampler(model, a.source_fps, 60, order=None, streams=S)


def resampled_frames():
    """The producer's frames through the StreamResampler: one launch per source frame, 0..4 frames at 60 fps out of each."""
    for j in range(prod_rot.shape[1]):
        n_out = resampler.push(prod_rot[:, j], prod_pos[:, j])
        for e in range(n_out):
            yield resampler.out["rot"][:, e], resampler.out["pos"][:, e]


at_60 = resampled_frames() if a.source_fps is not None else None


def push(f, characters=None):
    kw = dict(allow=[allow_mask] * S) if a.actions and f == allow_from else {}
    if mix_ids:
        characters = None                                             # a mix session's characters are its mix
        if mix_ramp:                                                  # the cross-fade: new weights in place, read by the replay
            t = min(max((f - first + 1) / mix_ramp, 0.0), 1.0)
            sess.mix_weights[:, 0].fill_(1.0 - t); sess.mix_weights[:, 1].fill_(t)
    if a.raw is not None:
        if kw:
            sess.set_allow(kw["allow"])
        if at_60 is not None:
            return sess.push_raw(*next(at_60), characters=characters)
        return sess.push_raw(raw_rot[:, f], raw_pos[:, f], characters=characters)
    return sess.push(*[torch.stack([src[s][k][f] for s in range(S)]) for k in range(4)],
                     *[torch.stack([per[s][k][f] for s in range(S)]) for k in range(4)], characters=characters, **kw)


push(0, characters=[0, 1])                                            # the first push captures the step
sess.reset()
if a.source_fps is not None:
    resampler.reset()
    at_60 = resampled_frames()
torch.cuda.synchronize(); t0 = time.perf_counter()
pos, eul, applied, seeded, head, rows_, cont_ = [], [], [], [], [], [], []
if a.actions:
    sess.allow.zero_()
gen0 = model._ctx.generation()
for f in range(F):
    chars = [1, 1] if f == a.switch else None
    if f == a.load_at:                                                # one more character while the session runs: no new bank, no new capture
        new = bank.add(*banks[2], labels=labels[2] if labels else None)
        chars = [1 if a.switch is not None and f >= a.switch else 0, new]
    if a.ours_per_character and a.load_at is not None and f == a.load_at + 10:      # the new character's CVAE arrives: stream order, no new capture
        cvaes.store(2, synthetic_cvae_state_dict(101, 1.0), *cvae_stats(5))
        sess.set_cvae(2, 2)
    o = push(f, characters=chars)
    if a.ours:
        seeded.append(o["seeded"].clone())
    if f >= first:                                                    # both streams started together: both are valid from here on
        pos.append(o["bvh_pos"].clone()); eul.append(o["bvh_euler"].clone())
        if a.actions:
            applied.append(o["applied"].clone())
        if a.coherent is not None:
            rows_.append(o["idx"].clone()); cont_.append(o["continued"].clone())
        if a.world:                                                   # the last bone's world position, kept on the device: no synchronisation here
            head.append(o["gpos"][:, -1].clone())
torch.cuda.synchronize(); dt = time.perf_counter() - t0
pos, eul = torch.stack(pos, 1), torch.stack(eul, 1)                   # (S, F - first, V, 3)

names = ["Joint%02d" % i for i in range(24)]
for s in range(S):
    p = os.path.join(a.out, f"{'Ours' if a.ours else 'mix' if mix_ids else 'soft' if soft else 'raw' if a.raw is not None else 'live'}_stream{s}.bvh")
    write_bvh(p, names, LAYOUTS["mocha"]["parents"], pos[s], eul[s])
    print(f"  {p}: {os.path.getsize(p)} bytes, {pos.shape[1]} frames")
if a.world:
    print(f"  world: palette {tuple(sess.out['palette'].shape)} {sess.out['palette'].dtype}, gpos {tuple(sess.out['gpos'].shape)}, "
          f"grot {tuple(sess.out['grot'].shape)}: one mocha_world_pose launch behind every captured step; bone {J - 1} of stream 0 in world space:")
    for f, g in enumerate(torch.stack(head, 1)[0].cpu().tolist()):
        print(f"    frame {first + f}: {g[0]:9.4f} {g[1]:9.4f} {g[2]:9.4f}")
if a.coherent is not None:
    rw, ct = torch.stack(rows_, 1).cpu(), torch.stack(cont_, 1).cpu()
    for s in range(S):
        jumps = int((rw[s, 1:] != rw[s, :-1] + 1).sum())
        print(f"  coherent matching, jump penalty {a.coherent}: stream {s} continued on {int(ct[s].sum())} of {rw.shape[1]} posed frames, "
              f"{jumps} transitions that are not 'next row'; generation {gen0} -> {model._ctx.generation()}")
if a.ours_per_character:
    sd = torch.stack(seeded, 1).cpu()
    print(f"  one CVAE per character: seed frames per stream {sd.sum(1).tolist()} of {F - first} posed frames; generation {gen0} -> {model._ctx.generation()}")
if a.switch is not None and first + 1 <= a.switch < F:
    step = (pos[0, 1:, 1:] - pos[0, :-1, 1:]).abs().amax(dim=(1, 2))     # per frame, the non-root bones of stream 0
    print(f"  stream 0 switches character at frame {a.switch}: largest bone-position step there {float(step[a.switch - first - 1]):.4f}, "
          f"median over the clip {float(step.median()):.4f}" + (f" (inertialized, half-life {a.inertial} s)" if a.inertial is not None else ""))
if a.load_at is not None and 0 <= a.load_at < F:
    print(f"  character 2 ({banks[2][0].shape[0]} entries) added to the resident bank at frame {a.load_at}, rows {bank.rows(2)}; stream 1 took it; "
          f"generation {gen0} -> {model._ctx.generation()}; {bank.free_rows} rows free")
if mix_ids:
    wt = o["weight"][0].tolist()
    what = f"cross-fade over {mix_ramp} frames from the first pose" if mix_ramp else f"splice {a.mix_parts.rpartition(':')[2]} by body part"
    print(f"  mix of characters {mix_ids[0]} and {mix_ids[1]} ({what}): final normalised weights of stream 0 {wt}; "
          f"generation {gen0} -> {model._ctx.generation()}")
if a.actions:
    ap_ = torch.stack(applied, 1)
    print(f"  actions {a.actions.partition(':')[0]} allowed from frame {allow_from}: " + ", ".join(
        f"stream {s}: {int((ap_[s] == 1).sum())} constrained, {int((ap_[s] == -1).sum())} fell back, {int((ap_[s] == 0).sum())} unconstrained"
        for s in range(S)))
print(f"{F} pushes of {S} streams in {dt * 1e3:.1f} ms ({dt / F * 1e3:.3f} ms per push, host loop included)")
assert bool(torch.isfinite(pos).all()) and bool(torch.isfinite(eul).all())
