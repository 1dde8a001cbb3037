#!/usr/bin/env python3
"""The reference demo (test_fullframework.py) end to end on synthetic data, entirely through the HIP path.

    local bone features of two clips  --featurize-->  X_raw  --(z-score fused)-->  encoder  -->  bank from the character clip
    NN branch   : characterize_pair -> pose heads -> root integration / foot-lock IK -> BVH        ("cm_" stream of the demo)
    Ours branch : CVAE session frame loop -> decoder -> pose heads -> post-processing -> BVH        (the demo's main output)

The reference's data (BVH clips, norm.npz, checkpoints) is not redistributable, so weights, norms and motions are synthetic;
with real assets replace `synthetic_state_dict` by torch.load(ckpt)['gen_ema'], the norms by norm.npz / cnt_norm.npz /
cvae_norm.npz and the bone features by the output of the reference's process_data (motion/bvh.py + preprocess).

With --from-raw both clips start as RAW mocap (synthetic.raw_walk_clip: Euler degrees and centimetres per joint, as a BVH file holds them)
and the reference's clip preparation runs on the device as well:

    raw clip  --ingest_clips-->  root bone, velocities, contacts  --clip_windows-->  60-frame windows  --featurize-->  X_raw  --> as above

The source's per-window inputs of the post-processing are then its own: root-local velocities of each window's last frame, the mean hip
speed of the window, the contacts of its last frame (test_fullframework.py:142-143, :493).  The pair call's output and the windows are
also written to <out>/from_raw.npz.

With --src-bvh A --cha-bvh B the same route starts from two BVH FILES (source, character; the 24-joint 'mocha' skeleton in file order,
at least 31 frames each): load_bvh reads the hierarchy on the host and parses the MOTION text on the device, and its two arrays go into
ingest_clips with the files' rotation order and frame rate.  A clip of n frames gives n - 15 windows; --frames is ignored.  The model, its
windows and the root fits are fixed to 60 frames per second: --resample 60 brings files of another rate there first (slerp / linear on the
device, load_bvh(fps=60)); without it a file's rate only scales the finite differences.

    file  --load_bvh-->  raw clip  --ingest_clips-->  ...  as --from-raw, <out>/from_raw.npz included
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mocha_sigasia2023_amd import (CVAE, ContextBank, Generator, OursSession, retarget_clip, retarget_clip_ours, synthetic,  # noqa: E402
                                   synthetic_state_dict, write_bvh)
from mocha_sigasia2023_amd import weights as W  # noqa: E402
from mocha_sigasia2023_amd.skeleton import LAYOUTS  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--frames", type=int, default=120, help="windows per clip (the demo clips have 585)")
ap.add_argument("--out", default="gpurun_out/demo")
ap.add_argument("--from-raw", action="store_true", help="start from raw mocap clips: ingest_clips -> clip_windows -> featurize")
ap.add_argument("--src-bvh", help="the source clip as a BVH file (with --cha-bvh): the --from-raw route on files")
ap.add_argument("--cha-bvh", help="the character clip as a BVH file")
ap.add_argument("--resample", type=float, metavar="R",
                help="with --src-bvh / --cha-bvh: bring files of another frame rate to R frames per second first (load_bvh(fps=R); the model "
                     "is fixed to 60)")
ap.add_argument("--world", metavar="OUT.npz", help="save the global bone positions of the source and of the two outputs: what the "
                                                     "reference hands to animation_plot (world_pose: quat.fk on the device)")
ap.add_argument("--coherent", type=float, metavar="L", help="coherent context matching for the NN branch: the source windows take a "
                "jump-penalised path through the character clip's windows (penalty L per transition that is not 'next window of the "
                "clip') instead of one nearest window each; prints the non-continuations with and without it")
ap.add_argument("--coherent-relative", action="store_true", help="L in units of the median nearest distance instead of the matcher's")
a = ap.parse_args()
if a.coherent_relative and a.coherent is None:
    ap.error("--coherent-relative goes with --coherent L")
if bool(a.src_bvh) != bool(a.cha_bvh):
    ap.error("--src-bvh and --cha-bvh go together")
if a.resample is not None and not a.src_bvh:
    ap.error("--resample applies to the --src-bvh / --cha-bvh route")
if a.src_bvh:
    a.from_raw = True
os.makedirs(a.out, exist_ok=True)
dev = torch.device("cuda:0")
N = a.frames

# ---- model, CVAE and (synthetic) statistics                                                  test_fullframework.py:40-98
model = Generator(device=dev).load_state_dict(synthetic_state_dict(1777, 1.0)).eval()
cvae = CVAE(device=dev).load_state_dict(W.synthetic_cvae_state_dict(99, 1.0)).eval()
rng = np.random.Generator(np.random.PCG64(0))
J, C = 25, 15
X_mean = (0.05 * rng.standard_normal((J, C))).astype(np.float32); X_std = rng.uniform(0.5, 1.5, (J, C)).astype(np.float32)
Y_mean = (0.05 * rng.standard_normal((J, C))).astype(np.float32); Y_std = rng.uniform(0.2, 0.6, (J, C)).astype(np.float32)
model.set_pose_norm(X_mean, X_std, Y_mean, Y_std)
cnt_mean, cnt_std = synthetic.cnt_norm(7)
stats = [(0.1 * rng.standard_normal((90, 256))).astype(np.float32), rng.uniform(0.5, 1.5, (90, 256)).astype(np.float32),
         (0.1 * rng.standard_normal((90, 256))).astype(np.float32), rng.uniform(0.5, 1.5, (90, 256)).astype(np.float32)]

# ---- the two clips as local bone features of N sixty-frame windows each                      :120-140, 203-222
if a.from_raw:
    from mocha_sigasia2023_amd import clip_windows, ingest_clips  # noqa: E402
    if a.src_bvh:
        from mocha_sigasia2023_amd import IngestConfig, load_bvh  # noqa: E402
        files = load_bvh(model, [a.src_bvh, a.cha_bvh], fps=a.resample)
        if len(files.names) != model.V or min(files.lengths) < 31:
            ap.error(f"the files must hold the {model.V} joints of the model's skeleton and at least 31 frames each"
                     + (f" at {a.resample:g} fps (they have {files.lengths} from {files.source_fps} fps)" if a.resample else ""))
        lengths, N = files.lengths, files.lengths[0] - 15
        fps = a.resample if a.resample is not None else round(1.0 / files.frametime)
        clips = ingest_clips(model, files.rot, files.pos, lengths, raw=IngestConfig(order=files.order, fps=fps))
    else:
        if N < 16:
            ap.error("--from-raw needs at least 16 windows per clip: a clip of N + 15 frames gives N windows, and 31 frames are the least")
        raw = [synthetic.raw_walk_clip(LAYOUTS["mocha"]["parents"], N + 15, seed=s) for s in (11, 12)]        # source, character
        lengths = [N + 15, N + 15]
        clips = ingest_clips(model, np.concatenate([r for r, _ in raw]), np.concatenate([p for _, p in raw]), lengths)
    win = clip_windows(clips, lengths, window=60, step=1)      # n - 15 windows per clip, the last 44 padded
    src_bones = tuple(win[k][:N] for k in ("Yrot", "Ypos", "Yvel", "Yang"))
    cha_bones = tuple(win[k][N:] for k in ("Yrot", "Ypos", "Yvel", "Yang"))
    rot0, vel0, ang0 = (win[k][:N, -1, 0].double().cpu().numpy() for k in ("Yrot", "Yvel", "Yang"))

    def inv_mul_vec(q, v):                                                     # quat.inv_mul_vec
        u = -q[:, 1:]
        t = 2.0 * np.cross(u, v)
        return v + q[:, :1] * t + np.cross(u, t)
    rvel, rang = inv_mul_vec(rot0, vel0).astype(np.float32), inv_mul_vec(rot0, ang0).astype(np.float32)
    src_speed = win["Yvel"][:N, :, 1].norm(dim=-1).mean(-1).cpu().numpy()
    contact = win["contact"][:N, -1].cpu().numpy()
else:
    src_bones = synthetic.bone_windows(11, N)
    cha_bones = synthetic.bone_windows(12, N)
    _, rvel, rang, hipvel, contact = synthetic.postprocess_inputs(5, N)       # root-local velocities / contacts of the source
    src_speed = np.linalg.norm(hipvel, axis=-1).mean(-1).astype(np.float32)

torch.cuda.synchronize(); t0 = time.perf_counter()
src_X = model.featurize(*src_bones)                                            # :141-185 on the device
cha_X = model.featurize(*cha_bones)
# ---- NN branch for the whole clip                                                            :188-194, 271-302, 438-443, 465-467
Y, idx, cha_enc, cha_nm = model.characterize_pair(src_X, cha_X, cnt_mean, cnt_std, return_index=True, return_bank=True, raw=True)
bank = ContextBank(model, cha_nm, cha_enc)
coherent = None
if a.coherent is not None:
    from mocha_sigasia2023_amd import CoherentMatch  # noqa: E402
    coherent = CoherentMatch(a.coherent, relative=a.coherent_relative)
    hard_idx = idx
    Y, idx = model.characterize_pair(src_X, cha_X, cnt_mean, cnt_std, return_index=True, raw=True, coherent=coherent)
    jumps = lambda ix: int(len(ix) - 1 - (ix[1:] == ix[:-1] + 1).sum())       # noqa: E731
    print(f"non-continuations over {N} windows: hard match {jumps(hard_idx)}, coherent (jump {a.coherent:g}"
          f"{' x median nearest distance' if a.coherent_relative else ''}) {jumps(idx)}")
# the reference's "cm_" stream takes the decoded poses as they are: no blending with the previous frame, no foot-lock IK
# (test_fullframework.py:512-527, 637-641)
from mocha_sigasia2023_amd import PostProcessor  # noqa: E402
nn = retarget_clip(bank, src_X, cnt_mean, cnt_std, rvel, rang, src_speed, contact, raw=True,
                   post=PostProcessor(model, ik_enabled=False, blend=False), coherent=coherent)
# ---- Ours branch: CVAE frame loop seeded with the first matched character feature            :298, 436, 446-457
src_enc, src_cnt = model.encode(src_X, raw=True)
sess = OursSession(model, cvae, *stats).reset(cha_enc[int(idx[0])])
ours = retarget_clip_ours(sess, src_enc[1:], src_cnt[1:], rvel[1:], rang[1:], src_speed[1:], contact[1:],
                          denorm=(Y_mean[1:], Y_std[1:]))
torch.cuda.synchronize(); dt = time.perf_counter() - t0

if a.from_raw:
    np.savez(os.path.join(a.out, "from_raw.npz"), Y=Y.cpu().numpy(), idx=idx.cpu().numpy(), contact=contact, src_speed=src_speed,
             **{"src_" + k: v.cpu().numpy() for k, v in zip(("Yrot", "Ypos", "Yvel", "Yang"), src_bones)})
names = ["Joint%02d" % i for i in range(24)]
parents = LAYOUTS["mocha"]["parents"]
write_bvh(os.path.join(a.out, "cm_trans.bvh"), names, parents, nn["bvh_pos"], nn["bvh_euler"], model=model)          # :690-713; the numbers are formatted on the device
write_bvh(os.path.join(a.out, "ours.bvh"), names, parents, ours["bvh_pos"], ours["bvh_euler"], model=model)
print(f"{N} windows per clip: featurize + NN branch + Ours branch + post-processing in {dt * 1e3:.1f} ms "
      f"({(N - 1) / dt:.0f} frames/s including the sequential CVAE loop); matched entries {idx[:8].tolist()} ...")
for k in ("cm_trans.bvh", "ours.bvh"):
    p = os.path.join(a.out, k)
    print(f"  {p}: {os.path.getsize(p)} bytes, {sum(1 for _ in open(p))} lines")
if a.world:                                                                    # :665-690: quat.fk of every stream, one launch each
    from mocha_sigasia2023_amd import world_pose  # noqa: E402
    dv = lambda x: torch.as_tensor(x).to(dev)                                  # noqa: E731
    glb = {"src": world_pose(model, dv(src_bones[0])[:, -1].contiguous(), dv(src_bones[1])[:, -1].contiguous()),      # fp32 locals
           "cm_trans": world_pose(model, nn["rot"], nn["pos"]), "ours": world_pose(model, ours["ik_rot"], ours["pos"])}
    np.savez(a.world, parents=np.asarray([-1] + [p + 1 for p in parents]), **{f"{k}_gpos": v["gpos"].cpu().numpy() for k, v in glb.items()},
             **{f"{k}_grot": v["grot"].cpu().numpy() for k, v in glb.items()})
    print(f"  {a.world}: global positions " + ", ".join(f"{k} {tuple(v['gpos'].shape)}" for k, v in glb.items()))
    assert all(torch.isfinite(v["gpos"]).all() for v in glb.values())
assert all(torch.isfinite(v).all() for v in nn.values()) and all(torch.isfinite(v).all() for v in ours.values())
