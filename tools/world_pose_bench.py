#!/usr/bin/env python3
"""Time the world-pose stage: whole clips through world_pose (mocha_world_pose) and one live launch at 1 and 16 streams.

    python tools/world_pose_bench.py [--clips 64 --frames 3600 --rounds 3 --out profiles/r22/world_pose.json]

Workload: `clips` x `frames` frames of float64 locals on the 24-joint skeleton (random unit quaternions, offsets of tens of centimetres:
the kernel's time does not depend on the values), a random bind, all three outputs, ONE call.  Per round:

  (a) the call timed with HIP events around it, then once more with the library's per-launch events (mocha_profile_start / _stop): the
      kernel alone, the bytes it moves and the share of the HBM peak; the same with fp32 inputs;
  (b) one launch on 1 and on 16 frames with `valid` set, as a live session issues it behind its captured step: 256 launches, per-launch
      events summed.

For scale, the NumPy restatement (tests/world_ref.py, float64, with the palette) on ONE clip on the host, once.

HBM fraction = bytes / time / 8.0e12 B/s (the MI355X's specified peak; about 6.3e12 is achievable with a plain copy).  The bytes are what
the host layer counts for the launch: every array it reads or writes once, `valid`, and the bind once per workgroup of 8 frames.  A report: nothing here is a threshold."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from mocha_sigasia2023_amd import Generator, SkinBind, world_pose  # noqa: E402
from mocha_sigasia2023_amd.skeleton import LAYOUTS  # noqa: E402

HBM_PEAK = 8.0e12
LAUNCHES = 256


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=64)
    ap.add_argument("--frames", type=int, default=3600)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r22", "world_pose.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("world_pose_bench: needs a ROCm device; nothing is measured without one")
    dev = torch.device("cuda:0")
    model = Generator(layout="mocha", device=dev)
    J = model.V + 1
    g = torch.Generator(device=dev).manual_seed(22)
    rot = torch.randn((a.clips, a.frames, J, 4), dtype=torch.float64, device=dev, generator=g)
    rot /= rot.norm(dim=-1, keepdim=True)
    pos = 30.0 * torch.randn((a.clips, a.frames, J, 3), dtype=torch.float64, device=dev, generator=g)
    rng = np.random.Generator(np.random.PCG64(22))
    bind = SkinBind(model, rng.uniform(-30, 30, (J, 3)), rng.standard_normal((J, 4)), [[0.01, 0, 0, 0], [0, 0, 0.01, 0], [0, 0.01, 0, 0]])
    rot32, pos32 = rot.float(), pos.float()
    out = world_pose(model, rot, pos, bind=bind)                    # warm-up: the code objects; the outputs every timed call reuses
    world_pose(model, rot32, pos32, bind=bind, out=out)
    torch.cuda.synchronize()

    def call(r, p):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        world_pose(model, r, p, bind=bind, out=out)
        e1.record()
        torch.cuda.synchronize()
        ms = e0.elapsed_time(e1)
        model.profile_start()
        world_pose(model, r, p, bind=bind, out=out)
        torch.cuda.synchronize()
        (v,) = [v for k, v in model.profile_stop()["sites"].items() if k.startswith("world.pose")]
        return {"call_ms": ms, "kernel_ms": v["ms"], "bytes": v["bytes"], "hbm_fraction": v["bytes"] / (v["ms"] * 1e-3) / HBM_PEAK}

    def live(S):
        valid = torch.ones((S,), dtype=torch.int32, device=dev)
        o = {k: t[0, :S] for k, t in out.items()}
        model.profile_start()
        for _ in range(LAUNCHES):
            world_pose(model, rot[0, :S], pos[0, :S], bind=bind, valid=valid, out=o)
        torch.cuda.synchronize()
        (v,) = [v for k, v in model.profile_stop()["sites"].items() if k.startswith("world.pose")]
        return v["ms"] * 1e3 / v["launches"]

    live(16)
    rounds = []
    for _ in range(a.rounds):
        rounds.append({"f64": call(rot, pos), "f32": call(rot32, pos32), "live_us_1_stream": live(1), "live_us_16_streams": live(16)})
    import world_ref as WR
    par = WR.bone_parents(LAYOUTS["mocha"]["parents"])
    r0, p0 = rot[0].cpu().numpy(), pos[0].cpu().numpy()
    t0 = time.perf_counter()
    gr, gp = WR.fk(r0, p0, par)
    WR.palette(gr, gp, bind.rest_rot.cpu().numpy(), bind.rest_pos.cpu().numpy(), np.eye(3, 4), par)
    host_s = time.perf_counter() - t0
    med = lambda f: float(np.median([f(r) for r in rounds]))      # noqa: E731
    n = a.clips * a.frames
    res = {"workload": f"{a.clips} clips x {a.frames} frames = {n} frames, 24 joints + root bone, float64 or fp32 locals in; gpos, grot "
                       "float64 and the fp32 palette out",
           "timing": "HIP events; (a) world_pose, one call, and its one launch alone; (b) one launch on 1 / 16 frames with valid, "
                     f"{LAUNCHES} launches, per-launch events summed; (c) the NumPy restatement on one clip on the host, wall clock, once",
           "hbm_peak_bytes_per_s": HBM_PEAK, "rounds": rounds, "numpy_restatement_one_clip_s": host_s,
           "median": {"f64_call_ms": med(lambda r: r["f64"]["call_ms"]), "f64_kernel_ms": med(lambda r: r["f64"]["kernel_ms"]),
                      "f64_bytes": rounds[0]["f64"]["bytes"], "f64_hbm_fraction": med(lambda r: r["f64"]["hbm_fraction"]),
                      "f32_call_ms": med(lambda r: r["f32"]["call_ms"]), "f32_kernel_ms": med(lambda r: r["f32"]["kernel_ms"]),
                      "f32_bytes": rounds[0]["f32"]["bytes"], "f32_hbm_fraction": med(lambda r: r["f32"]["hbm_fraction"]),
                      "live_us_1_stream": med(lambda r: r["live_us_1_stream"]), "live_us_16_streams": med(lambda r: r["live_us_16_streams"])}}
    res["median"]["f64_ns_per_frame"] = res["median"]["f64_kernel_ms"] * 1e6 / n
    res["median"]["numpy_one_clip_over_device_one_clip"] = host_s * 1e3 / (res["median"]["f64_call_ms"] / a.clips)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(res["median"], sort_keys=True))


if __name__ == "__main__":
    main()
