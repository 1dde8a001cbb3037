#!/usr/bin/env python3
"""Time the resampler: whole clips (mocha_resample_clips) and one streaming step (mocha_resample_step at 16 streams).

    python tools/resample_bench.py [--clips 64 --frames 7200 --source-fps 120 --rounds 3 --out profiles/r21/resample.json]

Workload: `clips` synthetic walks (synthetic.raw_walk_clip, 24 joints, Euler degrees + centimetres) of `frames` frames at `source-fps`,
resampled to 60 in ONE call.  Per round:

  (a) the call timed with HIP events around it (tables' upload and the stream wait included), then once more with the library's
      per-launch events (mocha_profile_start / _stop): ms, bytes moved and the HBM fraction of each of the three launches;
  (b) StreamResampler(streams=16): 256 pushes of frames already on the device, per-launch events summed.

For scale, the NumPy restatement (tests/resample_ref.py) on ONE clip on the host, once.

HBM fraction = bytes / time / 8.0e12 B/s (the MI355X's specified peak; about 6.3e12 is achievable with a plain copy).  The bytes are what
the host layer counts per launch: every array a launch reads or writes once."""
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
from mocha_sigasia2023_amd import Generator, StreamResampler, resample_clips, synthetic  # noqa: E402
from mocha_sigasia2023_amd.ingest import resample_ratio  # noqa: E402
from mocha_sigasia2023_amd.skeleton import LAYOUTS  # noqa: E402

HBM_PEAK = 8.0e12
PUSHES = 256


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=64)
    ap.add_argument("--frames", type=int, default=7200)
    ap.add_argument("--source-fps", type=float, default=120.0)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r21", "resample.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("resample_bench: needs a ROCm device; nothing is measured without one")
    dev = torch.device("cuda:0")
    model = Generator(layout="mocha", device=dev)
    par = LAYOUTS["mocha"]["parents"]
    base = [synthetic.raw_walk_clip(par, a.frames, seed=1000 + i) for i in range(min(a.clips, 8))]      # eight walks, repeated
    rot = torch.from_numpy(np.concatenate([base[i % len(base)][0] for i in range(a.clips)])).to(dev)
    pos = torch.from_numpy(np.concatenate([base[i % len(base)][1] for i in range(a.clips)])).to(dev)
    lengths = [a.frames] * a.clips
    num, den = resample_ratio(a.source_fps, 60)

    def clip_route():
        return resample_clips(model, rot, pos, lengths, a.source_fps, 60.0)

    rs = StreamResampler(model, a.source_fps, 60.0, streams=16)
    rs.rot.copy_(rot.view(a.clips, a.frames, 24, 3)[:16, 0] if a.clips >= 16 else rot[:16])
    rs.pos.copy_(pos.view(a.clips, a.frames, 24, 3)[:16, 0] if a.clips >= 16 else pos[:16])

    def streaming_route():
        rs.reset()
        model.profile_start()
        for _ in range(PUSHES):
            rs.replay()
        torch.cuda.synchronize()
        st = model.profile_stop()["sites"]
        (v,) = [v for k, v in st.items() if k.startswith("resample.step")]
        return v["launches"], v["ms"]

    _, _, new = clip_route()                                        # warm-up: code objects, the workspace
    rs.replay()
    torch.cuda.synchronize()
    rounds = []
    for _ in range(a.rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        clip_route()
        e1.record()
        torch.cuda.synchronize()
        call_ms = e0.elapsed_time(e1)
        model.profile_start()
        clip_route()
        torch.cuda.synchronize()
        sites = {k: v for k, v in model.profile_stop()["sites"].items() if k.startswith("resample.")}
        launches, step_ms = streaming_route()
        rounds.append({"clip_call_ms": call_ms,
                       "clip_launches": {k: {"ms": v["ms"], "bytes": v["bytes"], "hbm_fraction": v["bytes"] / (v["ms"] * 1e-3) / HBM_PEAK}
                                         for k, v in sites.items()},
                       "clip_launch_sum_ms": sum(v["ms"] for v in sites.values()),
                       "clip_us_per_source_frame": call_ms * 1e3 / (a.clips * a.frames),
                       "step_launches": launches, "step_us_per_launch": step_ms * 1e3 / launches})
    import resample_ref as RR
    t0 = time.perf_counter()
    RR.resample_clip(base[0][0], base[0][1], "zyx", num, den)
    host_s = time.perf_counter() - t0
    med = lambda k: float(np.median([r[k] for r in rounds]))      # noqa: E731
    out = {"workload": f"{a.clips} clips x {a.frames} frames at {a.source_fps:g} fps -> 60 fps ({num}/{den}): {sum(new)} output frames, "
                       "24 joints, Euler input",
           "timing": "HIP events; (a) mocha_resample_clips, one call, and its launches one by one; (b) mocha_resample_step at 16 streams, "
                     f"{PUSHES} pushes, per-launch events summed; (c) the NumPy restatement on one clip on the host, wall clock, once",
           "hbm_peak_bytes_per_s": HBM_PEAK, "rounds": rounds, "numpy_restatement_one_clip_s": host_s,
           "median": {k: med(k) for k in ("clip_call_ms", "clip_launch_sum_ms", "clip_us_per_source_frame", "step_us_per_launch")}}
    out["median"]["numpy_one_clip_over_device_one_clip"] = host_s * 1e3 / (out["median"]["clip_call_ms"] / a.clips)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(out["median"], sort_keys=True))
    for k, v in sorted(rounds[-1]["clip_launches"].items()):
        print(f"  {k:44s} {v['ms'] * 1e3:9.1f} us  {v['bytes'] / 1e6:9.1f} MB  HBM fraction {v['hbm_fraction']:.3f}")


if __name__ == "__main__":
    main()
