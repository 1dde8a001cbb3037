#!/usr/bin/env python3
"""Time the whole-clip mocap front end (mocha_ingest_clips) against the streaming one (Ingestor(raw=18, streams=16)) on the same frames.

    python tools/clip_ingest_bench.py [--clips 64 --frames 3600 --rounds 3 --out profiles/r14/clip_ingest.json]

Workload: `clips` synthetic walks (synthetic.raw_walk_clip, 24 joints, Euler degrees + centimetres) of `frames` frames, every clip plain
and mirrored in ONE call (2 x clips clip entries).  In the same process, alternating per round:

  (a) the clip route: the call timed with HIP events around it (tables' upload and the stream wait included), then once more with the
      library's per-launch events (mocha_profile_start / _stop): ms, bytes moved and the HBM fraction of every launch;
  (b) the streaming route: the same frames, 16 clips at a time as 16 streams, one frame per launch, per-launch events summed.  A stream
      emits frames 12 .. n-19 only and does not mirror, so (b) runs the plain and the "mirrored" entries alike, unmirrored: it is the cost
      of the launches that is compared, per frame pushed.

HBM fraction = bytes / time / 8.0e12 B/s (the MI355X's specified peak; about 6.3e12 is achievable with a plain copy).  The bytes are what
the host layer counts per launch: every array a launch reads or writes once, fit windows and difference neighbours taken as cached."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from mocha_sigasia2023_amd import Generator, IngestConfig, Ingestor, ingest_clips, synthetic  # noqa: E402
from mocha_sigasia2023_amd.skeleton import LAYOUTS  # noqa: E402

HBM_PEAK = 8.0e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=64)
    ap.add_argument("--frames", type=int, default=3600)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r14", "clip_ingest.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("clip_ingest_bench: needs a ROCm device; nothing is measured without one")
    dev = torch.device("cuda:0")
    model = Generator(layout="mocha", device=dev)
    par = LAYOUTS["mocha"]["parents"]
    raw = [synthetic.raw_walk_clip(par, a.frames, seed=1000 + i) for i in range(a.clips)]
    rot = torch.from_numpy(np.concatenate([r for r, _ in raw for _ in range(2)])).to(dev)
    pos = torch.from_numpy(np.concatenate([p for _, p in raw for _ in range(2)])).to(dev)
    C2, F = 2 * a.clips, 2 * a.clips * a.frames
    lengths, flags = [a.frames] * C2, [k == 1 for _ in range(a.clips) for k in range(2)]
    ing = Ingestor(model, IngestConfig(lookahead=18), streams=16)
    rot_c, pos_c = rot.view(C2, a.frames, -1, 3), pos.view(C2, a.frames, -1, 3)

    def clip_route():
        return ingest_clips(model, rot, pos, lengths, mirror=flags)

    def streaming_route():
        """Frames pushed, launches and their summed time; the events of one group of 16 clips are read before the next starts."""
        pushed, launches, ms = 0, 0, 0.0
        for g in range(0, C2, 16):
            n = min(16, C2 - g)
            ing.reset()
            model.profile_start()
            for f in range(a.frames):
                ing.rot[:n].copy_(rot_c[g:g + n, f])
                ing.pos[:n].copy_(pos_c[g:g + n, f])
                ing.replay()
            torch.cuda.synchronize()
            st = model.profile_stop()["sites"]["ingest.step|mocha_live_ingest"]
            pushed, launches, ms = pushed + n * a.frames, launches + st["launches"], ms + st["ms"]
        return pushed, launches, ms

    clip_route()                                                   # warm-up: code objects, the workspace, the fit rows
    ing.replay()
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
        sites = model.profile_stop()["sites"]
        pushed, launches, stream_ms = streaming_route()
        rounds.append({"clip_call_ms": call_ms,
                       "clip_launches": {k: {"ms": v["ms"], "bytes": v["bytes"], "hbm_fraction": v["bytes"] / (v["ms"] * 1e-3) / HBM_PEAK}
                                         for k, v in sites.items()},
                       "clip_launch_sum_ms": sum(v["ms"] for v in sites.values()),
                       "clip_us_per_frame": call_ms * 1e3 / F,
                       "stream_launches": launches, "stream_kernel_ms": stream_ms, "stream_frames_pushed": pushed,
                       "stream_us_per_launch": stream_ms * 1e3 / launches, "stream_us_per_frame": stream_ms * 1e3 / pushed})
    med = lambda k: float(np.median([r[k] for r in rounds]))      # noqa: E731
    out = {"workload": f"{a.clips} clips x {a.frames} frames, plain and mirrored: {C2} clip entries, {F} frames, 24 joints, Euler input",
           "timing": "HIP events; (a) mocha_ingest_clips, one call, and its launches one by one; (b) the same frames through "
                     "Ingestor(raw=18, streams=16), per-launch events summed; alternating in one process",
           "hbm_peak_bytes_per_s": HBM_PEAK, "rounds": rounds,
           "median": {k: med(k) for k in ("clip_call_ms", "clip_launch_sum_ms", "clip_us_per_frame", "stream_us_per_launch", "stream_us_per_frame")}}
    out["median"]["stream_over_clip_per_frame"] = out["median"]["stream_us_per_frame"] / out["median"]["clip_us_per_frame"]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(out["median"], sort_keys=True))
    for k, v in sorted(rounds[-1]["clip_launches"].items()):
        print(f"  {k:44s} {v['ms'] * 1e3:9.1f} us  {v['bytes'] / 1e6:9.1f} MB  HBM fraction {v['hbm_fraction']:.3f}")


if __name__ == "__main__":
    main()
