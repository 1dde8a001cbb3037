#!/usr/bin/env python3
"""Time BVH writing on the device (format_bvh_motion / mocha_bvh_format, write_bvh_clips) against the host route on the same data.

    python tools/bvh_write_bench.py [--clips 64 --frames 3600 --rounds 3 --out profiles/r18/bvh_write.json]

Workload: tools/bvh_parse_bench.py's in reverse - `clips` synthetic walks (synthetic.raw_walk_clip, 24 joints) of `frames` frames as
float64 channels on the device, the way mocha_postprocess leaves them.  In the same process, alternating per round, HIP events and clocks
untouched:

  (a) mocha_bvh_format into a text buffer already allocated: the call with HIP events around it (tables' upload and the stream wait
      included), then once more with the library's per-launch events (mocha_profile_start / _stop): ms of each of the three launches;
  (b) the device-to-host copy of the text into pinned memory (HIP events);
  (c) write_bvh_clips as a user calls it: format, copy, headers, one file per clip (host clock, ends with the files closed);
  (d) the host route, write_bvh without ``model``, on ONE clip, scaled to the clip count - and, in the first round only, on every clip.

Before anything is timed, the first and the last file of (c) are compared byte for byte with the host route's."""
import argparse
import ctypes as C
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from mocha_sigasia2023_amd import Generator, _C, synthetic, write_bvh, write_bvh_clips  # noqa: E402
from mocha_sigasia2023_amd.skeleton import LAYOUTS  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=64)
    ap.add_argument("--frames", type=int, default=3600)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r18", "bvh_write.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bvh_write_bench: needs a ROCm device; nothing is measured without one")
    dev = torch.device("cuda:0")
    model = Generator(layout="mocha", device=dev)
    par = LAYOUTS["mocha"]["parents"]
    names = ["Joint%02d" % i for i in range(24)]
    walks = [synthetic.raw_walk_clip(par, a.frames, seed=1000 + i) for i in range(a.clips)]
    rot_h = np.concatenate([w[0] for w in walks]).astype(np.float64)
    pos_h = np.concatenate([w[1] for w in walks]).astype(np.float64)
    del walks
    V, F = 24, a.clips * a.frames
    offs = [i * a.frames for i in range(a.clips + 1)]
    rot, pos = torch.from_numpy(rot_h).to(dev), torch.from_numpy(pos_h).to(dev)
    tmp = tempfile.mkdtemp(prefix="bvh_write_bench_")
    paths = [os.path.join(tmp, f"clip{i:03d}.bvh") for i in range(a.clips)]
    host_path = os.path.join(tmp, "host.bvh")

    def host_clip(i):
        write_bvh(host_path, names, par, pos_h[offs[i]: offs[i + 1]], rot_h[offs[i]: offs[i + 1]])

    visit = write_bvh_clips(model, paths, names, par, pos, rot, offs)                 # warm-up: code objects, the format buffer
    for i in (0, a.clips - 1):
        host_clip(i)
        assert open(paths[i], "rb").read() == open(host_path, "rb").read(), f"clip {i}: the device route's file differs from the host's"

    lib, ctx = model._ctx.lib, model._ctx
    bound = int(lib.mocha_bvh_text_bound(F, V, 0))
    text = torch.empty(bound, dtype=torch.uint8, device=dev)
    begin = (C.c_int64 * (a.clips + 1))()
    rep = _C.mocha_bvhw_report()
    off_c, visit_c, axes_c = (C.c_int32 * (a.clips + 1))(*offs), (C.c_int32 * V)(*visit), (C.c_int32 * 3)(2, 1, 0)

    def call():
        model._ctx.call("mocha_bvh_format", C.c_void_p(pos.data_ptr()), C.c_void_p(rot.data_ptr()), off_c, a.clips, V, visit_c, axes_c, 0,
                        C.c_void_p(text.data_ptr()), bound, begin, C.byref(rep), C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    call()
    torch.cuda.synchronize()
    text_bytes = int(rep.bytes)
    assert rep.first_bad == -1 and rep.tokens == F * 75 and begin[a.clips] == text_bytes
    pinned = torch.empty(text_bytes, dtype=torch.uint8, pin_memory=True)
    rounds = []
    for k in range(a.rounds):
        r = {"call_ms": timed(call), "d2h_pinned_ms": timed(lambda: pinned.copy_(text[:text_bytes], non_blocking=True))}
        model.profile_start()
        call()
        torch.cuda.synchronize()
        sites = model.profile_stop()["sites"]
        r["launches"] = {s: {"ms": v["ms"], "bytes": v["bytes"]} for s, v in sites.items()}
        r["launch_sum_ms"] = sum(v["ms"] for v in sites.values())
        t0 = time.perf_counter()
        write_bvh_clips(model, paths, names, par, pos, rot, offs)
        r["write_bvh_clips_ms"] = (time.perf_counter() - t0) * 1e3
        t0 = time.perf_counter()
        host_clip(k % a.clips)
        r["host_write_bvh_one_clip_ms"] = (time.perf_counter() - t0) * 1e3
        r["host_write_bvh_scaled_ms"] = r["host_write_bvh_one_clip_ms"] * a.clips
        if k == 0:
            t0 = time.perf_counter()
            for i in range(a.clips):
                host_clip(i)
            r["host_write_bvh_all_clips_ms"] = (time.perf_counter() - t0) * 1e3
        rounds.append(r)
    med = lambda key: float(np.median([r[key] for r in rounds]))      # noqa: E731
    keys = ("call_ms", "d2h_pinned_ms", "launch_sum_ms", "write_bvh_clips_ms", "host_write_bvh_one_clip_ms", "host_write_bvh_scaled_ms")
    out = {"workload": f"{a.clips} clips x {a.frames} frames, 24 joints, float64 channels on the device: {F * 75} tokens, {text_bytes} bytes of MOTION text",
           "timing": "HIP events around the call and the copy; the library's per-launch events for the launches; host clock for write_bvh_clips "
                     "(format, copy, headers, files) and for write_bvh without model; alternating in one process",
           "text_bytes": text_bytes, "rounds": rounds, "median": {key: med(key) for key in keys}}
    out["median"]["launches_ms"] = {s: float(np.median([r["launches"][s]["ms"] for r in rounds])) for s in rounds[0]["launches"]}
    out["median"]["host_write_bvh_all_clips_ms"] = rounds[0]["host_write_bvh_all_clips_ms"]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(out["median"], sort_keys=True))
    for p in paths + [host_path]:
        os.remove(p)
    os.rmdir(tmp)


if __name__ == "__main__":
    main()
