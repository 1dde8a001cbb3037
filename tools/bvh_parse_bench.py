#!/usr/bin/env python3
"""Time BVH reading (load_bvh / mocha_bvh_motion) against the reference's method on the host, on the same files.

    python tools/bvh_parse_bench.py [--clips 64 --frames 3600 --rounds 3 --out profiles/r16/bvh_parse.json]

Workload: `clips` synthetic walks (synthetic.raw_walk_clip, 24 joints) of `frames` frames written by write_bvh_clips, about 1.9 MB of text
each.  In the same process, alternating per round, HIP events and clocks untouched:

  (a) the host-to-device copy of the packed text, from pageable and from pinned memory (HIP events);
  (b) mocha_bvh_motion on the text already on the device: the call with HIP events around it (tables' upload and the stream wait included),
      then once more with the library's per-launch events (mocha_profile_start / _stop): ms of each of the four launches and the text
      bytes per second of their sum against the HBM peak;
  (c) load_bvh as a user calls it: files read, hierarchies parsed, text packed, copied and parsed (host clock, ends in a synchronise);
  (d) on the host, tests/bvh_ref.py - the reference's method: line split, float() per word - on ONE clip, scaled to the clip count.

HBM fraction = text bytes / summed launch time / 8.0e12 B/s (the MI355X's specified peak; about 6.3e12 is achievable with a plain copy)."""
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
sys.path.insert(0, os.path.join(ROOT, "tests"))
import bvh_ref  # noqa: E402
from mocha_sigasia2023_amd import Generator, _C, load_bvh, read_bvh_header, synthetic, write_bvh_clips  # noqa: E402
from mocha_sigasia2023_amd.skeleton import LAYOUTS  # noqa: E402

HBM_PEAK = 8.0e12
ALIGN = _C.BVH_ALIGN


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=64)
    ap.add_argument("--frames", type=int, default=3600)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r16", "bvh_parse.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bvh_parse_bench: needs a ROCm device; nothing is measured without one")
    dev = torch.device("cuda:0")
    model = Generator(layout="mocha", device=dev)
    par = LAYOUTS["mocha"]["parents"]
    names = ["Joint%02d" % i for i in range(24)]
    tmp = tempfile.mkdtemp(prefix="bvh_parse_bench_")
    paths = [os.path.join(tmp, f"clip{i:03d}.bvh") for i in range(a.clips)]
    walks = [synthetic.raw_walk_clip(par, a.frames, seed=1000 + i) for i in range(a.clips)]
    write_bvh_clips(model, paths, names, par, np.concatenate([w[1] for w in walks]), np.concatenate([w[0] for w in walks]),
                    [i * a.frames for i in range(a.clips + 1)])       # the input files: one format call on the device, the same bytes as write_bvh's
    del walks
    texts = [open(p, "rb").read() for p in paths]
    hdrs = [read_bvh_header(t) for t in texts]
    V, F = 24, a.clips * a.frames

    # the packed text, as load_bvh packs it
    begin, end, at = [], [], 0
    for h in hdrs:
        begin.append(at); end.append(at + h.motion_end - h.motion_begin)
        at += -(-(h.motion_end - h.motion_begin) // ALIGN) * ALIGN
    nbytes = at
    buf = np.full(nbytes, 0x0A, dtype=np.uint8)
    for t, h, s in zip(texts, hdrs, begin):
        buf[s: s + h.motion_end - h.motion_begin] = np.frombuffer(t, dtype=np.uint8, count=h.motion_end - h.motion_begin, offset=h.motion_begin)
    text_bytes = int(sum(e - b for b, e in zip(begin, end)))
    pinned = torch.from_numpy(buf).pin_memory()
    pageable = torch.from_numpy(buf)
    text_dev = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    rot = torch.empty((F, V, 3), dtype=torch.float32, device=dev)
    pos = torch.empty((F, V, 3), dtype=torch.float32, device=dev)
    off = (C.c_int32 * (a.clips + 1))(*[i * a.frames for i in range(a.clips + 1)])
    b_arr, e_arr = (C.c_int64 * a.clips)(*begin), (C.c_int64 * a.clips)(*end)
    offsets = np.ascontiguousarray(hdrs[0].offsets, np.float32)
    rep = _C.mocha_bvh_report()

    def call():
        model._ctx.call("mocha_bvh_motion", C.c_void_p(text_dev.data_ptr()), nbytes, buf.ctypes.data_as(C.c_void_p), b_arr, e_arr, off, a.clips,
                        V, hdrs[0].channels, None, V, offsets.ctypes.data_as(C.POINTER(C.c_float)), C.c_void_p(rot.data_ptr()),
                        C.c_void_p(pos.data_ptr()), C.byref(rep), C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    text_dev.copy_(pinned)                                         # warm-up: code objects, the parse buffer
    call()
    torch.cuda.synchronize()
    assert rep.first_bad == -1 and rep.tokens == F * 75, (rep.first_bad, rep.tokens)
    want = bvh_ref.load(texts[0])
    assert np.array_equal(rot[: a.frames].cpu().numpy().view(np.uint32), want["rotations"].astype(np.float32).view(np.uint32))
    rounds = []
    for _ in range(a.rounds):
        r = {"h2d_pageable_ms": timed(lambda: text_dev.copy_(pageable)), "h2d_pinned_ms": timed(lambda: text_dev.copy_(pinned, non_blocking=True)),
             "call_ms": timed(call)}
        model.profile_start()
        call()
        torch.cuda.synchronize()
        sites = model.profile_stop()["sites"]
        r["launches"] = {k: {"ms": v["ms"], "bytes": v["bytes"]} for k, v in sites.items()}
        r["launch_sum_ms"] = sum(v["ms"] for v in sites.values())
        r["text_bytes_per_s"] = text_bytes / (r["launch_sum_ms"] * 1e-3)
        r["hbm_fraction"] = r["text_bytes_per_s"] / HBM_PEAK
        t0 = time.perf_counter()
        got = load_bvh(model, paths)
        torch.cuda.synchronize()
        r["load_bvh_ms"] = (time.perf_counter() - t0) * 1e3
        assert got.slow_tokens == 0
        t0 = time.perf_counter()
        bvh_ref.load(texts[0])
        r["host_line_split_one_clip_ms"] = (time.perf_counter() - t0) * 1e3
        r["host_line_split_scaled_ms"] = r["host_line_split_one_clip_ms"] * a.clips
        rounds.append(r)
    med = lambda k: float(np.median([r[k] for r in rounds]))      # noqa: E731
    keys = ("h2d_pageable_ms", "h2d_pinned_ms", "call_ms", "launch_sum_ms", "text_bytes_per_s", "hbm_fraction", "load_bvh_ms",
            "host_line_split_one_clip_ms", "host_line_split_scaled_ms")
    out = {"workload": f"{a.clips} clips x {a.frames} frames, 24 joints, written by write_bvh: {text_bytes} bytes of MOTION text, {F * 75} tokens",
           "timing": "HIP events around the copies and the call; the library's per-launch events for the launches; host clock for load_bvh "
                     "(read, pack, copy, parse) and for tests/bvh_ref.py on one clip; alternating in one process",
           "hbm_peak_bytes_per_s": HBM_PEAK, "text_bytes": text_bytes, "rounds": rounds, "median": {k: med(k) for k in keys}}
    out["median"]["launches_ms"] = {k: float(np.median([r["launches"][k]["ms"] for r in rounds])) for k in rounds[0]["launches"]}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(out["median"], sort_keys=True))
    for p in paths:
        os.remove(p)
    os.rmdir(tmp)


if __name__ == "__main__":
    main()
