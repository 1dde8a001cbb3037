#!/usr/bin/env python3
"""Multi-character bank on one MI355X (mocha_bank_set_segments; tests/test_multi_character.py checks the results).

(a) the segmented scan (mocha_match_seg_scan) from a kernel trace: time per launch, the bytes it must read (sum over blocks of
    rows(segment) x 90*256 x bytes per value) and the fraction of 8 TB/s, for
      - 8 windows on 8 characters of 2 048 rows each (fp32 and bf16 banks),
      - 8 windows on one 2 048-row character, next to mocha_match_stream<f32> on the same rows,
      - 1 window on a 16 384-row single segment, next to mocha_match_stream<f32> on the same rows (option scan16 = 0),
    and, from the same trace, the soft matcher on the first case (k = 4): its all-keys scan (mocha_match_seg_keys, the same bytes as the
    hard scan plus 8 B written per row and query) and its selection (mocha_seg_topk_blend: one read of the keys and k bank rows per query;
    this tool asks for indices and distances only, so no blend is written).
(b) p50 / p99 of the 8-stream captured step (MultiStreamCharacterizer, 8 characters of 2 048 rows) next to what exists without it:
    8 contexts, each with its own current bank and StreamingCharacterizer, stepped one after another.

    python tools/multi_character_bench.py [--out DIR]     runs (a) in a child process under rocprofv3 --kernel-trace --stats, then (b)
"""
import argparse
import csv
import glob
import os
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from mocha_sigasia2023_amd import (ContextBank, Generator, MultiCharacterBank, MultiStreamCharacterizer, StreamingCharacterizer,  # noqa: E402
                                   synthetic, synthetic_state_dict)

D = 90 * 256
REPS = 20
HBM = 8e12
# (case, kernel name fragment, bytes per launch)
CASES = [
    ("8 windows x 8 characters x 2048 rows, fp32", "mocha_match_seg_scan<false>", 8 * 2048 * D * 4),
    ("8 windows x 8 characters x 2048 rows, bf16", "mocha_match_seg_scan<true>", 8 * 2048 * D * 2),
    ("8 windows x 1 character x 2048 rows, fp32", "mocha_match_seg_scan<false>", 2048 * D * 4),
    ("  same rows, mocha_match_stream<f32> (8 queries)", "mocha_match_stream<8, false>", 2048 * D * 4),
    ("1 window x 16384-row segment, fp32", "mocha_match_seg_scan<false>", 16384 * D * 4),
    ("  same rows, mocha_match_stream<f32> (1 query, scan16 = 0)", "mocha_match_stream<1, false>", 16384 * D * 4),
    ("soft k = 4: all-keys scan, 8 x 8 x 2048, fp32", "mocha_match_seg_keys<false>", 8 * 2048 * (D * 4 + 8)),
    ("  its selection (keys + 4 bank rows per query)", "mocha_seg_topk_blend<false>", 8 * (2048 * 8 + 4 * D * 4)),
    ("soft k = 4: all-keys scan, 8 x 8 x 2048, bf16", "mocha_match_seg_keys<true>", 8 * 2048 * (D * 2 + 8)),
    ("  its selection (keys + 4 bank rows per query)", "mocha_seg_topk_blend<true>", 8 * (2048 * 8 + 4 * D * 2)),
]


def model_and_data(dev):
    model = Generator(device=dev).load_state_dict(synthetic_state_dict(1777, 1.0)).eval()
    g = torch.Generator(device=dev); g.manual_seed(3)
    nm = torch.randn((8 * 2048, D), device=dev, generator=g)
    enc = torch.randn((8 * 2048, 90, 256), device=dev, generator=g)
    return model, nm, enc


def scan_cases():
    """The launches of (a), REPS of each, in CASES order (the trace is split by kernel name and order)."""
    dev = torch.device("cuda:0")
    model, nm, enc = model_and_data(dev)
    banks = [(nm[c * 2048:(c + 1) * 2048], enc[c * 2048:(c + 1) * 2048]) for c in range(8)]
    q = torch.randn((8, D), device=dev)
    for bf16 in (False, True):
        mb = MultiCharacterBank(model, banks, bf16=bf16, dec_cache=False)
        for _ in range(REPS):
            mb.query(q, list(range(8)))
        for _ in range(REPS):
            mb.query(q, list(range(8)), k=4)
    torch.cuda.synchronize()
    mb = MultiCharacterBank(model, banks, dec_cache=False)
    for _ in range(REPS):
        mb.query(q, [3] * 8)
    cb = ContextBank(model, banks[3][0], banks[3][1], dec_cache=False)
    for _ in range(REPS):
        cb.query(q)
    model.set_option("scan16", 0)
    one = MultiCharacterBank(model, [(nm, enc)], dec_cache=False)
    for _ in range(REPS):
        one.query(q[:1], [0])
    cb = ContextBank(model, nm, enc, dec_cache=False)
    for _ in range(REPS):
        cb.query(q[:1])
    torch.cuda.synchronize()


def profile_scans(out):
    tdir = os.path.join(out, "trace_scan")
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", tdir, "-o", "scan", "--",
           sys.executable, os.path.abspath(__file__), "--child-scan"]
    subprocess.run(["timeout", "-k", "10", "300"] + cmd, check=True)
    traces = glob.glob(os.path.join(tdir, "**", "*kernel_trace.csv"), recursive=True)
    if not traces:
        raise RuntimeError(f"no kernel trace under {tdir}")
    rows = []
    for t in traces:
        with open(t) as f:
            rows += list(csv.DictReader(f))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    seen = {}
    lines = [f"{'case':62s} {'us/launch':>10s} {'GB read':>8s} {'TB/s':>6s} {'of 8 TB/s':>9s}"]
    for name, frag, nbytes in CASES:
        ds = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-9 for r in rows if frag in r["Kernel_Name"]]
        k = seen.get(frag, 0)
        ds = ds[k:k + REPS]
        seen[frag] = k + REPS
        if len(ds) < REPS:
            lines.append(f"{name:62s} (only {len(ds)} launches of {frag} in the trace)")
            continue
        t = float(np.median(ds[2:]))
        lines.append(f"{name:62s} {t * 1e6:10.1f} {nbytes / 1e9:8.3f} {nbytes / t / 1e12:6.2f} {nbytes / t / HBM:9.2f}")
    return "\n".join(lines)


def steps():
    dev = torch.device("cuda:0")
    model, nm, enc = model_and_data(dev)
    mean, std = synthetic.cnt_norm(7)
    src = torch.from_numpy(synthetic.pose_windows(5, 8 * 64)).to(dev).reshape(64, 8, 60, 24, 15)
    banks = [(nm[c * 2048:(c + 1) * 2048], enc[c * 2048:(c + 1) * 2048]) for c in range(8)]
    out = []
    # the 8-stream captured step: one window per stream, stream k on character (k + step) % 8
    mb = MultiCharacterBank(model, banks)
    ms = MultiStreamCharacterizer(mb, mean, std, streams=8)
    ids = torch.arange(8, dtype=torch.int32, device=dev)
    lat = []
    for i in range(64 + 10):
        ms.input.copy_(src[i % 64]); ms.characters.copy_((ids + i) % 8)
        torch.cuda.synchronize()
        t0 = time.perf_counter(); ms.step(); torch.cuda.synchronize(); lat.append(time.perf_counter() - t0)
    lat = np.array(lat[10:]) * 1e3
    out.append(f"8-stream captured step (8 characters x 2048 rows, one bank): p50 {np.percentile(lat, 50):.3f} ms  p99 {np.percentile(lat, 99):.3f} ms")
    del ms, mb
    # today's alternative: 8 contexts, each its own current bank and captured per-window step, stepped one after another
    models = [Generator(device=dev).load_state_dict(synthetic_state_dict(1777, 1.0)).eval() for _ in range(8)]
    scs = [StreamingCharacterizer(ContextBank(models[c], *banks[c]), mean, std) for c in range(8)]
    lat = []
    for i in range(64 + 10):
        w = src[i % 64]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for k in range(8):
            scs[k].step(w[k])
        torch.cuda.synchronize(); lat.append(time.perf_counter() - t0)
    lat = np.array(lat[10:]) * 1e3
    out.append(f"8 contexts x StreamingCharacterizer, stepped in turn:          p50 {np.percentile(lat, 50):.3f} ms  p99 {np.percentile(lat, 99):.3f} ms")
    return "\n".join(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "bench_outputs", "multi_character"))
    ap.add_argument("--child-scan", action="store_true")
    ap.add_argument("--skip-scan", action="store_true")
    a = ap.parse_args()
    if a.child_scan:
        scan_cases()
        return
    os.makedirs(a.out, exist_ok=True)
    report = []
    if not a.skip_scan:
        report.append("(a) segmented scan, kernel trace (median of launches 3..%d)\n" % REPS + profile_scans(a.out))
    report.append("(b) streamed steps, host wall time per step incl. synchronisation (64 steps after 10 warm-up)\n" + steps())
    text = "\n\n".join(report)
    print(text)
    with open(os.path.join(a.out, "multi_character_bench.txt"), "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
