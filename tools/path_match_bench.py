"""Coherent context matching, measured: writes profiles/r23/path_match.json.

Shapes (queries x bank rows): 585 x 585, 1 024 x 4 096, 285 x 16 384, medians of 3 rounds of HIP-event timings:
  (a) the matrix (mocha_match_dist_matrix: the all-keys scan body, every group of 8 queries in one launch, and the unpack launch);
  (b) the same numbers through the only earlier route to them: the all-keys scan behind mocha_match_topk, ceil(Q / 8) bank passes;
  (c) the path launches (mocha_match_path) and the time per window;
  (d) the whole characterize with coherent= against the plain call (the pair route at 585 + 585, ContextBank.characterize otherwise).
Usage: python tools/path_match_bench.py [--out profiles/r23/path_match.json] [--rounds 3]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mocha_sigasia2023_amd import ContextBank, Generator, synthetic, weights  # noqa: E402

SHAPES = ((585, 585), (1024, 4096), (285, 16384))
D = 90 * 256


def timed(fn, rounds, inner=1):
    """Median over `rounds` of the mean time of `inner` calls, in milliseconds (one warm-up call first)."""
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(inner):
            fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) / inner)
    return statistics.median(out), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "r23", "path_match.json"))
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    model = Generator(layout="mixamo", device=dev).load_state_dict(weights.synthetic_state_dict(seed=1777, gain=1.0, layout="mixamo")).eval()
    mean, std = (torch.from_numpy(x).to(dev) for x in synthetic.cnt_norm(13))
    ptr = lambda t: C.c_void_p(t.data_ptr())      # noqa: E731
    st = lambda: C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)      # noqa: E731
    res = {"device": torch.cuda.get_device_name(0), "rounds": a.rounds, "shapes": []}
    for Q, N in SHAPES:
        g = torch.Generator(device=dev).manual_seed(Q + N)
        # a random-walk bank and queries that follow runs of it: the distances a path is meant for
        bank_nm = torch.cumsum(0.1 * torch.randn((N, D), generator=g, device=dev), 0)
        rows = (torch.arange(Q, device=dev) + N // 3) % N
        q = bank_nm[rows] + 6.66 * torch.randn((Q, D), generator=g, device=dev)
        enc = torch.randn((N, 90, 256), generator=g, device=dev)
        bank = ContextBank(model, bank_nm, enc, dec_cache=False)
        d = torch.empty((Q, N), dtype=torch.float32, device=dev)
        idx = torch.empty((Q, 1), dtype=torch.int32, device=dev)
        dist = torch.empty((Q, 1), dtype=torch.float32, device=dev)
        t_a = timed(lambda: model._ctx.call("mocha_match_dist_matrix", ptr(q), Q, C.c_int64(0), C.c_int64(N), ptr(d), C.c_int64(N), st()), a.rounds, 3)
        t_b = timed(lambda: model._ctx.call("mocha_match_topk", ptr(q), Q, 1, ptr(idx), ptr(dist), st()), a.rounds, 1)
        same = bool(torch.equal(d.min(1).values, dist[:, 0]))
        unit = float(d.min(1).values.median())
        # (c) mocha_match_path alone on the matrix (a) left in d: the start-bit, forward and backtrack launches and the list upload
        path = torch.empty((Q,), dtype=torch.int32, device=dev)
        pdist = torch.empty((Q,), dtype=torch.float32, device=dev)
        cont = torch.empty((Q,), dtype=torch.uint8, device=dev)
        seq = (C.c_int32 * 2)(0, Q)
        t_c = timed(lambda: model._ctx.call("mocha_match_path", ptr(d), Q, N, C.c_int64(N), seq, 1, None, 0, C.c_double(0.01 * unit), ptr(path),
                                            ptr(pdist), ptr(cont), st()), a.rounds, 3)
        hard = d.argmin(1)
        entry = {"Q": Q, "N": N, "matrix_ms": t_a[0], "matrix_ms_rounds": t_a[1], "topk_scan_ms": t_b[0], "topk_scan_ms_rounds": t_b[1],
                 "matrix_min_equals_topk_bits": same, "path_ms": t_c[0], "path_ms_rounds": t_c[1], "path_us_per_window": 1e3 * t_c[0] / Q, "jump": 0.01 * unit,
                 "non_continuations_hard": int(Q - 1 - (hard[1:] == hard[:-1] + 1).sum()), "non_continuations_path": int(Q - 1 - cont[1:].sum()),
                 "planted_rows_found_hard": int((hard == rows).sum()), "planted_rows_found_path": int((path == rows).sum())}
        del bank, enc
        # (d) the whole route on synthetic windows
        src = torch.from_numpy(synthetic.pose_windows(901, Q, model.V)).to(dev)
        if Q + N <= 1280:
            cha = torch.from_numpy(synthetic.pose_windows(902, N, model.V)).to(dev)
            plain = timed(lambda: model.characterize_pair(src, cha, mean, std), a.rounds, 1)
            coh = timed(lambda: model.characterize_pair(src, cha, mean, std, coherent=1.0), a.rounds, 1)
            entry.update(route="characterize_pair", plain_ms=plain[0], coherent_ms=coh[0])
        else:
            b2 = ContextBank(model, bank_nm, torch.zeros((N, 90, 256), device=dev))
            plain = timed(lambda: b2.characterize(src, mean, std), a.rounds, 1)
            coh = timed(lambda: b2.characterize(src, mean, std, coherent=1.0), a.rounds, 1)
            entry.update(route="ContextBank.characterize", plain_ms=plain[0], coherent_ms=coh[0])
            del b2
        print(json.dumps(entry), flush=True)
        res["shapes"].append(entry)
        del bank_nm, q, d
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
