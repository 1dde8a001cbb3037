"""Action-constrained segmented matching against the plain segmented matcher, on the shape of DESIGN.md 8.9: 8 characters x 2 048 rows
at D = 23 040, fp32 and bf16 banks, labels in runs of 128 rows (16 actions per character), 1 and 8 queries per character.

For every (bank, queries per character, admissible share) - share 1/16 (one action), 1/4 (four actions) and 1 (the all-labels mask) -
the device-event time of mocha_match_segmented_allow (k = 1) and, alternating in the same process, of mocha_match_segmented; the
admissible bytes computed from the shapes (blocks x admissible rows x D x bytes per value: what a scan that skips every inadmissible
workgroup has to read) and those bytes over the measured time as a share of 8 TB/s.  Nothing here is a threshold: DESIGN.md 8.15 says what
is expected and records what was measured.

    python tools/allow_match_bench.py [--reps 200] [--out profiles/r15/allow_match.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from mocha_sigasia2023_amd import Generator, MultiCharacterBank, synthetic_state_dict  # noqa: E402

D = 90 * 256
CHARS, ROWS, RUN = 8, 2048, 128
HBM = 8e12


def event_us(fn, reps):
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record()
        e1.synchronize()
        out.append(1e3 * e0.elapsed_time(e1))
    return np.asarray(out)


def stats(a):
    return {"p50_us": float(np.percentile(a, 50)), "p10_us": float(np.percentile(a, 10)), "p90_us": float(np.percentile(a, 90)), "n": int(len(a))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r15", "allow_match.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("allow_match_bench.py measures on the GPU: no ROCm device found")
    dev = torch.device("cuda:0")
    model = Generator(device=dev).load_state_dict(synthetic_state_dict(1777, 1.0)).eval()
    g = torch.Generator(device=dev); g.manual_seed(3)
    nm = torch.randn((CHARS * ROWS, D), device=dev, generator=g)
    labels = [(np.arange(ROWS) // RUN).astype(np.int32)] * CHARS
    res = {"shape": f"{CHARS} characters x {ROWS} rows, D = {D}, labels in runs of {RUN} rows ({ROWS // RUN} actions)",
           "timing": "HIP events around single calls; constrained and plain alternating in one process; p50 of --reps calls",
           "hbm_peak_bytes_per_s": HBM, "cases": []}
    for bf16 in (False, True):
        mb = MultiCharacterBank(model, [(nm[c * ROWS:(c + 1) * ROWS], nm[c * ROWS:(c + 1) * ROWS].view(-1, 90, 256)) for c in range(CHARS)],
                                bf16=bf16, dec_cache=False, labels=labels)
        bpv = 2 if bf16 else 4
        for per in (1, 8):
            Q = CHARS * per
            q = torch.randn((Q, D), device=dev, generator=g)
            ids = torch.arange(Q, dtype=torch.int32, device=dev) // per          # `per` queries of every character: one block per character
            plain = lambda: mb.query(q, ids)                                     # noqa: E731
            for share, mask in (("1/16", 1 << 3), ("1/4", 0b1111 << 4), ("1", (1 << 64) - 1)):
                n_adm = {"1/16": 1, "1/4": 4, "1": 16}[share] * RUN
                allow = torch.full((Q,), mask - (1 << 64) if mask >= 1 << 63 else mask, dtype=torch.int64, device=dev)
                cons = lambda: mb.query(q, ids, allow=allow)                     # noqa: E731
                for _ in range(a.warmup):
                    cons(); plain()
                torch.cuda.synchronize()
                d, i, ap_ = mb.query(q, ids, allow=allow, return_applied=True)
                assert bool((ap_ == 1).all()) and bool(((i[:, 0] // RUN) < 16).all())
                tc, tp = [], []
                for _ in range(a.reps):
                    tc.append(event_us(cons, 1)[0]); tp.append(event_us(plain, 1)[0])
                tc, tp = np.asarray(tc), np.asarray(tp)
                adm_bytes = CHARS * n_adm * D * bpv                              # one block per character, every admissible row once
                all_bytes = CHARS * ROWS * D * bpv
                e = {"bank": "bf16" if bf16 else "fp32", "queries_per_character": per, "admissible_share": share,
                     "constrained": stats(tc), "plain": stats(tp), "admissible_bytes": adm_bytes, "segment_bytes": all_bytes,
                     "constrained_share_of_hbm_peak": adm_bytes / (np.percentile(tc, 50) * 1e-6) / HBM,
                     "plain_share_of_hbm_peak": all_bytes / (np.percentile(tp, 50) * 1e-6) / HBM,
                     "constrained_over_plain_p50": float(np.percentile(tc, 50) / np.percentile(tp, 50))}
                res["cases"].append(e)
                print(json.dumps(e))
        del mb
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
