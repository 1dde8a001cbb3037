#!/usr/bin/env python3
"""bench.py — characterized frames/s of the MOCHA Generator hot path on MI355X.

Workload (BASELINE.json configs[1], SURVEY.md §8d "C2"): the demo pair — one source clip and
one character clip of 585 sixty-frame windows each (a 600-frame clip slid with step 1,
preprocess/generate_database.py:65-84), 15 channels per joint, fp32, synthetic N(0,1) z-scored poses, synthetic
weights of the reference architecture.  Joints: 22 by default — BASELINE.json quotes the metric "at T=60, 22 joints"
(the reference's 'mixamo' graph tables); `--joints 24` is the shipped 'mocha' model's layout (the two
differ only in the joint-level kernels; profiles/r01 holds both).

One step = one pass of the demo's NN ("cm_") pipeline over the pair
(test_fullframework.py:188-194, 271-277, 288-302, 438-443, 465-467), inputs resident in HBM:
    bank build : encode the character clip (mot_embedding, +pos_emb, encoder, cnt, z-score), row norms
    characterize: encode the source clip, z-score, exact 1-NN match against the bank, gather the
                  matched character features, decoder, to_mot  -> 585 characterized pose windows
and yields 585 characterized frames (one output pose per window, the [-1] slice).  By default the step runs through
mocha_characterize_pair (both clips share the mot_embedding / encoder / cnt launches; same arithmetic, bit-identical
output); --three-calls runs it as encode(cha) + ContextBank + characterize(src).

Multi-GPU (weak scaling, one process per GPU): every rank runs the same step on its own source
clip; the character clip and the cnt norm are owned by rank 0 and broadcast once over RCCL
before the timed region, and the character bank rank 0 builds from it is broadcast through the C ABI
(mocha_bank_broadcast: scatter + all-gather over xGMI; reported as bank_broadcast_ms); there is no
collective inside the timed region because windows are independent units.  `python bench.py --gpus N`
with N > 1 and no RANK in the environment spawns the N ranks itself (fresh child processes, started before
this process touches a GPU); under torch.distributed.run it reads RANK / LOCAL_RANK / WORLD_SIZE as usual.

Prints ONE JSON line on rank 0 (see the keys below).

A plain run (`--gpus N --steps K --warmup W`) does only what the headline needs: set-up, W warm-up steps, K timed steps, and the line
(`metric`, `value`, `unit`, `higher_is_better`, `dtype`, `ms_per_step` = milliseconds per timed step).  Every other record - sustained
timing, the other GEMM engines, the roofline leg and per-kernel figures, the matcher / streaming / mid-size / 24-joint records, the CPU
baseline, at N > 1 the C-ABI bank broadcast and the configs[3] sub-record; with `--workload bank4k` the index checksum and the pipelined
record - runs with `--full` only; its keys are null or absent otherwise.
`--dump-outputs DIR` writes what the last timed step returned (poses `Y`, matched indices `idx`) as DIR/<name>.npy; the inputs are
seeded, so two builds can be compared output for output.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

PEAK_F32_MFMA_TFLOPS = 157.3     # MI355X dense f32 MFMA peak (MI355X_MICROARCH.md, chip table)
PEAK_BF16_MFMA_TFLOPS = 16 * 157.3   # dense bf16 MFMA peak: the bf16 pipe runs 16 x the f32 MFMA rate per clock (same table: ~2.5 PF)
X3_PASSES = 6                    # bf16 MFMA passes per fp32 product in mocha_gemm_x3 (gemm_x3.hip)
PEAK_HBM_GBS = 8000.0
METRIC = {22: "characterized frames/sec (whole node) at T=60, 22 joints; 1/2/4/8 GPU",          # BASELINE.json "metric", verbatim
          24: "characterized frames/sec (whole node) at T=60, 24 joints (the shipped model's layout); 1/2/4/8 GPU"}


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--workload", default="demo", choices=("demo", "bank4k"),
                    help="demo: BASELINE configs[1] (default, the judged line); bank4k: configs[2]/[3], 1024 windows x 4096-entry bf16 bank, strong scaling")
    ap.add_argument("--windows", type=int, default=585, help="windows per clip (demo pair: 585)")
    ap.add_argument("--chunk", type=int, default=0, help="windows per internal chunk (0 = library default)")
    ap.add_argument("--joints", type=int, default=22, choices=(24, 22),
                    help="22 = BASELINE.json's metric (the reference's 'mixamo' layout); 24 = the shipped 'mocha' model")
    ap.add_argument("--full", action="store_true",
                    help="besides the headline, every other record: sustained timing with board power, the other GEMM engines, the roofline "
                         "leg with per-kernel figures, the matcher / streaming / mid-size / 24-joint records, the CPU baseline; at N > 1 the C-ABI "
                         "bank broadcast and the bank4k sub-record; with --workload bank4k the index checksum and the pipelined record "
                         "(--no-extras, --no-cpu-baseline, --no-bank4k and --sustained-s trim it)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write rank 0's outputs of the last timed step as DIR/<name>.npy (float32 / float64, at most 64 MB)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--three-calls", action="store_true",
                    help="run the step as encode(cha) + ContextBank + characterize(src) instead of the fused characterize_pair")
    ap.add_argument("--dual-stream", action="store_true",
                    help="add a second timing of the same step with the opt-in two-stream overlap (reported beside the headline, "
                         "never as it; off by default so that a rocprofv3 run of the default command sees only the headline kernels)")
    ap.add_argument("--cpu-sample", type=int, default=64, help="windows per clip of the CPU baseline leg's bounded sample (thread sweep, BASELINE.md section 3)")
    ap.add_argument("--cpu-full", type=int, default=-1, help="windows per clip of the ONE run of the full workload at the sweep's best configuration that cpu_baseline.value reports "
                    "(-1 = --windows, i.e. exactly the GPU workload: about 6 s at 585; 0 = skip it and report the best of the sample sweep)")
    ap.add_argument("--sustained-s", type=float, default=2.5, help="with --full: seconds of the extra back-to-back timing of the same step (0 = skip)")
    ap.add_argument("--launch-timeout", type=float, default=3600.0,
                    help="seconds after which `--gpus N`'s own launcher stops ranks that have not finished (0 = never)")
    ap.add_argument("--no-bank4k", action="store_true", help="N > 1 with --full: skip the configs[3] sub-record of the default line")
    ap.add_argument("--options", default="", help="context options for the measured model, name=value[,name=value...] (mocha_set_option); "
                    "recorded in config.options - e.g. gemm_f16x2=1 (the opt-in two-plane fp16 GEMM engine: NOT the default line's arithmetic)")
    ap.add_argument("--no-extras", action="store_true",
                    help="with --full: skip the extra records of the N=1 line (matcher roofline, bank4k, streaming)")
    return ap.parse_args()


def count_gpus():
    """GPUs visible to a process with this environment, counted by a short-lived CHILD (torch.cuda.device_count() there):
    the count honours *_VISIBLE_DEVICES and container device filtering exactly, and whatever the child initialises dies
    with it - this process makes no HIP call."""
    import subprocess
    out = subprocess.run([sys.executable, "-c", "import torch; print(torch.cuda.device_count())"], capture_output=True, text=True)
    try:
        return int(out.stdout.strip().splitlines()[-1])
    except (ValueError, IndexError):
        raise SystemExit(f"bench.py: could not count GPUs: {out.stderr.strip()[-300:]}")


def watch_ranks(procs, tails, timeout_s=0.0, poll_s=0.2, grace_s=5.0, err=sys.stderr):
    """Wait for the rank processes with a watchdog.  All exit 0 -> 0.  The FIRST rank that exits non-zero (or the deadline, if
    `timeout_s` > 0) ends the job: the others - which would otherwise sit in a barrier or a collective until its timeout - are sent
    SIGTERM, then SIGKILL after `grace_s`; the failing rank's stderr tail (`tails[r]`: its last lines) is printed and its code
    returned.  Only processes this launcher started are signalled, by their exact PIDs."""
    t0 = time.monotonic()
    bad = None
    while True:
        rcs = [p.poll() for p in procs]
        bad = next(((r, rc) for r, rc in enumerate(rcs) if rc not in (None, 0)), None)
        if bad or all(rc == 0 for rc in rcs):
            break
        if timeout_s > 0 and time.monotonic() - t0 > timeout_s:
            bad = (-1, 124)
            break
        time.sleep(poll_s)
    if not bad:
        return 0
    r, rc = bad
    alive = [p for p in procs if p.poll() is None]
    for p in alive:
        p.terminate()
    t1 = time.monotonic()
    while any(p.poll() is None for p in alive) and time.monotonic() - t1 < grace_s:
        time.sleep(0.05)
    for p in alive:
        if p.poll() is None:
            p.kill()
    for p in alive:
        p.wait()
    if r < 0:
        print(f"bench.py: ranks did not finish within {timeout_s:.0f} s; stopped {len(alive)} rank(s)", file=err, flush=True)
    else:
        print(f"bench.py: rank {r} exited with status {rc}; stopped the other {len(alive)} rank(s).  Its last stderr lines:", file=err)
        for line in list(tails[r]) if tails else []:
            print(f"  [rank {r}] {line}", file=err)
        err.flush()
    return abs(rc) or 1


def spawn_ranks(a):
    """`python bench.py --gpus N` without a launcher: start N fresh ranks of this script (RANK / LOCAL_RANK / WORLD_SIZE /
    MASTER_* set, rendezvous over 127.0.0.1) and watch them (watch_ranks: a rank that dies ends the job at once, with its stderr
    tail, instead of leaving the others in a collective until its timeout).  The children are new processes, not re-execs of
    this one, and this process never uses a GPU: devices are counted by a child process too (torch.cuda.device_count() may fall
    back to hipGetDeviceCount, which initialises the runtime)."""
    import collections
    import socket
    import subprocess
    import threading
    n_dev = a.gpus if os.environ.get("MOCHA_BENCH_ONE_GPU") == "1" else count_gpus()      # test hook: every rank on GPU 0
    if a.gpus > n_dev:
        raise SystemExit(f"bench.py --gpus {a.gpus}: this node exposes {n_dev} GPU(s)")
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    procs, tails, pumps = [], [], []

    def pump(pipe, tail):                 # the rank's stderr goes through to ours, and its last lines are kept for the watchdog
        for line in pipe:
            sys.stderr.write(line); sys.stderr.flush()
            tail.append(line.rstrip("\n"))
    for r in range(a.gpus):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(a.gpus), MASTER_ADDR="127.0.0.1",
                   MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
        p = subprocess.Popen([sys.executable, os.path.abspath(__file__)] + sys.argv[1:], env=env, stderr=subprocess.PIPE, text=True)
        tail = collections.deque(maxlen=40)
        t = threading.Thread(target=pump, args=(p.stderr, tail), daemon=True)
        t.start()
        procs.append(p); tails.append(tail); pumps.append(t)
    rc = watch_ranks(procs, tails, timeout_s=a.launch_timeout)
    for t in pumps:
        t.join(timeout=2.0)
    raise SystemExit(rc)


def strip_c_comments(text):
    """C / C++ source without its comments (string and character literals are kept as they are) and with every run of white space
    collapsed to one blank: two sources that compile to the same code - differing in comments, indentation or line breaks only - map
    to the same text."""
    out, i, n = [], 0, len(text)
    while i < n:
        c = text[i]
        if c == "/" and i + 1 < n and text[i + 1] == "/":
            j = text.find("\n", i)
            i = n if j < 0 else j
        elif c == "/" and i + 1 < n and text[i + 1] == "*":
            j = text.find("*/", i + 2)
            i = n if j < 0 else j + 2
            out.append(" ")
        elif c in "\"'":
            j = i + 1
            while j < n and text[j] != c:
                j += 2 if text[j] == "\\" else 1
            out.append(text[i:j + 1])
            i = j + 1
        else:
            out.append(c)
            i += 1
    return " ".join("".join(out).split())


def kernel_source_sha16():
    """Hash of what the GPU runs: the library's sources (csrc/*.hip, *.h, the host dispatch in mocha_api.cpp - which kernels and shapes a
    step launches is decided there - and include/mocha_hip.h) WITHOUT comments and white-space layout (strip_c_comments), so that a
    comment fix does not void a committed PMC summary (round 5 re-ran three profile passes for comment-only edits).
    tools/pmc_traffic.sh writes the hash into the traffic summary it produces, and the bench quotes PMC traffic only from a summary
    whose hash matches the sources of the library it is running."""
    import glob, hashlib
    h = hashlib.sha256()
    csrc = os.path.join(ROOT, "mocha_sigasia2023_amd", "csrc")
    for f in sorted(glob.glob(os.path.join(csrc, "*.hip")) + glob.glob(os.path.join(csrc, "*.h")) + glob.glob(os.path.join(csrc, "*.cpp"))
                    + [os.path.join(ROOT, "include", "mocha_hip.h")]):
        h.update(os.path.basename(f).encode())
        h.update(strip_c_comments(open(f, encoding="utf-8", errors="replace").read()).encode())
    return h.hexdigest()[:16]


def pmc_traffic_for(kernel_name):
    """HBM-side bytes per launch of `kernel_name` from the committed rocprofv3 PMC summary (separate
    --pmc FETCH_SIZE / WRITE_SIZE passes, read side x2 on gfx950; tools/pmc_traffic.sh).  (None, reason) if there is no
    summary, or if the newest one was measured on other kernel sources than the ones in the tree (its `# kernel_source_sha16`
    line): a kernel change must not keep quoting the old counters."""
    import glob, re
    files = sorted(glob.glob(os.path.join(ROOT, "profiles", "r*", "*pmc_traffic_summary.txt")))
    if not files:
        return None, "no committed PMC traffic summary"
    rel = os.path.relpath(files[-1], ROOT)
    text = open(files[-1]).read()
    m = re.search(r"^# kernel_source_sha16: (\w+)", text, re.M)
    now = kernel_source_sha16()
    if not m or m.group(1) != now:
        return None, (f"stale: {rel} was measured on kernel sources {m.group(1) if m else '(unrecorded)'}, the tree is {now}; "
                      "re-run tools/pmc_traffic.sh")
    key = re.sub(r"[ ,]", "", kernel_name.split("<")[0] + "<" + kernel_name.split("<")[1]) if "<" in kernel_name else kernel_name
    tot, n = 0.0, 0
    for line in text.splitlines():
        flat = re.sub(r"[ ,]", "", line)
        if key in flat:
            mm = re.search(r"\)\s+(\d+)\s+([\d.]+)\s+([\d.]+)\s*$", line)
            if mm:                                      # every template instance of the kernel, weighted by its launches
                tot += int(mm.group(1)) * (float(mm.group(2)) + float(mm.group(3))) * 1e6
                n += int(mm.group(1))
    if n:
        return tot / n, f"from profile: {rel} (rocprofv3 --pmc passes of this command on these kernel sources, committed; PMC counters cannot be read inside this process)"
    return None, f"{rel} has no line for {kernel_name}"


def dist_device_and_backend(local):
    """(device index, torch.distributed backend) of this rank.  Default: GPU `local`, "nccl" (= RCCL on ROCm).  Two test
    hooks let tests/test_multirank_standin.py run several ranks of this script on a one-GPU box: MOCHA_BENCH_ONE_GPU=1 puts
    every rank on GPU 0 and MOCHA_BENCH_BACKEND=gloo moves the side-channel collectives to the CPU (real RCCL refuses two
    ranks on one device; the C-ABI bank broadcast then runs over the library named by MOCHA_RCCL_LIBRARY)."""
    return (0 if os.environ.get("MOCHA_BENCH_ONE_GPU") == "1" else local), os.environ.get("MOCHA_BENCH_BACKEND", "nccl")


class PowerSampler:
    """Board power and shader clock of GPU 0 as rocm-smi reports them (read-only; nothing is set), sampled from a thread while a timed region
    runs: `with PowerSampler() as ps: ...; ps.record()`.  Any failure (no rocm-smi, another output format) leaves an empty record - the
    measurement never depends on it."""
    def __init__(self, period_s=0.15):
        self.period, self.samples, self._stop, self._th = period_s, [], False, None

    @staticmethod
    def read():
        import re, subprocess
        try:
            t = subprocess.run(["rocm-smi", "--showpower", "--showclocks", "--showmaxpower"], capture_output=True, text=True, timeout=5).stdout
        except Exception:                                  # noqa: BLE001
            return {}
        out = {}
        for line in t.splitlines():
            m = re.search(r"GPU\[0\].*Power \(W\):\s*([\d.]+)", line)
            if m:
                out["cap_w" if "Max" in line else "power_w"] = float(m.group(1))
            m = re.search(r"GPU\[0\].*sclk clock level.*\((\d+)Mhz\)", line)
            if m:
                out["sclk_mhz"] = float(m.group(1))
        return out

    def _run(self):
        while not self._stop:
            r = self.read()
            if r:
                self.samples.append(r)
            time.sleep(self.period)

    def __enter__(self):
        import threading
        self._th = threading.Thread(target=self._run, daemon=True)
        self._th.start()
        return self

    def __exit__(self, *exc):
        self._stop = True
        if self._th:
            self._th.join(timeout=10)

    def record(self):
        pw = [x["power_w"] for x in self.samples if "power_w" in x]
        ck = [x["sclk_mhz"] for x in self.samples if "sclk_mhz" in x]
        cap = [x["cap_w"] for x in self.samples if "cap_w" in x]
        if not pw:
            return {"samples": 0, "note": "rocm-smi gave no power reading here"}
        return {"samples": len(pw), "avg_w": sum(pw) / len(pw), "max_w": max(pw), "cap_w": cap[0] if cap else None,
                "frac_of_cap": (sum(pw) / len(pw) / cap[0]) if cap and cap[0] else None,
                "avg_sclk_mhz": sum(ck) / len(ck) if ck else None,
                "note": "rocm-smi (read-only) sampled while the sustained region ran: the step is power-bound (DESIGN.md section 8.1)"}


def cpu_model_name():
    try:
        with open("/proc/cpuinfo") as f:
            for line in f:
                if line.lower().startswith("model name"):
                    return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown"


def cpu_baseline(sd, V, n, mean, std, full=0):
    """The oracle (CPU restatement of the reference path, same op sequence on torch CPU) timed on the GPU box's host cores, per
    BASELINE.md section 3 (the reference's only timing code is model.py:311-318): a thread sweep with warm-up and medians on a BOUNDED
    sample of the same step (n source + n character windows: encode both, 1-NN match, decode, to_mot), at the encode / decode batch the
    reference's own scripts use (32, collect_CVAE_feature_action.py:167) and with the whole clip as one batch at the best thread count.
    Every configuration is in `sweep`; one thread runs a quarter of the sample (it is ~10x slower).  full > 0 (the default: the GPU
    workload's own 585 + 585 windows): one run of `full` + `full` windows at the sweep's best configuration - THAT is `value`, so that
    speedup_vs_cpu compares equal workloads; full = 0: `value` is the best median of the sample sweep."""
    from oracle import mocha_oracle as O      # checker / baseline only
    from mocha_sigasia2023_amd import synthetic
    tsd = O.to_torch_state(sd)
    src = torch.from_numpy(synthetic.pose_windows(901, max(n, full), V))
    cha = torch.from_numpy(synthetic.pose_windows(902, max(n, full), V))
    ncpu = os.cpu_count() or 1
    threads0 = torch.get_num_threads()
    counts = sorted({t for t in (1, 8, 16, 32, 64, threads0) if 1 <= t <= max(threads0, 1)})

    def timed(nw, batch, reps):
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            O.characterize(tsd, src[:nw], cha[:nw], mean, std, batch=batch)
            ts.append(time.perf_counter() - t0)
        return float(np.median(ts))

    sweep = []
    t_all = time.perf_counter()
    with torch.no_grad():
        for t in counts:
            torch.set_num_threads(t)
            nw = max(8, n // 4) if t == 1 else n
            for _ in range(3):                                    # warm-up: oneDNN primitive caches, thread pool at this size
                O.characterize(tsd, src[:8], cha[:8], mean, std, batch=8)
            dt = timed(nw, 32, 3)
            sweep.append({"threads": t, "batch": 32, "windows": nw, "median_s": dt, "frames_per_s": nw / dt})
        best = max(sweep, key=lambda r: r["frames_per_s"])
        torch.set_num_threads(best["threads"])
        dt = timed(n, n, 3)                                       # the whole clip as one batch (test_fullframework.py:190-192 encodes a clip at once)
        sweep.append({"threads": best["threads"], "batch": n, "windows": n, "median_s": dt, "frames_per_s": n / dt})
        best = max(sweep, key=lambda r: r["frames_per_s"])
        rec_full = None
        if full > 0:
            torch.set_num_threads(best["threads"])
            t0 = time.perf_counter()
            O.characterize(tsd, src[:full], cha[:full], mean, std, batch=min(best["batch"], full))
            dtf = time.perf_counter() - t0
            rec_full = {"windows": full, "seconds": dtf, "frames_per_s": full / dtf, "threads": best["threads"], "batch": best["batch"]}
    torch.set_num_threads(threads0)
    out = {"value": rec_full["frames_per_s"] if rec_full else best["frames_per_s"], "unit": "frames/s", "cores": best["threads"], "kind": "port",
           "sample": (f"value: ONE run of the full workload, {full} src + {full} cha windows, at the sweep's best configuration "
                      f"({best['threads']} threads, batch {min(best['batch'], full)}; {rec_full['seconds']:.1f} s).  Sweep: " if rec_full else "") +
                     f"{n} src + {n} cha windows through the same step (encode both, 1-NN match, decode, to_mot), torch-CPU oracle; best of a "
                     f"thread sweep {counts} at batch 32 plus the whole clip as one batch, 3 warm-up + median of 3 each ({time.perf_counter() - t_all:.0f} s "
                     f"in all); one thread on {max(8, n // 4)} + {max(8, n // 4)} windows",
           "best": {"threads": best["threads"], "batch": best["batch"]}, "sweep": sweep, "sweep_best_frames_per_s": best["frames_per_s"],
           "single_thread_frames_per_s": next(r["frames_per_s"] for r in sweep if r["threads"] == counts[0]),
           "cpu_model": cpu_model_name(), "os_cpu_count": ncpu, "torch_default_threads": threads0}
    if rec_full:
        out["full_workload"] = rec_full
    return out


# CRC-32 of the 1024 matched bank rows of the bank4k workload on ONE GPU (`python bench.py --workload bank4k`, synthetic seeds 1 / 2 / 7).
# The search is exact over the rounded bank, so an N-way split must reproduce the N = 1 answer OF THE SAME BUILD - but the value depends on
# the encoder's last bits (a near-tie flips with any legitimate numeric change), so it is INFORMATIONAL and keyed by the kernel sources' hash:
# `idx_matches_n1` is None unless the running library was built from exactly those sources.  The binding checks are
# tests/test_multirank_standin.py (N-rank CRC == a 1-rank run of the same build) and test_fullsize_parity.py (indices vs float64 search).
BANK4K_IDX_CRC32_N1 = {"545d209a9ac5cbed": {22: 4269089464, 24: 2772088534},      # profiles/r04/h_bank4k_v2{2,4}.json
                       "58ae42e49ecb4b74": {22: 4269089464, 24: 2772088534},      # profiles/r05/k_bank4k_v2{2,4}.json (unchanged by round 5's numerics)
                       "ad527b6ce6c3a29e": {22: 4269089464, 24: 2772088534},      # + pair_overlap host change
                       "4701c3d0797f58db": {22: 4269089464, 24: 2772088534},      # profiles/r05/q_bank4k_v2{2,4}.json
                       "776b690774403d41": {22: 4269089464, 24: 2772088534},      # + the opt-in gemm_h2.hip: profiles/r05/t_bank4k_v2{2,4}.json
                       "147d1ee70460bdde": {22: 4269089464, 24: 2772088534},      # profiles/r05/v_bank4k_v2{2,4}.json
                       "fe2e96e1e7691a5b": {22: 4269089464, 24: 2772088534},      # profiles/r05/w_bank4k_v2{2,4}.json
                       "cabe9d3fdec0f1e1": {22: 4269089464, 24: 2772088534},      # the final tree (w + comment fixes): profiles/r05/y_bank4k_v22.json
                       # round 6: the hash is over comment-stripped sources from here on (a comment fix no longer changes it)
                       "1418133355060f3c": {22: 4269089464, 24: 2772088534},      # round 6, first final pass
                       "74fcf8fc34e8e0df": {22: 4269089464, 24: 2772088534},      # round 6, second pass
                       "b40f0f8fc81d8e50": {22: 4269089464, 24: 2772088534},      # round 6, third pass
                       "29b99de141e943c4": {22: 4269089464, 24: 2772088534}}      # profiles/r06/final_bank4k_v2{2,4}.json (the committed tree)
XGMI_LINK_GBS = 153.0            # one xGMI link, one direction (MI355X: 7 links per GPU, point-to-point)


def parse_options(text):
    out = {}
    for kv in filter(None, (text or "").split(",")):
        k, v = kv.split("=")
        out[k.strip()] = int(v)
    return out


DUMP_LIMIT_BYTES = 64 * 10**6 - (1 << 16)      # --dump-outputs: 64 MB in all, the .npy headers included


def dump_outputs(path, **arrays):
    """`--dump-outputs`: every array as <path>/<name>.npy - float32 stays float32, anything else becomes float64 (integer indices are exact
    there).  If they come to more than DUMP_LIMIT_BYTES together, the largest one keeps a fixed, seeded sample of its rows (first axis), in
    ascending order, and the sampled row numbers are written as <name>_rows.npy: the same arguments give the same sample."""
    os.makedirs(path, exist_ok=True)
    host = {}
    for k, v in arrays.items():
        v = v.detach().cpu().numpy() if torch.is_tensor(v) else np.asarray(v)
        host[k] = np.ascontiguousarray(v, dtype=np.float32 if v.dtype == np.float32 else np.float64)
    total = sum(v.nbytes for v in host.values())
    if total > DUMP_LIMIT_BYTES:
        big = max(host, key=lambda k: host[k].nbytes)
        n = host[big].shape[0]
        row_bytes = host[big].nbytes // n + 8                     # + the row number itself, float64
        keep = (DUMP_LIMIT_BYTES - (total - host[big].nbytes)) // row_bytes
        if keep < 1:
            raise SystemExit(f"bench.py --dump-outputs: the outputs other than {big!r} already exceed {DUMP_LIMIT_BYTES} bytes")
        rows = np.sort(np.random.default_rng(0).choice(n, size=keep, replace=False))
        host[big] = np.ascontiguousarray(host[big][rows])
        host[big + "_rows"] = rows.astype(np.float64)
    for k, v in host.items():
        np.save(os.path.join(path, k + ".npy"), v)


def comm_record(model, backend, world):
    """The `rccl` record of an N > 1 line: what the C ABI's communicator REALLY is on every rank (mocha_comm_info: ncclCommCount,
    ncclGetVersion, the file the entry points came from, device and PCI bus id), gathered over the side channel - plus every
    test hook that is set in the environment, so that a stray variable cannot pass silently."""
    from mocha_sigasia2023_amd import distributed as D
    mine = D.comm_info(model)
    infos = [None] * world
    if torch.distributed.is_initialized() and world > 1:
        torch.distributed.all_gather_object(infos, mine)
    else:
        infos = [mine]
    libs = sorted({i["library"] for i in infos})
    hooks = {k: os.environ[k] for k in ("MOCHA_RCCL_LIBRARY", "MOCHA_BENCH_ONE_GPU", "MOCHA_BENCH_BACKEND", "MOCHA_FORCE_DIST") if k in os.environ}
    return {"nranks": infos[0]["nranks"], "nranks_agree": all(i["nranks"] == world for i in infos),
            "rccl_version": infos[0]["rccl_version"], "rccl_version_code": infos[0]["rccl_version_code"],
            "library": libs[0] if len(libs) == 1 else libs,
            "is_test_standin": any(i["rccl_version_code"] < 10000 for i in infos),
            "distinct_devices": len({i["pci_bus_id"] for i in infos}),
            "per_rank": [{"rank": i["rank"], "device": i["device"], "pci_bus_id": i["pci_bus_id"]} for i in infos],
            "torch_side_channel_backend": backend, "test_hooks_in_env": hooks}


def pipelined_pair_record(a, sd, layout, dev, V, W, src, cha, mean, std, contexts=2):
    """Extra (never the headline): the SAME demo step with consecutive steps overlapped - `contexts` Generators on their own streams take the
    steps in turn (independent steps; include/mocha_hip.h: several contexts of one process may be driven concurrently).  K steps are K steps;
    only their kernels interleave."""
    from mocha_sigasia2023_amd import Generator
    models = [Generator(layout=layout, device=dev).load_state_dict(sd).eval() for _ in range(contexts)]
    streams = [torch.cuda.Stream(device=dev) for _ in range(contexts)]
    def run(n):
        for i in range(n):
            with torch.cuda.stream(streams[i % contexts]):
                models[i % contexts].characterize_pair(src, cha, mean, std)
    with torch.no_grad():
        run(2 * contexts); torch.cuda.synchronize()
        t0 = time.perf_counter(); run(a.steps); torch.cuda.synchronize(); dt = time.perf_counter() - t0
    del models
    return {"contexts": contexts, "value": W * a.steps / dt, "ms_per_step": dt / a.steps * 1e3,
            "note": "consecutive demo steps on alternating contexts / streams; the headline runs them one after the other"}


def projected_scaling_record(a, model, dev, V, sd=None, layout=None):
    """N = 1 line only: what one GPU of the FINAL tree does with every per-rank share of BASELINE configs[3] (the 1024 windows of seed 1
    against the 4096-entry bf16 bank: 1024 / 512 / 256 / 128 windows = the shares at N = 1 / 2 / 4 / 8), measured back to back on this GPU,
    and the strong-scaling figures that follow from them if nothing else changes (no collective inside a step; the bank broadcast is a
    one-time set-up cost and is MODELLED here: scatter + all-gather, 153 GB/s per xGMI link and direction).  A projection, not a measurement
    of N GPUs: the driver's SCALE run is the measurement.  Also the weak-scaled headline's counterpart: the demo step's per-rank work does
    not change with N, so its projection is N x this line's value."""
    from mocha_sigasia2023_amd import ContextBank, synthetic
    NB, W = 4096, 1024
    full = torch.from_numpy(synthetic.pose_windows(1, W, V)).to(dev)
    m0, s0 = synthetic.cnt_norm(7)
    with torch.no_grad():
        _, cnt_all, _ = model.encode(full, torch.from_numpy(m0).to(dev), torch.from_numpy(s0).to(dev))
        mean = cnt_all.mean(dim=0).contiguous()
        std = (cnt_all.std(dim=0).clamp_min(1e-6) / torch.from_numpy(synthetic.temporal_weight(15, 6, 256)).to(dev)).contiguous()
        del cnt_all
        g = torch.Generator(device=dev); g.manual_seed(2)
        bank_nm = torch.randn((NB, 90 * 256), device=dev, generator=g)
        bank_enc = torch.randn((NB, 90, 256), device=dev, generator=g)
        bank = ContextBank(model, bank_nm, bank_enc, bf16=True)
        pipe = None
        if sd is not None:
            from mocha_sigasia2023_amd import BatchPipeline
            pipe = BatchPipeline(sd, bank_nm, bank_enc, layout=layout, device=dev, contexts=3, bf16=True, options=parse_options(a.options))
        shares = {}
        for n_gpus in (1, 2, 4, 8):
            share = W // n_gpus
            src = full[:share].contiguous()
            for _ in range(2):
                bank.characterize(src, mean, std)
            torch.cuda.synchronize(); t0 = time.perf_counter()
            reps = max(5, a.steps // 2)
            for _ in range(reps):
                bank.characterize(src, mean, std)
            torch.cuda.synchronize(); dt = (time.perf_counter() - t0) / reps
            bank_bytes = 2 * NB * 90 * 256 * 4
            shares[str(n_gpus)] = {"windows_per_gpu": share, "ms_per_step": dt * 1e3, "frames_per_s_per_gpu": share / dt,
                                   "projected_whole_job_frames_per_s": n_gpus * share / dt,
                                   "modelled_bank_broadcast_ms": (2.0 * bank_bytes / n_gpus / (XGMI_LINK_GBS * 1e9) * 1e3) if n_gpus > 1 else 0.0}
            if pipe is not None:                       # the same share with consecutive steps overlapped on three contexts (BatchPipeline)
                for _ in range(6):
                    pipe.characterize(src, mean, std)
                torch.cuda.synchronize(); t0 = time.perf_counter()
                for _ in range(3 * reps):
                    pipe.characterize(src, mean, std)
                torch.cuda.synchronize(); dtp = (time.perf_counter() - t0) / (3 * reps)
                shares[str(n_gpus)]["pipelined_3_contexts"] = {"ms_per_step": dtp * 1e3, "frames_per_s_per_gpu": share / dtp,
                                                               "projected_whole_job_frames_per_s": n_gpus * share / dtp}
        del bank, bank_nm, bank_enc, full, pipe
    base = shares["1"]["projected_whole_job_frames_per_s"]
    for k, v in shares.items():
        v["projected_strong_scaling_efficiency"] = v["projected_whole_job_frames_per_s"] / (int(k) * base)
        if "pipelined_3_contexts" in v:
            v["pipelined_3_contexts"]["projected_strong_scaling_efficiency_vs_serial_n1"] = v["pipelined_3_contexts"]["projected_whole_job_frames_per_s"] / (int(k) * base)
    return {"workload": "BASELINE configs[3]: 1024 windows x 4096-entry bank (bf16 cnt) split over N GPUs, per-rank share run on THIS GPU",
            "is_projection_from_one_gpu": True, "by_n_gpus": shares,
            "note": "per-rank step time of each share measured on one GPU of this tree; whole-job = N x share / time (no in-step collective); the "
                    "bank broadcast (755 MB fp32 rows + entries, scatter + all-gather) is modelled at 153 GB/s per link and paid once; "
                    "pipelined_3_contexts: the same shares with consecutive steps overlapped on three contexts / streams (BatchPipeline) - "
                    "a mid-size step is a latency chain that leaves most of the chip idle, independent steps fill each other's gaps"}


def bank4k_record(a, model, dev, V, rank, world, backend, sd=None, layout=None, dump_dir=None):
    """BASELINE configs[2] / [3]: 1024 synthetic source windows against a 4096-entry character bank stored bf16 for matching; with N
    GPUs the windows are split by shard_bounds (128 per GPU at N = 8: strong scaling) and rank 0's bank reaches every rank
    through the C ABI (mocha_bank_broadcast: RCCL scatter + all-gather over xGMI), timed on its own.  One step = encode, z-score, 1-NN
    (bf16 MFMA), gather, decoder, to_mot; no collective inside it.  Collective over the ranks; the record comes back on rank 0."""
    import zlib
    from mocha_sigasia2023_amd import ContextBank, distributed as D, synthetic
    NB, W = 4096, 1024
    dist_on = torch.distributed.is_initialized()
    lo, hi = D.shard_bounds(W, world, rank)
    full = torch.from_numpy(synthetic.pose_windows(1, W, V)).to(dev)
    src = full[lo:hi].contiguous()
    # cnt_mean / cnt_std as the reference makes them: statistics of the data's own cnt features per (token, channel), std divided by the
    # temporal weight (compute_cnt_norm.py:155-179, test_fullframework.py:73-76,89).  With arbitrary numbers instead, the z-scored
    # queries of a random-weight network are one tight cluster and every window matches the same bank row; standardised by their own
    # statistics they spread like the N(0,1) bank they are matched against.  Set-up, untimed, the same on every rank.
    m0, s0 = synthetic.cnt_norm(7)
    with torch.no_grad():
        _, cnt_all, _ = model.encode(full, torch.from_numpy(m0).to(dev), torch.from_numpy(s0).to(dev))
        mean = cnt_all.mean(dim=0).contiguous()
        std = (cnt_all.std(dim=0).clamp_min(1e-6) / torch.from_numpy(synthetic.temporal_weight(15, 6, 256)).to(dev)).contiguous()
        del full, cnt_all
    g = torch.Generator(device=dev); g.manual_seed(2)
    bank_nm = bank_enc = None
    if rank == 0:
        bank_nm = torch.randn((NB, 90 * 256), device=dev, generator=g)
        bank_enc = torch.randn((NB, 90, 256), device=dev, generator=g)
    bank = ContextBank(model, bank_nm, bank_enc, bf16=True) if rank == 0 else None
    bcast = None
    if dist_on:
        # the bank travels through the C ABI: mocha_bank_broadcast (scatter + all-gather over RCCL / xGMI), fp32 rows + fp32 entries;
        # every rank derives the bf16 copy, centroid and norms itself.  Twice: the first call also allocates the receivers' buffers
        # and warms RCCL's channels up, the second is the steady-state transfer.
        D.init_comm(model)
        times = []
        for _ in range(2):
            torch.cuda.synchronize(); D.barrier()
            t0 = time.perf_counter()
            got = D.bank_broadcast(model, bank, NB, root=0, bf16=True)
            torch.cuda.synchronize()
            times.append(D.max_over_ranks((time.perf_counter() - t0) * 1e3, dev))
        bank = got
        moved = 2 * NB * 90 * 256 * 4                    # bytes every non-root rank receives (cnt_nm + encoded, fp32)
        gbs = moved / (times[1] * 1e-3) / 1e9
        inbound = (world - 1) * XGMI_LINK_GBS            # what a rank's xGMI links to its peers can take in at once
        bcast = {"ms_first_call": times[0], "ms": times[1], "bytes_per_rank": moved, "GB/s_per_rank": gbs,
                 "xgmi_inbound_peak_GB/s": inbound, "frac_of_xgmi_inbound_peak": (gbs / inbound) if inbound > 0 else None,
                 "xgmi_links_per_gpu_peak_GB/s": 7 * XGMI_LINK_GBS,
                 "algorithm_bound_GB/s": world * XGMI_LINK_GBS / 2,
                 "note": "scatter (root -> rank r: bytes / N over its own link) + all-gather (every rank takes bytes / N from each peer); with "
                         "direct links both phases move bytes / N per link, so the algorithm's own ceiling is N x 153 / 2 GB/s per rank; includes "
                         "the header handshake (one stream synchronisation) and the receivers' derived data (bf16 copy, centroid, norms)"}
    with torch.no_grad():
        for _ in range(a.warmup):
            bank.characterize(src, mean, std)
        torch.cuda.synchronize(); D.barrier(); torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.steps):
            Y, idx = bank.characterize(src, mean, std, return_index=True)
        torch.cuda.synchronize(); D.barrier(); torch.cuda.synchronize()
        my = time.perf_counter() - t0
        elapsed = D.max_over_ranks(my, dev)
    per_rank = [(hi - lo) * a.steps / my]
    if dist_on and world > 1:
        vals = [None] * world
        torch.distributed.all_gather_object(vals, per_rank[0])
        per_rank = [float(v) for v in vals]
    if dump_dir and rank == 0:
        dump_outputs(dump_dir, Y=Y, idx=idx)
    checks = {}
    if a.full:
        # after the timed region: every rank's indices, in window order, as one checksum - the N-way split must reproduce the 1-GPU one
        idx_all = D.all_gather_rows(idx, W).cpu().numpy().astype(np.int32)
        y_abs = D.max_over_ranks(float(Y.abs().max()), dev)
        # ... and a per-window fingerprint of the poses (sum |Y| of 16 windows spread over all shards): a split that mixed windows up
        # would keep the index CRC when the indices happen to coincide, not this
        fp_all = D.all_gather_rows(Y.abs().sum(dim=(1, 2, 3)), W).cpu().numpy()
        crc = zlib.crc32(idx_all.tobytes())
        known = BANK4K_IDX_CRC32_N1.get(kernel_source_sha16(), {}).get(V)
        checks = {"idx_crc32": crc, "idx_crc32_n1_known": known, "idx_matches_n1": (crc == known) if known is not None else None,
                  "idx_head": idx_all[:8].tolist(), "idx_distinct": int(len(np.unique(idx_all))),
                  "max_abs_Y": y_abs, "y_fingerprint": [float(v) for v in fp_all[:: W // 16][:16]]}
    # extra: the same per-rank share with consecutive steps overlapped on three contexts / streams (BatchPipeline over the bank every rank
    # now holds); the poses of the last step must equal the serial ones
    pipelined = None
    if a.full and sd is not None and not os.environ.get("MOCHA_BENCH_NO_PIPELINE"):
        from mocha_sigasia2023_amd import BatchPipeline
        pipe, perr = None, None
        with torch.no_grad():
            try:                                      # set-up is local: a failure on one rank must not leave the others in a barrier
                p_nm, p_enc = bank.tensors()
                pipe = BatchPipeline(sd, p_nm, p_enc, layout=layout, device=dev, contexts=3, bf16=True, options=parse_options(a.options))
                for _ in range(6):
                    pipe.characterize(src, mean, std)
                torch.cuda.synchronize()
            except Exception as e:                    # noqa: BLE001  (reported in the record, the headline and the serial record stand)
                perr = f"rank {rank}: {type(e).__name__}: {e}"
            bad = D.max_over_ranks(0.0 if perr is None else 1.0, dev)
            if bad == 0.0:
                D.barrier(); torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(3 * a.steps):
                    Yp = pipe.characterize(src, mean, std)
                torch.cuda.synchronize(); D.barrier(); torch.cuda.synchronize()
                e_p = D.max_over_ranks(time.perf_counter() - t0, dev)
                pipelined = {"contexts": 3, "value": W * 3 * a.steps / e_p, "ms_per_step": e_p / (3 * a.steps) * 1e3,
                             "poses_equal_serial_on_rank0": bool(torch.equal(Yp, Y)),
                             "note": "consecutive steps of every rank overlapped on three contexts / streams (BatchPipeline); `value` above runs them one after the other"}
            else:
                pipelined = {"error": perr or "another rank failed to set the pipeline up"}
            pipe = None
    del bank, bank_nm, bank_enc
    if rank != 0:
        return None
    return {"value": W * a.steps / elapsed, "unit": "frames/s", "n_gpus": world, "steps": a.steps, "warmup": a.warmup,
            "ms_per_step": elapsed / a.steps * 1e3, "scaling": "strong", "dtype": "f32 (bf16 bank for matching)",
            "config": {"workload": f"BASELINE configs[2]/[3]: 1024 windows x 4096-entry bank (bf16 cnt), V={V}, "
                                   f"{W // world}{'+' if W % world else ''} windows per GPU",
                       "windows_per_gpu": [D.shard_bounds(W, world, r)[1] - D.shard_bounds(W, world, r)[0] for r in range(world)],
                       "parallelism": f"dp{world}, bank broadcast from rank 0, no in-step collective"},
            "per_rank_frames_per_s": per_rank,
            "bank_broadcast": bcast, "bank_broadcast_ms": bcast["ms"] if bcast else None, "bank_bytes": 2 * NB * 90 * 256 * 4,
            **checks,
            "pipelined_3_contexts": pipelined}


def bank4k(a):
    """`--workload bank4k`: the configs[2] / [3] record as the line itself."""
    from mocha_sigasia2023_amd import Generator, distributed as D, synthetic_state_dict
    rank, local, world = D.env_rank()
    local, backend = dist_device_and_backend(local)
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    if world > 1 or os.environ.get("MOCHA_FORCE_DIST"):
        D.init(backend, dev)
    fail_rank_hook(rank)
    V = a.joints
    layout = "mocha" if V == 24 else "mixamo"
    sd = synthetic_state_dict(1777, 1.0, layout)
    model = Generator(layout=layout, device=dev).load_state_dict(sd).eval()
    for k, v in parse_options(a.options).items():
        model.set_option(k, v)
    rec = bank4k_record(a, model, dev, V, rank, world, backend, sd, layout, dump_dir=a.dump_outputs)
    if rec is not None and parse_options(a.options):       # bank4k_record returns the record on rank 0 only: every other rank goes straight on to the collective below
        rec["config"]["options"] = parse_options(a.options)
    rccl = comm_record(model, backend, world) if torch.distributed.is_initialized() else None
    if rank == 0:
        rec = dict({"metric": METRIC[V]}, **rec, higher_is_better=True, vs_baseline=None, data="synthetic", rccl=rccl)
        print(json.dumps(rec), flush=True)
    if torch.distributed.is_initialized():
        D.barrier(); torch.distributed.destroy_process_group()


def fail_rank_hook(rank):
    """Test hook (tests/test_multirank_standin.py): MOCHA_BENCH_FAIL_RANK=r makes rank r die right after the rendezvous, while the
    others go on into their first collective - the launcher's watchdog must end the job."""
    if os.environ.get("MOCHA_BENCH_FAIL_RANK") == str(rank):
        print(f"bench.py: rank {rank}: injected failure (MOCHA_BENCH_FAIL_RANK)", file=sys.stderr, flush=True)
        os._exit(7)


def match_records(model, dev):
    """Roofline of the context-matching kernels on the shapes SURVEY.md §8(d) names for the HBM target: one streamed query
    against a 16 384-entry bank (configs[4]) and 128 queries against a 4 096-entry bf16 bank (configs[3], per-GPU share).
    Algorithmic bytes = N * 23040 * element size + Q * 23040 * 4 + 4 Q; `us` = one mocha_match call (all its kernels and the gaps
    between them), HIP events around 10 back-to-back calls; `kernels` = per-kernel event times of a profiled run."""
    from mocha_sigasia2023_amd import ContextBank
    D = 90 * 256
    out = {}
    g = torch.Generator(device=dev); g.manual_seed(16384)
    big = torch.randn((16384, D), device=dev, generator=g)
    for name, N, Q, bf16, scan16 in (("q1_x_16k_f32", 16384, 1, False, 1), ("q1_x_16k_f32_scan32", 16384, 1, False, 0),
                                     ("q1_x_16k_bf16", 16384, 1, True, 1), ("q128_x_4k_bf16", 4096, 128, True, 1),
                                     ("q128_x_4k_f32", 4096, 128, False, 1)):
        nm = big[:N]
        model.set_option("scan16", scan16)         # fp32 banks >= 4096 rows, <= 8 queries: scan of the centred bf16 copy + exact re-rank
        bank = ContextBank(model, nm, nm.view(N, 90, 256), bf16=bf16)
        q = torch.randn((Q, D), device=dev, generator=g)
        for _ in range(3):
            bank.query(q)
        torch.cuda.synchronize()
        reps = 10
        model.profile_start()
        for _ in range(reps):
            bank.query(q)
        prof = model.profile_stop()
        # the whole call as the caller sees it: an event pair around `reps` back-to-back calls on the stream, seven times, the MEDIAN
        # (round 5's driver line carried one pair only: a single host stall inside it made a 232 us scan read 7 321 us)
        pairs = []
        for _ in range(7):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                bank.query(q)
            e1.record()
            torch.cuda.synchronize()
            pairs.append(e0.elapsed_time(e1) / reps * 1e3)
        us = float(np.median(pairs))
        elt = 2 if bf16 else 4
        by = (N * elt + Q * 4) * D + 4 * Q
        fl = 2.0 * Q * N * D
        rec = {"us": us, "algorithmic_bytes": by, "GB/s": by / us / 1e3, "frac_of_hbm_peak": by / us / 1e3 / PEAK_HBM_GBS,
               "TFLOP/s": fl / us / 1e6, "kernels": {k: v["ms"] / reps * 1e3 for k, v in prof["kernels"].items()},
               "us_pairs_min_max": [float(min(pairs)), float(max(pairs))]}
        kernel_us = sum(rec["kernels"].values())
        if kernel_us > 0 and us > 3.0 * kernel_us:             # a call cannot take three times its own kernels: the wall time is not the kernels' (host stall, another tenant)
            rec["suspect"] = True
            rec["suspect_reason"] = f"median wall time {us:.1f} us per call against {kernel_us:.1f} us of kernels"
        if not bf16 and Q <= 8 and scan16 and N >= 4096:
            # the fp32 search answered from the bf16 copy: the roofline is priced on the bytes the kernels move (2 B per bank value,
            # the queries twice, 16 B of key per row written and read), not on the fp32 bank's size
            moved = (N * 2 + Q * 8) * D + 16 * Q * N
            rec.update({"bytes_moved": moved, "GB/s": moved / us / 1e3, "frac_of_hbm_peak": moved / us / 1e3 / PEAK_HBM_GBS,
                        "fp32_bank_bytes_per_s_equivalent_GB/s": by / us / 1e3,
                        "note": "exact fp32 search through the bank's centred bf16 copy + exact re-rank (mocha_match_refine); "
                                "q1_x_16k_f32_scan32 is the scan of the fp32 rows themselves"})
        out[name] = rec
    model.set_option("scan16", 1)
    # the opt-in one-byte first stage of the few-query scan (option "scan8", match_scan8.hip): a query planted next to a
    # row (the stage stays on: 1 B per bank value + the exact re-rank of a handful of rows) and a query against the independent N(0, 1)
    # rows of the records above (thousands of rows inside the byte image's bound: the stage switches itself off on the device after one
    # call, the steady state is the bf16 scan again)
    try:
        model.set_option("scan8", 1)
        nm = big[:16384]
        bank = ContextBank(model, nm, nm.view(16384, 90, 256))
        for name, q in (("planted", nm[4321:4322] + 0.02 * torch.randn((1, D), device=dev, generator=g)), ("random", torch.randn((1, D), device=dev, generator=g))):
            if name == "random":
                bank = ContextBank(model, nm, nm.view(16384, 90, 256))      # mocha_bank_set again: the stage's mode word starts from zero
            for _ in range(3):
                bank.query(q)
            torch.cuda.synchronize()
            pairs = []
            for _ in range(7):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(10):
                    bank.query(q)
                e1.record(); torch.cuda.synchronize()
                pairs.append(e0.elapsed_time(e1) / 10 * 1e3)
            us = float(np.median(pairs))
            moved = (16384 * (1 if name == "planted" else 2) + 8) * D + 16 * 16384
            out[f"q1_x_16k_f32_scan8_{name}"] = {"us": us, "bytes_moved": moved, "GB/s": moved / us / 1e3, "frac_of_hbm_peak": moved / us / 1e3 / PEAK_HBM_GBS,
                                                  "note": "option scan8 = 1 (default 0): " + ("1 B per bank value + exact re-rank; same index and distance as q1_x_16k_f32"
                                                          if name == "planted" else "the stage has switched itself off (steady state: the bf16 scan of q1_x_16k_f32)")}
    finally:
        model.set_option("scan8", 0)
    # ... and as `characterize` runs it: 128 windows against the 4 096-entry bf16 bank - the instance norm writes the
    # matcher's centred bf16 query plane itself, so the match is the coarse pass + the selection; per-kernel HIP events of the call sites
    bank = ContextBank(model, big[:4096], big[:4096].view(4096, 90, 256), bf16=True)
    from mocha_sigasia2023_amd import synthetic
    X = torch.from_numpy(synthetic.pose_windows(123, 128, model.V)).to(dev)
    m_, s_ = synthetic.cnt_norm(7)
    m_, s_ = torch.from_numpy(m_).to(dev), torch.from_numpy(s_).to(dev)
    for _ in range(3):
        bank.characterize(X, m_, s_)
    model.profile_start()
    for _ in range(10):
        bank.characterize(X, m_, s_)
    sites = model.profile_stop()["sites"]
    mk = {k.split("|")[1]: v["ms"] / v["launches"] * 1e3 for k, v in sites.items() if k.startswith("match.")}
    us = sum(mk.values())
    by = 4096 * D * 2 + 128 * D * 2 + 4 * 128
    out["q128_x_4k_bf16_in_characterize"] = {"us": us, "algorithmic_bytes": by, "GB/s": by / us / 1e3, "frac_of_hbm_peak": by / us / 1e3 / PEAK_HBM_GBS,
                                             "kernels": mk, "note": "sum of the match.* kernels inside ContextBank.characterize(128 windows) (HIP events per launch); "
                                                                    "the centred bf16 query plane comes from the instance norm (read as bf16: 2 B per query value)"}
    del big
    return out


def stream_record(model, dev, V):
    """BASELINE configs[4]: a 300-frame clip streamed window by window (285 windows) against a 16 384-entry bank through the
    captured per-window step (mocha_step_graph)."""
    from mocha_sigasia2023_amd import ContextBank, StreamingCharacterizer, synthetic
    D = 90 * 256
    g = torch.Generator(device=dev); g.manual_seed(7)
    nm = torch.randn((16384, D), device=dev, generator=g)
    m_, s_ = synthetic.cnt_norm(7)
    src = torch.from_numpy(synthetic.pose_windows(5, 285, V)).to(dev)
    out = {}
    for bf16, scan16 in ((False, 1), (False, 0), (True, 1)):
        model.set_option("scan16", scan16)
        bank = ContextBank(model, nm, nm.view(-1, 90, 256), bf16=bf16)
        sc = StreamingCharacterizer(bank, m_, s_, use_graph=True)
        for i in range(5):
            sc.step(src[i])
        torch.cuda.synchronize()
        lat = []
        t_all = time.perf_counter()
        for i in range(285):
            t0 = time.perf_counter()
            sc.step(src[i])
            torch.cuda.synchronize()
            lat.append(time.perf_counter() - t0)
        total = time.perf_counter() - t_all
        lat = np.sort(np.asarray(lat)) * 1e3
        rec = {"windows_per_s": 285 / total, "p50_ms": float(lat[142]), "p99_ms": float(lat[282])}
        # the same 285 per-window steps with up to `lanes` of them in flight (mocha_step_graph_lane: window i + 1's encode chain
        # under window i's bank scan), no host synchronisation per window: throughput of the streamed clip, not a latency
        for lanes in (1, 2, 3):
            scl = StreamingCharacterizer(bank, m_, s_, use_graph=True, lanes=lanes)
            scl.run_clip(src[:8]); torch.cuda.synchronize()
            t0 = time.perf_counter()
            Yp, ip = scl.run_clip(src)
            torch.cuda.synchronize()
            rec[f"pipelined_lanes{lanes}_windows_per_s"] = 285 / (time.perf_counter() - t0)
        model.set_option("lanes", 1)
        out["bf16_bank" if bf16 else ("f32_bank" if scan16 else "f32_bank_scan32")] = rec
    model.set_option("scan16", 1)
    # the same streamed clip against a bank that CONTAINS it: the 285 windows' own features (+ 1 % noise) planted at scattered rows, as in
    # tests/test_fullsize_parity.py::test_config4 - every query has ~300 stride-1 neighbours inside the coarse image's bound, all re-ranked
    # exactly; with the opt-in one-byte first stage (option scan8) beside the default
    try:
        nm0 = model.encode(src, m_, s_)[2].reshape(285, D)
        rows = torch.randperm(16384, device=dev, generator=g)[:285]
        planted = nm.clone()
        planted[rows] = nm0 + 0.01 * torch.randn((285, D), device=dev, generator=g)
        prec = {}
        for on in (0, 1):
            model.set_option("scan8", on)
            bank = ContextBank(model, planted, planted.view(-1, 90, 256))
            sc = StreamingCharacterizer(bank, m_, s_, use_graph=True)
            for i in range(5):
                sc.step(src[i])
            torch.cuda.synchronize()
            lat, hits = [], 0
            for i in range(285):
                t0 = time.perf_counter()
                _, ix = sc.step(src[i])
                torch.cuda.synchronize()
                lat.append(time.perf_counter() - t0)
                hits += int(ix.item()) == int(rows[i].item())
            lat = np.sort(np.asarray(lat)) * 1e3
            prec["scan8" if on else "default"] = {"p50_ms": float(lat[142]), "p99_ms": float(lat[282]), "planted_row_found": hits}
        out["f32_bank_planted_clip"] = prec
    finally:
        model.set_option("scan8", 0)
    return out


def ours_record(model, dev):
    """Row N1 (test_fullframework.py:446-457): the CVAE ("Ours") branch per frame - condition, CVAE.sample, de-normalise, decoder,
    to_mot through OursSession with graph replay - for 1 clip and for 8 clips advanced in lock step; host-timed per step with a
    one-element read-back as the synchronisation (the demo's loop consumes every frame's pose on the host)."""
    from mocha_sigasia2023_amd import CVAE, OursSession, synthetic
    from mocha_sigasia2023_amd import weights as Wt
    cvae = CVAE(device=dev).load_state_dict(Wt.synthetic_cvae_state_dict(99, 1.0)).eval()
    rng = np.random.Generator(np.random.PCG64(0))
    stats = [(0.1 * rng.standard_normal((90, 256))).astype(np.float32), rng.uniform(0.5, 1.5, (90, 256)).astype(np.float32),
             (0.1 * rng.standard_normal((90, 256))).astype(np.float32), rng.uniform(0.5, 1.5, (90, 256)).astype(np.float32)]
    out = {}
    for B in (1, 8):
        enc, cnt = model.encode(torch.from_numpy(synthetic.pose_windows(3, B, model.V)).to(dev))
        s = OursSession(model, cvae, *stats, use_graph=True).reset(enc)
        for _ in range(5):
            s.step(enc, cnt)
        torch.cuda.synchronize()
        lat = []
        for _ in range(200):
            t0 = time.perf_counter(); y, c = s.step(enc, cnt); y[0, 0, 0, 0].item(); lat.append(time.perf_counter() - t0)
        lat = np.sort(np.asarray(lat)) * 1e3
        out[f"clips{B}"] = {"ms_per_frame_p50": float(lat[100]), "ms_per_frame_p99": float(lat[197]), "frames_per_s": B / float(lat[100]) * 1e3}
    return out


def post_record(model, dev, W):
    """Rows N2 / N3 around the step, HIP events over 20 repetitions each: featurisation of W windows (mocha_featurize), last-frame
    pose heads of W decoded windows (mocha_pose_heads), and the sequential frame loop of one W-frame clip and of 64 such clips in
    one launch (mocha_post_clip: root integration, blending, foot-lock IK, BVH channels; one lane per clip)."""
    from mocha_sigasia2023_amd import postprocess as P
    r = np.random.Generator(np.random.PCG64(11))
    V, J = model.V, model.V + 1

    def ev(fn, reps=20):
        fn(); torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record(); torch.cuda.synchronize()
        return e0.elapsed_time(e1) / reps * 1e3
    rot = torch.from_numpy(r.standard_normal((W, 60, J, 4)).astype(np.float32)).to(dev)
    rot = rot / rot.norm(dim=-1, keepdim=True)
    pos, vel, ang = (torch.from_numpy(r.standard_normal((W, 60, J, 3)).astype(np.float32)).to(dev) for _ in range(3))
    Y = torch.from_numpy(r.standard_normal((W, 60, V, 15)).astype(np.float32)).to(dev)
    out = {"featurize_us_per_window": ev(lambda: model.featurize(rot, pos, vel, ang)) / W,
           "pose_heads_us_per_window": ev(lambda: P.pose_heads(model, Y)) / W}
    heads, speed = P.pose_heads(model, Y)
    # toe bones in the (V+1)-bone skeleton: 5 / 24 for the shipped 24-joint layout (test_fullframework.py:104), the 'mixamo'
    # tables' toes (joints 17 and 21, net/graph.py:18-31) for the 22-joint one
    pp = P.PostProcessor(model, contact_bones=(5, 24) if V == 24 else (18, 22))
    for clips in (1, 64):
        h = heads[None].expand(clips, -1, -1, -1).contiguous()
        sp = speed[None].expand(clips, -1).contiguous()
        rv = torch.from_numpy((0.01 * r.standard_normal((clips, W, 3))).astype(np.float32)).to(dev)
        ra = torch.from_numpy((0.01 * r.standard_normal((clips, W, 3))).astype(np.float32)).to(dev)
        ss = torch.from_numpy(np.abs(r.standard_normal((clips, W))).astype(np.float32)).to(dev)
        ct = torch.from_numpy((r.uniform(size=(clips, W, 2)) > 0.5).astype(np.uint8)).to(dev)
        us = ev(lambda: pp.run(h, sp, rv, ra, ss, ct, bvh=True), reps=5)
        out[f"post_clip_us_per_frame_{clips}_clip{'s' if clips > 1 else ''}"] = us / (clips * W)
    return out


def bank_build_record(model, dev, V):
    """Row N4: building a character bank on the device - 4 096 synthetic windows encoded (mot_embedding, encoder, cnt), the
    bank's cnt_mean / cnt_std (mocha_column_stats: compute_cnt_norm.py:157-179), the z-score, and mocha_bank_set with the bf16 copy,
    centroid, row norms (collect_CVAE_feature_action.py:167-189 + the demo's BallTree construction, test_fullframework.py:293-294).
    Wall clock with one synchronisation at the end, best of three."""
    from mocha_sigasia2023_amd import ContextBank, bank as BK, synthetic
    N = 4096
    X = torch.from_numpy(synthetic.pose_windows(77, N, V)).to(dev)
    tw = torch.from_numpy(synthetic.temporal_weight(15, 6, 256)).to(dev)

    def build():
        b = BK.build_bank(model, X)
        std = (b["cnt_std"].clamp_min(1e-6) / tw).contiguous()
        nm = ((b["cnt"] - b["cnt_mean"]) / std).reshape(N, -1)
        return ContextBank(model, nm, b["encoded"], bf16=True)
    best = None
    for _ in range(4):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        bank = build()
        torch.cuda.synchronize(); dt = time.perf_counter() - t0
        best = dt if best is None or dt < best else best
        del bank
    return {"windows": N, "ms": best * 1e3, "windows_per_s": N / best,
            "note": "encode 4 096 windows + cnt statistics + z-score + mocha_bank_set (bf16 copy, centroid, norms); the z-score is a torch expression here"}


def main():
    a = parse()
    if a.gpus > 1 and "RANK" not in os.environ:
        return spawn_ranks(a)
    if a.workload == "bank4k":
        return bank4k(a)
    from mocha_sigasia2023_amd import distributed as D
    rank, local, world = D.env_rank()
    dist_on = world > 1 or bool(os.environ.get("MOCHA_FORCE_DIST"))      # the env knob runs the RCCL plumbing with one rank
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a ROCm GPU (there is no CPU fallback for the product path)")
    local, backend = dist_device_and_backend(local)
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    if dist_on:
        D.init(backend, dev)                      # "nccl" is RCCL on ROCm
    fail_rank_hook(rank)

    from mocha_sigasia2023_amd import ContextBank, Generator, synthetic, synthetic_state_dict
    layout = "mocha" if a.joints == 24 else "mixamo"
    V, W = a.joints, a.windows
    sd = synthetic_state_dict(seed=1777, gain=1.0, layout=layout)
    model = Generator(layout=layout, device=dev).load_state_dict(sd).eval()
    if a.chunk:
        model.reserve(a.chunk)
    opts = parse_options(a.options)
    for k, v in opts.items():
        model.set_option(k, v)

    # ---- inputs, resident in HBM before the timed region
    src = torch.from_numpy(synthetic.pose_windows(1777 + 10 * rank, W, V)).to(dev)
    if rank == 0:
        cha = torch.from_numpy(synthetic.pose_windows(4242, W, V)).to(dev)
        m_, s_ = synthetic.cnt_norm(7)
        mean, std = torch.from_numpy(m_).to(dev), torch.from_numpy(s_).to(dev)
    else:
        cha = torch.empty((W, 60, V, 15), dtype=torch.float32, device=dev)
        mean = torch.empty((90, 256), dtype=torch.float32, device=dev)
        std = torch.empty_like(mean)
    bcast_ms = clip_bcast_ms = bcast_err = rccl = None
    if dist_on:
        torch.cuda.synchronize(); D.barrier()
        t0 = time.perf_counter()
        D.broadcast_([cha, mean, std], src=0)     # RCCL over xGMI, set-up only: rank 0 owns the character clip
        torch.cuda.synchronize()
        clip_bcast_ms = (time.perf_counter() - t0) * 1e3
    if dist_on and a.full:
        # north star: "RCCL broadcast of the character feature bank over xGMI".  Rank 0 builds the bank of the character clip and
        # hands it to every rank through the C ABI (mocha_bank_broadcast: scatter + all-gather); every rank checks what it got.
        # (The timed step below does not depend on this bank - every rank builds the pair's bank itself, as at N = 1 - so a failure
        # here is reported in the line, `bank_broadcast_error`, instead of costing the scaling measurement.)
        bcast_err = None
        try:
            D.init_comm(model)
            with torch.no_grad():
                enc_c, _, nm_c = model.encode(cha, mean, std)
                bank0 = ContextBank(model, nm_c, enc_c) if rank == 0 else None
                torch.cuda.synchronize(); D.barrier()
                t0 = time.perf_counter()
                got = D.bank_broadcast(model, bank0, W, root=0)
                torch.cuda.synchronize()
                bcast_ms = (time.perf_counter() - t0) * 1e3
                probe = got.query(nm_c[: min(W, 16)], return_distance=False)[:, 0].cpu().tolist()
            if probe != list(range(min(W, 16))):
                bcast_err = f"rank {rank}: the broadcast bank does not reproduce the owner's bank (probe {probe})"
        except RuntimeError as e:
            bcast_err = f"rank {rank}: {e}"
        if bcast_err:
            print("bench.py: " + bcast_err, file=sys.stderr, flush=True)
        errs = [None] * world
        torch.distributed.all_gather_object(errs, bcast_err)
        bcast_err = next((e for e in errs if e), None)
        bcast_ms = None if bcast_err else D.max_over_ranks(bcast_ms, dev)
        rccl = None if bcast_err else comm_record(model, backend, world)

    def step_three_calls():
        enc_c, cnt_c, nm_c = model.encode(cha, mean, std)               # bank build
        bank = ContextBank(model, nm_c, enc_c)                          # borrow + centroid + row norms
        return bank.characterize(src, mean, std, return_index=True)     # src encode, match, gather, decode, to_mot

    def step_pair():
        # the same work through mocha_characterize_pair: both clips share the mot_embedding / encoder / cnt launches
        return model.characterize_pair(src, cha, mean, std, return_index=True)

    step = step_three_calls if (a.three_calls or 2 * W > 1280) else step_pair

    def sync_all():
        torch.cuda.synchronize()
        D.barrier()
        torch.cuda.synchronize()

    with torch.no_grad():
        for _ in range(a.warmup):
            Y, idx = step()
        sync_all()
        t0 = time.perf_counter()
        for _ in range(a.steps):
            Y, idx = step()
        sync_all()
        elapsed = time.perf_counter() - t0
    if a.dump_outputs and rank == 0:
        dump_outputs(a.dump_outputs, Y=Y, idx=idx)
    my_elapsed = elapsed
    elapsed = D.max_over_ranks(elapsed, dev)
    ms_per_step = elapsed / a.steps * 1e3
    value = world * W * a.steps / elapsed
    per_rank = [W * a.steps / my_elapsed]
    if dist_on:
        vals = [None] * world
        torch.distributed.all_gather_object(vals, per_rank[0])
        per_rank = [float(v) for v in vals]

    # extra (not the headline): the same step back to back for >= --sustained-s seconds (the plane GEMMs run at the board's
    # power limit: the clock a 0.1 s burst holds is not the one a long run holds)
    sustained = None
    if a.full and a.sustained_s > 0 and world == 1:
        n_sus = max(a.steps, int(a.sustained_s / (ms_per_step * 1e-3)) + 1)
        with torch.no_grad(), PowerSampler() as ps:
            sync_all()
            t0 = time.perf_counter()
            for _ in range(n_sus):
                step()
            sync_all()
            e_s = time.perf_counter() - t0
        sustained = {"value": W * n_sus / e_s, "ms_per_step": e_s / n_sus * 1e3, "steps": n_sus, "seconds": e_s, "power": ps.record()}

    # extra (not the headline): the same step with the library's two-stream overlap enabled
    dual = None
    if a.dual_stream:
        model.set_option("dual_stream", 1)
        with torch.no_grad():
            for _ in range(a.warmup):
                step()
            sync_all()
            t0 = time.perf_counter()
            for _ in range(a.steps):
                step()
            sync_all()
            e2 = D.max_over_ranks(time.perf_counter() - t0, dev)
        dual = {"value": world * W * a.steps / e2, "ms_per_step": e2 / a.steps * 1e3,
                "note": "same step, mocha_set_option(dual_stream=1): batch halves on two HIP streams; kernels overlap, so per-kernel "
                        "roofline numbers are quoted on the single-stream run above"}
        model.set_option("dual_stream", 0)

    # extra (not the headline): the same step on the exact-f32 MFMA engine (mocha_set_option("gemm_bf16x3", 0))
    exact_f32 = None
    if a.full and world == 1 and not a.no_extras:
        model.set_option("gemm_bf16x3", 0)
        model.set_option("attention_bf16x3", 0)
        with torch.no_grad():
            for _ in range(a.warmup):
                step()
            sync_all()
            t0 = time.perf_counter()
            for _ in range(a.steps):
                step()
            sync_all()
            e3 = time.perf_counter() - t0
        exact_f32 = {"value": W * a.steps / e3, "ms_per_step": e3 / a.steps * 1e3,
                     "note": "same step with mocha_set_option(gemm_bf16x3=0, attention_bf16x3=0): every GEMM and the attention on "
                             "v_mfma_f32_32x32x2_f32 (gemm_f32.hip, attention.hip)"}
        model.set_option("gemm_bf16x3", 1)
        model.set_option("attention_bf16x3", 1)

    # extra (not the headline): the same step with the encoder's, decoder's and to_mot's plane GEMMs on two fp16 planes / three passes
    # (mocha_set_option("gemm_f16x2", 1), csrc/gemm_h2.hip); the poses are compared with the default engine's of the same inputs
    f16x2 = None
    if a.full and world == 1 and not a.no_extras and not opts.get("gemm_f16x2"):
        with torch.no_grad():
            Y0, i0 = model.characterize_pair(src, cha, mean, std, return_index=True)
            model.set_option("gemm_f16x2", 1)
            Y1, i1 = model.characterize_pair(src, cha, mean, std, return_index=True)
            same = (i0 == i1)
            dY = float((Y1 - Y0)[same].abs().max()) if bool(same.any()) else None
            for _ in range(a.warmup):
                step()
            sync_all()
            t0 = time.perf_counter()
            for _ in range(a.steps):
                step()
            sync_all()
            e4 = time.perf_counter() - t0
        f16x2 = {"value": W * a.steps / e4, "ms_per_step": e4 / a.steps * 1e3, "same_matches": float(same.float().mean()),
                 "max_abs_dY_vs_default_engine": dY, "max_abs_Y": float(Y0.abs().max()),
                 "note": "same step with mocha_set_option(gemm_f16x2=1): the encoder's, decoder's and to_mot's plane GEMMs as two fp16 planes, "
                         "three v_mfma_f32_32x32x16_f16 passes per product (22-bit operands, fp32 accumulation; GEMM error against float64 below "
                         "both fp32 engines': tests/test_gemm_f16x2.py) - opt-in, NOT the headline's arithmetic; the embedding GEMMs, the "
                         "attention and the matcher stay on three bf16 planes"}
        model.set_option("gemm_f16x2", 0)

    # N > 1: BASELINE configs[3] beside the weak-scaled headline - the same 1024 windows split over the ranks, the 4096-entry bank
    # through mocha_bank_broadcast (collective: every rank takes part; the record comes back on rank 0)
    bank4k_rec = None
    if a.full and dist_on and world > 1 and not a.no_bank4k and not bcast_err:
        with torch.no_grad():
            bank4k_rec = bank4k_record(a, model, dev, V, rank, world, backend, sd, layout)

    out = None
    if rank == 0:
        out = {
            "metric": METRIC[V],
            "value": value, "unit": "frames/s", "n_gpus": world, "steps": a.steps, "warmup": a.warmup,
            "ms_per_step": ms_per_step, "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
            "dtype": "f32" if not opts.get("gemm_f16x2") else "f32 in / out / accumulate; GEMM operands as two fp16 planes = 22 bits (--options gemm_f16x2=1)",
            "data": "synthetic",
            "config": {"options": opts, "workload": f"demo pair (BASELINE configs[1]): {W} src x {W} cha windows, T=60, V={V}, C=15, "
                                   f"bank build + encode/match/decode/to_mot per step "
                                   f"({'encode + ContextBank + characterize' if step is step_three_calls else 'characterize_pair'})",
                       "windows_per_gpu": W,
                       "joints": V, "bank_entries": W, "parallelism": f"dp{world} (independent windows, no in-step collective)"},
            "roofline": None, "kernel_breakdown": None, "match_sites": None,      # --full: the roofline leg below
            "bank_broadcast_ms": bcast_ms, "bank_broadcast_error": bcast_err, "clip_broadcast_ms": clip_bcast_ms,
            "per_rank_frames_per_s": per_rank,
            "rccl": rccl,
            "bank4k": bank4k_rec,
            "sustained": sustained,
            "dual_stream": dual,
            "exact_f32_engine": exact_f32,
            "f16x2_engine": f16x2,
        }
    if rank == 0 and a.full:
        # ---- roofline leg: the same step once more with a HIP-event pair around every launch
        with torch.no_grad():
            for _ in range(max(a.warmup, 5)):       # the extras above ran other engines / workloads: bring the board back to this step's state first
                step()
            torch.cuda.synchronize(dev)              # rank 0 only here: no barrier
            model.profile_start()
            for _ in range(3):
                step()
            prof = model.profile_stop()
        kern = prof["kernels"]
        dom = max(kern, key=lambda k: kern[k]["ms"])
        d = kern[dom]
        total_ms = sum(k["ms"] for k in kern.values())
        ach = d["flops"] / (d["ms"] * 1e-3) / 1e12
        traffic, traffic_src = pmc_traffic_for(dom)
        # mocha_gemm_x3 computes every fp32 product as six bf16 MFMA passes: it is priced on the bf16 pipe with the FLOPs it
        # executes (6 x the algorithmic fp32 FLOPs); the fp32-equivalent rate is given beside it
        on_h2 = dom.startswith("mocha_gemm_h2")        # --options gemm_f16x2=1: two fp16 planes, three passes, same pipe peak as bf16
        on_bf16 = dom.startswith("mocha_gemm_x3") or on_h2
        exe = ach * (3 if on_h2 else X3_PASSES) if on_bf16 else ach
        peak = PEAK_BF16_MFMA_TFLOPS if on_bf16 else PEAK_F32_MFMA_TFLOPS
        roofline = {
            "kernel": dom, "bound": "mfma", "achieved": exe, "peak": peak, "unit": "TFLOP/s",
            "frac": exe / peak,
            "pipe": ("fp16 MFMA (v_mfma_f32_32x32x16_f16, fp32 accumulate): each fp32 operand as two fp16 planes (22 bits), three passes per "
                     "product; 'achieved' counts the executed fp16 FLOPs") if on_h2 else
                    ("bf16 MFMA (v_mfma_f32_32x32x16_bf16, fp32 accumulate): each fp32 operand as three bf16 planes, six passes per "
                     "product; 'achieved' counts the executed bf16 FLOPs") if on_bf16 else "f32 MFMA (v_mfma_f32_32x32x2_f32)",
            "fp32_equivalent": {"achieved": ach, "f32_mfma_peak": PEAK_F32_MFMA_TFLOPS, "frac": ach / PEAK_F32_MFMA_TFLOPS},
            # the honest reading of `frac` for an emulated product: the USEFUL (algorithmic fp32) FLOPs against the peak of the pipe
            # the kernel runs on - six bf16 passes per fp32 product cap this at 1/6
            "useful_frac_of_pipe_peak": ach / peak,
            "traffic": traffic,
            "traffic_source": traffic_src,
            "algorithmic_bytes_per_launch": d["bytes"] / d["launches"],
            "launches_per_step": d["launches"] // 3, "avg_launch_us": d["ms"] / d["launches"] * 1e3,
            "algorithmic_flops_per_launch": d["flops"] / d["launches"],
            "share_of_step_kernel_time": d["ms"] / total_ms,
        }
        # the whole step in fp32-equivalent terms: the FLOPs the kernels are asked for after the algebraic identities, and the
        # reference's literal count for the same step (1 517.7 MFLOP per encoded window, 815.9 per decoded one,
        # 2 * 23040 per query-row pair of the search), both over the timed step
        step_flops = sum(k["flops"] for k in kern.values()) / 3
        ref_flops = (2 * W * 1517.7e6 + W * 815.9e6 + 2.0 * W * W * 23040)
        roofline["whole_step_fp32_equivalent_tflops"] = step_flops / (ms_per_step * 1e-3) / 1e12
        roofline["whole_step"] = {"algorithmic_gflop_after_identities": step_flops / 1e9, "tflops": step_flops / (ms_per_step * 1e-3) / 1e12,
                                  "reference_literal_gflop": ref_flops / 1e9,
                                  "reference_literal_tflops_equivalent": ref_flops / (ms_per_step * 1e-3) / 1e12,
                                  "frac_of_f32_mfma_peak": step_flops / (ms_per_step * 1e-3) / 1e12 / PEAK_F32_MFMA_TFLOPS}
        mk = {k: v for k, v in prof["sites"].items() if k.startswith("match.")}
        breakdown = {k: {"ms_per_step": v["ms"] / 3, "launches_per_step": v["launches"] // 3,
                         "tflops": (v["flops"] / (v["ms"] * 1e-3) / 1e12) if v["ms"] > 0 else 0.0,
                         "gbs": (v["bytes"] / (v["ms"] * 1e-3) / 1e9) if v["ms"] > 0 else 0.0}
                     for k, v in sorted(kern.items(), key=lambda kv: -kv[1]["ms"])}
        out.update(roofline=roofline, kernel_breakdown=breakdown, match_sites={k: {"ms_per_step": v["ms"] / 3} for k, v in mk.items()})
        if world == 1 and not a.no_extras:
            # extra records measured in the same process (not the headline): the matcher's own roofline on the shapes the
            # north star's ">= 50 % HBM in the context-matching kernel" is evaluated on, the streamed configs[4] step, the
            # shipped model's 24-joint layout, and the (f) rows around the step (CVAE branch, featurisation, post-processing)
            with torch.no_grad():
                out["match"] = match_records(model, dev)
                out["stream_16k"] = stream_record(model, dev, V)
                out["ours"] = ours_record(model, dev)
                out["post"] = post_record(model, dev, W)
                out["bank_build"] = bank_build_record(model, dev, V)
                out["projected_scaling"] = projected_scaling_record(a, model, dev, V, sd, layout)
                out["pipelined_steps"] = pipelined_pair_record(a, sd, layout, dev, V, W, src, cha, mean, std)
                if V != 24:
                    sd24 = synthetic_state_dict(seed=1777, gain=1.0, layout="mocha")
                    m24 = Generator(layout="mocha", device=dev).load_state_dict(sd24).eval()
                    s24 = torch.from_numpy(synthetic.pose_windows(1777, W, 24)).to(dev)
                    c24 = torch.from_numpy(synthetic.pose_windows(4242, W, 24)).to(dev)
                    for _ in range(a.warmup):
                        m24.characterize_pair(s24, c24, mean, std)
                    torch.cuda.synchronize(); t0 = time.perf_counter()
                    for _ in range(a.steps):
                        m24.characterize_pair(s24, c24, mean, std)
                    torch.cuda.synchronize(); e24 = time.perf_counter() - t0
                    out["joints24"] = {"value": W * a.steps / e24, "ms_per_step": e24 / a.steps * 1e3,
                                       "note": "the same step on the shipped model's 24-joint 'mocha' layout (configs/config.yaml:8-10,17)"}
                    del m24, s24, c24
        if not a.no_cpu_baseline and world == 1:         # the CPU leg runs at N=1 only (the other ranks would idle through it)
            m_, s_ = synthetic.cnt_norm(7)
            cpu_full = W if a.cpu_full < 0 else a.cpu_full
            out["cpu_baseline"] = cpu_baseline(sd, V, a.cpu_sample, m_, s_, full=cpu_full)
            out["speedup_vs_cpu"] = value / out["cpu_baseline"]["value"]
            out["config"]["cpu_baseline_sample"] = (f"value: {cpu_full} + {cpu_full} windows once (the GPU workload is {W} + {W}); " if cpu_full else "") + \
                                                   f"thread sweep on {a.cpu_sample} + {a.cpu_sample} windows"
    if rank == 0:
        print(json.dumps(out), flush=True)
    if dist_on:
        D.barrier()
        torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main()
