#!/usr/bin/env python3
"""Option "walk" per call site: one process, one build, the demo-pair step with walk = A and walk = B alternating, `--rounds` rounds of
`--steps` profiled steps each (HIP events per launch inside libmocha_hip.so, as tools/profile_sites.py).  Prints us per launch for both
settings, their difference and the min - max over the rounds, and the wall time of un-profiled steps per round."""
import argparse, os, sys, time
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from mocha_sigasia2023_amd import Generator, synthetic, synthetic_state_dict
ap = argparse.ArgumentParser()
ap.add_argument("--windows", type=int, default=585); ap.add_argument("--rounds", type=int, default=6); ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--a", type=int, default=0, help="walk value of setting A"); ap.add_argument("--b", type=int, default=1, help="walk value of setting B")
ap.add_argument("--joints", type=int, default=22, choices=(22, 24))
a = ap.parse_args()
dev = torch.device("cuda:0")
layout = "mocha" if a.joints == 24 else "mixamo"
model = Generator(layout=layout, device=dev).load_state_dict(synthetic_state_dict(seed=1777, gain=1.0, layout=layout)).eval()
W, V = a.windows, a.joints
src = torch.from_numpy(synthetic.pose_windows(1, W, V)).to(dev); cha = torch.from_numpy(synthetic.pose_windows(2, W, V)).to(dev)
m_, s_ = synthetic.cnt_norm(7); mean, std = torch.from_numpy(m_).to(dev), torch.from_numpy(s_).to(dev)
step = lambda: model.characterize_pair(src, cha, mean, std)
for _ in range(3): step()
torch.cuda.synchronize()
sites = {}          # site -> [[us per launch, per round] for A, the same for B]
wall = [[], []]
for r in range(a.rounds):
    for k, walk in enumerate((a.a, a.b)):
        model.set_option("walk", walk)
        for _ in range(2): step()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.steps): step()
        torch.cuda.synchronize()
        wall[k].append((time.perf_counter() - t0) / a.steps * 1e3)
        model.profile_start()
        for _ in range(a.steps): step()
        p = model.profile_stop()
        for name, v in p["sites"].items():
            sites.setdefault(name, [[], []])[k].append((v["ms"] / v["launches"] * 1e3, v["launches"] // a.steps))
print(f"walk = {a.a} (A) against walk = {a.b} (B): {W} + {W} windows, {a.joints} joints, {a.rounds} rounds of {a.steps} steps, alternating")
for k, nm in enumerate("AB"):
    print(f"wall ms/step {nm}: " + " ".join(f"{x:.3f}" for x in wall[k]) + f"   min {min(wall[k]):.3f} max {max(wall[k]):.3f}")
print(f"{'site|kernel':58s} {'n':>3s} {'A us':>8s} {'A min-max':>15s} {'B us':>8s} {'B min-max':>15s} {'B-A us':>7s} {'B-A %':>6s} {'step us':>8s}")
tot = 0.0
mean_of = lambda xs: sum(x for x, _ in xs) / len(xs)
for name, (A, B) in sorted(sites.items(), key=lambda kv: -mean_of(kv[1][0]) * kv[1][0][0][1]):
    if not A or not B: continue
    ma, mb, n = mean_of(A), mean_of(B), A[0][1]
    tot += (mb - ma) * n
    print(f"{name:58s} {n:3d} {ma:8.1f} {min(x for x, _ in A):7.1f}-{max(x for x, _ in A):<7.1f} {mb:8.1f} {min(x for x, _ in B):7.1f}-{max(x for x, _ in B):<7.1f} "
          f"{mb - ma:7.1f} {100 * (mb - ma) / ma if ma else 0:6.1f} {(mb - ma) * n:8.1f}")
print(f"sum over sites of (B - A) x launches: {tot:.1f} us per step")
