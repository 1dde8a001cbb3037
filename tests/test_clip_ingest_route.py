"""The two batch chains that start from raw clips, on the MI355X (run with -m gpu):

  raw clip -> build_database_from_clips -> write_database / load_database -> build_bank_from_database, against the reference's own
  process_data of the fixture clip, plain and mirrored (tests/golden/clip_ingest.npz), within the bound of test_clip_ingest_kernel.py;
  raw clip pair -> ingest_clips -> clip_windows -> featurize -> characterize_pair: examples/demo_pair.py --from-raw run as a program gives
  the pair call's output of the same windows prepared by the staged calls here, bit for bit."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import clip_ingest_ref as CR  # noqa: E402
from mocha_sigasia2023_amd import Generator, IngestConfig, clip_windows, ingest_clips, synthetic, synthetic_state_dict, weights  # noqa: E402
from mocha_sigasia2023_amd.bank import build_bank_from_database, build_database_from_clips, load_database, write_database  # noqa: E402
from mocha_sigasia2023_amd.skeleton import LAYOUTS  # noqa: E402

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(REPO, "tests", "golden", "clip_ingest.npz")
KEYS = {"bone_positions": "pos", "bone_velocities": "vel", "bone_rotations": "rot", "bone_angular_velocities": "ang"}


def test_database_from_clips(tmp_path):
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    gold = np.load(GOLD)
    model = Generator(device="cuda:0").load_state_dict(weights.synthetic_state_dict(13, 1.0)).eval()
    db = build_database_from_clips(model, [(gold["rot"], gold["pos"])], [3], [1], mirror=True)
    assert db["range_starts"].tolist() == [0, 100] and db["range_stops"].tolist() == [100, 200]
    assert db["style_labels"].tolist() == [3, 3] and db["action_labels"].tolist() == [1, 1]
    assert db["bone_parents"].tolist() == [-1] + [p + 1 for p in LAYOUTS["mocha"]["parents"]]
    for tag, lo, e in (("plain", 0, CR.E), ("mirror", 100, CR.E_MIRROR)):
        for k, short in KEYS.items():
            ref = gold[f"{tag}_100_{short}"]
            err = np.abs(db[k][lo:lo + 100].astype(np.float64) - ref)
            bound = np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64) + 4.0 * e
            assert np.all(err <= bound), (tag, k, float((err / bound).max()))
        assert np.array_equal(db["contact_states"][lo:lo + 100].astype(bool), gold[f"{tag}_100_contact"]), tag
    # the contact threshold is the configuration's: generate_database_bin.py's 0.2 m/s gives fewer contacts than process_data's 0.5
    low = build_database_from_clips(model, [(gold["rot"], gold["pos"])], [3], [1], mirror=False, raw=IngestConfig(contact_velocity_threshold=0.2))
    assert low["range_stops"].tolist() == [100] and np.array_equal(low["bone_positions"], db["bone_positions"][:100])
    assert 0 < low["contact_states"].sum() < db["contact_states"][:100].sum()
    path = str(tmp_path / "database.bin")
    write_database(path, db)
    back = load_database(path)
    for k in db:
        assert back[k].dtype == db[k].dtype and np.array_equal(back[k], db[k]), k
    rng = np.random.Generator(np.random.PCG64(5))
    model.set_pose_norm((0.05 * rng.standard_normal((25, 15))).astype(np.float32), rng.uniform(0.5, 1.5, (25, 15)).astype(np.float32),
                        np.zeros((25, 15), np.float32), np.ones((25, 15), np.float32))
    bank = build_bank_from_database(model, path, [3], [1], batch=32)
    assert bank["encoded"].shape == (80, 90, 256) and bank["range_stops"].tolist() == [40, 80]       # 100 - 60 windows per range
    assert bool(torch.isfinite(bank["encoded"]).all()) and bool(torch.isfinite(bank["cnt_std"]).all())


def test_demo_from_raw_is_the_staged_route(tmp_path):
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    N = 20
    out = str(tmp_path / "demo")
    r = subprocess.run([sys.executable, os.path.join(REPO, "examples", "demo_pair.py"), "--from-raw", "--frames", str(N), "--out", out],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    z = np.load(os.path.join(out, "from_raw.npz"))
    for name in ("cm_trans.bvh", "ours.bvh"):
        assert os.path.getsize(os.path.join(out, name)) > 0
    # the same windows through the staged calls: the demo's model, norms and clips (examples/demo_pair.py)
    model = Generator(device="cuda:0").load_state_dict(synthetic_state_dict(1777, 1.0)).eval()
    rng = np.random.Generator(np.random.PCG64(0))
    X_mean = (0.05 * rng.standard_normal((25, 15))).astype(np.float32); X_std = rng.uniform(0.5, 1.5, (25, 15)).astype(np.float32)   # noqa: E702
    Y_mean = (0.05 * rng.standard_normal((25, 15))).astype(np.float32); Y_std = rng.uniform(0.2, 0.6, (25, 15)).astype(np.float32)   # noqa: E702
    model.set_pose_norm(X_mean, X_std, Y_mean, Y_std)
    cnt_mean, cnt_std = synthetic.cnt_norm(7)
    n = N + 15
    raw = [synthetic.raw_walk_clip(LAYOUTS["mocha"]["parents"], n, seed=s) for s in (11, 12)]
    clips = ingest_clips(model, np.concatenate([a for a, _ in raw]), np.concatenate([b for _, b in raw]), [n, n])
    win = clip_windows(clips, [n, n])
    assert win["Yrot"].shape[0] == 2 * N
    for k in ("Yrot", "Ypos", "Yvel", "Yang"):
        assert np.array_equal(z["src_" + k], win[k][:N].cpu().numpy()), k
    ref = CR.process_clip(raw[0][0], raw[0][1], LAYOUTS["mocha"]["parents"], "zyx", (7, 9, 16, 1, 20), (5, 24))
    assert np.array_equal(z["contact"].astype(bool), CR.windows(ref, 60, 1)["contact"][:, -1])
    src_X = model.featurize(*(win[k][:N] for k in ("Yrot", "Ypos", "Yvel", "Yang")))
    cha_X = model.featurize(*(win[k][N:] for k in ("Yrot", "Ypos", "Yvel", "Yang")))
    Y, idx, _, _ = model.characterize_pair(src_X, cha_X, cnt_mean, cnt_std, return_index=True, return_bank=True, raw=True)
    assert np.array_equal(idx.cpu().numpy(), z["idx"]) and np.array_equal(Y.cpu().numpy(), z["Y"])
