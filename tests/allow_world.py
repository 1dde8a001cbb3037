"""The world of tests/test_allow_steps.py and tests/test_live_allow.py: the model and post-processing of tests/test_live_soft.py (mixamo
layout, synthetic weights), three characters of 33, 30 and 20 bank rows with action labels in runs, three streams of smooth clips."""
import numpy as np
import torch

from mocha_sigasia2023_amd import Generator, MultiCharacterBank, PostProcessor, build_bank, synthetic, weights

V, J = 22, 23
ROWS = (33, 30, 20)
# character 0: actions 0 / 1 / 2 in runs with edges at rows 15 and 17 (inside and across the 16-row workgroups); character 1: 0 / 1 aligned
# to 16; character 2: action 3 only - a mask of the actions 0 .. 2 finds nothing there and falls back
LABELS = (np.array([0] * 15 + [1] * 2 + [2] * 16, np.int32), np.array([0] * 16 + [1] * 14, np.int32), np.full(20, 3, np.int32))
SOFT = (3, 2.0)


def dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return torch.device("cuda:0")


def build(frames, streams=3):
    d = dev()
    model = Generator(layout="mixamo", device=d).load_state_dict(weights.synthetic_state_dict(1777, 1.0, "mixamo")).eval()
    rng = np.random.Generator(np.random.PCG64(0))
    X_mean = (0.05 * rng.standard_normal((J, 15))).astype(np.float32); X_std = rng.uniform(0.5, 1.5, (J, 15)).astype(np.float32)
    Y_mean = (0.05 * rng.standard_normal((J, 15))).astype(np.float32); Y_std = rng.uniform(0.2, 0.6, (J, 15)).astype(np.float32)
    model.set_pose_norm(X_mean, X_std, Y_mean, Y_std)
    mean_, std_ = synthetic.cnt_norm(7)
    mean, std = torch.from_numpy(mean_).to(d), torch.from_numpy(std_).to(d)
    banks = []
    for seed, n in zip((101, 102, 103), ROWS):
        clip = synthetic.smooth_bone_clip(seed, 60 + n - 1, J)
        X = model.featurize(*[torch.from_numpy(synthetic.slide_windows(a)) for a in clip])
        b = build_bank(model, X, raw=True)
        banks.append((((b["cnt"] - mean) / std).reshape(-1, 90 * 256), b["encoded"]))
    mb = MultiCharacterBank(model, banks, labels=LABELS)
    clips = [[torch.from_numpy(a).to(d) for a in synthetic.smooth_bone_clip(200 + s, frames, J, phase=0.3 * s)] for s in range(streams)]
    per = []
    for s in range(streams):
        _, rvel, rang, hipvel, contact = synthetic.postprocess_inputs(50 + s, frames)
        per.append([torch.from_numpy(np.ascontiguousarray(a)).to(d) for a in
                    (rvel, rang, np.linalg.norm(hipvel, axis=-1).mean(-1).astype(np.float32), contact)])
    post = PostProcessor(model, contact_bones=[18, 22])
    zeros = torch.zeros((streams, 60, J, 15), device=d)
    mb.characterize(zeros, [0] * streams, mean, std, raw=True)                # eager first: everything made on first use exists
    mb.characterize(zeros, [0] * streams, mean, std, raw=True, soft=SOFT)
    seg_start = np.concatenate([[0], np.cumsum(ROWS)]).astype(np.int64)
    return dict(model=model, mean=mean, std=std, mb=mb, banks=banks, clips=clips, per=per, post=post, streams=streams,
                rows=torch.cat([b[0] for b in banks]).cpu().numpy(), labels=np.concatenate(LABELS), seg_start=seg_start)


def windows(w, f):
    """The streams' windows ending at frame f, featurized: (S, 60, J, 15)."""
    S = w["streams"]
    return w["model"].featurize(*[torch.stack([w["clips"][s][k][f - 59: f + 1] for s in range(S)]) for k in range(4)])


def queries(w, X):
    """The z-scored context features of raw windows X, on the host: what the matcher is asked with."""
    _, _, nm = w["model"].encode(X, w["mean"], w["std"], raw=True)
    return nm.reshape(X.shape[0], -1).cpu().numpy()
