"""The world of tests/test_resident_bank.py and tests/test_resident_live.py: the recipe of tests/allow_world.py (mixamo layout, synthetic
weights, smooth_bone_clip banks, smooth stream clips) on TWO Generator instances with the same weights - a context has one current bank, so
the resident bank lives on `model` and the bank it is compared with on `ref_model` - and six characters A .. F of 33, 30, 20, 17, 16 and 1
bank rows (a row count <= 16 also takes the add path's forced-tiled style MLP) with action labels in runs whose edges lie inside and across
the 16-row granules."""
import numpy as np
import torch

from mocha_sigasia2023_amd import Generator, PostProcessor, build_bank, synthetic, weights

V, J = 22, 23
A, B, C, D, E, F = range(6)
ROWS = (33, 30, 20, 17, 16, 1)
# A: actions 0 / 1 / 2 with edges at rows 15 and 17; B: 0 / 1 aligned to 16; C: action 3 only; D: 4 / 5 with the edge at row 9 and one row
# (of action 5) in its second granule; E: 0 / 6 in one granule; F: one row of action 0 (added without labels)
LABELS = (np.array([0] * 15 + [1] * 2 + [2] * 16, np.int32), np.array([0] * 16 + [1] * 14, np.int32), np.full(20, 3, np.int32),
          np.array([4] * 9 + [5] * 8, np.int32), np.array([0] * 5 + [6] * 11, np.int32), np.zeros(1, np.int32))
CAPACITY, MAX_CHARACTERS, MAX_ROWS = 160, 6, 48
SOFT = (3, 2.0)


def dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return torch.device("cuda:0")


def _model(d):
    model = Generator(layout="mixamo", device=d).load_state_dict(weights.synthetic_state_dict(1777, 1.0, "mixamo")).eval()
    rng = np.random.Generator(np.random.PCG64(0))
    X_mean = (0.05 * rng.standard_normal((J, 15))).astype(np.float32); X_std = rng.uniform(0.5, 1.5, (J, 15)).astype(np.float32)
    Y_mean = (0.05 * rng.standard_normal((J, 15))).astype(np.float32); Y_std = rng.uniform(0.2, 0.6, (J, 15)).astype(np.float32)
    model.set_pose_norm(X_mean, X_std, Y_mean, Y_std)
    return model


def build(frames, streams=3):
    d = dev()
    model, ref_model = _model(d), _model(d)
    mean_, std_ = synthetic.cnt_norm(7)
    mean, std = torch.from_numpy(mean_).to(d), torch.from_numpy(std_).to(d)
    banks = []
    for seed, n in zip(range(101, 107), ROWS):
        clip = synthetic.smooth_bone_clip(seed, 60 + n - 1, J)
        X = model.featurize(*[torch.from_numpy(synthetic.slide_windows(a)) for a in clip])
        b = build_bank(model, X, raw=True)
        banks.append((((b["cnt"] - mean) / std).reshape(-1, 90 * 256).contiguous(), b["encoded"].contiguous()))
    clips = [[torch.from_numpy(a).to(d) for a in synthetic.smooth_bone_clip(200 + s, frames, J, phase=0.3 * s)] for s in range(streams)]
    per = []
    for s in range(streams):
        _, rvel, rang, hipvel, contact = synthetic.postprocess_inputs(50 + s, frames)
        per.append([torch.from_numpy(np.ascontiguousarray(a)).to(d) for a in
                    (rvel, rang, np.linalg.norm(hipvel, axis=-1).mean(-1).astype(np.float32), contact)])
    posts = {id(m): PostProcessor(m, contact_bones=[18, 22]) for m in (model, ref_model)}
    torch.cuda.synchronize()
    return dict(model=model, ref_model=ref_model, mean=mean, std=std, banks=banks, clips=clips, per=per, posts=posts, streams=streams)


def windows(w, f):
    """The streams' windows ending at frame f, featurized: (S, 60, J, 15)."""
    S = w["streams"]
    return w["model"].featurize(*[torch.stack([w["clips"][s][k][f - 59: f + 1] for s in range(S)]) for k in range(4)])


def frame(w, f):
    """The inputs of LiveSession.push for frame f of every stream."""
    S = w["streams"]
    bones = [torch.stack([w["clips"][s][k][f] for s in range(S)]) for k in range(4)]
    per = [torch.stack([w["per"][s][k][f] for s in range(S)]) for k in range(4)]
    return bones + per


def first_fit(free, units):
    """The test's own model of first fit over a list of per-unit flags (True = free): the first unit of the lowest run of `units` free
    units, which it takes; None when there is none."""
    run = 0
    for i, f in enumerate(free):
        run = run + 1 if f else 0
        if run == units:
            first = i - units + 1
            free[first:i + 1] = [False] * units
            return first
    return None
