"""LiveSession(world=...) / LiveOursSession(world=...) on the MI355X (run with -m gpu): 2 streams, a 2-character bank of 8 rows each, 62
pushes; stream 1 is reset before push 30, so it is still warming when stream 0 turns valid on push 60.

The session with world=bind returns the same bits in every existing output as the one without; its gpos, grot and palette equal the
stand-alone world_pose on the returned pos and ik_rot, bit for bit, on every valid frame; a warming stream's rows keep their initial fill -
both streams' through push 59, stream 1's to the end; world=True gives gpos and grot and no palette; one LiveOursSession push sequence
has the keys and equals the stand-alone call."""
import numpy as np
import pytest
import torch

import mocha_sigasia2023_amd as M
from mocha_sigasia2023_amd import synthetic, weights

pytestmark = pytest.mark.gpu
LAYOUT, J, V = "mixamo", 23, 22
TOES = (18, 22)
PUSHES, RESET_AT, FILL = 62, 30, 7.5
WORLD_KEYS = ("gpos", "grot", "palette")


def _pose_norm():
    rng = np.random.Generator(np.random.PCG64(0))
    return [(0.05 * rng.standard_normal((J, 15))).astype(np.float32), rng.uniform(0.5, 1.5, (J, 15)).astype(np.float32),
            (0.05 * rng.standard_normal((J, 15))).astype(np.float32), rng.uniform(0.2, 0.6, (J, 15)).astype(np.float32)]


def _stats():
    rng = np.random.Generator(np.random.PCG64(3))
    return [(0.1 * rng.standard_normal((90, 256))).astype(np.float32), rng.uniform(0.5, 1.5, (90, 256)).astype(np.float32),
            (0.1 * rng.standard_normal((90, 256))).astype(np.float32), rng.uniform(0.5, 1.5, (90, 256)).astype(np.float32)]


@pytest.fixture(scope="module")
def world():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    d = torch.device("cuda:0")
    model = M.Generator(layout=LAYOUT, device=d).load_state_dict(weights.synthetic_state_dict(1777, 1.0, LAYOUT)).eval()
    model.set_pose_norm(*_pose_norm())
    mean, std = (torch.from_numpy(a).to(d) for a in synthetic.cnt_norm(7))
    banks = []
    for seed in (121, 103):
        clip = synthetic.smooth_bone_clip(seed, 60 + 8 - 1, J)
        b = M.build_bank(model, model.featurize(*[torch.from_numpy(synthetic.slide_windows(a)) for a in clip]), raw=True)
        banks.append((((b["cnt"] - mean) / std).reshape(-1, 90 * 256), b["encoded"]))
    mb = M.MultiCharacterBank(model, banks)
    post = M.PostProcessor(model, contact_bones=list(TOES))
    rng = np.random.Generator(np.random.PCG64(22))
    rest_rot = rng.standard_normal((J, 4))
    rest_pos = rng.uniform(-0.3, 0.3, (J, 3))
    pre = np.array([[100.0, 0, 0, 1.0], [0, 0, 100.0, 2.0], [0, 100.0, 0, 3.0]])
    bind = M.SkinBind(model, rest_pos, rest_rot, pre)
    # the frames both streams are fed: (S, PUSHES, ...) per argument of push
    clips = [synthetic.smooth_bone_clip(200 + s, PUSHES, J, phase=0.3 * s) for s in range(2)]
    per = []
    for s in range(2):
        _, rvel, rang, hipvel, contact = synthetic.postprocess_inputs(50 + s, PUSHES, V=V)
        per.append((rvel, rang, np.linalg.norm(hipvel, axis=-1).mean(-1).astype(np.float32), contact))
    frames = [np.stack([clips[s][i] for s in range(2)]) for i in range(4)] + [np.stack([per[s][i] for s in range(2)]) for i in range(4)]
    frames = [torch.from_numpy(np.ascontiguousarray(a)).to(d) for a in frames]
    return dict(model=model, mean=mean, std=std, mb=mb, post=post, bind=bind, frames=frames)


def _fill(sess):
    for k in WORLD_KEYS:
        if k in sess.out:
            sess.out[k].fill_(FILL)


def _run(sess, w, check=None):
    """PUSHES pushes with stream 1 reset before push RESET_AT (counted from 1); returns per push a dict of host copies."""
    _fill(sess)
    rec = []
    for k in range(PUSHES):
        if k + 1 == RESET_AT:
            sess.reset([1])
        o = sess.push(*[a[:, k] for a in w["frames"]], characters=[0, 1] if k == 0 else None)
        if check is not None:
            check(k, o)
        torch.cuda.synchronize()
        rec.append({n: t.cpu().numpy().copy() for n, t in o.items()})
    return rec


def _against_standalone(w, bind):
    """The check a run applies after every push: the world outputs against world_pose on the frame just returned."""
    def check(k, o):
        alone = M.world_pose(w["model"], o["ik_rot"], o["pos"], bind=bind)
        torch.cuda.synchronize()
        valid = o["valid"].cpu().numpy().astype(bool)
        assert valid.tolist() == [k + 1 >= 60, False]
        for n in alone:
            got, ref = o[n].cpu().numpy(), alone[n].cpu().numpy()
            assert np.array_equal(got[valid], ref[valid]), (k, n)
            assert np.all(got[~valid] == FILL), (k, n, "a warming stream's rows were written")
            if valid.any():
                assert np.isfinite(got[valid]).all() and not np.any(got[valid] == FILL)
    return check


def test_world_session_keeps_every_existing_output_and_equals_the_standalone_call(world):
    w = world
    plain = _run(M.LiveSession(w["mb"], w["mean"], w["std"], streams=2, post=w["post"]), w)
    sess = M.LiveSession(w["mb"], w["mean"], w["std"], streams=2, post=w["post"], world=w["bind"])
    assert sess.out["gpos"].shape == (2, J, 3) and sess.out["grot"].shape == (2, J, 4) and sess.out["palette"].shape == (2, V, 12)
    assert sess.out["palette"].dtype == torch.float32 and sess.out["gpos"].dtype == sess.out["grot"].dtype == torch.float64
    ptrs = {k: t.data_ptr() for k, t in sess.out.items()}
    both = _run(sess, w, _against_standalone(w, w["bind"]))
    assert {k: t.data_ptr() for k, t in sess.out.items()} == ptrs                     # fixed tensors, overwritten in place
    assert sum(int(r["valid"][0]) for r in both) == 3 and not any(int(r["valid"][1]) for r in both[RESET_AT - 1:])
    for k, (a, b) in enumerate(zip(plain, both)):
        assert set(b) == set(a) | set(WORLD_KEYS)
        for n in a:
            assert np.array_equal(a[n], b[n], equal_nan=True), (k, n)


def test_world_true_gives_poses_without_a_palette(world):
    w = world
    sess = M.LiveSession(w["mb"], w["mean"], w["std"], streams=2, post=w["post"], world=True)
    assert "gpos" in sess.out and "grot" in sess.out and "palette" not in sess.out
    _run(sess, w, _against_standalone(w, None))
    with pytest.raises(TypeError):
        M.LiveSession(w["mb"], w["mean"], w["std"], streams=2, post=w["post"], world="yes")


def test_live_ours_session_has_the_keys(world):
    w = world
    csd = weights.synthetic_cvae_state_dict(99, 1.0)
    sess = M.LiveOursSession(w["mb"], w["mean"], w["std"], csd, *_stats(), streams=2, post=w["post"], noise="none", world=w["bind"])
    assert all(k in sess.out for k in WORLD_KEYS + ("seeded",))
    rec = _run(sess, w, _against_standalone(w, w["bind"]))
    assert [int(r["valid"][0]) for r in rec[-3:]] == [1, 1, 1] and int(rec[59]["seeded"][0]) == 1
