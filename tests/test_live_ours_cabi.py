"""The C entry points of the live CVAE branch: mocha_live_ours_state_bytes, mocha_live_ours_reset, mocha_live_step_ours.

CPU part: the header, the ctypes binding and the built library agree on the three names and on mocha_ours_cfg, the ABI version is still
6, the Python surface exists, a NULL context is refused before anything touches a device.

GPU part: every refusal of mocha_live_step_ours returns its code and leaves both session buffers as they were; the size of the state
buffer is the documented layout's."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import mocha_sigasia2023_amd as M
from mocha_sigasia2023_amd import _C, synthetic, weights

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["mocha_live_ours_state_bytes", "mocha_live_ours_reset", "mocha_live_step_ours"]
ERR_ARG, ERR_STATE = -1, -3
LAYOUT, J = "mixamo", 23
TOES = (18, 22)                                      # the contact bones of this skeleton (the default configuration names the demo skeleton's)


def _built():
    if not os.path.exists(_C.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _C.load_library()


def test_new_names_in_header_binding_and_library():
    txt = open(os.path.join(REPO, "include", "mocha_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    declared = set(re.findall(r"\b(mocha_[a-z_]+)\s*\(", code))
    lib = _built()
    for n in NEW:
        assert n in declared, f"{n} is not declared in include/mocha_hip.h"
        assert n in _C.SIGNATURES, f"{n} is not bound in _C.SIGNATURES"
        assert hasattr(lib, n), f"libmocha_hip.so does not export {n}"
    # the struct: the header's members in the header's order
    body = re.search(r"typedef struct mocha_ours_cfg \{(.*?)\} mocha_ours_cfg;", code, flags=re.S).group(1)
    members = re.findall(r"\*?\s*(\w+)\s*[,;]", body)
    assert members == [f[0] for f in _C.mocha_ours_cfg._fields_], members
    assert C.sizeof(_C.mocha_ours_cfg) == 4 * 8 + 8 + 8 + 8              # four pointers, int (padded), pointer, uint64
    assert len(_C.SIGNATURES["mocha_live_step_ours"][1]) == len(_C.SIGNATURES["mocha_live_step"][1]) + 3


def test_abi_version_unchanged():
    lib = _built()
    assert _C.ABI_VERSION == 6 and lib.mocha_abi_version() == 6          # additive: existing callers keep working


def test_python_surface():
    assert "LiveOursSession" in M.__all__ and issubclass(M.LiveOursSession, M.LiveSession)
    assert M.LiveOursSession.__module__ == "mocha_sigasia2023_amd.live"
    for name in ("push", "replay", "reset", "run_clip"):
        assert callable(getattr(M.LiveOursSession, name))
    assert isinstance(M.LiveOursSession.cha_encoded, property)
    assert callable(M.Generator.load_cvae) and callable(M.CVAE.load_state_dict)


def test_null_context_is_refused_without_a_device():
    lib = _built()
    buf = (C.c_double * 8)()                       # host memory standing in for device pointers: must never be dereferenced
    p = C.cast(buf, C.c_void_p)
    assert lib.mocha_live_step_ours(None, None, p, 1, *([p] * 22)) == ERR_ARG
    assert lib.mocha_live_ours_reset(None, p, p, 1, None, 0, None) == ERR_ARG
    assert lib.mocha_live_ours_state_bytes(None, 1) < 0


# ------------------------------------------------------------------------------------------------ GPU
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
    sd = weights.synthetic_state_dict(1777, 1.0, LAYOUT)
    model = M.Generator(layout=LAYOUT, device=d).load_state_dict(sd).eval()
    model.set_pose_norm(*_pose_norm())
    mean, std = (torch.from_numpy(a).to(d) for a in synthetic.cnt_norm(7))
    banks = []
    for seed in (121, 103):
        clip = synthetic.smooth_bone_clip(seed, 60 + 8 - 1, J)
        b = M.build_bank(model, model.featurize(*[torch.from_numpy(synthetic.slide_windows(a)) for a in clip]), raw=True)
        banks.append((((b["cnt"] - mean) / std).reshape(-1, 90 * 256), b["encoded"]))
    mb = M.MultiCharacterBank(model, banks)
    post = M.PostProcessor(model, contact_bones=list(TOES))
    return dict(sd=sd, model=model, mean=mean, std=std, mb=mb, post=post)


def _args(sess, **over):
    """The argument list of mocha_live_step_ours for `sess` (after the context), with overrides by name."""
    o = sess.out
    names = ["cfg", "live", "streams", "Yrot", "Ypos", "Yvel", "Yang", "src_rvel", "src_rang", "src_speed", "contact", "seg", "cnt_mean",
             "cnt_std", "ours", "ocfg", "pos", "rot", "ik_rot", "bvh_pos", "bvh_euler", "idx", "valid", "seeded", "stream"]
    p = lambda t: C.c_void_p(t.data_ptr())                                   # noqa: E731
    vals = [C.byref(sess.post.cfg), p(sess.live), sess.streams, p(sess.rot), p(sess.pos), p(sess.vel), p(sess.ang), p(sess.rvel), p(sess.rang),
            p(sess.speed), p(sess.contact), p(sess.ids), p(sess.mean), p(sess.std), p(sess.ours), C.byref(sess.ocfg), p(o["pos"]), p(o["rot"]),
            p(o["ik_rot"]), p(o["bvh_pos"]), p(o["bvh_euler"]), p(o["idx"]), p(o["valid"]), p(o["seeded"]),
            C.c_void_p(torch.cuda.current_stream().cuda_stream)]
    a = dict(zip(names, vals))
    a.update(over)
    return [a[n] for n in names]


def _ocfg(sess, **over):
    f = {n: getattr(sess.ocfg, n) for n, _ in _C.mocha_ours_cfg._fields_}
    f.update(over)
    return C.byref(_C.mocha_ours_cfg(**f))


@pytest.mark.gpu
def test_state_bytes_equal_the_documented_layout(world):
    lib, h = world["model"]._ctx.lib, world["model"]._ctx.h
    T = 90 * 256 * 4
    for S in (1, 3, 16):
        at = 0
        for n in (S * 12, S * T, S * T, S * 2 * T, S * T, S * 1024, S * 1024, S * 1024):
            at += (n + 255) // 256 * 256
        assert int(lib.mocha_live_ours_state_bytes(h, S)) == at
    assert lib.mocha_live_ours_state_bytes(h, 0) == ERR_ARG and lib.mocha_live_ours_state_bytes(h, 17) == ERR_ARG
    assert lib.mocha_abi_version() == 6


@pytest.mark.gpu
def test_refusals_return_their_code_and_leave_the_buffers_unchanged(world):
    model, lib = world["model"], world["model"]._ctx.lib
    csd = weights.synthetic_cvae_state_dict(99, 1.0)
    plain = M.LiveSession(world["mb"], world["mean"], world["std"], streams=2, post=world["post"])

    class Shell:                                                             # a session's buffers without a CVAE on the context yet
        pass
    # 1. the CVAE is not on this context: MOCHA_ERR_STATE
    sh = Shell()
    sh.__dict__.update(plain.__dict__)
    sh.ours = torch.zeros((int(lib.mocha_live_ours_state_bytes(model._ctx.h, 2)),), dtype=torch.uint8, device=model.device)
    stats = [torch.from_numpy(a).to(model.device) for a in _stats()]
    sh.eps = torch.zeros((2, 256), device=model.device)
    sh.ocfg = _C.mocha_ours_cfg(*[t.data_ptr() for t in stats], 1, sh.eps.data_ptr(), 0)
    sh.out = dict(plain.out, seeded=torch.zeros((2,), dtype=torch.int32, device=model.device))
    torch.cuda.synchronize()
    sh_ours0, sh_live0 = sh.ours.clone(), sh.live.clone()
    assert lib.mocha_live_step_ours(model._ctx.h, *_args(sh)) == ERR_STATE
    assert b"CVAE" in lib.mocha_last_error(model._ctx.h)
    torch.cuda.synchronize()
    assert torch.equal(sh.ours, sh_ours0) and torch.equal(sh.live, sh_live0)
    with pytest.raises(RuntimeError, match="load_cvae"):                     # no CVAE to reuse yet
        M.LiveOursSession(world["mb"], world["mean"], world["std"], None, *_stats(), streams=2, post=world["post"])
    # 2. argument refusals on a working session
    sess = M.LiveOursSession(world["mb"], world["mean"], world["std"], csd, *_stats(), streams=2, post=world["post"], noise="given")
    sess.ours.fill_(1)                                                       # recognisable contents (finite as floats)
    torch.cuda.synchronize()
    ours0, live0, out0 = sess.ours.clone(), sess.live.clone(), {k: v.clone() for k, v in sess.out.items()}
    h = model._ctx.h
    cases = [("ours", dict(ours=None)), ("ocfg", dict(ocfg=None)), ("seeded", dict(seeded=None)), ("live", dict(live=None)), ("Yrot", dict(Yrot=None)),
             ("seg", dict(seg=None)), ("cnt_std", dict(cnt_std=None)), ("idx", dict(idx=None)), ("bvh one of two", dict(bvh_pos=None)),
             ("streams 0", dict(streams=0)), ("streams 17", dict(streams=17)),
             ("noise 3", dict(ocfg=_ocfg(sess, noise=3))), ("noise -1", dict(ocfg=_ocfg(sess, noise=-1))), ("noise 1 without eps", dict(ocfg=_ocfg(sess, eps=None)))]
    cases += [(n, dict(ocfg=_ocfg(sess, **{n: None}))) for n in ("src_cnt_mean", "src_cnt_std", "cha_encoded_mean", "cha_encoded_std")]
    for name, over in cases:
        assert lib.mocha_live_step_ours(h, *_args(sess, **over)) == ERR_ARG, name
    assert lib.mocha_live_ours_reset(h, C.c_void_p(sess.live.data_ptr()), None, 2, None, 0, None) == ERR_ARG
    assert lib.mocha_live_ours_reset(h, C.c_void_p(sess.live.data_ptr()), C.c_void_p(sess.ours.data_ptr()), 2, (C.c_int32 * 1)(2), 1, None) == ERR_ARG
    # 3. state refusals on other contexts: no weights, no pose norm, no bank (the CVAE loaded)
    bare = M.Generator(layout=LAYOUT, device=model.device)
    assert lib.mocha_live_step_ours(bare._ctx.h, *_args(sess)) == ERR_STATE
    other = M.Generator(layout=LAYOUT, device=model.device).load_state_dict(world["sd"]).load_cvae(csd)
    assert lib.mocha_live_step_ours(other._ctx.h, *_args(sess)) == ERR_STATE and b"pose norm" in lib.mocha_last_error(other._ctx.h)
    other.set_pose_norm(*_pose_norm())
    assert lib.mocha_live_step_ours(other._ctx.h, *_args(sess)) == ERR_STATE and b"bank" in lib.mocha_last_error(other._ctx.h)
    # 4. a workspace limit below the number of streams: the branch runs all the streams in one piece, so the step refuses
    other.reserve(1)
    assert lib.mocha_live_step_ours(other._ctx.h, *_args(sess)) == ERR_ARG and b"mocha_reserve" in lib.mocha_last_error(other._ctx.h)
    torch.cuda.synchronize()
    assert torch.equal(sess.ours, ours0) and torch.equal(sess.live, live0)
    assert all(torch.equal(sess.out[k], out0[k]) for k in out0)
    # ... and the session still works: a reset through the C call, then a step
    sess.reset()
    torch.cuda.synchronize()
    assert not sess.ours[:24].any() and torch.equal(sess.ours[256:], ours0[256:])
    assert lib.mocha_live_step_ours(h, *_args(sess)) == 0
    torch.cuda.synchronize()
    assert sess.out["valid"].tolist() == [0, 0] and sess.out["seeded"].tolist() == [0, 0]
    # a second session reuses the model's CVAE: nothing is loaded, the context's generation does not move
    gen = model._ctx.generation()
    again = M.LiveOursSession(world["mb"], world["mean"], world["std"], None, *_stats(), streams=2, post=world["post"], noise="none")
    assert model._ctx.generation() == gen and again.ours.numel() == sess.ours.numel()
