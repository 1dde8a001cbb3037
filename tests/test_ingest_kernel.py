"""mocha_live_ingest_step on the MI355X (run with -m gpu): the streaming mocap front end against the reference's own process_data
(tests/golden/live_ingest.npz: V = 24, Euler degrees + centimetres, every prefix 31..100, L in {0, 2, 7, 18}) and against the NumPy
restatement tests/ingest_ref.py (V = 22, quaternion input in metres, L in {0, 1, 18}).

Three streams share every call: stream 0 runs from frame 0, stream 1 is reset after 5 pushes and starts the clip then, stream 2 is reset
after push 50 and starts over.  Per element |got - ref| <= np.spacing(float32(|ref|)) + 4 E: one rounding to fp32 (the precedent of
test_inertialize_kernel.py) plus a floor of four times the restatement's own measured deviation from the reference (ingest_ref.E) - device
libm and FMA contraction differ from NumPy by a few float64 ulps.  Contacts and `have` are exact, every output sits between guard words,
and a stream with have == 0 leaves its rows as they were."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ingest_ref as R  # noqa: E402
from mocha_sigasia2023_amd import Generator, IngestConfig, Ingestor, PostProcessor  # noqa: E402
from mocha_sigasia2023_amd.skeleton import LAYOUTS  # noqa: E402

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "live_ingest.npz")
S, LATE, RESET, PUSHES, GUARD = 3, 5, 50, 105, 64
FLOAT_KEYS = ("Yrot", "Ypos", "Yvel", "Yang", "src_rvel", "src_rang", "src_speed")
FILL = {torch.float32: 7.5, torch.uint8: 0xAB, torch.int32: -77}


def dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return torch.device("cuda:0")


def _guard(ing):
    """Every output of the stepper re-seated between GUARD sentinel words on either side; returns the padded buffers."""
    bufs = {}
    for k, t in ing.out.items():
        buf = torch.full((t.numel() + 2 * GUARD,), FILL[t.dtype], dtype=t.dtype, device=t.device)
        ing.out[k] = buf[GUARD: GUARD + t.numel()].view(t.shape)
        bufs[k] = buf
    return bufs


def _count(i, s):
    """Frames stream s has pushed since its last reset, after push i (0-based) - and the clip frame that push carried."""
    n = i + 1 if s == 0 else (i + 1 - LATE if i >= LATE else i + 1) if s == 1 else (i + 1 - RESET if i >= RESET else i + 1)
    return n, min(n - 1, 99)


def _drive(ing, rot, pos):
    """PUSHES calls; returns per key the outputs before the first and after every call stacked (1 + PUSHES, S, ...), on the host."""
    bufs = _guard(ing)
    seen = {k: [v.clone()] for k, v in ing.out.items()}
    for i in range(PUSHES):
        if i == LATE:
            ing.reset([1])
        if i == RESET:
            ing.reset([2])
        f = [_count(i, s)[1] for s in range(S)]
        o = ing.step(np.stack([rot[x] for x in f]), np.stack([pos[x] for x in f]))
        for k in seen:
            seen[k].append(o[k].clone())
    torch.cuda.synchronize()
    for k, buf in bufs.items():
        edge = torch.cat([buf[:GUARD], buf[-GUARD:]])
        assert bool((edge == FILL[buf.dtype]).all()), f"guard words of {k} were written"
    return {k: torch.stack(v).cpu().numpy() for k, v in seen.items()}


def _check(seen, expect):
    """expect(n) -> dict of float64 references for a stream that has pushed n >= 31 frames."""
    worst = {k: 0.0 for k in FLOAT_KEYS}
    for i in range(PUSHES):
        for s in range(S):
            n, _ = _count(i, s)
            if n < R.FIRST or n > 100:
                if n < R.FIRST:
                    assert seen["have"][i + 1, s] == 0, (i, s)
                    for k in seen:                                   # untouched: the sentinel, or what the stream held before its reset
                        if k != "have":
                            assert np.array_equal(seen[k][i + 1, s], seen[k][i, s]), (k, i, s)
                continue
            assert seen["have"][i + 1, s] == 1, (i, s)
            ref = expect(n)
            assert np.array_equal(seen["contact"][i + 1, s].astype(bool), ref["contact"]), (i, s, n)
            for k in FLOAT_KEYS:
                r = np.asarray(ref[k], np.float64)
                err = np.abs(seen[k][i + 1, s].astype(np.float64) - r)
                bound = np.spacing(np.abs(r).astype(np.float32)).astype(np.float64) + 4.0 * R.E
                worst[k] = max(worst[k], float((err / bound).max()))
                assert np.all(err <= bound), (k, i, s, n, float(err.max()), float((err / bound).max()))
    print("largest error / bound:", {k: f"{v:.3f}" for k, v in worst.items()})


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(GOLD))


@pytest.fixture(scope="module")
def model24():
    return Generator(layout="mocha", device=dev())


@pytest.fixture(scope="module")
def derived24(gold):
    """The restatement's src_rvel / src_rang / src_speed for the fixture's clip: the reference's process_data has no such outputs."""
    out = {}
    for L in gold["lookahead"]:
        st = R.IngestRef(gold["parents"], int(L), str(gold["order"]), (7, 9, 16, 1, 20), (5, 24))
        out[int(L)] = [st.push(gold["rot"][f], gold["pos"][f]) for f in range(100)]
    return out


@pytest.mark.parametrize("li", [0, 1, 2, 3], ids=["L0", "L2", "L7", "L18"])
def test_against_the_reference(gold, model24, derived24, li):
    L = int(gold["lookahead"][li])
    ing = Ingestor(model24, IngestConfig(lookahead=L, order=str(gold["order"])), streams=S)
    seen = _drive(ing, gold["rot"], gold["pos"])

    def expect(n):
        d = derived24[L][n - 1]
        return {"Yrot": gold["out_rot"][li, n - 31], "Ypos": gold["out_pos"][li, n - 31], "Yvel": gold["out_vel"][li, n - 31],
                "Yang": gold["out_ang"][li, n - 31], "contact": gold["out_contact"][li, n - 31], "src_rvel": d["src_rvel"],
                "src_rang": d["src_rang"], "src_speed": d["src_speed"]}
    _check(seen, expect)


@pytest.fixture(scope="module")
def world22():
    par = LAYOUTS["mixamo"]["parents"]
    rot, pos = R.walk_clip(par, 100, seed=77, legs=((18, 19, 20, 21), (14, 15, 16, 17)), shoulders=(6, 10), spine=(1, 2, 3), flip_bone=9)
    quat = R.euler_to_quat(rot)                                   # fp32, not unrolled: the wrap of flip_bone is a sign flip in the input
    metres = (pos.astype(np.float64) * 0.01).astype(np.float32)
    return dict(model=Generator(layout="mixamo", device=dev()), parents=par, quat=quat, pos=metres)


@pytest.mark.parametrize("L", [0, 1, 18])
def test_quaternion_input_against_the_restatement(world22, L):
    w = world22
    post = PostProcessor(w["model"], contact_bones=[22, 18])       # left and right toe of the mixamo layout, root bone in front
    ing = Ingestor(w["model"], IngestConfig(lookahead=L, order=None, unit_scale=1.0), streams=S, post=post)
    st = R.IngestRef(w["parents"], L, None, (3, 6, 10, 18, 14), (22, 18), unit_scale=1.0)
    ref = [st.push(w["quat"][f], w["pos"][f]) for f in range(100)]
    assert any(np.sum(w["quat"][f, 9].astype(np.float64) * w["quat"][f - 1, 9]) < 0 for f in range(1, 100)), "no sign flip in the input"
    seen = _drive(ing, w["quat"], w["pos"])

    def expect(n):
        d = ref[n - 1]
        return {"Yrot": d["rot"], "Ypos": d["pos"], "Yvel": d["vel"], "Yang": d["ang"], "contact": d["contact"], "src_rvel": d["src_rvel"],
                "src_rang": d["src_rang"], "src_speed": d["src_speed"]}
    _check(seen, expect)
    assert any(ref[n - 1]["contact"].any() for n in range(31, 101)) and not all(ref[n - 1]["contact"].all() for n in range(31, 101))
