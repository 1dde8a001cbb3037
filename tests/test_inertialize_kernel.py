"""mocha_inertialize at the kernel boundary on the MI355X (run with -m gpu): Inertializer.step, frame by frame, against the float64
restatement tests/inertial_ref.py (which tests/test_inertial_ref.py pins to the reference's own functions without a GPU).

Bound per element: np.spacing(float32(|ref|)) + 1e-12.  Device and NumPy float64 differ by a few float64 ulps (fused multiply-adds, libm), so
the single rounding to fp32 can land one fp32 ulp apart; the floor covers values near zero.  The inputs obey the two conditions that keep
the reference single-valued (no offset quaternion with |w| < 1e-3 before quat.abs, no length between 0 and 1e-3 at quat.log / quat.exp),
so no branch can be taken differently.  24 frames exercise the stored offsets.  Everything else compares runs of the same kernel and is
exact."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import inertial_ref as R                                                    # noqa: E402
from mocha_sigasia2023_amd import Generator, Inertializer, _C, synthetic_state_dict  # noqa: E402
from mocha_sigasia2023_amd.generator import _ptr                            # noqa: E402

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "inertialize.npz")
ERR_ARG = -1
F = 24


@pytest.fixture(scope="module")
def models():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return {22: Generator(layout="mixamo", device="cuda:0").load_state_dict(synthetic_state_dict(3, 1.0, "mixamo")).eval(),
            24: Generator(device="cuda:0").load_state_dict(synthetic_state_dict(3, 1.0)).eval()}


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(GOLD))


def _bits(t):
    return t.detach().cpu().numpy().view(np.uint32)


def _check(got, ref64, what):
    got = got.detach().cpu().numpy().astype(np.float64)
    err = np.abs(got - ref64)
    bound = R.ulp_bound(ref64)
    worst = float((err / bound).max())
    print(f"{what}: max |kernel - restatement| / bound = {worst:.3f}, max abs {float(err.max()):.3e}")
    assert (err <= bound).all(), (what, worst)


def _drive(inert, heads, ref, **per_frame):
    """Both sides frame by frame; the kernel runs out of place."""
    dev = inert.model.device
    n = heads.shape[1]
    state = inert.state(n)
    for f in range(heads.shape[0]):
        kw = {k: v[f] for k, v in per_frame.items()}
        want = ref.step(heads[f], **kw)
        got = inert.step(state, torch.from_numpy(heads[f]).to(dev), **{k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in kw.items()})
        ok = ~np.isnan(want).all(axis=(1, 2))                                # streams with valid == 0 have no output
        if ok.any():
            _check(got[torch.from_numpy(ok).to(dev)], want[ok], f"frame {f}")
    return state


def test_fixture_main_run(models, gold):
    g = gold
    inert = Inertializer(models[22], halflife=0.1)
    ref = R.InertialRef(3, 22, halflife=0.1)
    _drive(inert, g["heads"], ref, ids=g["ids"])
    assert ref.single_valued()


@pytest.mark.parametrize("i", range(4))
def test_fixture_half_lives(models, gold, i):
    """Stream 2 alone at half-lives 0.02, 0.1, 1.0 and 0, transitions as triggers, warming frames through valid."""
    g = gold
    hl = float(g["hl"][i])
    inert = Inertializer(models[22], halflife=hl)
    ref = R.InertialRef(1, 22, halflife=hl)
    _drive(inert, g["heads"][:, 2:3], ref, trigger=g["hl_trigger"][i][:, None], valid=g["hl_valid"][i][:, None])
    assert ref.single_valued()


@pytest.mark.parametrize("seed,n,V", R.SEEDED)
def test_seeded_streams(models, seed, n, V):
    heads, ids = R.switched_streams(seed, F, n, V)
    ref = R.InertialRef(n, V)
    _drive(Inertializer(models[V]), heads, ref, ids=ids)
    assert ref.single_valued()                                               # the conditions, checked on the CPU


def test_in_place_equals_out_of_place_and_guards_are_intact(models):
    V, n = 24, 17
    heads, ids = R.switched_streams(102, F, n, V)
    inert = Inertializer(models[V])
    dev = inert.model.device
    sa, sb = inert.state(n), inert.state(n)
    guard = 64
    for f in range(F):
        h = torch.from_numpy(heads[f]).to(dev)
        i = torch.from_numpy(ids[f]).to(dev)
        buf = torch.full((guard + n * V * 13 + guard,), -77.25, dtype=torch.float32, device=dev)
        out = buf[guard: guard + n * V * 13].view(n, V, 13)
        a = inert.step(sa, h, ids=i, out=out)
        assert a.data_ptr() == out.data_ptr()
        b = h.clone()
        assert inert.step(sb, b, ids=i, out=b) is b
        assert np.array_equal(_bits(a), _bits(b)), f
        assert bool((buf[:guard] == -77.25).all()) and bool((buf[-guard:] == -77.25).all()), f
    assert torch.equal(sa, sb)


def test_pass_through_is_bit_identical(models, gold):
    """Stream 0 never transitions: its rows come back bit for bit, the planted -0.0 included."""
    g = gold
    inert = Inertializer(models[22])
    dev = inert.model.device
    state = inert.state(3)
    for f in range(F):
        h = torch.from_numpy(g["heads"][f]).to(dev)
        out = inert.step(state, h, ids=torch.from_numpy(g["ids"][f]))
        assert np.array_equal(_bits(out[0]), g["heads"][f, 0].view(np.uint32)), f
        if f == 3:
            assert np.signbit(out[0, 2, 0].item())
    assert not np.array_equal(_bits(out[1]), g["heads"][F - 1, 1].view(np.uint32))       # stream 1 is being inertialized


def test_invalid_rows_are_untouched_and_clear_the_state(models, gold):
    g = gold
    inert = Inertializer(models[22])
    dev = inert.model.device
    state = inert.state(3)
    for f in range(8):                                                       # stream 1 has switched at 5 and 6: it is active
        inert.step(state, torch.from_numpy(g["heads"][f]).to(dev), ids=torch.from_numpy(g["ids"][f]))
    valid = torch.tensor([1, 0, 1], dtype=torch.int32)
    out = torch.full((3, 22, 13), 123.5, dtype=torch.float32, device=dev)
    inert.step(state, torch.from_numpy(g["heads"][8]).to(dev), ids=torch.from_numpy(g["ids"][8]), valid=valid, out=out)
    assert bool((out[1] == 123.5).all()) and not bool((out[0] == 123.5).any())
    # in place as well: the invalid stream's input rows stay as they are
    h = torch.from_numpy(g["heads"][9]).to(dev)
    keep = h.clone()
    inert.step(state, h, ids=torch.from_numpy(g["ids"][9]), valid=valid, out=h)
    assert torch.equal(h[1], keep[1])
    # the next valid frame of the cleared stream is a first frame: the input bit for bit, although its id differs from the last one seen
    h = torch.from_numpy(g["heads"][10]).to(dev)
    out = inert.step(state, h, ids=torch.tensor([0, 1, 3], dtype=torch.int32))
    assert np.array_equal(_bits(out[1]), g["heads"][10, 1].view(np.uint32))
    # ... and it equals a fresh state's first frame, then follows it through a switch
    fresh = inert.state(1)
    inert.step(fresh, h[1:2], ids=torch.tensor([1], dtype=torch.int32))
    h = torch.from_numpy(g["heads"][11]).to(dev)
    a = inert.step(state, h, ids=torch.tensor([0, 2, 3], dtype=torch.int32))
    b = inert.step(fresh, h[1:2], ids=torch.tensor([2], dtype=torch.int32))
    assert np.array_equal(_bits(a[1]), _bits(b[0])) and not np.array_equal(_bits(a[1]), g["heads"][11, 1].view(np.uint32))
    # zeroed bytes are a reset as well
    state[1].zero_()
    out = inert.step(state, h, ids=torch.tensor([0, 0, 3], dtype=torch.int32))
    assert np.array_equal(_bits(out[1]), g["heads"][11, 1].view(np.uint32))


def test_ids_and_triggers_give_the_same_bits(models, gold):
    g = gold
    inert = Inertializer(models[22])
    dev = inert.model.device
    sa, sb = inert.state(3), inert.state(3)
    for f in range(F):
        h = torch.from_numpy(g["heads"][f]).to(dev)
        trig = (g["ids"][f] != g["ids"][f - 1]).astype(np.int32) if f else np.zeros(3, np.int32)
        a = inert.step(sa, h, ids=torch.from_numpy(g["ids"][f]))
        b = inert.step(sb, h, trigger=torch.from_numpy(trig))
        assert np.array_equal(_bits(a), _bits(b)), f


def test_a_cloned_state_replays_the_frame(models, gold):
    g = gold
    inert = Inertializer(models[22])
    dev = inert.model.device
    state = inert.state(3)
    for f in range(F):
        h = torch.from_numpy(g["heads"][f]).to(dev)
        i = torch.from_numpy(g["ids"][f])
        snap = state.clone()
        a = inert.step(state, h, ids=i)
        b = inert.step(snap, h, ids=i)
        assert np.array_equal(_bits(a), _bits(b)) and torch.equal(state, snap), f


def test_no_streams_and_every_refusal(models):
    m = models[22]
    inert = Inertializer(m)
    lib, ctx = m._ctx.lib, m._ctx.h
    dev = m.device
    nbytes = lib.mocha_inert_state_bytes(ctx)
    assert nbytes > 0 and nbytes % 8 == 0 and lib.mocha_inert_state_bytes(None) == ERR_ARG
    assert inert.state(2).shape == (2, nbytes) and not bool(inert.state(2).any())
    out = inert.step(inert.state(0), torch.zeros((0, 22, 13), device=dev))
    assert out.shape == (0, 22, 13)
    assert lib.mocha_inertialize_step(ctx, None, None, None, None, None, None, None, 0, None) == 0       # n == 0: a no-op
    state = inert.state(1)
    h = torch.full((1, 22, 13), 0.5, device=dev)
    o = torch.full((1, 22, 13), -3.0, device=dev)
    cfg = _C.mocha_inert_cfg(0.1, 1 / 60)

    def call(cfg_, st, hi, ho, n=1):
        return lib.mocha_inertialize_step(ctx, C.byref(cfg_) if cfg_ is not None else None, _ptr(st), _ptr(hi), _ptr(ho), None, None, None, n, None)
    assert lib.mocha_inertialize_step(None, C.byref(cfg), _ptr(state), _ptr(h), _ptr(o), None, None, None, 1, None) == ERR_ARG
    assert call(cfg, None, h, o) == ERR_ARG and call(cfg, state, None, o) == ERR_ARG and call(cfg, state, h, None) == ERR_ARG
    assert call(cfg, state, h, o, n=-1) == ERR_ARG
    for bad in ((-0.1, 1 / 60), (0.1, 0.0), (0.1, -1.0), (float("nan"), 1 / 60), (0.1, float("inf")), (float("inf"), 1 / 60)):
        assert call(_C.mocha_inert_cfg(*bad), state, h, o) == ERR_ARG, bad
    torch.cuda.synchronize()
    assert bool((o == -3.0).all()) and not bool(state.any())                 # nothing was launched
    assert call(_C.mocha_inert_cfg(0.0, 1 / 60), state, h, o) == 0           # half-life 0 is legal
    assert call(None, state, h, o) == 0                                      # NULL = {0.1, 1/60}
    torch.cuda.synchronize()
    assert torch.equal(o, h)
    with pytest.raises(ValueError):
        inert.step(torch.zeros((1, nbytes), dtype=torch.uint8), h)
    with pytest.raises(ValueError):
        inert.step(state, h, ids=[0, 1])
