"""mocha_world_bind / mocha_world_pose on the MI355X (run with -m gpu), through the C ABI, on both shipped skeletons, against
tests/world_ref.py and the fixture tests/golden/world_pose.npz that test_world_ref.py pins to the reference's quat.fk / to_xform / normalize.
Frame counts sit around the kernel's frames per workgroup F = 8: 1, F-1, F, F+1 and 67 (nine workgroups, the last one of three frames).

float64 outputs: per frame, largest |device - longdouble restatement| / largest |restatement| of that output <= 4 E_ref, E_ref being the
same figure for the reference's own float64 quat.fk (stored in the fixture, reproduced by test_world_ref.py; 3.7e-16 .. 5.8e-16).  The
device and the reference run the same chain of a few roundings per tree level; FMA contraction and a different summation order justify a
small integer margin and no more.
Palette: |device - fp32(float64 restatement)| <= one fp32 spacing at the largest magnitude of the entry's own group (the 3x3 block or the
translation column of that matrix).  Exact: identity bind and identity pre give fp32([to_xform(grot) | gpos]) of the float64 outputs of the
same launch; at the rest-pose frame every bone's palette is `pre` within the same bound (the fixture stores its rest quaternions 256 long
for this: tests/golden/make_golden_world.py says why unit-length ones miss it by 6 to 9 spacings in exact arithmetic).
Bit for bit: n frames in a call against each frame alone; the fp32-input instance against the float64 one on the widened inputs; `valid`
with zeros leaves those rows' fill in all three outputs and changes no other row; a NaN frame changes its own rows only; any output NULL
leaves the others' bits; the guard words around every output stay.  Refusals return MOCHA_ERR_ARG and write nothing.

Measured on the MI355X (the figures test_float64_against_longdouble and test_palette print): device error 0.00 .. 0.79 E_ref for grot and
0.28 .. 1.14 E_ref for gpos, the largest at 67 frames on the 24-joint skeleton; palette error at most 0.0005 of its bound in every case
(the fp32 values are the restatement's everywhere but in entries that cancel at the rest-pose frame).  With the rest quaternions at unit
length (test_unit_length_rest_quaternions: every frame but the rest-pose one, same bound) no palette entry differs from the restatement."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import world_ref as WR  # noqa: E402
from mocha_sigasia2023_amd import Generator  # noqa: E402

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "world_pose.npz")
NAMES = ["mocha", "mixamo"]
FPB = 8                                        # WORLD_FPB of csrc/kernels.h
COUNTS = [1, FPB - 1, FPB, FPB + 1, 67]
GUARD, FILL, ERR_ARG = 64, 7.5, -1
KEYS = ("gpos", "grot", "palette")
WIDTH = {"gpos": 3, "grot": 4, "palette": 12}


def dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return torch.device("cuda:0")


def _ptr(t, at=0):
    return C.c_void_p(0 if t is None else t.data_ptr() + at * t.element_size())


def _stream():
    return C.c_void_p(torch.cuda.current_stream(dev()).cuda_stream)


class Rig:
    """One skeleton: the model, the fixture's arrays on the device, the fixture's bind and an identity bind."""

    def __init__(self, name, gold):
        self.g = g = {k[: -len(name) - 1]: v for k, v in gold.items() if k.endswith("_" + name)}
        self.par = WR.bone_parents(g["parents"])
        self.pre = gold["pre"]
        self.model = Generator(layout=name, device=dev())
        self.V, self.J = self.model.V, self.model.V + 1
        self.lib, self.h = self.model._ctx.lib, self.model._ctx.h
        self.rot, self.pos = self.up(g["rot"]), self.up(g["pos"])
        self.bind = self.make_bind(g["rest_rot"], g["rest_pos"], self.pre)
        self.bind_eye = self.make_bind(None, np.zeros((self.J, 3)), None)

    @staticmethod
    def up(a):
        return torch.from_numpy(np.ascontiguousarray(a)).to(dev())

    def make_bind(self, rest_rot, rest_pos, pre, expect=0):
        nbytes = int(self.lib.mocha_world_bind_bytes(self.h))
        assert nbytes > 0 and nbytes % 8 == 0
        buf = torch.full((nbytes // 8 + 2 * GUARD,), FILL, dtype=torch.float64, device=dev())
        rr = None if rest_rot is None else self.up(np.asarray(rest_rot, np.float64))
        rp = self.up(np.asarray(rest_pos, np.float64))
        arr = None if pre is None else (C.c_double * 12)(*np.asarray(pre, np.float64).reshape(-1).tolist())
        rc = self.lib.mocha_world_bind(self.h, _ptr(rr), _ptr(rp), arr, _ptr(buf, GUARD), _stream())
        torch.cuda.synchronize()
        assert rc == expect, (rc, self.lib.mocha_last_error(self.h))
        assert bool((torch.cat([buf[:GUARD], buf[-GUARD:]]) == FILL).all()), "guard words of the bind were written"
        if expect:
            assert bool((buf == FILL).all()), "a refused mocha_world_bind wrote the bind"
        return buf[GUARD: -GUARD]

    def buffers(self, n):
        """Guarded outputs for n frames: {key: (whole buffer, view (n, rows, width))}."""
        out = {}
        for k, rows, dt in (("gpos", self.J, torch.float64), ("grot", self.J, torch.float64), ("palette", self.V, torch.float32)):
            b = torch.full((n * rows * WIDTH[k] + 2 * GUARD,), FILL, dtype=dt, device=dev())
            out[k] = (b, b[GUARD: GUARD + n * rows * WIDTH[k]].view(n, rows, WIDTH[k]))
        return out

    def launch(self, rot, pos, n, bufs, want=KEYS, valid=None, bind="fixture", at=0, src=0, count=None):
        """mocha_world_pose on frames src .. src+count-1 of rot / pos into rows at .. of the wanted outputs.  Returns the status."""
        count = n if count is None else count
        b = {"fixture": self.bind, "eye": self.bind_eye, None: None}[bind] if not isinstance(bind, torch.Tensor) else bind
        ptr = {k: (_ptr(bufs[k][1], at * bufs[k][1].shape[1] * WIDTH[k]) if k in want else None) for k in KEYS}
        return self.lib.mocha_world_pose(self.h, _ptr(rot, src * self.J * 4), _ptr(pos, src * self.J * 3), 1 if rot.dtype == torch.float32 else 0,
                                         count, _ptr(valid), _ptr(b), ptr["gpos"], ptr["grot"], ptr["palette"], _stream())

    def run(self, rot, pos, n, want=KEYS, valid=None, bind="fixture"):
        """One call on the first n frames; checks the guards; returns {key: array on the host} with the fill where nothing was written."""
        bufs = self.buffers(n)
        rc = self.launch(rot, pos, n, bufs, want, valid, bind)
        torch.cuda.synchronize()
        assert rc == 0, (rc, self.lib.mocha_last_error(self.h))
        return self.read(bufs, want)

    @staticmethod
    def read(bufs, want=KEYS):
        for k, (b, v) in bufs.items():
            assert bool((torch.cat([b[:GUARD], b[-GUARD:]]) == FILL).all()), f"guard words of {k} were written"
            if k not in want:
                assert bool((b == FILL).all()), f"{k} was not asked for and was written"
        return {k: bufs[k][1].cpu().numpy() for k in KEYS}


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(GOLD))


@pytest.fixture(scope="module")
def rigs(gold):
    return {name: Rig(name, gold) for name in NAMES}


@pytest.fixture(scope="module")
def full(rigs):
    """All 67 frames, all three outputs, the fixture's bind: computed once, shared, never modified."""
    return {name: r.run(r.rot, r.pos, 67) for name, r in rigs.items()}


@pytest.fixture(scope="module")
def truth(rigs):
    """The longdouble restatement of the 67 frames: (grot, gpos)."""
    return {name: WR.fk(r.g["rot"], r.g["pos"], r.par, np.longdouble) for name, r in rigs.items()}


def _group_bound(ref):
    """One fp32 spacing at the largest magnitude of the 3x3 block / the translation column of every (..,12) matrix."""
    m = np.abs(ref.astype(np.float64)).reshape(ref.shape[:-1] + (3, 4))
    big = np.concatenate([np.broadcast_to(m[..., :3].max(axis=(-1, -2))[..., None, None], m.shape[:-1] + (3,)),
                          np.broadcast_to(m[..., 3].max(axis=-1)[..., None, None], m.shape[:-1] + (1,))], axis=-1)
    return np.spacing(big.astype(np.float32)).astype(np.float64).reshape(ref.shape)


@pytest.mark.parametrize("n", COUNTS)
@pytest.mark.parametrize("name", NAMES)
def test_float64_against_longdouble(rigs, truth, full, name, n):
    r = rigs[name]
    got = full[name] if n == 67 else r.run(r.rot, r.pos, n, want=("gpos", "grot"), bind=None)
    e_rot, e_pos = WR.frame_error(got["grot"][:n], truth[name][0][:n]), WR.frame_error(got["gpos"][:n], truth[name][1][:n])
    E_rot, E_pos = float(r.g["E_rot"]), float(r.g["E_pos"])
    print(f"{name} n={n}: device error rot {e_rot:.3g} = {e_rot / E_rot:.2f} E_ref, pos {e_pos:.3g} = {e_pos / E_pos:.2f} E_ref")
    assert e_rot <= 4.0 * E_rot and e_pos <= 4.0 * E_pos, (e_rot / E_rot, e_pos / E_pos)


@pytest.mark.parametrize("n", COUNTS)
@pytest.mark.parametrize("name", NAMES)
def test_palette(rigs, full, name, n):
    r = rigs[name]
    got = full[name] if n == 67 else r.run(r.rot, r.pos, n)
    ref = r.g["palette"][:n]
    err = np.abs(got["palette"][:n].astype(np.float64) - ref.astype(np.float64))
    bound = _group_bound(ref)
    print(f"{name} n={n}: palette, largest error / bound {float((err / bound).max()):.3f}")
    assert np.all(err <= bound), (float((err / bound).max()), np.argwhere(err > bound)[:4].tolist())
    if n >= 2:                                                      # frame 1 is the rest pose: every bone's matrix is pre
        pre = np.broadcast_to(r.pre.reshape(12), (r.V, 12))
        dev_ = np.abs(got["palette"][1].astype(np.float64) - pre)
        assert np.all(dev_ <= _group_bound(pre.astype(np.float32))), float((dev_ / _group_bound(pre.astype(np.float32))).max())


@pytest.mark.parametrize("name", NAMES)
def test_identity_bind_is_the_world_transform(rigs, name):
    r = rigs[name]
    got = r.run(r.rot, r.pos, 67, bind="eye")
    want = np.concatenate([WR.to_xform(got["grot"][:, 1:]), got["gpos"][:, 1:, :, None]], axis=-1).reshape(67, r.V, 12).astype(np.float32)
    assert np.array_equal(got["palette"], want)


@pytest.mark.parametrize("name", NAMES)
def test_each_frame_alone(rigs, full, name):
    r = rigs[name]
    bufs = r.buffers(67)
    for i in range(67):
        assert r.launch(r.rot, r.pos, 67, bufs, at=i, src=i, count=1) == 0
    torch.cuda.synchronize()
    alone = r.read(bufs)
    for k in KEYS:
        assert np.array_equal(alone[k], full[name][k]), k
    for n in COUNTS[:-1]:
        head = r.run(r.rot, r.pos, n)
        assert all(np.array_equal(head[k], full[name][k][:n]) for k in KEYS), n


@pytest.mark.parametrize("name", NAMES)
def test_fp32_inputs_are_the_widened_inputs(rigs, name):
    r = rigs[name]
    rot32, pos32 = r.g["rot"].astype(np.float32), r.g["pos"].astype(np.float32)
    a = r.run(r.up(rot32), r.up(pos32), 67)
    b = r.run(r.up(rot32.astype(np.float64)), r.up(pos32.astype(np.float64)), 67)
    for k in KEYS:
        assert np.array_equal(a[k], b[k]), k
    for n in (1, FPB + 1):
        h = r.run(r.up(rot32), r.up(pos32), n)
        assert all(np.array_equal(h[k], a[k][:n]) for k in KEYS), n


@pytest.mark.parametrize("name", NAMES)
def test_valid_rows_and_nan_frames(rigs, full, name):
    r = rigs[name]
    keep = np.ones(67, np.int32)
    keep[[0, 5, FPB - 1, FPB, 2 * FPB + 1, 40, 41, 42, 43, 44, 45, 46, 47, 66]] = 0      # singles, a workgroup's edge, one whole workgroup, the last
    got = r.run(r.rot, r.pos, 67, valid=r.up(keep))
    for k in KEYS:
        assert np.all(got[k][keep == 0] == FILL), k
        assert np.array_equal(got[k][keep == 1], full[name][k][keep == 1]), k
    rot = r.g["rot"].copy()
    pos = r.g["pos"].copy()
    rot[9, 1, 2], rot[FPB + 3, 1, 0], pos[FPB + 3, 0, 1] = np.nan, np.nan, np.nan      # bone 1, the hips: every bone hangs off it
    bad = r.run(r.up(rot), r.up(pos), 67)
    same = np.ones(67, bool)
    same[[9, FPB + 3]] = False
    for k in KEYS:
        assert np.array_equal(bad[k][same], full[name][k][same]), k
        assert np.isnan(bad[k][9]).any() and np.isnan(bad[k][FPB + 3]).any(), k


@pytest.mark.parametrize("name", NAMES)
def test_any_output_null(rigs, full, name):
    r = rigs[name]
    for want in (("gpos",), ("grot",), ("palette",), ("gpos", "grot"), ("gpos", "palette"), ("grot", "palette")):
        got = r.run(r.rot, r.pos, 67, want=want)
        for k in want:
            assert np.array_equal(got[k], full[name][k]), (want, k)


@pytest.mark.parametrize("name", NAMES)
def test_refusals(rigs, name):
    r = rigs[name]
    cases = {"palette without bind": dict(bind=None), "all outputs NULL": dict(want=()), "NULL rot": dict(rot=None), "NULL pos": dict(pos=None)}
    for what, kw in cases.items():
        bufs = r.buffers(9)
        want, bind = kw.get("want", KEYS), kw.get("bind", "fixture")
        ptr = {k: (_ptr(bufs[k][1]) if k in want else None) for k in KEYS}
        b = r.bind if bind == "fixture" else None
        rc = r.lib.mocha_world_pose(r.h, _ptr(kw.get("rot", r.rot)), _ptr(kw.get("pos", r.pos)), 0, 9, None, _ptr(b), ptr["gpos"], ptr["grot"],
                                    ptr["palette"], _stream())
        torch.cuda.synchronize()
        assert rc == ERR_ARG, (what, rc)
        assert all(bool((bufs[k][0] == FILL).all()) for k in KEYS), what
    bufs = r.buffers(9)
    assert r.launch(r.rot, r.pos, 9, bufs, count=0) == 0                        # n == 0: a no-op
    torch.cuda.synchronize()
    r.read(bufs, want=())
    for bad in (np.nan, np.inf, -np.inf):
        pre = r.pre.copy()
        pre[1, 2] = bad
        r.make_bind(r.g["rest_rot"], r.g["rest_pos"], pre, expect=ERR_ARG)
    nb = int(r.lib.mocha_world_bind_bytes(r.h)) // 8
    buf = torch.full((nb,), FILL, dtype=torch.float64, device=dev())
    assert r.lib.mocha_world_bind(r.h, None, None, None, _ptr(buf), _stream()) == ERR_ARG      # NULL rest_pos
    assert r.lib.mocha_world_bind(r.h, None, _ptr(r.up(r.g["rest_pos"])), None, None, _stream()) == ERR_ARG
    torch.cuda.synchronize()
    assert bool((buf == FILL).all())


@pytest.mark.parametrize("name", NAMES)
def test_unit_length_rest_quaternions(rigs, name):
    """The common case for callers: a rest pose stored at unit length.  quat.normalize leaves it 1e-8 short (see the module docstring), and
    the palette is still the definition's: every frame but the rest-pose one against the float64 restatement, within one fp32 spacing."""
    r = rigs[name]
    rest = r.g["rest_rot"] / np.sqrt(np.sum(r.g["rest_rot"] ** 2, axis=-1))[:, None]
    assert np.abs(np.sqrt(np.sum(rest ** 2, axis=-1)) - 1.0).max() < 1e-15
    bind = r.make_bind(rest, r.g["rest_pos"], r.pre)
    got = r.run(r.rot, r.pos, 67, bind=bind)
    ref = WR.palette(got["grot"], got["gpos"], rest, r.g["rest_pos"], r.pre, r.par)
    keep = np.arange(67) != 1
    err = np.abs(got["palette"].astype(np.float64) - ref.astype(np.float64))[keep]
    bound = _group_bound(ref)[keep]
    print(f"{name}: unit-length rest quaternions, largest palette error / bound {float((err / bound).max()):.3f}")
    assert np.all(err <= bound), float((err / bound).max())
