"""tests/world_ref.py against the reference's own quat.fk / to_xform / normalize (tests/golden/world_pose.npz, written by
tests/golden/make_golden_world.py): no GPU.  The float64 restatement of forward kinematics equals quat.fk bit for bit; the palette equals
the fixture's after the one rounding to fp32; E_ref - the largest error of the reference's own float64 grot / gpos against the
numpy.longdouble restatement, per frame relative to the frame's largest magnitude of that output - reproduces the value the fixture
stores (it sizes the bound of tests/test_world_pose_kernel.py); the fixture holds the cases it promises."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import world_ref as WR  # noqa: E402
from mocha_sigasia2023_amd.skeleton import LAYOUTS  # noqa: E402

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "world_pose.npz")
NAMES = ["mocha", "mixamo"]


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(GOLD))


def _of(gold, name):
    g = {k[: -len(name) - 1]: v for k, v in gold.items() if k.endswith("_" + name)}
    g["par"] = WR.bone_parents(g["parents"])
    return g


@pytest.mark.parametrize("name", NAMES)
def test_fixture_describes_itself(gold, name):
    g = _of(gold, name)
    V = {"mocha": 24, "mixamo": 22}[name]
    assert g["parents"].tolist() == list(LAYOUTS[name]["parents"]) and len(g["parents"]) == V
    assert g["rot"].shape == (67, V + 1, 4) and g["pos"].shape == (67, V + 1, 3) and g["rot"].dtype == g["pos"].dtype == np.float64
    assert g["palette"].shape == (67, V, 12) and g["palette"].dtype == np.float32
    assert os.path.getsize(GOLD) < 1 << 20
    length = np.sqrt(np.sum(g["rot"] ** 2, axis=-1))
    f, b = gold["off_unit"].tolist()
    assert abs(length[f, b] - 1.001) < 1e-12, "the quaternion that pins `no normalisation`"
    length[f, b] = 1.0
    assert np.abs(np.delete(length, 1, axis=0) - 1.0).max() < 1e-15 and np.abs(length[1] - 1.0).max() < 1e-10
    assert np.array_equal(g["rot"][0], np.tile([1.0, 0.0, 0.0, 0.0], (V + 1, 1)))                  # the all-identity frame
    assert np.array_equal(g["rot"][1], WR.normalize(g["rest_rot"])) and np.array_equal(g["pos"][1], g["rest_pos"])      # the rest pose
    assert np.abs(g["pos"][:, 0]).max() == 5000.0                                                 # translation rounding is exercised
    assert np.abs(np.sqrt(np.sum(g["rest_rot"] ** 2, axis=-1)) - 256.0).max() < 1e-10 and np.abs(g["rest_rot"][:, 1:]).min() > 0
    assert np.array_equal(gold["pre"], [[0.01, 0, 0, 0.5], [0, 0, 0.01, -0.25], [0, 0.01, 0, 1.0]])


@pytest.mark.parametrize("name", NAMES)
def test_float64_restatement_is_quat_fk_bit_for_bit(gold, name):
    g = _of(gold, name)
    grot, gpos = WR.fk(g["rot"], g["pos"], g["par"], np.float64)
    assert np.array_equal(grot, g["grot"]) and np.array_equal(gpos, g["gpos"])
    one = [WR.fk(g["rot"][i], g["pos"][i], g["par"]) for i in (0, 5, 66)]                          # a frame does not see its batch
    assert all(np.array_equal(r, g["grot"][i]) and np.array_equal(p, g["gpos"][i]) for (r, p), i in zip(one, (0, 5, 66)))


@pytest.mark.parametrize("name", NAMES)
def test_palette_equal_after_the_one_rounding(gold, name):
    g = _of(gold, name)
    pal = WR.palette(g["grot"], g["gpos"], g["rest_rot"], g["rest_pos"], gold["pre"], g["par"])
    assert pal.dtype == np.float32 and np.array_equal(pal, g["palette"])
    # the rest-pose frame: world o inverse(bind) is the identity, the palette is `pre`
    wide = WR.palette_wide(g["grot"][1], g["gpos"][1], g["rest_rot"], g["rest_pos"], gold["pre"], g["par"], np.longdouble)
    dev = np.abs(wide - gold["pre"])
    dev = max(float(dev[..., :3].max() / np.spacing(np.float32(0.01))), float(dev[..., 3].max() / np.spacing(np.float32(1.0))))
    print(f"{name}: rest-pose frame, |palette - pre| = {dev:.3g} fp32 spacings; {float(g['rest_dev_unit']):.3g} with unit-length rest quaternions")
    assert dev < 0.25 and abs(dev - float(g["rest_dev"])) < 1e-3          # quat.normalize's 1e-8: see make_golden_world.py
    # no bind rotation, no bind offset, no pre: the palette is the world transform itself
    plain = WR.palette(g["grot"], g["gpos"], None, np.zeros_like(g["rest_pos"]), None, g["par"])
    want = np.concatenate([WR.to_xform(g["grot"][:, 1:]), g["gpos"][:, 1:, :, None]], axis=-1).reshape(67, -1, 12).astype(np.float32)
    assert np.array_equal(plain, want)


@pytest.mark.parametrize("name", NAMES)
def test_e_ref_reproduces(gold, name):
    g = _of(gold, name)
    assert np.finfo(np.longdouble).eps < 2e-19, "numpy.longdouble is no wider than float64 on this machine"
    lrot, lpos = WR.fk(g["rot"], g["pos"], g["par"], np.longdouble)
    e_rot, e_pos = WR.frame_error(g["grot"], lrot), WR.frame_error(g["gpos"], lpos)
    print(f"{name}: E_ref rot {e_rot:.3g}, pos {e_pos:.3g}")
    assert e_rot == float(g["E_rot"]) and e_pos == float(g["E_pos"])
    assert 1e-17 < e_rot < 2e-15 and 1e-17 < e_pos < 2e-15                                        # a few float64 roundings per tree level
