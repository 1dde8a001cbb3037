"""The C entry points of BVH writing: mocha_bvh_text_bound and mocha_bvh_format, and the host route of write_bvh with its new keyword.

Without a GPU: the header, the ctypes binding and the built library agree on the two names, the ABI version is still 6,
mocha_bvh_text_bound returns frames * (C * 21 + 1), and every argument error the header lists under "nothing launched" comes back as
MOCHA_ERR_ARG with no context and no device - the arguments are judged before the context is looked at, and mocha_last_error(NULL) names
the reason, so that each refusal is seen to be the one meant (a call with good arguments and no context is refused for the context).
write_bvh without ``model`` reproduces the reference writer's own files: mocha24_rot.bvh, and mocha24_pos.bvh with save_positions=True."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bvh_fmt_ref as R  # noqa: E402
from mocha_sigasia2023_amd import _C, write_bvh  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden")
NEW = ["mocha_bvh_text_bound", "mocha_bvh_format"]
ERR_ARG = -1


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
    m = re.search(r"#define\s+MOCHA_BVHW_MAX_TOKEN\s+(\d+)", code)
    assert m and int(m.group(1)) == _C.BVHW_MAX_TOKEN == 21
    assert re.search(r"typedef struct mocha_bvhw_report \{ int64_t tokens, bytes, first_bad; \}", code)
    assert [f[0] for f in _C.mocha_bvhw_report._fields_] == ["tokens", "bytes", "first_bad"] and C.sizeof(_C.mocha_bvhw_report) == 24
    assert len(_C.SIGNATURES["mocha_bvh_format"][1]) == 14 and "NOT capture-safe" in txt


def test_abi_version_unchanged():
    lib = _built()
    assert _C.ABI_VERSION == 6 and lib.mocha_abi_version() == 6          # additive: existing callers keep working


def test_text_bound():
    lib = _built()
    assert lib.mocha_bvh_text_bound(40, 24, 0) == 40 * (75 * 21 + 1)
    assert lib.mocha_bvh_text_bound(40, 24, 1) == 40 * (144 * 21 + 1)
    assert lib.mocha_bvh_text_bound(1, 1, 0) == 6 * 21 + 1 and lib.mocha_bvh_text_bound(0, 256, 1) == 0
    assert lib.mocha_bvh_text_bound(64 * 3600, 24, 0) == 230400 * 1576      # the benchmark's call: 363 MB, below 2^31
    assert lib.mocha_bvh_text_bound(-1, 24, 0) == -1 and lib.mocha_bvh_text_bound(1, 0, 0) == -1


def _call(lib, **kw):
    """mocha_bvh_format with NO context on good arguments (host memory stands in for the device pointers: it must never be
    dereferenced), one of them replaced.  Returns (status, mocha_last_error(NULL))."""
    V = kw.pop("V", 3)
    buf = (C.c_double * 64)()
    p = C.cast(buf, C.c_void_p)
    a = dict(pos=p, euler=p, offsets=(C.c_int32 * 3)(0, 2, 5), n_clips=2, n_joints=V, visit=(C.c_int32 * max(V, 1))(*range(max(V, 1))),
             axes=(C.c_int32 * 3)(2, 1, 0), save_positions=0, text=p, capacity=1 << 20, begin=(C.c_int64 * 3)(),
             report=C.byref(_C.mocha_bvhw_report()))
    a.update(kw)
    rc = lib.mocha_bvh_format(None, a["pos"], a["euler"], a["offsets"], a["n_clips"], a["n_joints"], a["visit"], a["axes"], a["save_positions"],
                              a["text"], a["capacity"], a["begin"], a["report"], None)
    return rc, lib.mocha_last_error(None).decode()


CASES = {
    "pos NULL": (dict(pos=None), "null argument"),
    "euler NULL": (dict(euler=None), "null argument"),
    "visit NULL": (dict(visit=None), "null argument"),
    "axes NULL": (dict(axes=None), "null argument"),
    "text NULL": (dict(text=None), "null argument"),
    "clip_text_begin NULL": (dict(begin=None), "null argument"),
    "clip_offsets NULL": (dict(offsets=None), "null argument"),
    "no joints": (dict(V=0), "n_joints must be"),
    "too many joints": (dict(n_joints=257, visit=(C.c_int32 * 257)(*range(257))), "n_joints must be"),
    "visit repeats": (dict(visit=(C.c_int32 * 3)(0, 1, 1)), "permutation of the joints"),
    "visit out of range": (dict(visit=(C.c_int32 * 3)(0, 1, 3)), "permutation of the joints"),
    "visit negative": (dict(visit=(C.c_int32 * 3)(0, -1, 2)), "permutation of the joints"),
    "axes repeat": (dict(axes=(C.c_int32 * 3)(0, 0, 1)), "permutation of 0, 1, 2"),
    "axes out of range": (dict(axes=(C.c_int32 * 3)(0, 1, 3)), "permutation of 0, 1, 2"),
    "offsets not from 0": (dict(offsets=(C.c_int32 * 3)(1, 2, 5)), "clip_offsets[0] must be 0"),
    "offsets do not increase": (dict(offsets=(C.c_int32 * 3)(0, 2, 2)), "clip_offsets must increase"),
    "no clips": (dict(n_clips=0), "n_clips must be at least 1"),
    "negative capacity": (dict(capacity=-1), "negative capacity"),
    # 3 + 3 * 3 = 12 columns: 12 * 21 + 1 = 253 bytes per frame at most; 8488078 frames reach 2^31, one fewer does not
    "bound reaches 2^31": (dict(offsets=(C.c_int32 * 3)(0, 2, 8488078)), "2^31 bytes or more"),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_argument_errors_without_a_device(name):
    lib = _built()
    change, reason = CASES[name]
    rc, msg = _call(lib, **dict(change))
    assert rc == ERR_ARG and reason in msg, (rc, msg)


def test_good_arguments_are_refused_only_for_the_context():
    lib = _built()
    assert 8488078 * 253 >= 2 ** 31 > 8488077 * 253
    for change in (dict(), dict(offsets=(C.c_int32 * 3)(0, 2, 8488077)), dict(save_positions=1), dict(report=None), dict(capacity=0),
                   dict(n_joints=256, visit=(C.c_int32 * 256)(*reversed(range(256))), offsets=(C.c_int32 * 3)(0, 1, 2))):
        rc, msg = _call(lib, **change)
        assert rc == ERR_ARG and "null context" in msg, (rc, msg)


@pytest.mark.parametrize("tag,save_positions", (("mocha24_rot", False), ("mocha24_pos", True)))
def test_host_route_writes_the_golden_files(tmp_path, tag, save_positions):
    gold = dict(np.load(os.path.join(GOLDEN, "bvh_parse.npz")))
    names, parents, pos, rot, offsets, order, frametime = R.golden_arrays(gold, tag)
    path = str(tmp_path / "out.bvh")
    visit = write_bvh(path, names, parents, pos, rot, offsets=offsets, order=order, frametime=frametime, save_positions=save_positions)
    assert visit == list(range(24))
    with open(path, "rb") as f:
        got = f.read()
    want = R.golden_file(os.path.join(GOLDEN, "bvh", tag + ".bvh"), tag)
    assert got == want, next((i, got[max(i - 40, 0): i + 40], want[max(i - 40, 0): i + 40]) for i in range(min(len(got), len(want)) + 1)
                             if got[i: i + 1] != want[i: i + 1])
