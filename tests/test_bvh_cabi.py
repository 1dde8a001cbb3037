"""The C entry points of BVH reading: mocha_bvh_header and mocha_bvh_motion.

Without a GPU: the header, the ctypes binding and the built library agree on the two names and on the size of the header struct, the ABI
version is still 6, mocha_bvh_header runs with no context and no device, mocha_bvh_motion refuses a NULL context before anything touches a
device.  The sentences that said the library cannot read BVH text are gone."""
import ctypes as C
import os
import re

from mocha_sigasia2023_amd import _C

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["mocha_bvh_header", "mocha_bvh_motion"]
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
    for name, value in (("MOCHA_BVH_MAX_JOINTS", _C.BVH_MAX_JOINTS), ("MOCHA_BVH_ALIGN", _C.BVH_ALIGN), ("MOCHA_BVH_MAX_SLOW", _C.BVH_MAX_SLOW)):
        m = re.search(r"#define\s+%s\s+(\d+)" % name, code)
        assert m and int(m.group(1)) == value, name
    assert "motion/bvh.py:22-138" in txt and "NOT capture-safe" in txt
    for doc in ("include/mocha_hip.h", "DESIGN.md", "INTEGRATION.md", "mocha_sigasia2023_amd/ingest.py"):
        text = open(os.path.join(REPO, doc)).read()
        assert "no BVH text parsing" not in text and "Not provided: BVH text parsing" not in text, doc


def test_abi_version_unchanged():
    lib = _built()
    assert _C.ABI_VERSION == 6 and lib.mocha_abi_version() == 6          # additive: existing callers keep working


def test_header_runs_without_a_device():
    lib = _built()
    text = (b"HIERARCHY\nROOT Hips\n{\n OFFSET 1 2 3\n CHANNELS 6 Xposition Yposition Zposition Zrotation Xrotation Yrotation\n"
            b" End Site\n {\n  OFFSET 0 0 0\n }\n}\nMOTION\nFrames: 1\nFrame Time: 0.01\n1 2 3 4 5 6\n")
    hdr = _C.mocha_bvh_hdr()
    assert lib.mocha_bvh_header(text, len(text), C.byref(hdr)) == 0
    assert hdr.n_joints == 1 and hdr.channels == 6 and list(hdr.order) == [2, 0, 1] and hdr.frames == 1 and hdr.frame_time == 0.01
    assert hdr.parents[0] == -1 and [hdr.offsets[0][a] for a in range(3)] == [1.0, 2.0, 3.0] and hdr.error_offset == -1
    assert text[hdr.name_offset[0]: hdr.name_offset[0] + hdr.name_length[0]] == b"Hips"
    assert text[hdr.motion_begin: hdr.motion_end] == b"1 2 3 4 5 6\n"
    assert lib.mocha_bvh_header(text, 40, C.byref(hdr)) == ERR_ARG and hdr.error_offset >= 0 and hdr.error
    assert lib.mocha_bvh_header(None, 0, C.byref(hdr)) == ERR_ARG and lib.mocha_bvh_header(text, len(text), None) == ERR_ARG


def test_motion_refuses_a_null_context_without_a_device():
    lib = _built()
    buf = (C.c_double * 8)()                       # host memory standing in for device pointers: must never be dereferenced
    p = C.cast(buf, C.c_void_p)
    one = (C.c_int64 * 1)(0)
    off = (C.c_int32 * 2)(0, 1)
    rep = _C.mocha_bvh_report()
    assert lib.mocha_bvh_motion(None, p, 4096, None, one, one, off, 1, 1, 6, None, 1, None, p, p, C.byref(rep), None) == ERR_ARG
