"""The C entry points of the clip ingester: mocha_ingest_clips, mocha_clip_window_count, mocha_clip_windows and mocha_mirror_map_default are
declared in the header, bound in _C.SIGNATURES and exported by the built library; the ABI version is still 6 and mocha_ingest_cfg keeps its
fields; the default mirror maps are involutions that commute with the parents; the host-only helpers work and a NULL context is refused
before anything touches a device.  No GPU."""
import ctypes as C
import inspect
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import clip_ingest_ref as CR  # noqa: E402
import mocha_sigasia2023_amd as M  # noqa: E402
from mocha_sigasia2023_amd import _C  # noqa: E402
from mocha_sigasia2023_amd.ingest import clip_window_counts, default_mirror_map  # noqa: E402
from mocha_sigasia2023_amd.skeleton import LAYOUTS  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["mocha_ingest_clips", "mocha_clip_window_count", "mocha_clip_windows", "mocha_mirror_map_default"]
ERR_ARG = -1
FIELDS = ["lookahead", "rot_format", "euler_order", "unit_scale", "fps", "contact_velocity_threshold", "spine", "shoulder_l", "shoulder_r",
          "upleg_l", "upleg_r"]


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
    # argument counts of the binding against the header's declarations
    for n in NEW:
        args = re.search(r"\b" + n + r"\s*\((.*?)\)\s*;", code, flags=re.S).group(1)
        assert len(args.split(",")) == len(_C.SIGNATURES[n][1]), n
    assert [f[0] for f in _C.mocha_ingest_cfg._fields_] == FIELDS             # additive: the struct is as it was


def test_abi_version_unchanged():
    lib = _built()
    assert _C.ABI_VERSION == 6 and lib.mocha_abi_version() == 6


def test_default_mirror_maps():
    lib = _built()
    for layout, lid in (("mocha", 0), ("mixamo", 1)):
        par = LAYOUTS[layout]["parents"]
        m = default_mirror_map(layout)
        assert len(m) == len(par) and sorted(m) == list(range(len(par)))
        assert all(m[m[v]] == v for v in range(len(par))), "no involution"
        assert m[0] == 0 and all(par[m[v]] == m[par[v]] for v in range(1, len(par))), "does not commute with the parents"
        assert sum(m[v] != v for v in range(len(par))) == 16                 # two legs and two arms of four joints change sides
    assert default_mirror_map("mocha")[1:5] == [20, 21, 22, 23] and default_mirror_map("mocha")[9:13] == [16, 17, 18, 19]
    assert default_mirror_map("mixamo")[6:10] == [10, 11, 12, 13] and default_mirror_map("mixamo")[14:18] == [18, 19, 20, 21]
    buf = (C.c_int32 * 32)()
    assert lib.mocha_mirror_map_default(2, buf) == ERR_ARG and lib.mocha_mirror_map_default(-1, buf) == ERR_ARG
    assert lib.mocha_mirror_map_default(0, None) == ERR_ARG


def test_window_count_is_divide_clips():
    lib = _built()
    for window, step in ((60, 1), (60, 30), (60, 7), (4, 1), (61, 3)):
        lengths = [1, 14, 15, 16, 31, 59, 60, 61, 100, 3600]
        assert clip_window_counts(lengths, window, step) == [CR.window_count(n, window, step) for n in lengths], (window, step)
    off, counts = (C.c_int32 * 3)(0, 31, 131), (C.c_int64 * 2)()
    assert lib.mocha_clip_window_count(off, 2, 60, 1, counts) == 0 and list(counts) == [16, 85]
    assert lib.mocha_clip_window_count(off, 2, 3, 1, counts) == ERR_ARG and lib.mocha_clip_window_count(off, 2, 60, 0, counts) == ERR_ARG
    assert lib.mocha_clip_window_count(None, 2, 60, 1, counts) == ERR_ARG and lib.mocha_clip_window_count(off, 2, 60, 1, None) == ERR_ARG
    assert lib.mocha_clip_window_count((C.c_int32 * 3)(0, 31, 31), 2, 60, 1, counts) == ERR_ARG


def test_null_context_is_refused_without_a_device():
    lib = _built()
    buf = (C.c_double * 8)()                       # host memory standing in for device pointers: must never be dereferenced
    p = C.cast(buf, C.c_void_p)
    cfg = _C.mocha_ingest_cfg()
    lib.mocha_ingest_cfg_default(C.byref(cfg), 0)
    off = (C.c_int32 * 2)(0, 100)
    assert lib.mocha_ingest_clips(None, C.byref(cfg), None, p, p, off, 1, None, None, p, p, p, p, p, None) == ERR_ARG
    assert lib.mocha_clip_windows(None, p, p, p, p, p, 2, off, 1, 60, 1, p, p, p, p, p, None) == ERR_ARG


def test_python_surface():
    assert "ingest_clips" in M.__all__ and "clip_windows" in M.__all__
    assert list(inspect.signature(M.ingest_clips).parameters) == ["model", "rot", "pos", "lengths", "raw", "mirror", "post"]
    assert list(inspect.signature(M.clip_windows).parameters) == ["processed", "lengths", "window", "step", "model"]
    assert inspect.signature(M.clip_windows).parameters["window"].default == 60
    assert M.IngestConfig().mirror_map is None and M.IngestConfig(mirror_map=range(24)).mirror_map == list(range(24))
    from mocha_sigasia2023_amd import bank
    assert list(inspect.signature(bank.build_database_from_clips).parameters)[:6] == ["model", "clips", "style_labels", "action_labels", "mirror",
                                                                                     "raw"]
