"""The C entry points of the world-pose stage: mocha_world_bind_bytes, mocha_world_bind and mocha_world_pose are declared in the header, bound
in _C.SIGNATURES and exported by the built library with matching argument counts; the ABI version is still 6; a NULL context is refused
before anything touches a device; the Python surface is as documented.  A context cannot be created without a device, so that
mocha_world_bind_bytes is positive - and is not a device call - is checked in the part marked gpu."""
import ctypes as C
import inspect
import os
import re
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mocha_sigasia2023_amd as M  # noqa: E402
from mocha_sigasia2023_amd import _C  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["mocha_world_bind_bytes", "mocha_world_bind", "mocha_world_pose"]
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
        args = re.search(r"\b" + n + r"\s*\((.*?)\)\s*;", code, flags=re.S).group(1)
        assert len(args.split(",")) == len(_C.SIGNATURES[n][1]), n
    assert _C.SIGNATURES["mocha_world_bind_bytes"][0] is C.c_int64
    for cite in ("quat.py:166-173", ":112-120", ":128-130", "quat.py:27-40", "test_fullframework.py:672-690"):
        assert cite in txt, f"the header does not cite {cite}"


def test_abi_version_unchanged():
    lib = _built()
    assert _C.ABI_VERSION == 6 and lib.mocha_abi_version() == 6


def test_null_context_is_refused_without_a_device():
    lib = _built()
    buf = (C.c_double * 16)(*([7.5] * 16))         # host memory standing in for device pointers: must never be dereferenced
    p = C.cast(buf, C.c_void_p)
    pre = (C.c_double * 12)(1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0)
    assert lib.mocha_world_bind_bytes(None) == ERR_ARG
    assert lib.mocha_world_bind(None, p, p, pre, p, None) == ERR_ARG
    assert lib.mocha_world_pose(None, p, p, 0, 1, None, p, p, p, None, None) == ERR_ARG
    assert lib.mocha_world_pose(None, p, p, 0, 0, None, None, None, None, None, None) == ERR_ARG
    assert list(buf) == [7.5] * 16


def test_python_surface():
    for name in ("SkinBind", "world_pose"):
        assert name in M.__all__ and hasattr(M, name), name
    assert list(inspect.signature(M.SkinBind.__init__).parameters) == ["self", "model", "rest_pos", "rest_rot", "pre"]
    assert list(inspect.signature(M.SkinBind.from_bvh_header).parameters) == ["model", "offsets", "rest_rot", "pre"]
    sig = inspect.signature(M.world_pose)
    assert list(sig.parameters) == ["model", "rot", "pos", "bind", "valid", "out"]
    assert all(sig.parameters[k].default is None for k in ("bind", "valid", "out"))
    for cls in (M.LiveSession, M.LiveOursSession):
        assert inspect.signature(cls.__init__).parameters["world"].default is None
    assert "not" in M.LiveSession.__doc__ and "BEHIND the captured graph" in M.LiveSession.__doc__


@pytest.mark.gpu
def test_bind_bytes_is_positive_and_host_only():
    import torch
    for layout, V in (("mocha", 24), ("mixamo", 22)):
        model = M.Generator(layout=layout, device=torch.device("cuda:0"))
        ctx = model._ctx
        assert int(ctx.lib.mocha_world_bind_bytes(ctx.h)) == (V + 2) * 12 * 8
