"""The C entry points of the inertializer, without a GPU: mocha_inert_state_bytes, mocha_inertialize_step and mocha_live_step_inert are
declared in the header, bound in _C.SIGNATURES and exported by the built library; mocha_inert_cfg matches; the ABI version is still 6;
the Python surface exists; a NULL context is refused before anything touches a device; the CVAE session refuses the option."""
import ctypes as C
import inspect
import os
import re

import pytest

import mocha_sigasia2023_amd as M
from mocha_sigasia2023_amd import _C

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["mocha_inert_state_bytes", "mocha_inertialize_step", "mocha_live_step_inert"]
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
    body = re.search(r"typedef struct mocha_inert_cfg \{(.*?)\} mocha_inert_cfg;", code, flags=re.S).group(1)
    assert re.findall(r"(\w+)\s*[,;]", body) == [f[0] for f in _C.mocha_inert_cfg._fields_] == ["halflife", "dt"]
    assert C.sizeof(_C.mocha_inert_cfg) == 16
    # the arguments of mocha_live_step_soft, then `inert` and `icfg`
    assert _C.SIGNATURES["mocha_live_step_inert"][1] == _C.SIGNATURES["mocha_live_step_soft"][1] + [C.c_void_p, C.c_void_p]
    assert _C.SIGNATURES["mocha_inert_state_bytes"] == _C.SIGNATURES["mocha_post_state_bytes"]


def test_abi_version_unchanged():
    lib = _built()
    assert _C.ABI_VERSION == 6 and lib.mocha_abi_version() == 6          # additive: existing callers keep working


def test_python_surface():
    assert "Inertializer" in M.__all__ and M.Inertializer.__module__ == "mocha_sigasia2023_amd.postprocess"
    sig = inspect.signature(M.Inertializer.__init__)
    assert sig.parameters["halflife"].default == 0.1 and sig.parameters["dt"].default == 1 / 60
    assert list(inspect.signature(M.Inertializer.step).parameters) == ["self", "state", "heads", "ids", "trigger", "valid", "out"]
    assert callable(M.Inertializer.state)
    assert inspect.signature(M.LiveSession.__init__).parameters["inertial"].default is None


def test_null_context_is_refused_without_a_device():
    lib = _built()
    buf = (C.c_double * 8)()                       # host memory standing in for device pointers: must never be dereferenced
    p = C.cast(buf, C.c_void_p)
    cfg = _C.mocha_inert_cfg(0.1, 1 / 60)
    assert lib.mocha_inert_state_bytes(None) == ERR_ARG
    assert lib.mocha_inertialize_step(None, C.byref(cfg), p, p, p, p, p, p, 1, None) == ERR_ARG
    assert lib.mocha_live_step_inert(None, None, p, 1, *([p] * 11), 0, 0.0, *([p] * 9), None, p, C.byref(cfg)) == ERR_ARG


def test_the_cvae_session_refuses_the_option():
    with pytest.raises(ValueError, match="inertial"):
        M.LiveOursSession(None, None, None, None, None, None, None, None, inertial=0.1)
