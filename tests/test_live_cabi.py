"""CPU-side checks of the live-session entry points (no GPU): the header, the ctypes binding and the built library agree on the five
new C names, the ABI version did not move, the Python surface exists, and a NULL context is refused before anything touches a device."""
import ctypes as C
import os
import re

import mocha_sigasia2023_amd as M
from mocha_sigasia2023_amd import _C

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["mocha_post_state_bytes", "mocha_postprocess_step", "mocha_live_state_bytes", "mocha_live_reset", "mocha_live_step"]
MOCHA_ERR_ARG = -1


def _built():
    if not os.path.exists(_C.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _C.load_library()


def test_new_names_in_header_binding_and_library():
    txt = open(os.path.join(REPO, "include", "mocha_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    declared = set(re.findall(r"\b(mocha_[a-z_]+)\s*\(", txt))
    lib = _built()
    for n in NEW:
        assert n in declared, f"{n} is not declared in include/mocha_hip.h"
        assert n in _C.SIGNATURES, f"{n} is not bound in _C.SIGNATURES"
        assert hasattr(lib, n), f"libmocha_hip.so does not export {n}"


def test_abi_version_unchanged():
    lib = _built()
    assert _C.ABI_VERSION == 6 and lib.mocha_abi_version() == 6          # additive: existing callers keep working


def test_python_surface():
    assert "LiveSession" in M.__all__ and "retarget_frame_ours" in M.__all__
    assert callable(M.LiveSession) and M.LiveSession.__module__ == "mocha_sigasia2023_amd.live"
    for name in ("push", "reset", "run_clip"):
        assert callable(getattr(M.LiveSession, name))
    assert callable(M.PostProcessor.step) and callable(M.PostProcessor.state)
    assert callable(M.retarget_frame_ours)


def test_null_context_is_refused_without_a_device():
    lib = _built()
    buf = (C.c_double * 8)()                       # host memory standing in for device pointers: must never be dereferenced
    p = C.cast(buf, C.c_void_p)
    assert lib.mocha_postprocess_step(None, None, p, p, p, p, p, p, p, 1, p, p, p, None, None, None) == MOCHA_ERR_ARG
    assert lib.mocha_live_step(None, None, p, 1, *([p] * 19)) == MOCHA_ERR_ARG
    assert lib.mocha_live_reset(None, p, 1, None, 0, None) == MOCHA_ERR_ARG
    assert lib.mocha_post_state_bytes(None) < 0 and lib.mocha_live_state_bytes(None, 1) < 0


def test_product_package_does_not_import_the_oracle():
    pkg = os.path.join(REPO, "mocha_sigasia2023_amd")
    for root, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".cpp", ".hip", ".h")):
                src = open(os.path.join(root, f)).read()
                assert not re.search(r"^\s*(from|import)\s+oracle\b", src, flags=re.M), f
