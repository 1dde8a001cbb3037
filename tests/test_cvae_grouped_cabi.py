"""The C entry points of the per-character CVAE weight bank: mocha_cvae_bank_create / _store / _clear / _info,
mocha_cvae_sample_grouped, mocha_linear_grouped, mocha_live_step_ours_grouped.

No GPU: the header, the ctypes binding and the built library agree on the seven names, the ABI version is still 6, the Python surface
exists (CVAEBank exported, LiveOursSession.set_cvae), a NULL context is refused before anything touches a device."""
import ctypes as C
import os
import re

import mocha_sigasia2023_amd as M
from mocha_sigasia2023_amd import _C

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["mocha_cvae_bank_create", "mocha_cvae_bank_store", "mocha_cvae_bank_clear", "mocha_cvae_bank_info", "mocha_cvae_sample_grouped",
       "mocha_linear_grouped", "mocha_live_step_ours_grouped"]
ERR_ARG = -1


def _built():
    if not os.path.exists(_C.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _C.load_library()


def _declared():
    txt = open(os.path.join(REPO, "include", "mocha_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return code, set(re.findall(r"\b(mocha_[a-z_0-9]+)\s*\(", code))


def test_new_names_in_header_binding_and_library():
    code, declared = _declared()
    lib = _built()
    for n in NEW:
        assert n in declared, f"{n} is not declared in include/mocha_hip.h"
        assert n in _C.SIGNATURES, f"{n} is not bound in _C.SIGNATURES"
        assert hasattr(lib, n), f"libmocha_hip.so does not export {n}"
    # the argument counts of the bindings are those of the header's prototypes
    for n in NEW:
        proto = re.search(r"\b" + n + r"\s*\((.*?)\)\s*;", code, flags=re.S).group(1)
        assert len(proto.split(",")) == len(_C.SIGNATURES[n][1]), (n, proto)
    assert len(_C.SIGNATURES["mocha_live_step_ours_grouped"][1]) == len(_C.SIGNATURES["mocha_live_step_ours"][1]) + 1
    assert len(_C.SIGNATURES["mocha_cvae_sample_grouped"][1]) == len(_C.SIGNATURES["mocha_cvae_sample"][1]) + 1


def test_abi_version_unchanged():
    lib = _built()
    assert _C.ABI_VERSION == 6 and lib.mocha_abi_version() == 6          # additive: existing callers keep working


def test_python_surface():
    assert "CVAEBank" in M.__all__ and M.CVAEBank.__module__ == "mocha_sigasia2023_amd.generator"
    for name in ("store", "clear", "sample"):
        assert callable(getattr(M.CVAEBank, name))
    assert isinstance(M.CVAEBank.stored, property)
    assert callable(M.LiveOursSession.set_cvae)
    import inspect
    p = inspect.signature(M.LiveOursSession.__init__).parameters
    assert p["cvaes"].default is None and p["cvae_of"].default is None


def test_null_context_is_refused_without_a_device():
    lib = _built()
    buf = (C.c_double * 8)()                       # host memory standing in for device pointers: must never be dereferenced
    p = C.cast(buf, C.c_void_p)
    assert lib.mocha_cvae_bank_create(None, 3) == ERR_ARG
    assert lib.mocha_cvae_bank_store(None, 0, p, p, p, p, None) == ERR_ARG
    assert lib.mocha_cvae_bank_clear(None, 0, None) == ERR_ARG
    assert lib.mocha_cvae_bank_info(None, None, None) == ERR_ARG
    assert lib.mocha_cvae_sample_grouped(None, p, 1, p, p, p, p, p, None) == ERR_ARG
    assert lib.mocha_linear_grouped(None, p, p, p, p, p, p, 16, 1, 1, 16, 16, 1, 0, None, 0, None) == ERR_ARG
    assert lib.mocha_live_step_ours_grouped(None, None, p, 1, *([p] * 23)) == ERR_ARG
