"""The C entry points of coherent matching in live sessions are declared in the header, bound in _C.SIGNATURES and exported by the built
library with matching argument counts; the ABI version is still 6; a NULL context is refused before anything touches a device; the state
size is the documented one; the Python surface is as documented."""
import ctypes as C
import inspect
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mocha_sigasia2023_amd as M  # noqa: E402
from mocha_sigasia2023_amd import _C  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["mocha_bank_set_starts", "mocha_bank_resident_set_starts", "mocha_path_state_bytes", "mocha_path_state_reset", "mocha_match_path_advance",
       "mocha_match_path_segmented", "mocha_characterize_segmented_path", "mocha_live_step_path", "mocha_live_step_raw_path"]
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
    for n in ("mocha_match_path_advance", "mocha_match_path_segmented", "mocha_characterize_segmented_path", "mocha_live_step_path",
              "mocha_live_step_raw_path"):
        assert C.c_double in _C.SIGNATURES[n][1], n                        # the penalty is a double, by value
    # the live steps with the path: the plain live step's arguments, then the six of the path
    assert _C.SIGNATURES["mocha_live_step_path"][1][:23] == _C.SIGNATURES["mocha_live_step"][1]
    for cite in ("coherent matching in live sessions", "Capture-safe", "no fixed-lag smoothing", "fp32 rows are read also on bf16 banks"):
        assert cite in txt, f"the header does not say {cite}"
    assert "#define MOCHA_PATH_MAX_ROWS 16384" in txt


def test_abi_version_unchanged():
    lib = _built()
    assert _C.ABI_VERSION == 6 and lib.mocha_abi_version() == 6


def test_null_context_is_refused_without_a_device():
    lib = _built()
    buf = (C.c_float * 16)(*([7.5] * 16))          # host memory standing in for device pointers: must never be dereferenced
    p = C.cast(buf, C.c_void_p)
    one = (C.c_int32 * 1)(0)
    one64 = (C.c_int64 * 1)(0)
    assert lib.mocha_bank_set_starts(None, one64, 1, None) == ERR_ARG
    assert lib.mocha_bank_resident_set_starts(None, 0, one, 1, None) == ERR_ARG
    assert lib.mocha_path_state_bytes(None, 1, 16) < 0
    assert lib.mocha_path_state_reset(None, p, 1, 16, None, 0, None) == ERR_ARG
    assert lib.mocha_match_path_advance(None, p, 1, 16, p, 16, p, p, None, 0, None, None, 1.0, p, p, p, None) == ERR_ARG
    assert lib.mocha_match_path_segmented(None, p, 1, 16, p, p, None, 1.0, p, p, p, None, 0, None) == ERR_ARG
    assert lib.mocha_characterize_segmented_path(None, p, 1, p, p, p, p, 16, 1.0, None, p, p, p, p, 0, None) == ERR_ARG
    assert lib.mocha_live_step_path(None, None, p, 1, *([p] * 19), p, 16, 1.0, None, p, p) == ERR_ARG
    assert lib.mocha_live_step_raw_path(None, None, None, p, p, 1, *([p] * 13), p, 16, 1.0, None, p, p) == ERR_ARG
    assert list(buf) == [7.5] * 16


def test_python_surface():
    for name in ("OnlinePath", "CoherentMatch", "bank_starts"):
        assert name in M.__all__ and hasattr(M, name), name
    sig = inspect.signature(M.OnlinePath.__init__)
    assert list(sig.parameters)[:4] == ["self", "bank", "streams", "jump"]
    for meth in ("step", "advance", "reset"):
        assert callable(getattr(M.OnlinePath, meth))
    assert "starts" in inspect.signature(M.MultiCharacterBank.__init__).parameters
    assert list(inspect.signature(M.MultiCharacterBank.set_starts).parameters) == ["self", "character", "starts"]
    for fn in (M.ResidentCharacterBank.add, M.ResidentCharacterBank.replace):
        assert inspect.signature(fn).parameters["starts"].default is None, fn
    for cls in (M.MultiCharacterBank, M.ResidentCharacterBank):
        assert inspect.signature(cls.characterize).parameters["coherent"].default is None, cls
    assert inspect.signature(M.LiveSession.__init__).parameters["coherent"].default is None
    assert "query_path" in M.LiveSession.__doc__
