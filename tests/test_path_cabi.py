"""The C entry points of coherent context matching: mocha_match_dist_matrix, mocha_match_path, mocha_characterize_path and
mocha_characterize_pair_path are declared in the header, bound in _C.SIGNATURES and exported by the built library with matching argument
counts; the ABI version is still 6; a NULL context is refused before anything touches a device; the Python surface is as documented."""
import ctypes as C
import inspect
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mocha_sigasia2023_amd as M  # noqa: E402
from mocha_sigasia2023_amd import _C  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["mocha_match_dist_matrix", "mocha_match_path", "mocha_characterize_path", "mocha_characterize_pair_path"]
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
    assert C.c_double in _C.SIGNATURES["mocha_match_path"][1]          # the penalty is a double
    for cite in ("test_fullframework.py:440-443", "collect_CVAE_feature_action.py:119-125", "NOT capture-safe", "What it is not"):
        assert cite in txt, f"the header does not say {cite}"
    assert "#define MOCHA_PATH_MAX_ROWS 16384" in txt


def test_abi_version_unchanged():
    lib = _built()
    assert _C.ABI_VERSION == 6 and lib.mocha_abi_version() == 6


def test_null_context_is_refused_without_a_device():
    lib = _built()
    buf = (C.c_float * 16)(*([7.5] * 16))          # host memory standing in for device pointers: must never be dereferenced
    p = C.cast(buf, C.c_void_p)
    seq = (C.c_int32 * 2)(0, 2)
    assert lib.mocha_match_dist_matrix(None, p, 2, 0, 2, p, 2, None) == ERR_ARG
    assert lib.mocha_match_path(None, p, 2, 2, 2, seq, 1, None, 0, 1.0, p, p, p, None) == ERR_ARG
    assert lib.mocha_characterize_path(None, p, 2, p, p, seq, 1, None, 0, 1.0, 0, p, p, p, 0, None) == ERR_ARG
    assert lib.mocha_characterize_pair_path(None, p, 2, p, 2, p, p, seq, 1, None, 0, 1.0, 1, p, p, p, None, None, 0, None) == ERR_ARG
    assert list(buf) == [7.5] * 16 and list(seq) == [0, 2]


def test_python_surface():
    for name in ("CoherentMatch", "bank_starts"):
        assert name in M.__all__ and hasattr(M, name), name
    sig = inspect.signature(M.ContextBank.query_path)
    assert list(sig.parameters) == ["self", "query_nm", "jump", "starts", "bank_starts", "relative"]
    assert sig.parameters["starts"].default is None and sig.parameters["bank_starts"].default is None
    assert sig.parameters["relative"].default is False
    assert list(inspect.signature(M.ContextBank.distances).parameters)[:2] == ["self", "query_nm"]
    for cls in (M.MultiCharacterBank, M.ResidentCharacterBank):
        assert list(inspect.signature(cls.query_path).parameters)[:4] == ["self", "query_nm", "character", "jump"]
    for fn in (M.ContextBank.characterize, M.Generator.characterize_pair, M.retarget_clip):
        assert inspect.signature(fn).parameters["coherent"].default is None, fn
    sig = inspect.signature(M.CoherentMatch.__init__)
    assert list(sig.parameters) == ["self", "jump", "relative", "bank_starts", "src_starts"]
    assert sig.parameters["relative"].default is False
    co = M.CoherentMatch.of(0.5)
    assert (co.jump, co.relative, co.bank_starts, co.src_starts) == (0.5, False, None, None)
    assert M.CoherentMatch.of(co) is co
    for bad in (-1.0, float("nan"), float("inf")):
        try:
            M.CoherentMatch(bad)
        except ValueError:
            continue
        raise AssertionError(f"CoherentMatch({bad}) was accepted")
    assert M.bank_starts({"range_starts": [0, 40, 17]}) == [0, 17, 40] and M.bank_starts({}) == [0]
    assert "not" in M.ContextBank.query_path.__doc__.lower()
