"""The C entry points of soft context matching on a multi-character bank: mocha_match_topk_segmented,
mocha_characterize_soft_segmented, mocha_step_graph_soft_segmented, mocha_live_step_soft.

No GPU: the header, the ctypes binding and the built library agree on the four names, the ABI version is still 6, a NULL context is
refused before anything touches a device, and the Python surface takes ``soft`` / ``k``."""
import ctypes as C
import inspect
import os
import re

import pytest

import mocha_sigasia2023_amd as M
from mocha_sigasia2023_amd import _C

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["mocha_match_topk_segmented", "mocha_characterize_soft_segmented", "mocha_step_graph_soft_segmented", "mocha_live_step_soft"]
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
    assert re.search(r"#define\s+MOCHA_SOFT_MAX_K\s+8\b", code)
    # the bindings carry the header's argument counts: the hard call's arguments plus (k, temperature) and the (.., k) outputs
    sig = _C.SIGNATURES
    assert len(sig["mocha_match_topk_segmented"][1]) == len(sig["mocha_match_segmented"][1]) + 1
    assert len(sig["mocha_characterize_soft_segmented"][1]) == len(sig["mocha_characterize_segmented"][1]) + 3
    assert len(sig["mocha_step_graph_soft_segmented"][1]) == len(sig["mocha_step_graph_segmented"][1]) + 3
    assert len(sig["mocha_live_step_soft"][1]) == len(sig["mocha_live_step"][1]) + 4
    for n in NEW[1:]:
        assert sig[n][1].count(C.c_float) == 1, n                      # the temperature travels as a float


def test_abi_version_unchanged():
    lib = _built()
    assert _C.ABI_VERSION == 6 and lib.mocha_abi_version() == 6          # additive: existing callers keep working


def test_null_context_is_refused_without_a_device():
    lib = _built()
    buf = (C.c_double * 8)()                       # host memory standing in for device pointers: must never be dereferenced
    p = C.cast(buf, C.c_void_p)
    assert lib.mocha_match_topk_segmented(None, p, 1, p, 4, p, p, None) == ERR_ARG
    assert lib.mocha_characterize_soft_segmented(None, p, 1, p, 4, 2.0, p, p, p, p, p, 0, None) == ERR_ARG
    assert lib.mocha_step_graph_soft_segmented(None, p, 1, p, 4, 2.0, p, p, p, p, p, 0, None) == ERR_ARG
    assert lib.mocha_live_step_soft(None, None, p, 1, *([p] * 11), 4, 2.0, *([p] * 9), None) == ERR_ARG


def test_python_surface():
    assert "soft" in inspect.signature(M.LiveSession.__init__).parameters
    assert inspect.signature(M.LiveSession.__init__).parameters["soft"].default is None
    assert inspect.signature(M.MultiStreamCharacterizer.__init__).parameters["soft"].default is None
    assert inspect.signature(M.MultiCharacterBank.characterize).parameters["soft"].default is None
    assert inspect.signature(M.MultiCharacterBank.query).parameters["k"].default == 1
    from mocha_sigasia2023_amd.multi_character import soft_params
    assert soft_params(None, "x") is None and soft_params((4, 2), "x") == (4, 2.0)
    for bad in ((0, 1.0), (9, 1.0), (2, 0.0), (2, -1.0), (2.5, 1.0), 3):
        with pytest.raises(ValueError):
            soft_params(bad, "x")
    # the CVAE branch's decoder already reads a sampled feature: it refuses soft before it looks at anything else
    with pytest.raises(ValueError, match="soft"):
        M.LiveOursSession(None, None, None, None, None, None, None, None, soft=(2, 1.0))
