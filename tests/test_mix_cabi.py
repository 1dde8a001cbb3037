"""Character mixing at the drop-in boundary, without a GPU: the five new entry points exist in the library, the header declares them with
the argument lists the ctypes prototypes have, the ABI version is still 6, and a NULL context comes back as MOCHA_ERR_ARG."""
import ctypes as C
import os
import re

import pytest

from mocha_sigasia2023_amd import _C
from mocha_sigasia2023_amd import multi_character as MC
from mocha_sigasia2023_amd import skeleton

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MIX_SYMBOLS = ("mocha_match_mix_segmented", "mocha_characterize_mix_segmented", "mocha_step_graph_mix_segmented", "mocha_live_step_mix",
               "mocha_live_step_raw_mix")
ERR_ARG = -1


def _built():
    if not os.path.exists(_C.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _C.load_library()


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "mocha_hip.h")).read(), flags=re.S)


def _ctype_of(decl: str):
    """One C parameter declaration -> the ctypes type the binding must use for it."""
    decl = decl.strip()
    if "*" in decl:
        return C.c_void_p
    words = decl.split()[:-1]
    if words == ["int"]:
        return C.c_int
    if words == ["float"]:
        return C.c_float
    raise AssertionError(f"unexpected parameter {decl!r}")


@pytest.mark.parametrize("name", MIX_SYMBOLS)
def test_symbol_header_and_prototype_agree(name):
    lib = _built()
    assert hasattr(lib, name), f"libmocha_hip.so does not export {name}"
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", _header())
    assert m, f"include/mocha_hip.h does not declare {name}"
    want = [_ctype_of(p) for p in m.group(1).split(",")]
    res, args = _C.SIGNATURES[name]
    assert res is C.c_int and args == want, (name, len(args), len(want))


def test_abi_version_and_limits():
    lib = _built()
    assert lib.mocha_abi_version() == 6 == _C.ABI_VERSION
    h = _header()
    assert re.search(r"#define\s+MOCHA_MIX_MAX\s+4\b", h) and re.search(r"#define\s+MOCHA_MIX_PARTS\s+6\b", h)
    assert (MC.MIX_MAX, MC.MIX_PARTS) == (4, 6)


@pytest.mark.parametrize("name", MIX_SYMBOLS)
def test_null_context_is_an_argument_error(name):
    lib = _built()
    _, args = _C.SIGNATURES[name]
    call = [None if a is C.c_void_p else (1.0 if a is C.c_float else 2) for a in args]       # a NULL context, J = 2 where it stands
    assert getattr(lib, name)(*call) == ERR_ARG


def test_part_names_follow_the_pool_matrix():
    """One name per column of the layout's pool matrix; left / right limbs hold the joints the reference's groups give them."""
    for layout, names in skeleton.PART_NAMES.items():
        assert len(names) == 6 == len(set(names)) == skeleton.pool_matrix(layout).shape[1]
        assert set(names) == {"Spine", "Neck", "LeftArm", "RightArm", "LeftLeg", "RightLeg"}
        assert names[0] == "Spine" and 0 in skeleton.LAYOUTS[layout]["parts"][0]         # the hips belong to the spine part


def test_mix_tensors_shapes_and_refusals():
    import numpy as np
    import torch
    ids, w = MC.mix_tensors(([0, 2], [0.25, 0.75]), 3, "cpu", "t")
    assert ids.shape == (3, 2) and ids.dtype == torch.int32 and w.shape == (3, 2, 6) and w.dtype == torch.float32
    assert ids.tolist() == [[0, 2]] * 3 and bool((w[:, 0] == 0.25).all()) and bool((w[:, 1] == 0.75).all())
    m = np.array([[1, 0, 1, 1, 0, 0], [0, 1, 0, 0, 1, 1]], dtype=np.float32)
    ids, w = MC.mix_tensors((np.array([[0, 1], [1, 0], [2, 2]]), m), 3, "cpu", "t", J=2)
    assert np.array_equal(w[1].numpy(), m)
    _, w = MC.mix_tensors((np.zeros((3, 2), np.int64), np.arange(6, dtype=np.float32).reshape(3, 2)), 3, "cpu", "t")
    assert w[2, 1].tolist() == [5.0] * 6
    for bad in ((np.zeros((3, 5), np.int32), np.zeros((3, 5))), (np.zeros((3, 0), np.int32), np.zeros((3, 0))), ([0.5, 1.0], [1, 1]),
                ([0, 1], [1.0, 1.0, 1.0]), (np.zeros((2, 2), np.int32), [1, 1]), 7):
        with pytest.raises(ValueError):
            MC.mix_tensors(bad, 3, "cpu", "t")
    with pytest.raises(ValueError):
        MC.mix_tensors(([0, 1], [1, 1]), 3, "cpu", "t", J=3)
    for bad in (0, 5, 2.0, True):
        with pytest.raises(ValueError):
            MC.mix_count(bad, "t")
    assert MC.mix_count(4, "t") == 4
