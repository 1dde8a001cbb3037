"""CPU-side checks of the multi-character bank's C ABI (ABI 6): the segmented entry points are declared, bound and exported (no compute
calls here: there is no GPU; tests/test_multi_character.py runs them on the MI355X)."""
import os

from mocha_sigasia2023_amd import MultiCharacterBank, MultiStreamCharacterizer, _C

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("mocha_bank_set_segments", "mocha_match_segmented", "mocha_characterize_segmented", "mocha_step_graph_segmented")


def _built():
    if not os.path.exists(_C.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _C.load_library()


def test_segmented_entry_points_declared_bound_and_exported():
    header = open(os.path.join(REPO, "include", "mocha_hip.h")).read()
    lib = _built()
    for name in NEW:
        assert f"{name}(" in header, name
        assert name in _C.SIGNATURES, name
        assert hasattr(lib, name), f"libmocha_hip.so does not export {name}"
    assert "#define MOCHA_BANK_NO_DEC_CACHE 4" in header
    assert _C.ABI_VERSION == 6
    assert lib.mocha_abi_version() == 6


def test_python_classes_exported():
    import mocha_sigasia2023_amd as pkg
    assert "MultiCharacterBank" in pkg.__all__ and "MultiStreamCharacterizer" in pkg.__all__
    assert callable(MultiCharacterBank.query) and callable(MultiStreamCharacterizer.step)
