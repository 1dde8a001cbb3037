"""CPU-side checks of the resident bank's C ABI: the four entry points are declared in the header, bound in _C.py and exported by the
library, the ABI version stays 6 (the entry points are additive), and the Python class is exported (no compute calls here: there is no
GPU; tests/test_resident_bank.py and tests/test_resident_live.py run them on the MI355X)."""
import os

from mocha_sigasia2023_amd import MultiCharacterBank, ResidentCharacterBank, _C

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("mocha_bank_resident_create", "mocha_bank_resident_add", "mocha_bank_resident_retire", "mocha_bank_resident_info")


def _built():
    if not os.path.exists(_C.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _C.load_library()


def test_resident_entry_points_declared_bound_and_exported():
    header = open(os.path.join(REPO, "include", "mocha_hip.h")).read()
    lib = _built()
    for name in NEW:
        assert f"int {name}(" in header, name
        assert name in _C.SIGNATURES, name
        assert hasattr(lib, name), f"libmocha_hip.so does not export {name}"
    assert len(_C.SIGNATURES["mocha_bank_resident_create"][1]) == 6 and len(_C.SIGNATURES["mocha_bank_resident_add"][1]) == 8
    assert len(_C.SIGNATURES["mocha_bank_resident_retire"][1]) == 3 and len(_C.SIGNATURES["mocha_bank_resident_info"][1]) == 6
    assert _C.ABI_VERSION == 6
    assert lib.mocha_abi_version() == 6


def test_null_context_is_an_error_code():
    lib = _built()
    assert lib.mocha_bank_resident_info(None, -1, None, None, None, None) == -1
    assert lib.mocha_bank_resident_retire(None, 0, None) == -1
    assert lib.mocha_bank_resident_add(None, -1, None, None, 1, None, None, None) == -1
    assert lib.mocha_bank_resident_create(None, 16, 1, 16, 0, None) == -1


def test_python_class_exported_and_shares_the_segmented_calls():
    import mocha_sigasia2023_amd as pkg
    assert "ResidentCharacterBank" in pkg.__all__
    for name in ("add", "retire", "replace", "rows", "query", "characterize", "_ids", "_allow", "_ensure"):
        assert callable(getattr(ResidentCharacterBank, name)), name
    assert isinstance(ResidentCharacterBank.free_rows, property) and isinstance(ResidentCharacterBank.largest_free, property)
    # one implementation of the segmented calls, not a copy
    assert ResidentCharacterBank.query is MultiCharacterBank.query and ResidentCharacterBank.characterize is MultiCharacterBank.characterize
    assert ResidentCharacterBank._ids is MultiCharacterBank._ids and ResidentCharacterBank._allow is MultiCharacterBank._allow
