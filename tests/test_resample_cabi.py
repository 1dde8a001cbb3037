"""The C entry points of the resampler: mocha_resample_frames, mocha_resample_clips, mocha_resample_state_bytes, mocha_resample_reset and
mocha_resample_step are declared in the header, bound in _C.SIGNATURES and exported by the built library with matching argument counts; the
ABI version is still 6 and mocha_ingest_cfg keeps its fields; the host-only count is the Fraction-based one, 64-bit results included; bad
arguments and a NULL context are refused before anything touches a device; the Python surface is as documented.  No GPU."""
import ctypes as C
import inspect
import os
import re
import sys
from fractions import Fraction

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mocha_sigasia2023_amd as M  # noqa: E402
from mocha_sigasia2023_amd import _C  # noqa: E402
from mocha_sigasia2023_amd.ingest import resample_lengths, resample_ratio  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["mocha_resample_frames", "mocha_resample_clips", "mocha_resample_state_bytes", "mocha_resample_reset", "mocha_resample_step"]
ERR_ARG = -1
FIELDS = ["lookahead", "rot_format", "euler_order", "unit_scale", "fps", "contact_velocity_threshold", "spine", "shoulder_l", "shoulder_r",
          "upleg_l", "upleg_r"]
RATIOS = [(2, 1), (1, 2), (3, 2), (5, 3), (5, 6), (2, 5), (1, 1)]


def _built():
    if not os.path.exists(_C.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _C.load_library()


def _count(n, num, den):
    """Outputs k = 0, 1, ... whose position k num / den does not pass the last source frame n - 1."""
    return int((n - 1) / Fraction(num, den)) + 1


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
    assert _C.SIGNATURES["mocha_resample_frames"][0] is C.c_int64 and _C.SIGNATURES["mocha_resample_state_bytes"][0] is C.c_int64
    assert [f[0] for f in _C.mocha_ingest_cfg._fields_] == FIELDS             # additive: the struct is as it was


def test_abi_version_unchanged():
    lib = _built()
    assert _C.ABI_VERSION == 6 and lib.mocha_abi_version() == 6


def test_frames_is_the_fraction_count():
    lib = _built()
    for num, den in RATIOS + [(4096, 1), (1, 4096), (4096, 4095), (1001, 2000)]:
        for n in list(range(1, 201)) + [4099, 2 ** 31 - 1]:
            assert lib.mocha_resample_frames(n, num, den) == _count(n, num, den), (n, num, den)
    big = lib.mocha_resample_frames(2 ** 31 - 1, 1, 4)
    assert big == (2 ** 31 - 2) * 4 + 1 and big > 2 ** 32                       # past int32: the 64-bit path
    for n, num, den in ((0, 1, 1), (-3, 1, 1), (2 ** 31, 1, 1), (5, 0, 1), (5, 1, 0), (5, 4097, 1), (5, 1, 4097), (5, -1, 1)):
        assert lib.mocha_resample_frames(n, num, den) < 0, (n, num, den)


def test_null_context_is_refused_without_a_device():
    lib = _built()
    buf = (C.c_double * 8)()                       # host memory standing in for device pointers: must never be dereferenced
    p = C.cast(buf, C.c_void_p)
    order = (C.c_int * 3)(2, 1, 0)
    off, one, n_out = (C.c_int32 * 2)(0, 5), (C.c_int32 * 1)(1), C.c_int32(-7)
    assert lib.mocha_resample_clips(None, 1, order, p, p, off, one, one, 1, off, p, p, None) == ERR_ARG
    assert lib.mocha_resample_state_bytes(None, 1) == ERR_ARG
    assert lib.mocha_resample_reset(None, p, 1, None, 0, None) == ERR_ARG
    assert lib.mocha_resample_step(None, 1, order, p, 1, p, p, 2, 1, 0, p, p, C.byref(n_out), None) == ERR_ARG
    assert n_out.value == -7


def test_python_surface():
    for name in ("resample_clips", "resample_lengths", "StreamResampler"):
        assert name in M.__all__ and hasattr(M, name), name
    sig = inspect.signature(M.resample_clips)
    assert list(sig.parameters) == ["model", "rot", "pos", "lengths", "source_fps", "target_fps", "order"]
    assert sig.parameters["target_fps"].default == 60.0 and sig.parameters["order"].default == "zyx"
    assert list(inspect.signature(M.resample_lengths).parameters) == ["lengths", "source_fps", "target_fps"]
    sig = inspect.signature(M.StreamResampler.__init__)
    assert list(sig.parameters) == ["self", "model", "source_fps", "target_fps", "order", "streams"]
    assert sig.parameters["target_fps"].default == 60.0 and sig.parameters["order"].default == "zyx" and sig.parameters["streams"].default == 1
    for method in ("push", "restart", "reset"):
        assert callable(getattr(M.StreamResampler, method))
    assert list(inspect.signature(M.StreamResampler.push).parameters) == ["self", "rot", "pos"]
    assert list(inspect.signature(M.StreamResampler.restart).parameters) == ["self", "streams"]
    sig = inspect.signature(M.load_bvh)
    assert list(sig.parameters) == ["model", "paths", "joints", "fps", "source_fps"]
    assert sig.parameters["fps"].default is None and sig.parameters["source_fps"].default is None
    from mocha_sigasia2023_amd import bank
    sig = inspect.signature(bank.build_database_from_bvh)
    assert list(sig.parameters) == ["model", "paths", "style_labels", "action_labels", "mirror", "raw", "post", "joints", "fps"]
    assert sig.parameters["fps"].default is None
    # pinned: the resampler is a stage in front of these two, not a change to them
    assert list(inspect.signature(M.ingest_clips).parameters) == ["model", "rot", "pos", "lengths", "raw", "mirror", "post"]
    assert list(inspect.signature(M.clip_windows).parameters) == ["processed", "lengths", "window", "step", "model"]


def test_ratios_and_lengths_on_the_host():
    _built()
    assert resample_ratio(120, 60) == (2, 1) and resample_ratio(30) == (1, 2) and resample_ratio(90, 60.0) == (3, 2)
    assert resample_ratio(100, 60) == (5, 3) and resample_ratio(Fraction(30000, 1001), 60) == (500, 1001) and resample_ratio(24, 60) == (2, 5)
    assert resample_ratio(119.88, 59.94) == (2, 1)                                # floats go through limit_denominator(1000)
    assert resample_lengths([1, 2, 3, 7, 45, 7200], 120, 60) == [1, 1, 2, 4, 23, 3600]
    assert resample_lengths([45, 45, 45], [120, 30, 60]) == [23, 89, 45]
    assert resample_lengths([45], Fraction(90), Fraction(60)) == [_count(45, 3, 2)] == [30]
    with pytest.raises(ValueError):
        resample_ratio(0, 60)
    with pytest.raises(ValueError):
        resample_ratio(4097, 1)
    with pytest.raises(ValueError):
        resample_lengths([45, 45], [120], 60)
    with pytest.raises(ValueError):
        resample_lengths([0], 120, 60)
