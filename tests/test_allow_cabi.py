"""The C entry points of action-constrained matching: mocha_bank_set_labels, mocha_match_segmented_allow,
mocha_characterize_segmented_allow, mocha_step_graph_segmented_allow, mocha_live_step_allow, mocha_live_step_raw_allow.

Without a GPU: the header, the ctypes binding and the built library agree on the six names, the ABI version is still 6, a NULL context is
refused before anything touches a device.  On the GPU: one ctypes round trip without the Python wrappers."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from mocha_sigasia2023_amd import _C

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["mocha_bank_set_labels", "mocha_match_segmented_allow", "mocha_characterize_segmented_allow", "mocha_step_graph_segmented_allow",
       "mocha_live_step_allow", "mocha_live_step_raw_allow"]
ERR_ARG, ERR_STATE = -1, -3


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
    # what is not covered is said in the header
    for phrase in ("NOT covered", "mocha_live_step_ours", "inertializing a CHANGE"):
        assert phrase in txt, phrase


def test_abi_version_unchanged():
    lib = _built()
    assert _C.ABI_VERSION == 6 and lib.mocha_abi_version() == 6          # additive: existing callers keep working
    m = re.search(r"MOCHA_ERR_STATE\s*=\s*(-?\d+)", open(os.path.join(REPO, "include", "mocha_hip.h")).read())
    assert m and int(m.group(1)) == ERR_STATE


def test_null_context_is_refused_without_a_device():
    lib = _built()
    buf = (C.c_double * 8)()                       # host memory standing in for device pointers: must never be dereferenced
    p = C.cast(buf, C.c_void_p)
    assert lib.mocha_bank_set_labels(None, None, None) == ERR_ARG
    assert lib.mocha_match_segmented_allow(None, p, 1, p, p, 1, p, p, p, None) == ERR_ARG
    assert lib.mocha_characterize_segmented_allow(None, p, 1, p, p, 0, 0.0, p, p, p, p, p, p, 0, None) == ERR_ARG
    assert lib.mocha_step_graph_segmented_allow(None, p, 1, p, p, 0, 0.0, p, p, p, p, p, p, 0, None) == ERR_ARG
    assert lib.mocha_live_step_allow(None, None, p, 1, *([p] * 11), 0, 0.0, *([p] * 9), None, None, None, p, p) == ERR_ARG
    assert lib.mocha_live_step_raw_allow(None, None, None, p, p, 1, *([p] * 5), 0, 0.0, *([p] * 9), None, None, None, p, p) == ERR_ARG


@pytest.mark.gpu
def test_ctypes_round_trip():
    """mocha_bank_set_segments + mocha_bank_set_labels + mocha_match_segmented_allow through ctypes alone: 2 characters of 3 rows in D = 23 040;
    query = character 0's row 0 (label 0).  Mask {1}: row 1 or 2, whichever is nearer; mask 0: row 0; mask {5}: falls back to row 0."""
    import torch
    from mocha_sigasia2023_amd import Generator, weights
    dev = torch.device("cuda:0")
    m = Generator(layout="mixamo", device=dev).load_state_dict(weights.synthetic_state_dict(1777, 1.0, "mixamo")).eval()
    lib, h = m._ctx.lib, m._ctx.h
    D = 90 * 256
    g = torch.Generator(device="cpu"); g.manual_seed(3)
    bank = torch.randn((6, D), generator=g)
    bank[2] = bank[0] + 0.5 * (bank[2] - bank[0])                      # row 2 nearer to row 0 than row 1 is
    q = bank[[0, 0, 0, 3]].clone()
    dbank, dq = bank.to(dev), q.to(dev)
    seg_start = (C.c_int64 * 3)(0, 3, 6)
    p = lambda t: C.c_void_p(t.data_ptr())                              # noqa: E731
    assert lib.mocha_bank_set_segments(h, p(dbank), p(dbank), 6, seg_start, 2, 1, None) == 0
    seg = torch.tensor([0, 0, 0, 1], dtype=torch.int32, device=dev)
    allow = torch.tensor([2, 0, 32, 2], dtype=torch.int64, device=dev)
    idx = torch.full((4,), -7, dtype=torch.int32, device=dev)
    dist = torch.full((4,), -7.0, device=dev)
    applied = torch.full((4,), -7, dtype=torch.int32, device=dev)
    args = (h, p(dq), 4, p(seg), p(allow), 1, p(idx), p(dist), p(applied), None)
    assert lib.mocha_match_segmented_allow(*args) == ERR_STATE            # no labels yet
    gen0 = lib.mocha_generation(h)
    bad = (C.c_int32 * 6)(0, 1, 1, 0, 64, 1)
    assert lib.mocha_bank_set_labels(h, bad, None) == ERR_ARG and lib.mocha_generation(h) == gen0
    torch.cuda.synchronize()
    assert (idx == -7).all() and (dist == -7).all() and (applied == -7).all()          # refusals write nothing
    lab = (C.c_int32 * 6)(0, 1, 1, 0, 1, 1)
    assert lib.mocha_bank_set_labels(h, lab, None) == 0 and lib.mocha_generation(h) > gen0
    assert lib.mocha_match_segmented_allow(*args) == 0
    torch.cuda.synchronize()
    assert idx.tolist() == [2, 0, 0, 1 if float((bank[4] - bank[3]).norm()) < float((bank[5] - bank[3]).norm()) else 2]
    assert applied.tolist() == [1, 0, -1, 1]
    want = float((bank[2].double() - bank[0].double()).norm())
    assert abs(float(dist[0]) - want) <= 1e-5 * want and float(dist[1]) == 0.0 and float(dist[2]) == 0.0
    assert lib.mocha_match_segmented_allow(h, p(dq), 4, p(seg), p(allow), 9, p(idx), p(dist), p(applied), None) == ERR_ARG
    assert lib.mocha_bank_set_labels(h, None, None) == 0                  # removed: constrained calls are refused again
    assert lib.mocha_match_segmented_allow(*args) == ERR_STATE
    assert np.array_equal(applied.cpu().numpy(), [1, 0, -1, 1])
