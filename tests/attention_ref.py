"""ctypes loader of the test-only probe of the attention launchers (tests/gemm_probe/attention_probe.cpp, built by
`make -C tests/gemm_probe`) and the restatement of what a launch MEANS: the formula of csrc/kernels.h written with torch on the CPU in the
dtype it is given - float64 is the truth, float32 the evaluation that sizes a bound.  Used by tests/test_attention_kernels.py only.
Nothing here is transcribed from the kernels: no tiles, no lane maps, no planes in the arithmetic.

Also here: `kv_encode`, the inverse of pointwise_ref.kv_decode - fp32 keys and values into the pre-split image launch_attention_x3_kv
reads (layout comment at the top of csrc/attention_kv.hip), so that the kernel can be given arbitrary keys, not only instance-normalised ones.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np
import torch

import pointwise_ref as pr

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "gemm_probe", "libmocha_attention_probe.so")
BAD_ARGUMENT = -2
INVALID_VALUE = 1          # hipErrorInvalidValue
F32, X3, KV = 0, 1, 2
KV_IMG_BYTES = pr.KV_IMG_BYTES

_vp, _i, _ll, _f = C.c_void_p, C.c_int, C.c_longlong, C.c_float


class at_params(C.Structure):
    _fields_ = ([(n, _vp) for n in ("q", "k", "v", "out", "kv_idx", "kv")] + [("kv_rows", _ll)] +
                [(n, _i) for n in ("ldq", "ldk", "ldv", "ldo", "B", "heads", "dh", "nq", "nk", "hsk", "hsv", "split_max", "reverse", "pairs")] +
                [("scale", _f)])


# AttnParams' own defaults (csrc/kernels.h)
DEFAULTS = dict(hsk=-1, hsv=-1, split_max=192, reverse=0, pairs=0, kv_rows=0)
_lib = None


def load():
    """The probe library; a missing build is an error (no fallback)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(f"{LIB_PATH} is missing: run __graft_entry__.build() (make -C tests/gemm_probe)")
        lib = C.CDLL(LIB_PATH)
        lib.at_attention.restype, lib.at_attention.argtypes = _i, [C.POINTER(at_params), _i, _vp]
        lib.at_sane.restype, lib.at_sane.argtypes = _i, [C.POINTER(at_params), _i]
        lib.at_kv_img_bytes.restype, lib.at_kv_img_bytes.argtypes = _i, []
        _lib = lib
    return _lib


def make_params(**kw) -> at_params:
    p = at_params()
    vals = dict(DEFAULTS)
    vals.update(kw)
    for k, v in vals.items():
        if not hasattr(p, k):
            raise KeyError(k)
        setattr(p, k, v)
    return p


def instance(which, *, dh, nq, nk, B, heads, split_max=192, pairs=0):
    """The kernel instance a launcher takes for these parameters (the dispatch rules stated in csrc/kernels.h and the launchers' comments)."""
    if which == F32:
        if nq <= 96 and nk <= 96:
            return f"f32<{dh},3,3>"
        return "f32<64,6,3>" if nq <= 96 else "f32<64,6,6>"
    if which == X3:
        if dh == 256 and B * heads <= split_max:
            return "x3 split<256>"
        return f"x3<{dh},{'true' if B * heads <= 256 else 'false'}>"
    return "kv<256,4>" if heads % 4 == 0 and not pairs else "kv<256,2>"


# ------------------------------------------------------------------------------------------------------------------ the operation
def attention(q, k, v, *, B, heads, dh, nq, nk, scale, hsk=-1, hsv=-1, kv_idx=None, kv_rows=0):
    """csrc/kernels.h: q [>= B nq, ldq], k and v [rows, ld] (torch CPU tensors of one dtype; views with any strides) ->
    out [B, nq, heads dh]:  out[b, i, h dh + d] = sum_j softmax_j(scale q_i . k_j) v_j[d]  with q_i = row b nq + i of q at column h dh,
    k_j = row bk nk + j of k at column h hsk, v_j = row bk nk + j of v at column h hsv; bk = b, or clamp(kv_idx[b], 0, kv_rows - 1);
    hsk / hsv < 0 means dh."""
    hsk, hsv = (dh if hsk < 0 else hsk), (dh if hsv < 0 else hsv)
    bk = torch.arange(B) if kv_idx is None else torch.as_tensor(np.asarray(kv_idx), dtype=torch.int64).clamp(0, kv_rows - 1)
    rows = bk[:, None] * nk + torch.arange(nk)[None, :]                           # [B, nk]
    d = torch.arange(dh)
    Q = q[:B * nq, :heads * dh].reshape(B, nq, heads, dh)
    K = k[rows][:, :, (torch.arange(heads) * hsk)[:, None] + d[None, :]]           # [B, nk, heads, dh]
    V = v[rows][:, :, (torch.arange(heads) * hsv)[:, None] + d[None, :]]
    s = torch.einsum("bihd,bjhd->bhij", Q, K) * scale
    p = torch.softmax(s, dim=-1)
    return torch.einsum("bhij,bjhd->bihd", p, V).reshape(B, nq, heads * dh)


def kv_encode(K, V):
    """fp32 K, V [B, n <= 96, 256] -> uint8 [B, KV_IMG_BYTES], the image launch_attention_x3_kv reads: the three bf16 planes of every
    value (pointwise_ref.plane_chain), 16 stages - stage c < 8 = K dims 32c .. 32c + 31, stage 8 + c = V the same dims -, a stage =
    [plane][row 96][64 B]; a K row's four 16-byte pieces XOR-swizzled by (row >> 2) & 3, V rows plain; rows n .. 95 zero."""
    K, V = np.asarray(K, dtype=np.float32), np.asarray(V, dtype=np.float32)
    B, n, _ = K.shape
    assert K.shape == V.shape == (B, n, 256) and 1 <= n <= 96

    def stages(x):                                                                  # -> [B, 8 stages, 3 planes, 96 rows, 4 pieces, 8 bf16]
        p = np.zeros((3, B, 96, 256), dtype=np.uint16)
        p[:, :, :n] = pr.plane_chain(x)
        return p.transpose(1, 0, 2, 3).reshape(B, 3, 96, 8, 4, 8).transpose(0, 3, 1, 2, 4, 5)

    rows = np.arange(96)
    at = np.arange(4)[None, :] ^ ((rows[:, None] >> 2) & 3)                        # an involution: where piece j is stored = which piece sits at j
    img = np.concatenate([stages(K)[:, :, :, rows[:, None], at], stages(V)], axis=1)
    return np.ascontiguousarray(img).view(np.uint8).reshape(B, KV_IMG_BYTES)


def planes_value(planes):
    """uint16 [3, ...] bf16 planes -> the float64 value they stand for (their exact sum)."""
    return pr.bf16_value(planes).astype(np.float64).sum(0)


errors, ulp_of_largest, ptr = pr.errors, pr.ulp_of_largest, pr.ptr
