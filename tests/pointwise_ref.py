"""ctypes loader of the test-only probe of the norm / pointwise launchers (tests/gemm_probe/pointwise_probe.cpp, built by
`make -C tests/gemm_probe`) and one restatement per operation of what it MEANS: the formulas of csrc/kernels.h and the model lines they
cite, written with torch on the CPU in the dtype they are given - float64 is the truth, float32 the evaluation that sizes a bound.  Used by
tests/test_pointwise_kernels.py only.  Nothing here is transcribed from the kernels: no token groups, no rings, no lane maps.

Also here: bf16 round-to-nearest-even in numpy integer arithmetic, the three-plane chain in fp32, and a decoder of the decoder attention's
key / value image written from the layout comment at the top of csrc/attention_kv.hip.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np
import torch
import torch.nn.functional as F

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "gemm_probe", "libmocha_pointwise_probe.so")
BAD_ARGUMENT = -2
INVALID_VALUE = 1          # hipErrorInvalidValue
EPS = 1e-5
KV_STAGE_BYTES = 3 * 96 * 64
KV_IMG_BYTES = 16 * KV_STAGE_BYTES
QSTAT_PARTS = 4

_vp, _i, _ll, _f = C.c_void_p, C.c_int, C.c_longlong, C.c_float


class pw_inorm(C.Structure):
    _fields_ = ([(n, _vp) for n in ("x", "out", "mean_out", "gm", "gs", "zn", "centre", "zc", "zc16", "qstat", "table", "row_idx", "copy_out",
                                    "kvimg", "mean64")] +
                [("plane_stride", _ll), ("table_rows", _ll)] + [(n, _i) for n in ("split_max", "reverse", "B", "n")])


_SIGNATURES = {
    "pw_instnorm": [C.POINTER(pw_inorm), _i, _vp],
    "pw_adain": [_vp, _vp, _i, _vp, _vp, _i, _i, _i, _vp, _ll, _i, _i, _vp],
    "pw_embed_front": [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _vp, _vp, _i, _i, _i, _vp],
    "pw_embed_sums": [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _vp, _vp, _i, _i, _i, _vp],
    "pw_window_sums": [_vp, _vp, _i, _i, _vp],
    "pw_body_front": [_vp, _vp, _vp, _i, _i, _vp],
    "pw_joint_expand": [_vp, _vp, _vp, _i, _i, _i, _vp],
    "pw_final_proj": [_vp, _vp, _vp, _vp, _i, _i, _i, _vp, _vp, _i, _i, _vp],
    "pw_linear_f64": [_vp, _i, _i, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _vp],
    "pw_rownorm2": [_vp, _vp, _vp, _ll, _i, _i, _vp],
    "pw_sub_rows": [_vp, _vp, _vp, _ll, _i, _vp],
    "pw_center_rows": [_vp, _vp, _vp, _i, _vp, _vp, _ll, _i, _i, _vp],
    "pw_column_mean": [_vp, _ll, _i, _vp, _vp, _ll, _vp],
    "pw_column_stats": [_vp, _ll, _i, _vp, _vp, _vp],
    "pw_absmax": [_vp, _ll, _ll, _vp, _f, _f, _vp],
}
_lib = None


def load():
    """The probe library; a missing build is an error (no fallback)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(f"{LIB_PATH} is missing: run __graft_entry__.build() (make -C tests/gemm_probe)")
        lib = C.CDLL(LIB_PATH)
        for name, args in _SIGNATURES.items():
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = _i, args
        lib.pw_column_mean_scratch_doubles.restype, lib.pw_column_mean_scratch_doubles.argtypes = _ll, [_i]
        _lib = lib
    return _lib


def ptr(t):
    """Device (or host) address of a tensor, 0 for None."""
    return 0 if t is None else t.data_ptr()


# ------------------------------------------------------------------------------------------------------------------ bf16 and planes
def bf16_bits(x):
    """fp32 array -> bf16 bit patterns (uint16), round to nearest even, in integer arithmetic; a NaN stays a (quiet) NaN."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)
    nan = (u & 0x7FFFFFFF) > 0x7F800000
    return np.where(nan, ((u >> 16) | 0x40).astype(np.uint16), r)


def bf16_value(bits):
    """bf16 bit patterns -> the fp32 values they stand for."""
    return (np.asarray(bits).astype(np.uint32) << 16).view(np.float32)


def plane_chain(x, nplanes=3):
    """x0 = bf16(x), x1 = bf16(x - x0), x2 = bf16(x - x0 - x1), the subtractions in fp32: uint16 [nplanes, ...]."""
    r = np.ascontiguousarray(x, dtype=np.float32).copy()
    out = []
    for _ in range(nplanes):
        b = bf16_bits(r)
        out.append(b)
        r = (r - bf16_value(b)).astype(np.float32)
    return np.stack(out)


def kv_decode(img):
    """The key / value image of csrc/attention_kv.hip, one window per row of `img` (uint8 [B, KV_IMG_BYTES]) -> (K, V), each uint16
    [B, 3 planes, 96 rows, 256 head dims].  Layout: 16 stages; stage c < 8 = K dims 32c .. 32c + 31, stage 8 + c = V the same dims; a
    stage = [plane][row][64 B]; a K row's four 16-byte pieces sit XOR-swizzled by (row >> 2) & 3, V rows are plain."""
    B = img.shape[0]
    s = np.ascontiguousarray(img).view(np.uint16).reshape(B, 16, 3, 96, 4, 8)             # stage, plane, row, piece, bf16 of the piece
    rows = np.arange(96)
    piece = np.arange(4)[None, :] ^ ((rows[:, None] >> 2) & 3)                            # where logical piece j of row r is stored
    k = s[:, :8][:, :, :, rows[:, None], piece]                                            # [B, 8, 3, 96, 4, 8]
    v = s[:, 8:]
    def dims(a):
        return a.reshape(B, 8, 3, 96, 32).transpose(0, 2, 3, 1, 4).reshape(B, 3, 96, 256)
    return dims(k), dims(v)


# ------------------------------------------------------------------------------------------------------------------ norms
def instnorm(x):
    """net/transformer.py:13-20 on x (B, n, 256): per (window, channel) over the n tokens, unbiased std, eps outside the root.
    Returns (out, mean (B, 256))."""
    n = x.shape[1]
    mean = x.sum(1, keepdim=True) / n
    d = x - mean
    std = ((d * d).sum(1, keepdim=True) / (n - 1)).sqrt()
    return d / (std + EPS), mean[:, 0]


def adain_literal(x, gamma, beta):
    """net/transformer.py:108-113 then :49-56 in the order written: xad = (1 + gamma) IN(x) + beta, qin = IN(xad); gamma, beta (B, 256)."""
    xad = (1 + gamma)[:, None] * instnorm(x)[0] + beta[:, None]
    return xad, instnorm(xad)[0]


def adain_closed(x, gamma, beta):
    """The same from the first statistics (csrc/kernels.h; tests/test_adain_identity.py): qin = (1+g)(x-m) / (|1+g| s + eps (s + eps))."""
    n = x.shape[1]
    m = x.sum(1, keepdim=True) / n
    d = x - m
    s = ((d * d).sum(1, keepdim=True) / (n - 1)).sqrt()
    g1 = (1 + gamma)[:, None]
    return g1 * d / (s + EPS) + beta[:, None], g1 * d / (g1.abs() * s + EPS * (s + EPS))


# ------------------------------------------------------------------------------------------------------------------ front ends
def embed_front(X, W1, b1, AP, xmean=None, xstd=None, raw_root=0):
    """csrc/kernels.h: X (frames, V + raw_root, Cin) -> 1x1 conv Cin -> 64 + bias -> LeakyReLU(0.2) -> AP' (3, V, 6) = hop-partitioned
    adjacency times the joint -> part pool -> rows (frame, part p) x (hop k * 64 + c), returned as (frames, 6, 192).
    xmean / xstd ((V + raw_root) * Cin): the frame is z-scored on load; raw_root = 1: the root bone in front is dropped (after the z-score's
    vectors have been indexed WITH it)."""
    if xmean is not None:
        X = (X - xmean.reshape(1, *X.shape[1:])) / xstd.reshape(1, *X.shape[1:])
    X = X[:, raw_root:]
    h = F.leaky_relu(X @ W1.T + b1, 0.2)                                  # (frames, V, 64)
    return torch.einsum("kvp,fvc->fpkc", AP, h).reshape(X.shape[0], 6, 192)


def reflect60(t):
    """Reflect padding without edge repeat on a 60-frame line (net/blocks.py:112-118)."""
    t = np.abs(t)
    return np.where(t > 59, 118 - t, t)


def window_sums(y):
    """csrc/kernels.h: y (B, 60, 6, C) -> u (B, 15, 6, 5 C): u[b, t', p, dt C + c] = 1/4 sum_{j<4} y[b, refl(4 t' + j + dt - 2), p, c]."""
    B, _, P, Cc = y.shape
    t = 4 * np.arange(15)[:, None, None] + np.arange(4)[None, None, :] + np.arange(5)[None, :, None] - 2       # [t', dt, j]
    g = y[:, torch.from_numpy(reflect60(t))]                              # (B, 15, 5, 4, 6, C)
    return (g.sum(3) * 0.25).permute(0, 1, 3, 2, 4).reshape(B, 15, P, 5 * Cc)


def body_front(x, Ab):
    """x (frames, 6, 256), Ab (2, 6, 6) -> (frames, 6, 512): out[f, w, k 256 + c] = sum_v Ab[k][v][w] lrelu(x[f, v, c])."""
    return torch.einsum("kvw,fvc->fwkc", Ab, F.leaky_relu(x, 0.2)).reshape(x.shape[0], 6, 512)


def joint_expand(g, AU):
    """g (frames, 6, 192), AU (3, 6, V) -> (frames, V, 64): out[f, w, c] = sum_k sum_p AU[k][p][w] g[f, p, k 64 + c]."""
    return torch.einsum("kpw,fpkc->fwc", AU, g.reshape(g.shape[0], 6, 3, 64))


def final_proj(z, W6, b6, V, ymean=None, ystd=None, phased=False):
    """model.py:77-79: Y[m] = W6 lrelu(z[m]) + b6 on rows (window, frame, joint), optionally de-normalised with row joint + 1 of
    ymean / ystd ((V + 1, Cout): the root row comes first and belongs to no output row).
    phased: z is (windows, 15, V, 256); output row (window, t, joint), t < 60, reads channels (t & 3) * 64 .. + 63 of input row
    (window, t >> 2, joint)."""
    if phased:
        W = z.shape[0]
        t = torch.arange(60)
        z = z.reshape(W, 15, V, 4, 64)[:, t >> 2, :, t & 3]                # advanced indices first: (60, W, V, 64)
        z = z.permute(1, 0, 2, 3).reshape(W * 60 * V, 64)
    y = F.leaky_relu(z, 0.2) @ W6.T + b6
    if ymean is not None:
        v = torch.arange(y.shape[0]) % V
        y = y * ystd.reshape(V + 1, -1)[v + 1] + ymean.reshape(V + 1, -1)[v + 1]
    return y


def linear_f64(X, W, bias, N, K, L, xcol, act):
    """csrc/kernels.h: L independent column blocks, block l: act(X[:, l xcol : l xcol + K] W[l]^T + bias[l]) -> columns [l N, (l + 1) N).
    numpy.longdouble throughout.  Returns (y (M, L N), sum_k |x||w| of every element): the second sizes the float64 kernels' bound."""
    Xl, Wl = X.astype(np.longdouble), W.astype(np.longdouble).reshape(L, N, K)
    ys, mags = [], []
    for l in range(L):
        xs = Xl[:, l * xcol:l * xcol + K]
        y = xs @ Wl[l].T
        if bias is not None:
            y = y + bias.astype(np.longdouble)[l * N:(l + 1) * N]
        ys.append(np.where(y > 0, y, y * np.longdouble(0.2)) if act == 2 else y)
        mags.append(np.abs(X[:, l * xcol:l * xcol + K]) @ np.abs(W.reshape(L, N, K)[l]).T)      # float64: a bound needs no more
    return np.concatenate(ys, 1), np.concatenate(mags, 1)


# ------------------------------------------------------------------------------------------------------------------ bounds
def errors(y, ref64):
    d = (y.double() - ref64).flatten()
    return float(d.abs().max()), float(d.pow(2).mean().sqrt())


def ulp_of_largest(ref64):
    return float(np.spacing(np.float32(float(ref64.abs().max()))))
