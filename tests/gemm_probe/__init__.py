"""ctypes loader of the test-only GEMM probe (probe.cpp, built by `make -C tests/gemm_probe`; __graft_entry__.build() does it) and the
float64 restatement of what a launch computes.  Used by tests/test_gemm_instances.py only.

Nothing here reads the kernels' text: `gather_rows` restates the formula of csrc/kernels.h once in numpy integer arithmetic, and
`reference` evaluates  epilogue(Aop W^T)  with torch on the CPU in the dtype it is given.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libmocha_gemm_probe.so")

UNSUPPORTED, BAD_ARGUMENT = -1, -2
ENGINES = {"f32": 1, "x3": 2, "h2": 3, "x3r": 4}
PREDICATES = ("skinny16", "skinny", "small", "narrow", "x3", "h2", "x3r")

_vp, _i = C.c_void_p, C.c_int


class probe_params(C.Structure):
    _fields_ = ([(n, _vp) for n in ("A", "W", "wsub", "C", "bias", "rowbias", "residual", "a_amax", "c_amax")] + [("slab_stride", C.c_longlong)] +
                [(n, _i) for n in ("M", "N", "K", "lda", "ldc", "ldr", "rb_mod", "act", "a_lrelu", "gather",
                                   "T_out", "V", "ntaps", "pad", "stride", "R", "T_full", "tshift", "Cc", "T_src", "tstep")] +
                [("ascale", C.c_float)] +
                [(n, _i) for n in ("ksplit", "persistent", "persistent_max_n", "tile64_below", "rows_per_win", "x3r_grid")])


# GemmParams' own defaults (csrc/kernels.h)
DEFAULTS = dict(rb_mod=1, act=0, a_lrelu=0, gather=0, T_out=1, V=1, ntaps=1, pad=0, stride=1, R=1, T_full=1, tshift=0, Cc=0, T_src=1, tstep=1,
                ascale=1.0, ksplit=1, slab_stride=0, persistent=768, persistent_max_n=512, tile64_below=0, rows_per_win=90, x3r_grid=0, ldr=0)

_lib = None


def load():
    """The probe library; a missing build is an error (no fallback)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(f"{LIB_PATH} is missing: run __graft_entry__.build() (make -C tests/gemm_probe)")
        lib = C.CDLL(LIB_PATH)
        lib.probe_gemm.restype = _i
        lib.probe_gemm.argtypes = [C.POINTER(probe_params), _i, _vp]
        lib.probe_select.restype = _i
        lib.probe_select.argtypes = [C.POINTER(probe_params), C.POINTER(_i)]
        _lib = lib
    return _lib


def make_params(**kw) -> probe_params:
    p = probe_params()
    vals = dict(DEFAULTS)
    vals.update(kw)
    for k, v in vals.items():
        if not hasattr(p, k):
            raise KeyError(k)
        setattr(p, k, v)
    return p


def select(p: probe_params) -> dict:
    """gemm_is_skinny16 / _skinny / _small / _narrow and the three *_supports() for these parameters (host code; no GPU involved)."""
    out = (_i * 7)()
    rc = load().probe_select(C.byref(p), out)
    assert rc == 0, rc
    return {n: bool(out[i]) for i, n in enumerate(PREDICATES)}


def instance(engine: str, p: probe_params, sel: dict) -> str:
    """The kernel instance a launcher takes, from the exported predicates and - where only file-static rules of the launcher separate two
    instances (x3: 64 x 64 against 64 x 128 tiles, persistent against tiled) - from the fields that force either side."""
    if engine == "f32":
        if sel["skinny16"]:
            return "skinny16"
        if sel["skinny"]:
            return "skinny"
        if sel["small"]:
            return "f32<64,2,2,1,1>"
        return "f32<64,4,1,1,2>" if sel["narrow"] else "f32<128,2,2,2,2>"
    if engine == "x3r":
        return "x3r<%d>" % (1 if (p.bias and p.act == 1) else 0 if p.bias else -1)
    small, odd = sel["small"], p.N % 128 != 0
    if engine == "x3":
        if p.persistent > 0 and p.ksplit <= 1 and not odd and p.N <= p.persistent_max_n and not small:
            return "x3p<%d>" % (1 if p.residual else 2 if p.rowbias else 0)
        t64x128 = ((p.M + 63) // 64) * ((p.N + 127) // 128)
        if p.ksplit <= 1 and p.N % 64 == 0 and small and (odd or t64x128 < p.tile64_below):
            return "x3<64x64>"
        if p.ksplit <= 1 and odd:
            return "x3<128x64>"
        return "x3<64x128>" if (p.ksplit <= 1 and small) else "x3<128x128>"
    assert engine == "h2"
    if odd:
        return "h2<64x64>" if small else "h2<128x64>"
    return "h2<64x128>" if small else "h2<128x128>"


def run(p: probe_params, engine: str, stream: int = 0) -> int:
    return load().probe_gemm(C.byref(p), ENGINES[engine], stream)


# ------------------------------------------------------------------------------------------------------------------ the reference
def gather_rows(M, *, T_out, V, ntaps, pad, stride=1, R=1, T_full, tshift=0, T_src, tstep=1):
    """csrc/kernels.h: output row m = (b, t, v); operand block `tap` is the sum over j < R of source row
    (b, refl(t * stride + j + tap * tstep - pad, T_full) >> tshift, v), rows of a window being (frame, node).  Returns int64 [M, ntaps, R]."""
    m = np.arange(M, dtype=np.int64)
    v, bt = m % V, m // V
    t, b = bt % T_out, bt // T_out
    tap = np.arange(ntaps, dtype=np.int64)[None, :, None]
    j = np.arange(R, dtype=np.int64)[None, None, :]
    tf = t[:, None, None] * stride + j + tap * tstep - pad
    tf = np.abs(tf)                                                    # reflect at the front (no edge repeat) ...
    tf = np.where(tf >= T_full, 2 * (T_full - 1) - tf, tf)             # ... and at the back
    assert tf.min() >= 0 and tf.max() < T_full
    src_t = tf >> tshift
    assert src_t.max() < T_src
    return (b[:, None, None] * T_src + src_t) * V + v[:, None, None]


def operand(A, M, K, g=None, a_lrelu=False):
    """Aop [M, K] in A's dtype (torch CPU tensor [rows, lda]); g = keyword arguments of gather_rows plus Cc and ascale, or None for plain rows."""
    import torch
    if g is None:
        X = A[:M, :K]
    else:
        g = dict(g)
        Cc, ascale = g.pop("Cc"), g.pop("ascale", 1.0)
        rows = torch.from_numpy(gather_rows(M, **g))                   # [M, ntaps, R]
        X = A[:, :Cc][rows]                                            # [M, ntaps, R, Cc]
        X = X[:, :, 0] if rows.shape[2] == 1 else X.sum(2) * ascale
        X = X.reshape(M, K)
    return torch.nn.functional.leaky_relu(X, 0.2) if a_lrelu else X


def _matmul(X, Wt, chain):
    """X Wt in the operands' dtype: torch's own GEMM (its BLAS sums K in blocks of its choosing), or - chain - one accumulator per element
    that takes the K products one after the other, in k order."""
    import torch
    if not chain:
        return X @ Wt
    acc = torch.zeros((X.shape[0], Wt.shape[1]), dtype=X.dtype)
    Xc = X.T.contiguous()
    for k in range(Wt.shape[0]):
        acc.addcmul_(Xc[k, :, None], Wt[k, None, :])
    return acc


def reference(A, W, M, N, K, *, g=None, a_lrelu=False, bias=None, rowbias=None, rb_mod=1, act=0, residual=None, kslice=None, chunk=8192,
              rows=None, chain=False):
    """epilogue(Aop W^T) on the CPU in the operands' dtype, in row chunks: + bias, + rowbias[row % rb_mod], activation (1 exact-erf GELU,
    2 LeakyReLU(0.2), 3 ReLU), + residual.  kslice = (k0, k1): the raw partial sum over that K range (no epilogue).
    rows (int64 tensor): only these output rows, in this order (default: all M).  chain: the K sum as one k-ordered chain (_matmul)."""
    import torch
    F = torch.nn.functional
    Wt = W[:N, :K].T.contiguous()
    X = operand(A, M, K, g, a_lrelu)
    rows = torch.arange(M) if rows is None else rows
    X = X[rows]
    out = torch.empty((len(rows), N), dtype=A.dtype)
    for r0 in range(0, len(rows), chunk):
        r1 = min(len(rows), r0 + chunk)
        if kslice is not None:
            out[r0:r1] = _matmul(X[r0:r1, kslice[0]:kslice[1]].contiguous(), Wt[kslice[0]:kslice[1]], chain)
            continue
        y = _matmul(X[r0:r1], Wt, chain)
        if bias is not None:
            y = y + bias[:N]
        if rowbias is not None:
            y = y + rowbias[rows[r0:r1] % rb_mod, :N]
        if act == 1:
            y = F.gelu(y)
        elif act == 2:
            y = F.leaky_relu(y, 0.2)
        elif act == 3:
            y = F.relu(y)
        if residual is not None:
            y = y + residual[rows[r0:r1], :N]
        out[r0:r1] = y
    return out
