"""Several characters served per call from one multi-character bank (``mocha_bank_set_segments``).

An application that drives several characters at once - several players or NPCs, each streamed to its own target character - keeps
every character's bank as one row segment of a single bank on one context.  Each window names the character it is matched against
(``characters``: one id per window); the match is the exact 1-NN within that character's rows only, and the returned index is the row
LOCAL to that character's bank, as ``BallTree(that character's cnt_nm).query(k=1)`` and ``ContextBank(that character).query`` return it.
Encoding, z-score, gather, decoder and to_mot are the batched kernels of ``ContextBank.characterize``.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence, Tuple

import numpy as np
import torch

from .generator import DIM, NTOK, Generator, _dev_f32, _ptr, _stream

_BORROW, _BF16, _NO_DEC_CACHE = 1, 2, 4          # mocha_bank_set flags (include/mocha_hip.h)
SOFT_MAX_K = 8                                   # MOCHA_SOFT_MAX_K


def soft_params(soft, who: str):
    """``soft=(k, temperature)`` checked on the host -> (int k, float temperature), or None for the hard 1-NN."""
    if soft is None:
        return None
    try:
        k, t = soft
    except (TypeError, ValueError):
        raise ValueError(f"{who}: soft must be None or a (k, temperature) pair") from None
    if int(k) != k or not 1 <= int(k) <= SOFT_MAX_K:
        raise ValueError(f"{who}: soft k must be an integer in 1 .. {SOFT_MAX_K}")
    if not float(t) > 0.0:
        raise ValueError(f"{who}: soft temperature must be positive")
    return int(k), float(t)


class MultiCharacterBank:
    """``banks``: a sequence of ``(cnt_nm, encoded)`` pairs, one per character (cnt_nm (N_c, 90*256) z-scored with the SAME global
    cnt_mean / cnt_std as every other character, encoded (N_c, 90, 256)).  They are concatenated once into device tensors this object
    owns and lends to the context.  ``bf16`` / ``dec_cache`` mean what they mean for ``ContextBank``."""

    def __init__(self, model: Generator, banks: Sequence[Tuple[torch.Tensor, torch.Tensor]], bf16: bool = False, dec_cache: bool = True):
        model._need()
        self.model = model
        if len(banks) < 1:
            raise ValueError("MultiCharacterBank: needs at least one character")
        dev = model.device
        nms, encs, sizes = [], [], []
        for c, (nm, enc) in enumerate(banks):
            nm = _dev_f32(nm, dev, None, f"banks[{c}].cnt_nm").reshape(-1, NTOK * DIM)
            enc = _dev_f32(enc, dev, (NTOK, DIM), f"banks[{c}].encoded").reshape(-1, NTOK, DIM)
            if nm.shape[0] != enc.shape[0]:
                raise ValueError(f"banks[{c}]: cnt_nm and encoded have different entry counts")
            if nm.shape[0] < 1:
                raise ValueError(f"banks[{c}]: a character needs at least one entry")
            nms.append(nm); encs.append(enc); sizes.append(int(nm.shape[0]))
        self.cnt_nm = torch.cat(nms).contiguous()
        self.encoded = torch.cat(encs).contiguous()
        self.N = int(self.cnt_nm.shape[0])
        self.S = len(sizes)
        self.seg_start = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
        self._bf16 = bool(bf16)
        self._dec_cache = bool(dec_cache)
        self.activate()

    def rows(self, c: int) -> Tuple[int, int]:
        """(start, stop) of character ``c``'s rows in the concatenated bank."""
        if not 0 <= c < self.S:
            raise IndexError(f"character {c} out of range 0 .. {self.S - 1}")
        return int(self.seg_start[c]), int(self.seg_start[c + 1])

    def activate(self):
        """Make this bank (with its segment table) the context's current bank; the no-cache intent travels as a flag of this one call."""
        flags = _BORROW | (_BF16 if self._bf16 else 0) | (0 if self._dec_cache else _NO_DEC_CACHE)
        seg = (C.c_int64 * (self.S + 1))(*self.seg_start.tolist())
        self.model._ctx.call("mocha_bank_set_segments", _ptr(self.cnt_nm), _ptr(self.encoded), self.N, seg, self.S, flags, _stream())
        self.model._bank = self
        return self

    def _ensure(self):
        if getattr(self.model, "_bank", None) is not self:
            self.activate()

    def _ids(self, characters, n: int) -> torch.Tensor:
        """Character ids as a device int32 vector of n entries.  Host data (list, numpy, CPU tensor) is checked here, before anything is
        launched; ids already on the device are the caller's to keep in range (an id outside [0, S) gives index -1, never a bad read)."""
        if isinstance(characters, torch.Tensor) and characters.device.type != "cpu":
            ids = characters.reshape(-1)
            if ids.dtype != torch.int32:
                ids = ids.to(torch.int32)
            ids = ids.to(self.model.device).contiguous()
        else:
            a = characters.numpy() if isinstance(characters, torch.Tensor) else np.asarray(characters)
            a = np.asarray(a).reshape(-1)
            if a.size and not np.issubdtype(a.dtype, np.integer):
                raise ValueError(f"characters: integer ids expected, got {a.dtype}")
            if a.size and (a.min() < 0 or a.max() >= self.S):
                raise ValueError(f"characters: ids must lie in 0 .. {self.S - 1}")
            ids = torch.from_numpy(a.astype(np.int32)).to(self.model.device)
        if ids.shape[0] != n:
            raise ValueError(f"characters: {ids.shape[0]} ids for {n} queries")
        return ids

    def query(self, query_nm, characters, k: int = 1):
        """Exact 1-NN of each query within its character's rows -> (dist (Q,1), idx (Q,1)), idx local to that character's bank.
        ``k > 1`` (up to 8): the k nearest rows of that character, nearest first, ties to the lower row -> (dist (Q,k), idx (Q,k)); a
        character with fewer than k rows gives idx -1 / dist +inf in the columns it cannot fill (``mocha_match_topk_segmented``)."""
        self._ensure()
        q = _dev_f32(query_nm, self.model.device, None, "query").reshape(-1, NTOK * DIM)
        Q = q.shape[0]
        ids = self._ids(characters, Q)
        if int(k) != k or not 1 <= int(k) <= SOFT_MAX_K:
            raise ValueError(f"query: k must be an integer in 1 .. {SOFT_MAX_K}")
        if k > 1:
            k = int(k)
            idx = torch.empty((Q, k), dtype=torch.int32, device=q.device)
            dist = torch.empty((Q, k), dtype=torch.float32, device=q.device)
            self.model._ctx.call("mocha_match_topk_segmented", _ptr(q), Q, _ptr(ids), k, _ptr(idx), _ptr(dist), _stream())
            return dist, idx
        idx = torch.empty((Q,), dtype=torch.int32, device=q.device)
        dist = torch.empty((Q,), dtype=torch.float32, device=q.device)
        self.model._ctx.call("mocha_match_segmented", _ptr(q), Q, _ptr(ids), _ptr(idx), _ptr(dist), _stream())
        return dist[:, None], idx[:, None]

    def characterize(self, src_X, characters, cnt_mean, cnt_std, return_index: bool = False, raw: bool = False, soft=None):
        """``ContextBank.characterize`` with every window matched against its own character: Y (B,T,V,C) [, idx (B,) local rows].
        ``soft=(k, temperature)``: the decoder reads the softmax(-dist / temperature)-weighted blend of the window's k nearest entries
        instead of the nearest one (``mocha_characterize_soft_segmented``); with ``return_index`` -> (Y, idx_k (B,k), weight (B,k))."""
        self._ensure()
        m = self.model
        X = m._xraw(src_X, "src_X_raw") if raw else m._x(src_X, "src_X")
        B = X.shape[0]
        ids = self._ids(characters, B)
        mean = _dev_f32(cnt_mean, m.device, (NTOK, DIM), "cnt_mean")
        std = _dev_f32(cnt_std, m.device, (NTOK, DIM), "cnt_std")
        Y = torch.empty((B, m.cfg["nframes"], m.V, m.cfg["mot_in_dim"]), dtype=torch.float32, device=m.device)
        sp = soft_params(soft, "characterize")
        if sp is not None:
            k, t = sp
            idx_k = torch.empty((B, k), dtype=torch.int32, device=m.device)
            w_k = torch.empty((B, k), dtype=torch.float32, device=m.device)
            m._ctx.call("mocha_characterize_soft_segmented", _ptr(X), B, _ptr(ids), k, t, _ptr(mean), _ptr(std), _ptr(Y), _ptr(idx_k), _ptr(w_k),
                        1 if raw else 0, _stream())
            return (Y, idx_k, w_k) if return_index else Y
        idx = torch.empty((B,), dtype=torch.int32, device=m.device)
        m._ctx.call("mocha_characterize_segmented", _ptr(X), B, _ptr(ids), _ptr(mean), _ptr(std), _ptr(Y), _ptr(idx), 1 if raw else 0, _stream())
        return (Y, idx) if return_index else Y


class MultiStreamCharacterizer:
    """One window of each of ``streams`` streams per step, every stream matched against its own character: the segmented characterize of
    the ``streams`` windows captured once into a HIP graph (``mocha_step_graph_segmented``) and replayed.  The character of each stream
    may change from step to step: the ids live in a device buffer the graph reads, so a change does not re-capture.
    ``soft=(k, temperature)``: the soft characterize (``mocha_step_graph_soft_segmented``); ``step`` then returns
    (Y, idx_k (streams,k), weight (streams,k))."""

    def __init__(self, bank: MultiCharacterBank, cnt_mean, cnt_std, streams: int, raw: bool = False, soft=None):
        if not 1 <= streams <= 16:
            raise ValueError("streams must be 1..16")
        self.bank, self.model = bank, bank.model
        m = self.model
        self.streams = int(streams)
        self.raw = bool(raw)
        self.mean = _dev_f32(cnt_mean, m.device, (NTOK, DIM), "cnt_mean")
        self.std = _dev_f32(cnt_std, m.device, (NTOK, DIM), "cnt_std")
        shape = (self.streams, m.cfg["nframes"], m.V, m.cfg["mot_in_dim"])
        in_shape = (self.streams, m.cfg["nframes"], m.V + 1, m.cfg["mot_in_dim"]) if self.raw else shape
        self.x = torch.zeros(in_shape, dtype=torch.float32, device=m.device)
        self.y = torch.empty(shape, dtype=torch.float32, device=m.device)
        self.idx = torch.zeros((self.streams,), dtype=torch.int32, device=m.device)
        self.ids = torch.zeros((self.streams,), dtype=torch.int32, device=m.device)
        self.soft = soft_params(soft, "MultiStreamCharacterizer")
        if self.soft is not None:
            self.idx_k = torch.full((self.streams, self.soft[0]), -1, dtype=torch.int32, device=m.device)
            self.weight = torch.zeros((self.streams, self.soft[0]), dtype=torch.float32, device=m.device)
        bank._ensure()

    @property
    def input(self) -> torch.Tensor:
        """The captured step's own input windows (streams, 60, V, 15): a producer may write them in place and call ``step()``."""
        return self.x

    @property
    def characters(self) -> torch.Tensor:
        """The captured step's own character ids (streams,) int32 on the device: a producer may write them in place and call ``step()``."""
        return self.ids

    def step(self, windows: Optional[torch.Tensor] = None, characters=None):
        """windows (streams, 60, V, 15) [, characters: one id per stream] -> (Y (streams, 60, V, 15) view, idx (streams,) view); both are
        overwritten by the next step.  Without arguments the windows and ids already in ``input`` / ``characters`` are used."""
        if characters is not None:
            self.ids.copy_(self.bank._ids(characters, self.streams), non_blocking=True)
        if windows is not None:
            self.x.copy_(windows.reshape(self.x.shape), non_blocking=True)
        self.bank._ensure()
        if self.soft is not None:
            self.model._ctx.call("mocha_step_graph_soft_segmented", _ptr(self.x), self.streams, _ptr(self.ids), self.soft[0], self.soft[1],
                                 _ptr(self.mean), _ptr(self.std), _ptr(self.y), _ptr(self.idx_k), _ptr(self.weight), 1 if self.raw else 0,
                                 _stream())
            return self.y, self.idx_k, self.weight
        self.model._ctx.call("mocha_step_graph_segmented", _ptr(self.x), self.streams, _ptr(self.ids), _ptr(self.mean), _ptr(self.std),
                             _ptr(self.y), _ptr(self.idx), 1 if self.raw else 0, _stream())
        return self.y, self.idx
