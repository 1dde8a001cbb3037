"""Several characters served per call from one multi-character bank (``mocha_bank_set_segments``).

An application that drives several characters at once - several players or NPCs, each streamed to its own target character - keeps
every character's bank as one row segment of a single bank on one context.  Each window names the character it is matched against
(``characters``: one id per window); the match is the exact 1-NN within that character's rows only, and the returned index is the row
LOCAL to that character's bank, as ``BallTree(that character's cnt_nm).query(k=1)`` and ``ContextBank(that character).query`` return it.
Encoding, z-score, gather, decoder and to_mot are the batched kernels of ``ContextBank.characterize``.

Action-constrained matching: a bank built with ``labels`` (one action label 0 .. 63 per entry, e.g. ``load_bank(path)["action_label"]``)
accepts ``allow=`` in ``query`` / ``characterize`` / ``step``: per query a 64-bit mask of admissible actions (``action_mask``).  The match is
then the exact nearest entry among that character's entries of those actions; a zero mask asks for nothing, and a mask naming no action
the character has falls back to the whole character (``applied``: 1 / 0 / -1).

Character mixing: ``mix=(ids, weights)`` in ``query`` / ``characterize`` (and ``MultiStreamCharacterizer(mix=J)``, ``LiveSession(mix=J)``)
characterizes a window by up to 4 components - a character id and six body-part weights each (``skeleton.PART_NAMES``) - instead of one
character: every present component is matched exactly in its own character and the decoder reads the part-wise weighted blend of the
matched entries (``mix_tensors``).  It does not combine with ``soft`` or ``allow``.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence, Tuple

import numpy as np
import torch

from .generator import DIM, MAX_PATH_ROWS, NTOK, CoherentMatch, Generator, _dev_f32, _dist_matrix, _match_path, _ptr, _relative_jump, _stream

_BORROW, _BF16, _NO_DEC_CACHE = 1, 2, 4          # mocha_bank_set flags (include/mocha_hip.h)
SOFT_MAX_K = 8                                   # MOCHA_SOFT_MAX_K
MIX_MAX, MIX_PARTS = 4, 6                        # MOCHA_MIX_MAX, MOCHA_MIX_PARTS


def action_mask(actions) -> int:
    """The 64-bit allow mask of a set of action labels: bit ``a`` set for every label ``a`` in ``actions`` (an iterable of integers, or one
    integer).  ``ValueError`` for a label outside 0 .. 63.  An empty set gives 0: nothing asked."""
    if isinstance(actions, (int, np.integer)):
        actions = [actions]
    m = 0
    for a in actions:
        if isinstance(a, (bool, np.bool_)) or not isinstance(a, (int, np.integer)):
            raise ValueError(f"action_mask: integer labels expected, got {a!r}")
        if not 0 <= int(a) <= 63:
            raise ValueError(f"action_mask: label {int(a)} is outside 0 .. 63")
        m |= 1 << int(a)
    return m


def _mask_of(entry, who: str) -> int:
    """One query's ``allow`` entry -> its mask: None (0), an int bit pattern 0 .. 2**64 - 1, or an iterable of labels."""
    if entry is None:
        return 0
    if isinstance(entry, (int, np.integer)) and not isinstance(entry, (bool, np.bool_)):
        if not 0 <= int(entry) < 1 << 64:
            raise ValueError(f"{who}: an allow mask must lie in 0 .. 2**64 - 1")
        return int(entry)
    return action_mask(entry)


def allow_masks(allow, n: int, device, who: str) -> torch.Tensor:
    """``allow`` -> the (n,) int64 device tensor of bit patterns the constrained calls read.  A device int64 tensor is taken as it is (the
    caller's to keep meaningful); an int is one mask for all n queries; any other sequence holds one entry per query, each an int mask,
    an iterable of labels, or None.  Host data is checked here, before anything is launched."""
    if isinstance(allow, torch.Tensor) and allow.device.type != "cpu":
        if allow.dtype != torch.int64:
            raise ValueError(f"{who}: a device allow tensor must be int64 (the masks' bit patterns)")
        t = allow.reshape(-1).to(device).contiguous()
        if t.shape[0] != n:
            raise ValueError(f"{who}: {t.shape[0]} allow masks for {n} queries")
        return t
    if isinstance(allow, torch.Tensor):
        allow = allow.tolist()
    if isinstance(allow, (int, np.integer)) and not isinstance(allow, (bool, np.bool_)):
        masks = [_mask_of(allow, who)] * n
    else:
        entries = list(allow)
        if len(entries) != n:
            raise ValueError(f"{who}: {len(entries)} allow entries for {n} queries")
        masks = [_mask_of(e, who) for e in entries]
    signed = [m - (1 << 64) if m >= 1 << 63 else m for m in masks]          # the bit pattern as int64
    return torch.tensor(signed, dtype=torch.int64).to(device)


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


def mix_count(J, who: str) -> int:
    """``mix=J`` of a streamer or a session checked on the host -> int J in 1 .. MIX_MAX."""
    if isinstance(J, (bool, np.bool_)) or not isinstance(J, (int, np.integer)) or not 1 <= int(J) <= MIX_MAX:
        raise ValueError(f"{who}: mix must be an integer in 1 .. {MIX_MAX} (components per window)")
    return int(J)


def mix_tensors(mix, n: int, device, who: str, J: Optional[int] = None):
    """``mix=(ids, weights)`` -> (ids (n,J) int32, weights (n,J,6) float32) on the device, as the mix calls read them.  ids: (n,J), or
    (J,) for every window; weights: (n,J,6), (n,J) (one weight per component, broadcast over the six body parts), or (J,6) / (J,) for
    every window.  1 <= J <= 4 (``J``: the count a streamer or session was built for).  The VALUES are the device's to judge: an id that
    names no loaded character and a weight that is not in (0, FLT_MAX] simply do not take part."""
    try:
        ids, w = mix
    except (TypeError, ValueError):
        raise ValueError(f"{who}: mix must be an (ids, weights) pair") from None
    if not isinstance(ids, torch.Tensor):
        a = np.asarray(ids)
        if a.size and not np.issubdtype(a.dtype, np.integer):
            raise ValueError(f"{who}: mix ids must be integers, got {a.dtype}")
        ids = torch.from_numpy(np.ascontiguousarray(a.astype(np.int32)))
    elif ids.dtype.is_floating_point or ids.dtype == torch.bool:
        raise ValueError(f"{who}: mix ids must be integers, got {ids.dtype}")
    if ids.dim() == 1:
        ids = ids[None].expand(n, -1)
    if ids.dim() != 2 or ids.shape[0] != n:
        raise ValueError(f"{who}: mix ids must have shape ({n}, J) or (J,), got {tuple(ids.shape)}")
    Jn = int(ids.shape[1])
    if not 1 <= Jn <= MIX_MAX:
        raise ValueError(f"{who}: {Jn} mix components; 1 .. {MIX_MAX} are served")
    if J is not None and Jn != J:
        raise ValueError(f"{who}: {Jn} mix components where mix={J} was asked")
    if not isinstance(w, torch.Tensor):
        w = torch.from_numpy(np.ascontiguousarray(np.asarray(w, dtype=np.float32)))
    shape = tuple(w.shape)
    if shape == (n, Jn, MIX_PARTS):
        pass
    elif shape == (n, Jn):
        w = w[:, :, None].expand(n, Jn, MIX_PARTS)
    elif shape == (Jn, MIX_PARTS):
        w = w[None].expand(n, Jn, MIX_PARTS)
    elif shape == (Jn,):
        w = w[None, :, None].expand(n, Jn, MIX_PARTS)
    else:
        raise ValueError(f"{who}: mix weights must have shape ({n}, {Jn}, 6), ({n}, {Jn}), ({Jn}, 6) or ({Jn},), got {shape}")
    return ids.to(device=device, dtype=torch.int32).contiguous(), w.to(device=device, dtype=torch.float32).contiguous()


def _refuse_with_mix(who: str, **others):
    for name, v in others.items():
        if v:
            raise ValueError(f"{who}: mix= does not combine with {name} (mix is hard matching per component)")


def _host_starts(starts, n: int, who: str) -> np.ndarray:
    """A character's clip starts (local rows) checked on the host -> sorted unique int32 array inside [0, n)."""
    a = np.asarray([] if starts is None else (starts.tolist() if hasattr(starts, "tolist") else list(starts)), dtype=np.int64).reshape(-1)
    if a.size and (np.any(np.diff(a) <= 0) or a[0] < 0 or a[-1] >= n):
        raise ValueError(f"{who}: starts must increase strictly and lie in 0 .. {n - 1}")
    return np.ascontiguousarray(a.astype(np.int32))


class OnlinePath:
    """Coherent matching one window at a time (include/mocha_hip.h, "coherent matching in live sessions"): per stream, the forward
    recursion of ``query_path`` advanced by one window per ``step``, its row kept on the device.  The row it returns at window t is the
    last row of the whole-clip path over windows 0 .. t of the same run - the filtered row, no lookahead.  ``bank``: a
    ``MultiCharacterBank`` or ``ResidentCharacterBank``; ``streams``: 1 .. 16; ``jump``: the penalty, a number or a ``CoherentMatch``
    without ``relative`` (a live stream has no clip to take a median from: run ``query_path(..., relative=True)`` on a recorded clip for a
    unit).  The clip starts are the bank's (``MultiCharacterBank(starts=)``, ``set_starts``, ``ResidentCharacterBank.add(starts=)``).
    A stream restarts when its character changes, when that character is replaced, after ``reset`` and where ``restart`` - a (streams,)
    int32 device tensor a producer may write in place - is non-zero (the step clears it); a stream whose id names no loaded character
    sits the step out (idx -1, dist +inf)."""

    def __init__(self, bank, streams: int, jump, state_rows: Optional[int] = None):
        if not 1 <= int(streams) <= 16:
            raise ValueError("OnlinePath: streams must be 1..16")
        co = CoherentMatch.of(jump)
        if co.relative:
            raise ValueError("OnlinePath: a relative jump needs a clip to take the median from; use query_path(..., relative=True) on a "
                             "recorded clip for the unit and pass the absolute penalty")
        self.bank, self.model = bank, bank.model
        self.streams, self.jump = int(streams), co.jump
        self.state_rows = int(state_rows if state_rows is not None else bank.max_rows)
        ctx, dev = self.model._ctx, self.model.device
        nbytes = int(ctx.lib.mocha_path_state_bytes(ctx.h, self.streams, self.state_rows))
        if nbytes <= 0:
            raise ValueError(f"OnlinePath: a state of {self.state_rows} rows is not served (1 .. {MAX_PATH_ROWS})")
        self.state = torch.zeros((nbytes,), dtype=torch.uint8, device=dev)
        self.restart = torch.zeros((self.streams,), dtype=torch.int32, device=dev)
        self.idx = torch.full((self.streams,), -1, dtype=torch.int32, device=dev)
        self.dist = torch.full((self.streams,), float("inf"), dtype=torch.float32, device=dev)
        self.continued = torch.zeros((self.streams,), dtype=torch.uint8, device=dev)

    def reset(self, which=None):
        """The named streams (None: all) stop running: their next step restarts.  Enqueued on the current stream."""
        if which is None:
            self.model._ctx.call("mocha_path_state_reset", _ptr(self.state), self.streams, self.state_rows, None, 0, _stream())
        else:
            ids = [int(s) for s in which]
            arr = (C.c_int32 * max(len(ids), 1))(*ids)
            self.model._ctx.call("mocha_path_state_reset", _ptr(self.state), self.streams, self.state_rows, arr, len(ids), _stream())
        return self

    def step(self, query_nm, characters, return_distances: bool = False):
        """One window per stream: query_nm (streams, 90*256) z-scored, characters one id per stream -> (dist (streams,), idx (streams,)
        int32 local rows, continued (streams,) uint8), views the next step overwrites.  ``return_distances`` adds the (streams,
        state_rows) matrix of every row's distance (columns past a character's rows are not written)."""
        self.bank._ensure()
        q = _dev_f32(query_nm, self.model.device, None, "query").reshape(-1, NTOK * DIM)
        if q.shape[0] != self.streams:
            raise ValueError(f"OnlinePath.step: {q.shape[0]} queries for {self.streams} streams")
        ids = self.bank._ids(characters, self.streams)
        rows = torch.full((self.streams, self.state_rows), float("nan"), dtype=torch.float32, device=q.device) if return_distances else None
        self.model._ctx.call("mocha_match_path_segmented", _ptr(self.state), self.streams, self.state_rows, _ptr(q), _ptr(ids), _ptr(self.restart),
                             C.c_double(self.jump), _ptr(self.idx), _ptr(self.dist), _ptr(self.continued), _ptr(rows), C.c_int64(self.state_rows),
                             _stream())
        return (self.dist, self.idx, self.continued, rows) if return_distances else (self.dist, self.idx, self.continued)

    def advance(self, dist_rows, ids, rows, start_bits=None, bit_off=None):
        """The pure form (``mocha_match_path_advance``), no bank read: dist_rows (streams, ld) fp32 on the device, ids (streams,) int32
        (negative: sits out; a change restarts), rows (streams,) int32, ``start_bits`` an int32 device tensor of packed bits (bit
        ``bit_off[s] + j``: row j of stream s starts a clip) -> (dist, idx, continued) as ``step``."""
        dev = self.model.device
        d = _dev_f32(dist_rows, dev, None, "dist_rows")
        if d.dim() != 2 or d.shape[0] != self.streams:
            raise ValueError(f"OnlinePath.advance: dist_rows must be ({self.streams}, ld)")
        ids = torch.as_tensor(ids, dtype=torch.int32).to(dev).contiguous()
        rows = torch.as_tensor(rows, dtype=torch.int32).to(dev).contiguous()
        if ids.shape != (self.streams,) or rows.shape != (self.streams,):
            raise ValueError(f"OnlinePath.advance: ids and rows must have {self.streams} entries")
        bits = off = None
        n_bits = 0
        if start_bits is not None:
            bits = start_bits.to(dev).contiguous()
            if bits.dtype != torch.int32:
                raise ValueError("OnlinePath.advance: start_bits must be an int32 tensor of packed bits")
            n_bits = 32 * bits.numel()
            if bit_off is not None:
                off = torch.as_tensor(bit_off, dtype=torch.int32).to(dev).contiguous()
        elif bit_off is not None:
            raise ValueError("OnlinePath.advance: bit_off needs start_bits")
        self.model._ctx.call("mocha_match_path_advance", _ptr(self.state), self.streams, self.state_rows, _ptr(d), C.c_int64(d.stride(0)), _ptr(ids),
                             _ptr(rows), _ptr(bits), C.c_int64(n_bits), _ptr(off), _ptr(self.restart), C.c_double(self.jump), _ptr(self.idx),
                             _ptr(self.dist), _ptr(self.continued), _stream())
        return self.dist, self.idx, self.continued


class _SegmentedBank:
    """What ``MultiCharacterBank`` and ``ResidentCharacterBank`` share: the segmented calls on the model's current bank.  A subclass
    provides ``model``, ``S`` (ids are 0 .. S - 1), ``labels`` (None: no action labels) and ``_ensure()``."""

    def _allow(self, allow, n: int, who: str) -> torch.Tensor:
        if self.labels is None:
            raise RuntimeError(f"{who}: allow= needs a bank with action labels (MultiCharacterBank(labels=) or set_labels)")
        return allow_masks(allow, n, self.model.device, who)

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

    def query(self, query_nm, characters=None, k: int = 1, allow=None, return_applied: bool = False, mix=None):
        """Exact 1-NN of each query within its character's rows -> (dist (Q,1), idx (Q,1)), idx local to that character's bank.
        ``k > 1`` (up to 8): the k nearest rows of that character, nearest first, ties to the lower row -> (dist (Q,k), idx (Q,k)); a
        character with fewer than k rows gives idx -1 / dist +inf in the columns it cannot fill (``mocha_match_topk_segmented``).
        ``allow`` (see ``allow_masks``): the match among the rows of each query's admissible actions (``mocha_match_segmented_allow``);
        fewer than k such rows leave -1 / +inf; ``return_applied`` adds applied (Q,) int32: 1 constrained, 0 nothing asked, -1 fell back.
        ``mix=(ids, weights)`` (see ``mix_tensors``; no ``characters``): every query matched in each of its J components' characters
        (``mocha_match_mix_segmented``) -> (dist (Q,J), idx (Q,J), weight (Q,J,6) normalised per body part, out (Q,90,256) the part-wise
        blend of the matched entries' encoded features); a component that is not present has -1 / +inf / 0."""
        self._ensure()
        q = _dev_f32(query_nm, self.model.device, None, "query").reshape(-1, NTOK * DIM)
        Q = q.shape[0]
        if mix is not None:
            _refuse_with_mix("query", characters=characters is not None, **{"k > 1": k != 1}, allow=allow is not None, return_applied=return_applied)
            mids, mw = mix_tensors(mix, Q, q.device, "query")
            J = mids.shape[1]
            idx = torch.empty((Q, J), dtype=torch.int32, device=q.device)
            dist = torch.empty((Q, J), dtype=torch.float32, device=q.device)
            wn = torch.empty((Q, J, MIX_PARTS), dtype=torch.float32, device=q.device)
            out = torch.empty((Q, NTOK, DIM), dtype=torch.float32, device=q.device)
            self.model._ctx.call("mocha_match_mix_segmented", _ptr(q), Q, _ptr(mids), _ptr(mw), J, _ptr(idx), _ptr(dist), _ptr(wn), _ptr(out),
                                 _stream())
            return dist, idx, wn, out
        if characters is None:
            raise ValueError("query: characters (one id per query) or mix= is needed")
        ids = self._ids(characters, Q)
        if int(k) != k or not 1 <= int(k) <= SOFT_MAX_K:
            raise ValueError(f"query: k must be an integer in 1 .. {SOFT_MAX_K}")
        if allow is not None:
            k = int(k)
            masks = self._allow(allow, Q, "query")
            idx = torch.empty((Q, k), dtype=torch.int32, device=q.device)
            dist = torch.empty((Q, k), dtype=torch.float32, device=q.device)
            applied = torch.empty((Q,), dtype=torch.int32, device=q.device)
            self.model._ctx.call("mocha_match_segmented_allow", _ptr(q), Q, _ptr(ids), _ptr(masks), k, _ptr(idx), _ptr(dist), _ptr(applied),
                                 _stream())
            return (dist, idx, applied) if return_applied else (dist, idx)
        if return_applied:
            raise ValueError("query: return_applied needs allow=")
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

    def distances(self, query_nm, character: int):
        """(Q, rows of ``character``) fp32 distances (``ContextBank.distances``) against that character's rows alone."""
        self._ensure()
        r0, r1 = self.rows(int(character))
        if r1 <= r0:
            raise ValueError(f"character {character} holds no rows")
        return _dist_matrix(self.model, query_nm, r0, r1 - r0)

    def query_path(self, query_nm, character: int, jump: float, starts=None, bank_starts=None, relative: bool = False):
        """``ContextBank.query_path`` over the rows of ONE character (a loaded character of a ``MultiCharacterBank``, an occupied slot of a
        ``ResidentCharacterBank``; the rows come from the host's table) -> (dist (Q,), idx (Q,) int32 GLOBAL rows, continued (Q,) uint8).
        ``bank_starts`` are local to the character's rows.  It does not combine with ``k``, ``allow`` or ``mix``."""
        d = self.distances(query_nm, character)
        lam = _relative_jump(d, CoherentMatch(jump).jump) if relative and d.shape[0] else CoherentMatch(jump).jump
        dist, idx, cont = _match_path(self.model._ctx, d, lam, starts, bank_starts)
        return dist, idx + self.rows(int(character))[0], cont

    def characterize(self, src_X, characters, cnt_mean, cnt_std, return_index: bool = False, raw: bool = False, soft=None, allow=None,
                     mix=None, coherent=None):
        """``allow`` (see ``allow_masks``): every window matched among its character's entries of the admissible actions
        (``mocha_characterize_segmented_allow``); with ``return_index`` the outputs gain applied (B,) int32 at the end.
        ``ContextBank.characterize`` with every window matched against its own character: Y (B,T,V,C) [, idx (B,) local rows].
        ``soft=(k, temperature)``: the decoder reads the softmax(-dist / temperature)-weighted blend of the window's k nearest entries
        instead of the nearest one (``mocha_characterize_soft_segmented``); with ``return_index`` -> (Y, idx_k (B,k), weight (B,k)).
        ``mix=(ids, weights)`` (see ``mix_tensors``; ``characters`` is then None): the decoder reads the part-wise weighted blend of the
        entries matched in each component's character (``mocha_characterize_mix_segmented``); with ``return_index`` -> (Y, idx (B,J),
        weight (B,J,6)).  It does not combine with ``soft`` or ``allow``.
        ``coherent=OnlinePath``: window s is the next window of stream s of that path (B = its streams) and is matched by one step of it
        (``mocha_characterize_segmented_path``); with ``return_index`` -> (Y, idx (B,), dist (B,), continued (B,) uint8), views the path's
        next step overwrites.  It does not combine with ``soft``, ``allow`` or ``mix``."""
        self._ensure()
        m = self.model
        X = m._xraw(src_X, "src_X_raw") if raw else m._x(src_X, "src_X")
        B = X.shape[0]
        if coherent is not None:
            if not isinstance(coherent, OnlinePath) or coherent.bank is not self:
                raise ValueError("characterize: coherent= takes an OnlinePath of this bank (a clip goes through ContextBank.characterize or query_path)")
            if soft is not None or allow is not None or mix is not None:
                raise ValueError("characterize: coherent= does not combine with soft, allow or mix")
            if B != coherent.streams:
                raise ValueError(f"characterize: {B} windows for an OnlinePath of {coherent.streams} streams")
            ids = self._ids(characters, B)
            mean = _dev_f32(cnt_mean, m.device, (NTOK, DIM), "cnt_mean")
            std = _dev_f32(cnt_std, m.device, (NTOK, DIM), "cnt_std")
            Y = torch.empty((B, m.cfg["nframes"], m.V, m.cfg["mot_in_dim"]), dtype=torch.float32, device=m.device)
            p = coherent
            m._ctx.call("mocha_characterize_segmented_path", _ptr(X), B, _ptr(ids), _ptr(mean), _ptr(std), _ptr(p.state), p.state_rows,
                        C.c_double(p.jump), _ptr(p.restart), _ptr(Y), _ptr(p.idx), _ptr(p.dist), _ptr(p.continued), 1 if raw else 0, _stream())
            return (Y, p.idx, p.dist, p.continued) if return_index else Y
        if mix is not None:
            _refuse_with_mix("characterize", characters=characters is not None, soft=soft is not None, allow=allow is not None)
            mids, mw = mix_tensors(mix, B, m.device, "characterize")
            J = mids.shape[1]
            mean = _dev_f32(cnt_mean, m.device, (NTOK, DIM), "cnt_mean")
            std = _dev_f32(cnt_std, m.device, (NTOK, DIM), "cnt_std")
            Y = torch.empty((B, m.cfg["nframes"], m.V, m.cfg["mot_in_dim"]), dtype=torch.float32, device=m.device)
            idx = torch.empty((B, J), dtype=torch.int32, device=m.device)
            wn = torch.empty((B, J, MIX_PARTS), dtype=torch.float32, device=m.device)
            m._ctx.call("mocha_characterize_mix_segmented", _ptr(X), B, _ptr(mids), _ptr(mw), J, _ptr(mean), _ptr(std), _ptr(Y), _ptr(idx),
                        _ptr(wn), 1 if raw else 0, _stream())
            return (Y, idx, wn) if return_index else Y
        ids = self._ids(characters, B)
        mean = _dev_f32(cnt_mean, m.device, (NTOK, DIM), "cnt_mean")
        std = _dev_f32(cnt_std, m.device, (NTOK, DIM), "cnt_std")
        Y = torch.empty((B, m.cfg["nframes"], m.V, m.cfg["mot_in_dim"]), dtype=torch.float32, device=m.device)
        sp = soft_params(soft, "characterize")
        if allow is not None:
            masks = self._allow(allow, B, "characterize")
            k, t = sp if sp is not None else (0, 0.0)
            idx_k = torch.empty((B, k) if k else (B,), dtype=torch.int32, device=m.device)
            w_k = torch.empty((B, k), dtype=torch.float32, device=m.device) if k else None
            applied = torch.empty((B,), dtype=torch.int32, device=m.device)
            m._ctx.call("mocha_characterize_segmented_allow", _ptr(X), B, _ptr(ids), _ptr(masks), k, t, _ptr(mean), _ptr(std), _ptr(Y),
                        _ptr(idx_k), _ptr(w_k) if k else None, _ptr(applied), 1 if raw else 0, _stream())
            if not return_index:
                return Y
            return (Y, idx_k, w_k, applied) if k else (Y, idx_k, applied)
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


class MultiCharacterBank(_SegmentedBank):
    """``banks``: a sequence of ``(cnt_nm, encoded)`` pairs, one per character (cnt_nm (N_c, 90*256) z-scored with the SAME global
    cnt_mean / cnt_std as every other character, encoded (N_c, 90, 256)).  They are concatenated once into device tensors this object
    owns and lends to the context.  ``bf16`` / ``dec_cache`` mean what they mean for ``ContextBank``.  ``labels``: one integer array
    (N_c,) of action labels 0 .. 63 per character (``set_labels``).  ``starts``: per character the local rows that begin a clip
    (``bank_starts(load_bank(path))``; None: the character is one clip), read by ``OnlinePath`` and ``LiveSession(coherent=)``
    (``set_starts``)."""

    def __init__(self, model: Generator, banks: Sequence[Tuple[torch.Tensor, torch.Tensor]], bf16: bool = False, dec_cache: bool = True,
                 labels=None, starts=None):
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
        self.labels = None if labels is None else self._check_labels(labels)
        if starts is not None and len(starts) != self.S:
            raise ValueError(f"starts: {len(starts)} lists for {self.S} characters")
        self.starts = [_host_starts(None if starts is None else starts[c], sizes[c], f"starts[{c}]") for c in range(self.S)]
        self.activate()

    @property
    def max_rows(self) -> int:
        """Rows of the largest character: the rows an ``OnlinePath`` state must hold."""
        return int(np.diff(self.seg_start).max())

    def _send_starts(self):
        g = np.concatenate([self.starts[c].astype(np.int64) + self.seg_start[c] for c in range(self.S)])
        if g.size == 0 and not getattr(self, "_starts_sent", False):
            return                                         # the table is zero from mocha_bank_set_segments on
        arr = (C.c_int64 * max(g.size, 1))(*g.tolist())
        self.model._ctx.call("mocha_bank_set_starts", arr, int(g.size), _stream())
        self._starts_sent = True

    def set_starts(self, character: int, starts):
        """The local rows of ``character`` that begin a clip (None: none but its first row).  Enqueued on the current stream; a captured
        step keeps replaying."""
        r0, r1 = self.rows(int(character))
        self.starts[int(character)] = _host_starts(starts, r1 - r0, "set_starts")
        self._ensure()
        self._starts_sent = True
        self._send_starts()
        return self

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
        self._send_labels()
        self._starts_sent = False                          # (mocha_bank_set_segments zeroed the table)
        self._send_starts()
        return self

    def _check_labels(self, labels) -> np.ndarray:
        if len(labels) != self.S:
            raise ValueError(f"labels: {len(labels)} arrays for {self.S} characters")
        out = []
        for c, lab in enumerate(labels):
            a = lab.cpu().numpy() if isinstance(lab, torch.Tensor) else np.asarray(lab)
            a = a.reshape(-1)
            n = int(self.seg_start[c + 1] - self.seg_start[c])
            if a.shape[0] != n:
                raise ValueError(f"labels[{c}]: {a.shape[0]} labels for {n} entries")
            if not np.issubdtype(a.dtype, np.integer):
                raise ValueError(f"labels[{c}]: integer labels expected, got {a.dtype}")
            if a.min() < 0 or a.max() > 63:
                raise ValueError(f"labels[{c}]: labels must lie in 0 .. 63")
            out.append(a.astype(np.int32))
        return np.ascontiguousarray(np.concatenate(out))

    def _send_labels(self):
        if self.labels is None:
            return
        self.model._ctx.call("mocha_bank_set_labels", self.labels.ctypes.data_as(C.POINTER(C.c_int32)), _stream())

    def set_labels(self, labels):
        """Action labels of every character's entries (one integer array (N_c,) per character, 0 .. 63), or None to remove them.
        ``allow=`` needs them."""
        self._ensure()
        if labels is None:
            self.labels = None
            self.model._ctx.call("mocha_bank_set_labels", None, _stream())
            return self
        self.labels = self._check_labels(labels)
        self._send_labels()
        return self

    def _ensure(self):
        if getattr(self.model, "_bank", None) is not self:
            self.activate()


class ResidentCharacterBank(_SegmentedBank):
    """A multi-character bank whose characters are added and retired IN PLACE (``mocha_bank_resident_create``): storage for
    ``capacity_rows`` rows (rounded up to 16), ``max_characters`` slots and up to ``max_rows_per_character`` rows per character are
    reserved once, on the model's context; ``add`` / ``retire`` / ``replace`` then only enqueue work on the current stream - the
    character's own bytes and its own decoder constants - and the captured steps of ``MultiStreamCharacterizer``, ``LiveSession`` and
    ``LiveOursSession`` keep replaying: the model's generation does not move.  fp32 only.  A character's id is its slot, 0 ..
    ``max_characters - 1``, whether or not the slot holds a character: a query that names an empty slot gets idx -1 / dist +inf, a
    live stream that names one sits the step out as a warming stream does (``valid == 0``).  Every character is labelled (``add``
    without labels gives every entry action 0), so ``allow=`` always applies.  A resident bank cannot be rebuilt from the host: once
    another bank has been activated on the model, this object's calls raise."""

    def __init__(self, model: Generator, capacity_rows: int, max_characters: int, max_rows_per_character: int, dec_cache: bool = True):
        model._need()
        self.model = model
        self.S = int(max_characters)
        self.max_rows_per_character = int(max_rows_per_character)
        model._ctx.call("mocha_bank_resident_create", int(capacity_rows), self.S, self.max_rows_per_character, 0 if dec_cache else _NO_DEC_CACHE,
                        _stream())
        model._bank = self
        self.labels = [None] * self.S                  # per slot: the character's labels as given (None: empty, or added without)

    @property
    def max_rows(self) -> int:
        """The reserved maximum of rows per character: the rows an ``OnlinePath`` state must hold."""
        return self.max_rows_per_character

    def _ensure(self):
        if getattr(self.model, "_bank", None) is not self:
            raise RuntimeError("ResidentCharacterBank: another bank has been activated on this model; a resident bank cannot be rebuilt "
                               "from the host - create a new one and add its characters again")

    def _info(self, slot: int):
        self._ensure()
        out = [C.c_int64(0) for _ in range(4)]
        ctx = self.model._ctx
        rc = ctx.lib.mocha_bank_resident_info(ctx.h, int(slot), *[C.byref(v) for v in out])
        if rc == -1:                                   # MOCHA_ERR_ARG: the only argument that can be wrong is the slot
            raise IndexError(f"ResidentCharacterBank: slot {slot} out of range 0 .. {self.S - 1}")
        if rc != 0:                                    # MOCHA_ERR_STATE: the context's current bank is no longer this one
            raise RuntimeError(f"mocha_bank_resident_info failed (status {rc}): the context's current bank is not a resident bank "
                               "(it was replaced through the C ABI)")
        return [int(v.value) for v in out]

    def rows(self, slot: int) -> Tuple[int, int]:
        """(start, stop) of the rows the character in ``slot`` occupies in the bank; start == stop for an empty slot."""
        if not 0 <= int(slot) < self.S:
            raise IndexError(f"slot {slot} out of range 0 .. {self.S - 1}")
        first, n, _, _ = self._info(slot)
        return first, first + n

    @property
    def free_rows(self) -> int:
        """Rows not occupied by any character (whole 16-row granules)."""
        return self._info(-1)[2]

    @property
    def largest_free(self) -> int:
        """Rows of the largest free extent: the largest character ``add`` can still take (extents never move)."""
        return self._info(-1)[3]

    def add(self, cnt_nm, encoded, labels=None, slot: Optional[int] = None, starts=None) -> int:
        """One more character: cnt_nm (n, 90*256) z-scored as every other character's, encoded (n, 90, 256), ``labels`` (n,) integer
        action labels 0 .. 63 (host data is range-checked here; a device int32 tensor is taken as it is and read as label & 63) or None:
        action 0 for every entry.  ``slot``: the slot to fill, or None for the lowest empty one.  Returns the slot - the character's id.
        ``starts``: the local rows that begin a clip (None: the character is one clip), read by ``OnlinePath`` / ``LiveSession(coherent=)``.
        Enqueued on the current stream, no synchronisation; ``RuntimeError`` when the slot is occupied, no slot is empty or no free
        extent holds n rows (the message names the largest one)."""
        self._ensure()
        dev = self.model.device
        nm = _dev_f32(cnt_nm, dev, None, "cnt_nm").reshape(-1, NTOK * DIM)
        enc = _dev_f32(encoded, dev, (NTOK, DIM), "encoded").reshape(-1, NTOK, DIM)
        n = int(nm.shape[0])
        if enc.shape[0] != n:
            raise ValueError("add: cnt_nm and encoded have different entry counts")
        st = _host_starts(starts, n, "add")
        if slot is not None and not 0 <= int(slot) < self.S:
            raise IndexError(f"add: slot {slot} out of range 0 .. {self.S - 1}")
        lab = kept = None
        if labels is not None:
            if isinstance(labels, torch.Tensor) and labels.device.type != "cpu":
                if labels.dtype != torch.int32:
                    raise ValueError("add: device labels must be int32")
                lab = labels.reshape(-1).to(dev).contiguous()
                kept = lab
            else:
                a = (labels.numpy() if isinstance(labels, torch.Tensor) else np.asarray(labels)).reshape(-1)
                if a.size and not np.issubdtype(a.dtype, np.integer):
                    raise ValueError(f"add: integer labels expected, got {a.dtype}")
                if a.size and (a.min() < 0 or a.max() > 63):
                    raise ValueError("add: labels must lie in 0 .. 63")
                kept = np.ascontiguousarray(a.astype(np.int32))
                lab = torch.from_numpy(kept).to(dev)
            if lab.shape[0] != n:
                raise ValueError(f"add: {lab.shape[0]} labels for {n} entries")
        got = C.c_int32(-1)
        self.model._ctx.call("mocha_bank_resident_add", -1 if slot is None else int(slot), _ptr(nm), _ptr(enc), n, _ptr(lab) if lab is not None else None,
                             C.byref(got), _stream())
        self.labels[got.value] = kept if kept is not None else np.zeros(n, np.int32)
        if st.size:
            self.model._ctx.call("mocha_bank_resident_set_starts", int(got.value), st.ctypes.data_as(C.POINTER(C.c_int32)), int(st.size), _stream())
        return int(got.value)

    def retire(self, slot: int):
        """The character in ``slot`` leaves: the slot is empty and its rows are free from the next call on the current stream on."""
        self._ensure()
        if not 0 <= int(slot) < self.S:
            raise IndexError(f"retire: slot {slot} out of range 0 .. {self.S - 1}")
        self.model._ctx.call("mocha_bank_resident_retire", int(slot), _stream())
        self.labels[int(slot)] = None
        return self

    def replace(self, slot: int, cnt_nm, encoded, labels=None, starts=None) -> int:
        """Another character under the same id: ``retire(slot)`` (if it holds one) then ``add(..., slot=slot)``, on the current stream."""
        first, stop = self.rows(slot)
        if first != stop:
            self.retire(slot)
        return self.add(cnt_nm, encoded, labels=labels, slot=slot, starts=starts)


class MultiStreamCharacterizer:
    """One window of each of ``streams`` streams per step, every stream matched against its own character: the segmented characterize of
    the ``streams`` windows captured once into a HIP graph (``mocha_step_graph_segmented``) and replayed.  The character of each stream
    may change from step to step: the ids live in a device buffer the graph reads, so a change does not re-capture.
    ``soft=(k, temperature)``: the soft characterize (``mocha_step_graph_soft_segmented``); ``step`` then returns
    (Y, idx_k (streams,k), weight (streams,k)).
    ``constrained=True``: the action-constrained step (``mocha_step_graph_segmented_allow``); ``allow`` is then a (streams,) int64 device
    tensor of allow masks the graph reads - a producer may write it in place, new masks do not re-capture - and ``step`` returns
    ``applied`` (streams,) int32 as its last output.
    ``mix=J`` (1 .. 4): the mix characterize (``mocha_step_graph_mix_segmented``); ``mix_ids`` (streams,J) int32 and ``mix_weights``
    (streams,J,6) float32 are device tensors the graph reads - a producer may write them in place, new ids or weights do not re-capture -
    and ``step`` returns (Y, idx (streams,J), weight (streams,J,6)).  It does not combine with ``soft`` or ``constrained``."""

    def __init__(self, bank: MultiCharacterBank, cnt_mean, cnt_std, streams: int, raw: bool = False, soft=None, constrained: bool = False,
                 mix=None):
        if not 1 <= streams <= 16:
            raise ValueError("streams must be 1..16")
        self.mix = None
        if mix is not None:
            self.mix = mix_count(mix, "MultiStreamCharacterizer")
            _refuse_with_mix("MultiStreamCharacterizer", soft=soft is not None, constrained=constrained)
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
        self.constrained = bool(constrained)
        if self.constrained:
            if bank.labels is None:
                raise RuntimeError("MultiStreamCharacterizer: constrained=True needs a bank with action labels")
            self.allow = torch.zeros((self.streams,), dtype=torch.int64, device=m.device)
            self.applied = torch.zeros((self.streams,), dtype=torch.int32, device=m.device)
        if self.mix is not None:
            self.mix_ids = torch.full((self.streams, self.mix), -1, dtype=torch.int32, device=m.device)
            self.mix_weights = torch.zeros((self.streams, self.mix, MIX_PARTS), dtype=torch.float32, device=m.device)
            self.mix_idx = torch.full((self.streams, self.mix), -1, dtype=torch.int32, device=m.device)
            self.weight = torch.zeros((self.streams, self.mix, MIX_PARTS), dtype=torch.float32, device=m.device)
        bank._ensure()

    @property
    def input(self) -> torch.Tensor:
        """The captured step's own input windows (streams, 60, V, 15): a producer may write them in place and call ``step()``."""
        return self.x

    @property
    def characters(self) -> torch.Tensor:
        """The captured step's own character ids (streams,) int32 on the device: a producer may write them in place and call ``step()``."""
        return self.ids

    def step(self, windows: Optional[torch.Tensor] = None, characters=None, allow=None, mix=None):
        """windows (streams, 60, V, 15) [, characters: one id per stream] -> (Y (streams, 60, V, 15) view, idx (streams,) view); both are
        overwritten by the next step.  Without arguments the windows and ids already in ``input`` / ``characters`` are used.
        ``allow`` (constrained only): new allow masks, one per stream (see ``allow_masks``), copied into ``self.allow``.
        ``mix`` (mix=J only): new (ids, weights) (see ``mix_tensors``), copied into ``mix_ids`` / ``mix_weights``."""
        if mix is not None:
            if self.mix is None:
                raise RuntimeError("step: mix= needs MultiStreamCharacterizer(mix=J)")
            mids, mw = mix_tensors(mix, self.streams, self.model.device, "step", self.mix)
            self.mix_ids.copy_(mids, non_blocking=True)
            self.mix_weights.copy_(mw, non_blocking=True)
        if self.mix is not None:
            if characters is not None:
                raise ValueError("step: a mix streamer takes mix=, not characters")
            if windows is not None:
                self.x.copy_(windows.reshape(self.x.shape), non_blocking=True)
            self.bank._ensure()
            self.model._ctx.call("mocha_step_graph_mix_segmented", _ptr(self.x), self.streams, _ptr(self.mix_ids), _ptr(self.mix_weights),
                                 self.mix, _ptr(self.mean), _ptr(self.std), _ptr(self.y), _ptr(self.mix_idx), _ptr(self.weight),
                                 1 if self.raw else 0, _stream())
            return self.y, self.mix_idx, self.weight
        if allow is not None:
            if not self.constrained:
                raise RuntimeError("step: allow= needs MultiStreamCharacterizer(constrained=True)")
            self.allow.copy_(self.bank._allow(allow, self.streams, "step"), non_blocking=True)
        if characters is not None:
            self.ids.copy_(self.bank._ids(characters, self.streams), non_blocking=True)
        if windows is not None:
            self.x.copy_(windows.reshape(self.x.shape), non_blocking=True)
        self.bank._ensure()
        if self.constrained:
            k, t = self.soft if self.soft is not None else (0, 0.0)
            self.model._ctx.call("mocha_step_graph_segmented_allow", _ptr(self.x), self.streams, _ptr(self.ids), _ptr(self.allow), k, t,
                                 _ptr(self.mean), _ptr(self.std), _ptr(self.y), _ptr(self.idx_k if k else self.idx),
                                 _ptr(self.weight) if k else None, _ptr(self.applied), 1 if self.raw else 0, _stream())
            return (self.y, self.idx_k, self.weight, self.applied) if k else (self.y, self.idx, self.applied)
        if self.soft is not None:
            self.model._ctx.call("mocha_step_graph_soft_segmented", _ptr(self.x), self.streams, _ptr(self.ids), self.soft[0], self.soft[1],
                                 _ptr(self.mean), _ptr(self.std), _ptr(self.y), _ptr(self.idx_k), _ptr(self.weight), 1 if self.raw else 0,
                                 _stream())
            return self.y, self.idx_k, self.weight
        self.model._ctx.call("mocha_step_graph_segmented", _ptr(self.x), self.streams, _ptr(self.ids), _ptr(self.mean), _ptr(self.std),
                             _ptr(self.y), _ptr(self.idx), 1 if self.raw else 0, _stream())
        return self.y, self.idx
