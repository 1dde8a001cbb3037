"""BVH files in: the first link of file -> ``ingest_clips`` -> windows -> ``characterize_pair`` -> post-processing -> ``write_bvh``.

``read_bvh_header`` reads the HIERARCHY block and the ``Frames:`` / ``Frame Time:`` lines on the host (``mocha_bvh_header``; no GPU).
``load_bvh`` parses the MOTION blocks of one or many files on the device (``mocha_bvh_motion``): the numeric text of all files is packed
into one buffer, copied over once, and comes back as the two fp32 device arrays ``ingest_clips`` reads - what the reference's loader
(motion/bvh.py:22-138) returns, rounded to fp32 once: Euler degrees in file channel order and positions in file units per joint, joints
in file order.  Refused, where the reference reads silently and wrongly: 9-channel joints, joints that disagree on their channels or
rotation order, lines with the wrong number of values, a frame count that does not match the text.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import List, Optional, Sequence, Union

import numpy as np
import torch

from . import _C
from .generator import Generator, _ptr, _stream

_AXIS = "xyz"
_MAX_CALL_BYTES = (1 << 31) - _C.BVH_ALIGN      # mocha_bvh_motion takes less than 2^31 bytes of text per call


class BvhHeader:
    """``names``, ``parents`` (file order, the root's -1), ``offsets`` (V,3) float64 (End Site offsets ignored), ``order`` ('zyx', ...),
    ``channels`` (3: only the root has position channels; 6: every joint has), ``frames``, ``frametime`` and the byte range
    ``motion_begin`` .. ``motion_end`` of the numeric block."""

    def __init__(self, names, parents, offsets, order, channels, frames, frametime, motion_begin, motion_end):
        self.names, self.parents, self.offsets, self.order, self.channels = names, parents, offsets, order, channels
        self.frames, self.frametime, self.motion_begin, self.motion_end = frames, frametime, motion_begin, motion_end

    def same_hierarchy(self, other: "BvhHeader") -> bool:
        return (self.names == other.names and np.array_equal(self.parents, other.parents) and self.channels == other.channels
                and self.order == other.order)


def _read(path_or_bytes) -> bytes:
    if isinstance(path_or_bytes, (bytes, bytearray, memoryview)):
        return bytes(path_or_bytes)
    with open(os.fspath(path_or_bytes), "rb") as f:
        return f.read()


def _header(text: bytes, what: str) -> BvhHeader:
    hdr = _C.mocha_bvh_hdr()
    rc = _C.load_library().mocha_bvh_header(text, len(text), C.byref(hdr))
    if rc != 0:
        raise ValueError(f"{what}: not a BVH file this library reads: {hdr.error.decode()} (line at byte {hdr.error_offset})")
    V = hdr.n_joints
    names = [text[hdr.name_offset[j]: hdr.name_offset[j] + hdr.name_length[j]].decode("utf-8", "replace") for j in range(V)]
    offsets = np.array([[hdr.offsets[j][a] for a in range(3)] for j in range(V)], dtype=np.float64).reshape(V, 3)
    return BvhHeader(names, np.array(hdr.parents[:V], dtype=np.int64), offsets, "".join(_AXIS[hdr.order[a]] for a in range(3)),
                     int(hdr.channels), int(hdr.frames), float(hdr.frame_time), int(hdr.motion_begin), int(hdr.motion_end))


def read_bvh_header(path_or_bytes) -> BvhHeader:
    """The hierarchy of a BVH file (a path, or the file's bytes).  Raises ValueError, with the byte offset of the offending line, for
    what ``mocha_bvh_header`` refuses."""
    return _header(_read(path_or_bytes), "read_bvh_header" if not isinstance(path_or_bytes, (str, os.PathLike)) else os.fspath(path_or_bytes))


class BvhClips:
    """``load_bvh``'s result: ``rot`` / ``pos`` (F,V,3) fp32 on the device, the clips concatenated along the frame axis; ``lengths``
    their frame counts; ``names``, ``parents``, ``offsets`` (V,3) float64 of the selected joints in output order; ``order``;
    ``frametime`` (the first file's); ``tokens`` / ``slow_tokens``: how many numbers were read, and how many of them the host converted;
    ``source_fps``: each file's frame rate.  After resampling (``load_bvh(fps=R)`` on files of another rate) ``order`` is None, ``rot``
    is (F',V,4) unit quaternions, ``lengths`` are the new frame counts and ``frametime`` is 1 / R."""

    def __init__(self, rot, pos, lengths, names, parents, offsets, order, frametime, tokens, slow_tokens, source_fps=None):
        self.rot, self.pos, self.lengths, self.names, self.parents, self.offsets = rot, pos, lengths, names, parents, offsets
        self.order, self.frametime, self.tokens, self.slow_tokens, self.source_fps = order, frametime, tokens, slow_tokens, source_fps

    def clips(self):
        """[(rot, pos)] per clip: views of the device arrays, as ``bank.build_database_from_clips`` takes them."""
        stops = np.cumsum(self.lengths)
        return [(self.rot[e - n: e], self.pos[e - n: e]) for n, e in zip(self.lengths, stops)]


def _select(hdr: BvhHeader, joints) -> List[int]:
    if joints is None:
        return list(range(len(hdr.names)))
    pick = []
    for j in joints:
        if isinstance(j, str):
            if j not in hdr.names:
                raise ValueError(f"load_bvh: the files have no joint named {j!r}")
            j = hdr.names.index(j)
        j = int(j)
        if not 0 <= j < len(hdr.names) or j in pick:
            raise ValueError(f"load_bvh: joint {j} is outside the file's {len(hdr.names)} joints or selected twice")
        pick.append(j)
    if not pick:
        raise ValueError("load_bvh: joints selects nothing")
    return pick


def load_bvh(model: Generator, paths: Union[str, os.PathLike, bytes, Sequence], joints: Optional[Sequence] = None, fps=None,
             source_fps=None) -> BvhClips:
    """One or many BVH files (paths, or the files' bytes) -> ``BvhClips`` on ``model``'s device.  All files must share one hierarchy
    (names, parents, channels, rotation order), else ValueError.  ``joints``: names or file joint indices in the order the output should
    have (the model layout's); None = every joint in file order.  The parents of a selection are the nearest selected ancestors.
    With three channels per joint a joint's position is its file's OFFSET (bvh.py:97): files with equal OFFSETs share a call of
    ``mocha_bvh_motion`` (up to 2 GiB of text), a file whose OFFSETs differ starts a new one; ``offsets`` of the result are the first
    file's.  Waits for the current stream once per call; not for graph capture.
    ``fps=R``: the clips are brought to R frames per second (``ingest.resample_clips``, one call for all files).  A file's own rate is
    ``round(1 / frametime)``; ``source_fps`` (one value, or one per file) overrides it.  If every file is at R already the result is the
    Euler arrays as read; otherwise ``order`` is None, ``rot`` holds quaternions and ``frametime`` is 1 / R.  ``fps=None``: as read."""
    if isinstance(paths, (str, os.PathLike, bytes, bytearray, memoryview)):
        paths = [paths]
    if not len(paths):
        raise ValueError("load_bvh: no file")
    texts = [_read(p) for p in paths]
    label = [os.fspath(p) if isinstance(p, (str, os.PathLike)) else f"file {i}" for i, p in enumerate(paths)]
    hdrs = [_header(t, w) for t, w in zip(texts, label)]
    h0 = hdrs[0]
    for h, w in zip(hdrs, label):
        if not h.same_hierarchy(h0):
            raise ValueError(f"load_bvh: {w} does not share the hierarchy of {label[0]} (names, parents, channels, order)")
        if h.frames < 1:
            raise ValueError(f"load_bvh: {w} has no frames")
    pick = _select(h0, joints)
    V, V_out, dev = len(h0.names), len(pick), model.device
    lengths = [h.frames for h in hdrs]
    F = int(sum(lengths))
    if F >= 2 ** 31:
        raise ValueError("load_bvh: fewer than 2^31 frames in all")
    jmap = (C.c_int32 * V)(*([-1] * V))
    for o, j in enumerate(pick):
        jmap[j] = o
    rot = torch.empty((F, V_out, 3), dtype=torch.float32, device=dev)
    pos = torch.empty((F, V_out, 3), dtype=torch.float32, device=dev)
    align = _C.BVH_ALIGN
    padded = [max(-(-(h.motion_end - h.motion_begin) // align), 1) * align for h in hdrs]
    tokens = slow = 0
    first, frame0 = 0, 0

    def shares_offsets(i, j):      # a call has ONE offsets_out: with three channels per joint, files whose OFFSETs differ get calls of their own
        return h0.channels == 6 or np.array_equal(hdrs[i].offsets, hdrs[j].offsets)
    while first < len(texts):
        last, nbytes = first, 0                                   # files first .. last-1 share a call
        while last < len(texts) and (last == first or (nbytes + padded[last] <= _MAX_CALL_BYTES and shares_offsets(last, first))):
            nbytes += padded[last]
            last += 1
        if nbytes > _MAX_CALL_BYTES:
            raise ValueError(f"load_bvh: the motion text of {label[first]} alone exceeds 2 GiB")
        n = last - first
        buf = np.full(nbytes, 0x0A, dtype=np.uint8)               # gaps and the tail are '\n'
        begin, end = (C.c_int64 * n)(), (C.c_int64 * n)()
        at = 0
        for i in range(first, last):
            h = hdrs[i]
            m = h.motion_end - h.motion_begin
            buf[at: at + m] = np.frombuffer(texts[i], dtype=np.uint8, count=m, offset=h.motion_begin)
            begin[i - first], end[i - first] = at, at + max(m, 1)
            at += padded[i]
        offs = np.concatenate([[0], np.cumsum(lengths[first:last])])
        text_dev = torch.from_numpy(buf).to(dev)                  # the one copy of the text
        off_first = np.ascontiguousarray(hdrs[first].offsets[pick], dtype=np.float32)
        rep = _C.mocha_bvh_report()
        nf = int(offs[-1])
        try:
            model._ctx.call("mocha_bvh_motion", _ptr(text_dev), nbytes, buf.ctypes.data_as(C.c_void_p), begin, end,
                            (C.c_int32 * (n + 1))(*[int(v) for v in offs]), n, V, h0.channels, jmap, V_out,
                            off_first.ctypes.data_as(C.POINTER(C.c_float)), _ptr(rot[frame0: frame0 + nf]), _ptr(pos[frame0: frame0 + nf]),
                            C.byref(rep), _stream())
        except RuntimeError as e:
            if rep.first_bad < 0:
                raise
            c = max(i for i in range(n) if begin[i] <= rep.first_bad)
            where = hdrs[first + c].motion_begin + min(rep.first_bad, end[c]) - begin[c]
            raise ValueError(f"load_bvh: {label[first + c]}: the MOTION block does not hold {lengths[first + c]} frames of "
                             f"{3 + 3 * V if h0.channels == 3 else 6 * V} numbers each, or a token is no decimal number: first bad byte "
                             f"{where} of the file") from e
        tokens, slow = tokens + int(rep.tokens), slow + int(rep.slow)
        first, frame0 = last, frame0 + nf
    index = {j: o for o, j in enumerate(pick)}
    parents = []
    for j in pick:                                                # the nearest selected ancestor
        q = int(h0.parents[j])
        while q >= 0 and q not in index:
            q = int(h0.parents[q])
        parents.append(index[q] if q >= 0 else -1)
    if source_fps is None:
        rates = [int(round(1.0 / h.frametime)) if h.frametime > 0 else 0 for h in hdrs]
    elif isinstance(source_fps, (list, tuple, np.ndarray)):
        rates = list(source_fps)
        if len(rates) != len(hdrs):
            raise ValueError("load_bvh: source_fps is one value, or one per file")
    else:
        rates = [source_fps] * len(hdrs)
    order, frametime = h0.order, h0.frametime
    if fps is not None:
        from .ingest import resample_clips, resample_ratio
        for r, w in zip(rates, label):
            if not r > 0:
                raise ValueError(f"load_bvh: {w} has no usable frame time; pass source_fps=")
        if any(resample_ratio(r, fps) != (1, 1) for r in rates):
            rot, pos, lengths = resample_clips(model, rot, pos, lengths, rates, target_fps=fps, order=h0.order)
            order, frametime = None, 1.0 / float(fps)
    return BvhClips(rot, pos, lengths, [h0.names[j] for j in pick], np.array(parents, dtype=np.int64), h0.offsets[pick].copy(), order,
                    frametime, tokens, slow, rates)
