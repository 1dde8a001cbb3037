"""CPU ORACLE for a live session (mocha_live_step, one stream) — TEST INFRASTRUCTURE.

The live loop restated from the oracle parts that are pinned against the reference on their own, and from nothing else: a Python list
of the last 60 frames -> ``featurize_oracle.featurize`` on the materialised window (re-rooted on the frame just pushed) -> z-score with
the pose norm (test_fullframework.py:186) -> ``mocha_oracle.encode`` -> ``znorm`` -> exact float64 1-NN within the stream's OWN
character -> ``mocha_oracle.decoder`` / ``to_mot`` on the matched row -> de-normalisation (:303) -> ``postprocess_oracle.pose_heads``
-> one ``PostProcess.step`` -> ``bvh_channels``.  No import from the library's csrc, no GPU.

Pose norm convention (the library's ``raw=True`` path, tests/test_hip_parity.py::test_fused_pose_normalisation): the four arrays hold
(V+1, 15) rows with the root bone first; the network sees bones 1.., so X is normalised and Y de-normalised with rows 1.. .

``float64=True`` runs the network part (weights, normalised input, bank rows, de-normalisation) in double; featurisation (float32 by
definition of the reference's arrays) and everything from ``pose_heads`` on are the same in both modes."""
from __future__ import annotations

import numpy as np
import torch

from mocha_sigasia2023_amd.skeleton import LAYOUTS
from mocha_sigasia2023_amd.synthetic import slide_windows

from . import featurize_oracle as FO
from . import mocha_oracle as O
from . import postprocess_oracle as P

WINDOW = 60


def torch_state(state_dict, float64=False):
    """The oracle's weights: float32 as ``mocha_oracle.to_torch_state`` gives them, or cast to double."""
    sd = O.to_torch_state(state_dict)
    return {k: v.double() for k, v in sd.items()} if float64 else sd


def _norm_rows(pose_norm):
    return tuple(np.asarray(a, np.float32).reshape(-1, 15) for a in pose_norm)


def encode_windows(sd, X_raw, pose_norm, float64=False):
    """X_raw (B, 60, V+1, 15) float32 un-normalised, root bone first -> (encoded, cnt) (B, 90, 256) torch tensors, one window per call
    of the network (the same arithmetic whether the windows come one by one or as a clip)."""
    Xm, Xs, _, _ = _norm_rows(pose_norm)
    if float64:
        Xn = (X_raw[:, :, 1:].astype(np.float64) - Xm[None, None, 1:]) / Xs[None, None, 1:]
    else:
        Xn = (X_raw[:, :, 1:] - Xm[None, None, 1:]) / Xs[None, None, 1:]           # test_fullframework.py:186
    enc, cnt = [], []
    with torch.no_grad():
        for i in range(len(Xn)):
            e, c = O.encode(sd, torch.from_numpy(np.ascontiguousarray(Xn[i:i + 1])))
            enc.append(e); cnt.append(c)
    return torch.cat(enc), torch.cat(cnt)


def bank_from_clip(state_dict, layout, pose_norm, cnt_mean, cnt_std, clip, float64=False):
    """A character's bank from a clip of local bone features (rot (F,J,4), pos, vel, ang): every window of the clip featurised and
    encoded by the oracle -> (cnt_nm (N, 90, 256), encoded (N, 90, 256)) NumPy arrays, float32 or float64."""
    sd = torch_state(state_dict, float64)
    X = FO.featurize(*[slide_windows(np.asarray(a, np.float32), WINDOW) for a in clip], FO.full_parents(LAYOUTS[layout]["parents"]))
    enc, cnt = encode_windows(sd, X, pose_norm, float64)
    return O.znorm(cnt.numpy(), np.asarray(cnt_mean), np.asarray(cnt_std)), enc.numpy()


def search(query_nm, bank_nm):
    """Exact Euclidean distances in float64, direct form: (order of the rows by distance, distances (N,))."""
    q = np.asarray(query_nm, np.float64).reshape(-1)
    k = np.asarray(bank_nm, np.float64).reshape(len(bank_nm), -1)
    d = np.sqrt(((k - q[None]) ** 2).sum(1))
    return np.argsort(d, kind="stable"), d


def decode(sd, src_encoded, cha_row, pose_norm, float64=False):
    """decoder + to_mot on one matched row, de-normalised: Y (60, V, 15)."""
    _, _, Ym, Ys = _norm_rows(pose_norm)
    cha = torch.from_numpy(np.ascontiguousarray(cha_row))[None].to(src_encoded.dtype)
    with torch.no_grad():
        Y = O.to_mot(sd, O.decoder(sd, src_encoded, cha)).numpy()[0]
    if float64:
        return Y * Ys[None, 1:].astype(np.float64) + Ym[None, 1:].astype(np.float64)
    return Y * Ys[None, 1:] + Ym[None, 1:]                                         # test_fullframework.py:303


class LiveOracle:
    """One live stream.  ``banks``: per character ``(cnt_nm, encoded)`` (N_c, 90, 256) (``bank_from_clip``); ``pose_norm``: (X_mean,
    X_std, Y_mean, Y_std), (V+1, 15) each; ``contact_bones`` / ``post_kw``: as ``postprocess_oracle.PostProcess`` takes them."""

    def __init__(self, state_dict, layout, pose_norm, cnt_mean, cnt_std, banks, contact_bones, post_kw=None, float64=False):
        self.float64 = bool(float64)
        self.sd = torch_state(state_dict, self.float64)
        self.parents = FO.full_parents(LAYOUTS[layout]["parents"])
        self.pose_norm = _norm_rows(pose_norm)
        self.cnt_mean, self.cnt_std = np.asarray(cnt_mean, np.float32), np.asarray(cnt_std, np.float32)
        self.banks = [(np.asarray(nm).reshape(len(nm), -1), np.asarray(enc)) for nm, enc in banks]
        self.contact_bones = tuple(int(b) for b in contact_bones)
        self.post_kw = dict(post_kw or {})
        self.reset()

    def reset(self):
        self.frames = []
        self.post = P.PostProcess(self.parents, contact_bones=self.contact_bones, **self.post_kw)
        return self

    def push(self, rot, pos, vel, ang, rvel, rang, speed, contact, character, forced_row=None):
        """One frame: rot (J,4), pos / vel / ang (J,3) local bone data, root first; rvel / rang (3,), speed (), contact (n_contact,) of
        the source; the stream's character.  ``forced_row``: decode on this row of the character instead of the matched one (the
        match is still reported).  While fewer than 60 frames are held: {"valid": 0}, and nothing but the frame list moves."""
        self.frames.append(tuple(np.asarray(a, np.float32) for a in (rot, pos, vel, ang)))
        if len(self.frames) > WINDOW:
            self.frames.pop(0)
        if len(self.frames) < WINDOW:
            return {"valid": 0}
        X_raw = FO.featurize(*[np.stack([f[k] for f in self.frames])[None] for k in range(4)], self.parents)
        enc, cnt = encode_windows(self.sd, X_raw, self.pose_norm, self.float64)
        nm, encoded = self.banks[int(character)]
        order, d = search(O.znorm(cnt.numpy(), self.cnt_mean, self.cnt_std), nm)
        idx = int(order[0])
        row = idx if forced_row is None else int(forced_row)
        Y = decode(self.sd, enc, encoded[row], self.pose_norm, self.float64)
        heads, hspeed = P.pose_heads(Y[None])
        p, r, ik = self.post.step(heads[0], hspeed[0], rvel, rang, speed, contact)
        bp, be = P.bvh_channels(p[None], ik[None])
        return {"valid": 1, "X_raw": X_raw[0], "idx": idx, "dist": float(d[idx]), "dist2": float(d[order[1]]) if len(d) > 1 else np.inf,
                "dists": d, "Y": Y, "heads": heads[0], "speed": hspeed[0], "pos": p, "rot": r, "ik_rot": ik, "bvh_pos": bp[0],
                "bvh_euler": be[0]}
