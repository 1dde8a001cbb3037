"""NumPy restatement of coherent matching in live sessions (include/mocha_hip.h, "coherent matching in live sessions"): one step of the
path's forward recursion per stream, float64, sequential, with the state a live session keeps between steps.

Per stream: running, the previous (id, first row, rows, epoch), m_prev, M and the row R (float64).  One step with effective id e:

    e invalid (id < 0, rows outside 1..limit):  idx -1, dist +inf, continued 0, running = 0; R is not touched; a restart word is not consumed
    restart (not running, id / extent / epoch changed, restart word set):  R[j] = d[j]; the word is cleared
    otherwise:  a = R_prev[j-1] - M_prev if row j has a predecessor else +inf;  cont = a < lam (a tie jumps);  R[j] = d[j] + (a if cont else lam)
    M = min_j R[j], m the lowest j attaining it;  idx = m, dist = d[m], continued = not restart and m == m_prev + 1 and row m has a predecessor

Row j has a predecessor iff j > 0 and j is not a start.  tests/path_ref.py is the whole-clip path; the row this gives at step t is the
last row of path_ref over the windows 0..t of the same run (tests/test_path_step_ref.py).
"""
import numpy as np


class StreamState:
    def __init__(self):
        self.running = False
        self.key = None              # (id, first row, rows, epoch)
        self.m = 0
        self.M = 0.0
        self.R = None


class PathStepRef:
    def __init__(self, streams, lam):
        lam = float(lam)
        if not (np.isfinite(lam) and lam >= 0):
            raise ValueError("the jump penalty is finite and >= 0")
        self.lam = lam
        self.st = [StreamState() for _ in range(streams)]

    def reset(self, which=None):
        for s in (range(len(self.st)) if which is None else which):
            self.st[s] = StreamState()

    def step_stream(self, s, d, e, first=0, epoch=0, starts=(), restart=False, is_start=None):
        """d: the (rows,) distances of the stream's character, or None when the stream sits out.  starts: local rows that start a clip
        (is_start: the same as a bool array over the rows).  -> (idx, dist, continued, restart word consumed)."""
        st = self.st[s]
        if d is None or e < 0 or len(d) < 1:
            st.running = False
            return -1, np.float32(np.inf), 0, False
        d = np.asarray(d)
        n = len(d)
        pred = np.ones(n, dtype=bool)
        pred[0] = False
        for b in starts:
            if 0 <= b < n:
                pred[b] = False
        if is_start is not None:
            pred &= ~np.asarray(is_start, dtype=bool)
        key = (int(e), int(first), n, int(epoch))
        fresh = (not st.running) or st.key != key or bool(restart)
        if fresh:
            R = d.astype(np.float64)
        else:
            a = np.full(n, np.inf)
            a[1:] = st.R[:-1] - st.M
            a[~pred] = np.inf
            R = d.astype(np.float64) + np.where(a < self.lam, a, self.lam)
        m = int(np.argmin(R))                      # (numpy's argmin is the first of equal values)
        cont = int((not fresh) and m == st.m + 1 and bool(pred[m]))
        st.running, st.key, st.m, st.M, st.R = True, key, m, float(R[m]), R
        return m, d[m], cont, bool(restart)

    def advance(self, d, ids, rows, start_bits=None, bit_off=None, restart=None, limit=None):
        """The pure form for every stream: d (S, ld); ids, rows (S,); start_bits a bool array of bits (or None), bit_off (S,) or None;
        restart an int array (S,) that is cleared where consumed (or None).  limit: rows above it sit out (the state's rows).
        -> idx (S,) int32, dist (S,) float32, continued (S,) uint8."""
        S = len(self.st)
        idx = np.zeros(S, dtype=np.int32)
        dist = np.zeros(S, dtype=np.float32)
        cont = np.zeros(S, dtype=np.uint8)
        ld = d.shape[1]
        cap = ld if limit is None else min(ld, limit)
        for s in range(S):
            n = int(rows[s])
            ok = ids[s] >= 0 and 1 <= n <= cap
            is_start = None
            if ok and start_bits is not None:
                at = np.arange(n) + (0 if bit_off is None else int(bit_off[s]))
                inside = (at >= 0) & (at < len(start_bits))                   # a bit outside the table reads as not set
                is_start = np.zeros(n, dtype=bool)
                is_start[inside] = np.asarray(start_bits)[at[inside]]
            flag = bool(restart[s]) if restart is not None else False
            idx[s], dist[s], cont[s], used = self.step_stream(s, d[s, :n] if ok else None, int(ids[s]), 0, 0, (), flag, is_start)
            if used:
                restart[s] = 0
        return idx, dist, cont
