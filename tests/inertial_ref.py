"""float64 NumPy restatement of the inertializer of the pose heads (include/mocha_hip.h, "Inertialized character switches"), written from
that description and from the formulas of motion/Inertialization.py:10-37, 71-91 and motion/quat.py:18-19, 109-120, 149-164 - not from the
HIP source.  tests/test_inertial_ref.py pins it to tests/golden/inertialize.npz, which the reference's own functions produced.

A head row is [pos 3 | quat wxyz 4 | vel 3 | ang 3].  ``InertialRef.step`` takes fp32 heads and returns the float64 result BEFORE the single
rounding to fp32 (pass-through rows are the input converted exactly), so both the fixture (1e-12) and the kernel (one fp32 ulp) can be
held to it.  ``monitor`` collects the quantities whose distance from a branch point keeps the reference single-valued."""
import numpy as np

EPS = 1e-5
POS, ROT, VEL, ANG = slice(0, 3), slice(3, 7), slice(7, 10), slice(10, 13)


def _length(x):
    return np.sqrt(np.sum(x * x, axis=-1))


def qmul(x, y):
    x0, x1, x2, x3 = x[..., 0:1], x[..., 1:2], x[..., 2:3], x[..., 3:4]
    y0, y1, y2, y3 = y[..., 0:1], y[..., 1:2], y[..., 2:3], y[..., 3:4]
    return np.concatenate([y0 * x0 - y1 * x1 - y2 * x2 - y3 * x3,
                           y0 * x1 + y1 * x0 - y2 * x3 + y3 * x2,
                           y0 * x2 + y1 * x3 + y2 * x0 - y3 * x1,
                           y0 * x3 - y1 * x2 + y2 * x1 + y3 * x0], axis=-1)


def qinv(q):
    return np.array([1.0, -1.0, -1.0, -1.0]) * q


def qabs(q):
    return np.where(q[..., 0:1] > 0.0, q, -q)


def to_scaled_angle_axis(q, monitor=None):
    ln = _length(q[..., 1:])[..., None]
    if monitor is not None:
        monitor["len"].append(ln.ravel().copy())
    with np.errstate(invalid="ignore", divide="ignore"):
        half = np.where(ln < EPS, np.ones_like(ln), np.arctan2(ln, q[..., 0:1]) / ln)
    return 2.0 * (half * q[..., 1:])


def from_scaled_angle_axis(v, monitor=None):
    x = v / 2.0
    h = _length(x)[..., None]
    if monitor is not None:
        monitor["len"].append(h.ravel().copy())
    with np.errstate(invalid="ignore", divide="ignore"):
        c = np.where(h < EPS, np.ones_like(h), np.cos(h))
        s = np.where(h < EPS, np.ones_like(h), np.sin(h) / h)
    return np.concatenate([c, s * x], axis=-1)


def spring(halflife, dt):
    """(y, exp(-y dt)) of the critically damped spring: the damping of halflife_to_damping / 2 and the rational fast_negexpf."""
    y = (4.0 * np.log(2.0)) / (halflife + EPS) / 2.0
    x = y * dt
    return y, 1.0 / (1.0 + x + 0.48 * x * x + 0.235 * x * x * x)


class InertialRef:
    """State of n streams of V bones; ``step`` is one frame."""

    def __init__(self, n, V, halflife=0.1, dt=1.0 / 60.0):
        self.n, self.V, self.halflife, self.dt = n, V, halflife, dt
        self.monitor = {"w": [], "len": []}
        self.reset()

    def reset(self, which=None):
        if which is None:
            n, V = self.n, self.V
            self.seen = np.zeros(n, bool); self.active = np.zeros(n, bool); self.last_id = np.zeros(n, np.int64)
            self.prev = np.zeros((n, V, 13))
            self.off_pos = np.zeros((n, V, 3)); self.off_vel = np.zeros((n, V, 3)); self.off_ang = np.zeros((n, V, 3))
            self.off_rot = np.zeros((n, V, 4)); self.off_rot[..., 0] = 1.0
            return
        for s in which:
            self._clear(s)

    def _clear(self, s):
        self.seen[s] = self.active[s] = False
        self.off_pos[s] = 0; self.off_vel[s] = 0; self.off_ang[s] = 0; self.off_rot[s] = (1.0, 0.0, 0.0, 0.0)

    def clone(self):
        import copy
        return copy.deepcopy(self)

    def step(self, heads, ids=None, trigger=None, valid=None, halflife=None):
        """heads (n,V,13) fp32 -> (n,V,13) float64; rows of streams with valid == 0 are NaN (the kernel leaves them untouched)."""
        heads = np.asarray(heads)
        assert heads.dtype == np.float32 and heads.shape == (self.n, self.V, 13)
        hl = self.halflife if halflife is None else halflife
        y, eydt = spring(hl, self.dt)
        dt = self.dt
        out = np.full((self.n, self.V, 13), np.nan)
        for s in range(self.n):
            if valid is not None and valid[s] == 0:
                self._clear(s)
                continue
            x = heads[s].astype(np.float64)
            ident = int(ids[s]) if ids is not None else (int(self.last_id[s]) if self.seen[s] else 0)
            if not self.seen[s]:
                self._clear(s)
                self.seen[s] = True
                out[s] = x
            else:
                if (ids is not None and ident != self.last_id[s]) or (trigger is not None and trigger[s] != 0):
                    p = self.prev[s]
                    self.off_pos[s] = (p[:, POS] + self.off_pos[s]) - x[:, POS]
                    self.off_vel[s] = (p[:, VEL] + self.off_vel[s]) - x[:, VEL]
                    q = qmul(qmul(self.off_rot[s], p[:, ROT]), qinv(x[:, ROT]))
                    self.monitor["w"].append(q[:, 0].copy())
                    self.off_rot[s] = qabs(q)
                    self.off_ang[s] = (self.off_ang[s] + p[:, ANG]) - x[:, ANG]
                    self.active[s] = True
                if not self.active[s]:
                    out[s] = x
                else:
                    j1 = self.off_vel[s] + self.off_pos[s] * y
                    self.off_pos[s] = eydt * (self.off_pos[s] + j1 * dt)
                    self.off_vel[s] = eydt * (self.off_vel[s] - j1 * y * dt)
                    j0 = to_scaled_angle_axis(self.off_rot[s], self.monitor)
                    j1 = self.off_ang[s] + j0 * y
                    self.off_rot[s] = from_scaled_angle_axis(eydt * (j0 + j1 * dt), self.monitor)
                    self.off_ang[s] = eydt * (self.off_ang[s] - j1 * y * dt)
                    out[s, :, POS] = x[:, POS] + self.off_pos[s]
                    out[s, :, VEL] = x[:, VEL] + self.off_vel[s]
                    out[s, :, ROT] = qmul(self.off_rot[s], x[:, ROT])
                    out[s, :, ANG] = self.off_ang[s] + x[:, ANG]
            self.prev[s] = x
            self.last_id[s] = ident
        return out

    def single_valued(self, margin=1e-3):
        """The two conditions under which a restatement and the reference cannot take different branches: every offset quaternion has
        |w| >= margin before quat.abs, and every vector-part length / half-angle fed to quat.log / quat.exp is exactly 0 or >= margin."""
        w = np.concatenate(self.monitor["w"]) if self.monitor["w"] else np.ones(1)
        ln = np.concatenate(self.monitor["len"]) if self.monitor["len"] else np.zeros(1)
        return bool(np.all(np.abs(w) >= margin)) and bool(np.all((ln == 0.0) | (ln >= margin)))


def ulp_bound(ref64):
    """Per-element bound of the kernel against this restatement: device and NumPy float64 differ by a few float64 ulps, so the single
    rounding to fp32 can land one fp32 ulp apart; the floor covers values near zero."""
    return np.spacing(np.abs(ref64).astype(np.float32)).astype(np.float64) + 1e-12


# ------------------------------------------------------------------------------------------------------------------ smooth synthetic inputs
def smooth_clip(rng, frames, V, fps=60.0):
    """One character's heads (frames, V, 13) float64: smooth, unrelated per-channel motions; unit quaternions from a smooth rotation vector."""
    t = (np.arange(frames) / fps)[:, None, None]

    def wave(amp, k):
        a = rng.uniform(0.5, 1.0, (1, V, k)) * amp
        f = rng.uniform(0.5, 2.0, (1, V, k))
        ph = rng.uniform(0, 2 * np.pi, (1, V, k))
        return a * np.sin(2 * np.pi * f * t + ph) + rng.uniform(-1, 1, (1, V, k)) * amp

    h = np.empty((frames, V, 13))
    h[..., POS] = wave(0.3, 3)
    v = wave(1.0, 3)
    h[..., ROT] = from_scaled_angle_axis(v)
    h[..., VEL] = wave(1.0, 3)
    h[..., ANG] = wave(2.0, 3)
    return h


def switched_streams(seed, frames, n, V, n_char=3, first=8):
    """n streams of smooth clips that switch between n_char unrelated characters at random frames >= first: heads (frames,n,V,13) fp32
    and ids (frames,n) int32.  Stream 0 of several never switches."""
    rng = np.random.Generator(np.random.PCG64(seed))
    clips = [[smooth_clip(rng, frames, V) for _ in range(n_char)] for _ in range(n)]
    ids = np.zeros((frames, n), np.int32)
    for s in range(1 if n > 1 else 0, n):
        cur = int(rng.integers(n_char))
        cuts = sorted(rng.choice(np.arange(first, frames), size=int(rng.integers(1, 4)), replace=False).tolist())
        for f in range(frames):
            if f in cuts:
                cur = (cur + 1 + int(rng.integers(n_char - 1))) % n_char
            ids[f, s] = cur
    heads = np.stack([np.stack([clips[s][ids[f, s]][f] for s in range(n)]) for f in range(frames)]).astype(np.float32)
    return heads, ids


# (seed, n, V) of the seeded inputs the kernel test runs: every one obeys single_valued() (tests/test_inertial_ref.py checks it on the CPU)
SEEDED = [(100, 1, 22), (100, 1, 24), (100, 3, 22), (100, 3, 24), (100, 17, 22), (102, 17, 24)]
