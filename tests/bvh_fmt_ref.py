"""The BVH writer's number format restated in Python integers, for the tests: what csrc/fmt_f6.h computes, and what Python's "%f" gives.

A finite float64 x = +-m 2^e (m < 2^53; a denormal is e = -1074 without the hidden bit).  |x| 10^6 = P 2^(e+6) exactly with P = m 15625.
With s = -(e+6): N = P >> s, plus one when the shifted-out remainder is above half, or exactly half with N odd.  The token is [-] (the
sign BIT), the decimal digits of N // 10^6 (at least one), '.', the six digits of N % 10^6.  Admitted: finite, |x| < 1e12; ``token``
returns None for everything else (NaN, +-inf, |x| >= 1e12), which the device refuses.

Also here, shared by the writer's tests: the hard list, the seeded random values, the motion block of the reference's writer
(motion/bvh.py:210-224) built from "%f " on the host, and the arrays of the golden files put back into the writer's axis order."""
import math
import struct

import numpy as np

AXIS = {"x": 0, "y": 1, "z": 2}


def token(x: float):
    u = struct.unpack("<Q", struct.pack("<d", x))[0]
    neg, ex, frac = u >> 63, (u >> 52) & 0x7FF, u & ((1 << 52) - 1)
    if ex == 0x7FF or abs(x) >= 1e12:
        return None
    m, e = (frac | (1 << 52), ex - 1075) if ex else (frac, -1074)
    P, s = m * 15625, -(e + 6)
    assert s >= 7
    N, rem, half = P >> s, P & ((1 << s) - 1), 1 << (s - 1)
    if rem > half or (rem == half and N & 1):
        N += 1
    return ("-" if neg else "") + str(N // 10 ** 6) + "." + str(N % 10 ** 6).zfill(6)


def hard_values():
    """The hard list, each value and its negation: zero, the neighbourhood of half a unit of the last place, the smallest denormal, ties
    j / 2^k (k = 7..20: exactly representable, six decimals cut them on a 5), carries into a new digit, one value of every
    integer-digit count 1..12, the largest admitted value."""
    v = [0.0, 5e-7, 4.9e-7, 5.1e-7, 1e-9, 5e-324]
    for k in range(7, 21):
        v += [j / 2.0 ** k for j in (1, 3, 5, 2 ** k + 1, 3 * 2 ** k - 1)]
    v += [0.9999995, 0.9999994999, 9.9999995, 99999.9999995, 999999.9999995]
    v += [10.0 ** n - 4e-7 for n in range(1, 10)]           # 9.9999996 -> 10.000000, ...: the float64 nearest 9.9999995 lies BELOW the tie
    v += [float("7" + "3" * (n - 1) + ".25") for n in range(1, 13)]
    v += [math.nextafter(1e12, 0.0)]
    return [s * a for a in v for s in (1.0, -1.0)]


def random_values(seed: int, count: int) -> np.ndarray:
    """Seeded float64 values: random sign and mantissa, binary exponent uniform in -40 .. 39; the few at or above 1e12 (the top of the
    last binade) are halved, so that every value is admitted."""
    rng = np.random.Generator(np.random.PCG64(seed))
    mant = rng.integers(0, 1 << 52, size=count, dtype=np.uint64)
    ex = rng.integers(1023 - 40, 1023 + 40, size=count, dtype=np.uint64)
    sign = rng.integers(0, 2, size=count, dtype=np.uint64)
    x = (sign << np.uint64(63) | ex << np.uint64(52) | mant).view(np.float64)
    return np.where(np.abs(x) >= 1e12, x * 0.5, x)


def columns(pos, rot, visit, order, save_positions):
    """The writer's (frames, C) matrix (motion/bvh.py:210-222) from positions / rotations (F,V,3) in axis order x, y, z."""
    ax = [AXIS[c] for c in order]
    if save_positions:
        cols = [a for j in visit for a in (pos[:, j, :], rot[:, j][:, ax])]
    else:
        cols = [pos[:, 0, :]] + [rot[:, j][:, ax] for j in visit]
    return np.concatenate(cols, axis=1)


def motion_text(M, fmt=None) -> bytes:
    """Every number of the (frames, C) matrix as "%f " and a newline behind every frame; ``fmt`` replaces "%f" % x (``token``)."""
    fmt = fmt or (lambda x: "%f" % x)
    return "".join("".join(fmt(x) + " " for x in row) + "\n" for row in M.tolist()).encode()


def golden_arrays(gold, tag):
    """(names, parents, positions, rotations in axis order, offsets, order, frametime) of fixture file ``tag`` from bvh_parse.npz: the
    loader returns the angles in FILE channel order, the writer takes them by axis (rots[.., ordermap[order[k]]], bvh.py:217)."""
    order = str(gold[f"{tag}_order"])
    loaded = gold[f"{tag}_rotations"]
    rot = np.empty_like(loaded)
    for k, c in enumerate(order):
        rot[..., AXIS[c]] = loaded[..., k]
    return ([str(n) for n in gold[f"{tag}_names"]], [int(p) for p in gold[f"{tag}_parents"]], gold[f"{tag}_positions"], rot,
            gold[f"{tag}_offsets"], order, float(gold[f"{tag}_frametime"]))


def golden_file(path, tag) -> bytes:
    """The fixture file as the reference's writer left it: mixamo22.bvh with its documented edits undone (every line end back to \\n, the
    appended blank line dropped - tests/golden/make_golden_bvh.py)."""
    with open(path, "rb") as f:
        text = f.read()
    if tag == "mixamo22":
        assert text.endswith(b"\r\n\r\n")
        text = text[:-2].replace(b"\r\n", b"\n")
    return text
