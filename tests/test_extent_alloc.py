"""ExtentAlloc (csrc/extent_alloc.h), the host-only extent bookkeeping of a resident bank: first fit over 16-row units, release with merge
of the neighbours, free units, largest free extent.  The header and a driver with its own main (tests/extent_alloc_main.cpp) are compiled
by g++ with the address and undefined-behaviour sanitizers linked statically and run once as a child process - nothing is loaded into
Python - on a seeded sequence of a few thousand operations; every answer is compared with the model below (one flag per unit).  The
sequence mixes takes that fit, takes that do not, releases of live extents in random order (so free neighbours merge on either side, on
both and on none) and releases the allocator must refuse: twice the same extent, a part of a free one - from its first unit and from a
unit inside it -, outside the range.  No GPU."""
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
UNITS = 97


class Model:
    """The same answers from one flag per unit."""

    def __init__(self, units):
        self.used = [False] * units

    def runs(self):
        """The free extents as (first, units), ascending."""
        out, u = [], self.used
        for i in range(len(u)):
            if not u[i] and (i == 0 or u[i - 1]):
                out.append([i, 0])
            if not u[i]:
                out[-1][1] += 1
        return out

    def take(self, n):
        first = next((f for f, k in self.runs() if k >= n), -1) if n >= 1 else -1
        if first >= 0:
            self.used[first:first + n] = [True] * n
        return first

    def release(self, first, n):
        ok = n >= 1 and first >= 0 and first + n <= len(self.used) and all(self.used[first:first + n])
        if ok:
            self.used[first:first + n] = [False] * n
        return ok

    def stats(self):
        r = self.runs()
        return sum(k for _, k in r), max([k for _, k in r], default=0)


def _sequence(seed, count):
    """(operation lines, expected answer lines): the model decides which extents are live, so releases hit real extents."""
    rng = np.random.Generator(np.random.PCG64(seed))
    m, live, ops, want = Model(UNITS), [], [f"u {UNITS}"], ["u"]
    for _ in range(count):
        p = rng.random()
        if p < 0.5 or not live:
            n = int(rng.integers(0, 14)) if p < 0.45 else int(rng.integers(30, 120))       # (0 and the large ones are refused)
            first = m.take(n)
            if first >= 0:
                live.append((first, n))
            ops.append(f"t {n}")
            want.append("t %d %d %d" % ((first,) + m.stats()))
        elif p < 0.9:
            first, n = live.pop(int(rng.integers(0, len(live))))
            assert m.release(first, n)
            ops.append(f"r {first} {n}")
            want.append("r 1 %d %d" % m.stats())
        else:                                                   # a release that must be refused and change nothing
            kind = int(rng.integers(0, 5))
            free = [f for f, k in m.runs()]
            wide = [(f, k) for f, k in m.runs() if k >= 2]
            if kind == 0 and free:
                first, n = free[int(rng.integers(0, len(free)))], 1                        # the first unit of a free extent
            elif kind == 4 and wide:
                f0, k0 = wide[int(rng.integers(0, len(wide)))]                              # starts strictly INSIDE a free extent (the
                first, n = f0 + int(rng.integers(1, k0)), int(rng.integers(1, 4))           # neighbour below overlaps), 1 .. 3 units
            elif kind == 1:
                first, n = UNITS - 1, 2                                                     # leaves the range
            elif kind == 2:
                first, n = -1, 1
            else:
                f0, n0 = live[int(rng.integers(0, len(live)))]
                first, n = f0, n0 + 1                                                       # a live extent and one unit more: free, or the range's end,
                if first + n <= UNITS and m.used[first + n - 1]:                            # or somebody else's unit, which only the owner's
                    continue                                                                # bookkeeping could tell: not the allocator's to refuse
            assert not m.release(first, n)
            ops.append(f"r {first} {n}")
            want.append("r 0 %d %d" % m.stats())
    return ops, want


def test_sequence_reaches_every_refusal():
    """The seeded sequence holds refused releases that start strictly inside a free extent, at its first unit, and outside the range."""
    m, inside, at_first, outside = Model(UNITS), 0, 0, 0
    ops, want = _sequence(20261, 4000)
    for o, w_ in zip(ops[1:], want[1:]):
        a = [int(v) for v in o.split()[1:]]
        if o[0] == "t":
            m.take(a[0])
        elif w_.startswith("r 1"):
            assert m.release(*a)
        else:
            runs = m.runs()
            inside += any(f < a[0] < f + k for f, k in runs)
            at_first += any(f == a[0] for f, k in runs)
            outside += a[0] < 0 or a[0] + a[1] > UNITS
    assert inside > 20 and at_first > 20 and outside > 20, (inside, at_first, outside)


def test_model_is_first_fit():
    """The model itself on a hand-made case: the lowest extent that fits, merge on release, the figures info() reports."""
    m = Model(10)
    assert [m.take(3), m.take(2), m.take(2)] == [0, 3, 5] and m.stats() == (3, 3)
    assert m.release(3, 2) and m.stats() == (5, 3) and m.take(3) == 7 and m.take(2) == 3
    assert m.release(0, 3) and m.release(3, 2) and m.runs() == [[0, 5]] and not m.release(0, 1)


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("extent") / "extent_alloc_main")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan",
           "-static-libubsan", os.path.join(HERE, "extent_alloc_main.cpp"), "-o", exe]
    built = subprocess.run(cmd, capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
    return exe


def test_seeded_sequence_under_sanitizers(driver, tmp_path):
    ops, want = _sequence(20261, 4000)
    assert sum(o.startswith("t") for o in ops) > 1500 and sum(w.startswith("r 1") for w in want) > 1000
    assert sum(w.startswith("r 0") for w in want) > 100 and sum(w.startswith("t -1") for w in want) > 100
    path = tmp_path / "ops.txt"
    path.write_text("\n".join(ops) + "\n")
    run = subprocess.run([driver, str(path)], capture_output=True, text=True)
    assert run.returncode == 0 and "ERROR" not in run.stderr, run.stdout[-2000:] + run.stderr
    got = run.stdout.split("\n")
    assert got[len(want)] == f"replayed {len(ops)} operations"
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, (i, ops[i], g, w)


def test_the_resident_bank_tests_sequence(driver, tmp_path):
    """The extents tests/test_resident_bank.py expects, in units: A 3, B 2, C 2; retire B; D 2 lands there; E 1, F 1; retire A; B 2 lands in
    A's extent and leaves one unit; a further 2 units: refused with 2 units free, the largest extent 1."""
    ops = ["u 10", "t 3", "t 2", "t 2", "r 3 2", "t 2", "t 1", "t 1", "r 0 3", "t 2", "t 2"]
    path = tmp_path / "ops.txt"
    path.write_text("\n".join(ops) + "\n")
    run = subprocess.run([driver, str(path)], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.split("\n")[:11] == ["u", "t 0 7 7", "t 3 5 5", "t 5 3 3", "r 1 5 3", "t 3 3 3", "t 7 2 2", "t 8 1 1", "r 1 4 3", "t 0 2 1",
                                           "t -1 2 1"]
