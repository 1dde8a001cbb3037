"""csrc/fmt_f6.h, the "%f" of a float64 in integers that the device's BVH writer and the host share, as a host program: the header and a
driver with its own main (tests/fmt_f6_main.cpp) are compiled by g++ alone (no HIP header) with the address and undefined-behaviour
sanitizers linked statically and run once as a child process - nothing is loaded into Python.  The driver compares every token with
snprintf("%f") over the hard list (zero and its negation, the neighbourhood of half a unit, denormals, the ties j / 2^k for k = 7..20,
carries into a new digit, every integer-digit count 1..12, nextafter(1e12, 0)) and 2 000 000 seeded values (random sign and mantissa,
binary exponent uniform in -40 .. 39; the top of the last binade lies above 1e12 and must be refused), formats each into an exactly
sized heap buffer, and checks that NaN, +-inf and |x| >= 1e12 are reported as refused with nothing written.  No GPU."""
import os
import re
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
HEADER = os.path.join(os.path.dirname(HERE), "mocha_sigasia2023_amd", "csrc", "fmt_f6.h")


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("fmt_f6") / "fmt_f6_main")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan",
           "-static-libubsan", os.path.join(HERE, "fmt_f6_main.cpp"), "-o", exe]
    built = subprocess.run(cmd, capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
    return exe


def test_header_needs_no_hip():
    text = open(HEADER).read()
    assert "hip/" not in text and "#include <stdint.h>" in text and "__host__ __device__" in text


def test_every_token_equals_snprintf_under_sanitizers(driver):
    run = subprocess.run([driver, "20261", "2000000"], capture_output=True, text=True)
    assert run.returncode == 0 and "ERROR" not in run.stderr and "MISMATCH" not in run.stdout and "NOT REFUSED" not in run.stdout, \
        run.stdout[-2000:] + run.stderr[-2000:]
    m = re.fullmatch(r"checked (\d+) tokens, (\d+) refusals\n", run.stdout)
    assert m, run.stdout[-500:]
    checked, refused = int(m.group(1)), int(m.group(2))
    assert checked + refused > 2000000 + 200 and checked > 1990000       # the hard list twice over, the random stream
    assert 14 < refused < 10000                                        # the fixed refusals and the random values of [1e12, 2^40)
