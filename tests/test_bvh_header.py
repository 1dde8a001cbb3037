"""read_bvh_header / mocha_bvh_header (csrc/bvh_header.cpp): the hierarchy of the three fixture files against what the reference's loader
returned (tests/golden/bvh_parse.npz), every refusal the header documents on an authored text, and a run of the parser under the address
and undefined-behaviour sanitizers as a stand-alone host program (tests/bvh_header_main.cpp: every byte-length prefix of every fixture
file's header region, each in an exactly sized heap buffer).  No GPU: the parser needs no context."""
import os
import subprocess

import numpy as np
import pytest

from mocha_sigasia2023_amd import read_bvh_header

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLDEN = os.path.join(HERE, "golden")
TAGS = ("mocha24_rot", "mocha24_pos", "mixamo22")
FILES = [os.path.join(GOLDEN, "bvh", t + ".bvh") for t in TAGS]


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(os.path.join(GOLDEN, "bvh_parse.npz")))


@pytest.mark.parametrize("tag", TAGS)
def test_header_equals_the_reference(gold, tag):
    path = os.path.join(GOLDEN, "bvh", tag + ".bvh")
    with open(path, "rb") as f:
        text = f.read()
    for h in (read_bvh_header(path), read_bvh_header(text)):
        assert h.names == [str(n) for n in gold[f"{tag}_names"]]
        assert np.array_equal(h.parents, gold[f"{tag}_parents"])
        assert h.offsets.dtype == np.float64 and np.array_equal(h.offsets.view(np.uint64), gold[f"{tag}_offsets"].view(np.uint64))
        assert h.order == str(gold[f"{tag}_order"])
        assert h.channels == (6 if tag == "mocha24_pos" else 3)
        assert h.frames == gold[f"{tag}_rotations"].shape[0] == 40
        assert h.frametime == float(gold[f"{tag}_frametime"])
        # the numeric block starts at the first motion line, right behind the Frame Time: line, and runs to the end of the file
        line = text.index(b"Frame Time:")
        assert h.motion_begin == text.index(b"\n", line) + 1 and h.motion_end == len(text)
        first = text[h.motion_begin:].split(b"\n", 1)[0].split()
        assert len(first) == (6 * len(h.names) if h.channels == 6 else 3 + 3 * len(h.names))
        assert float(first[0]) == gold[f"{tag}_positions"][0, 0, 0]


def _bvh(root_channels="CHANNELS 6 Xposition Yposition Zposition Zrotation Yrotation Xrotation", a="CHANNELS 3 Zrotation Yrotation Xrotation",
         b="CHANNELS 3 Zrotation Yrotation Xrotation", motion="MOTION\n", frames="Frames: 2\n", frametime="Frame Time: 0.016667\n",
         close="}\n", extra=""):
    return ("HIERARCHY\nROOT mixamorig:Hips\n{\n\tOFFSET 0.0 1.5 -2e0\n\t" + root_channels + "\n"
            "\tJOINT A\n\t{\n\t\tOFFSET 1 2 3\n\t\t" + a + "\n\t\tEnd Site\n\t\t{\n\t\t\tOFFSET 9 9 9\n\t\t}\n\t}\n"
            "\tJOINT B\n\t{\n\t\tOFFSET 4 5 6\n\t\t" + b + "\n" + extra + "\t}\n" + close + motion + frames + frametime
            + "0 0 0 1 2 3 4 5 6 7 8 9\n0 0 0 1 2 3 4 5 6 7 8 9\n").encode()


def test_authored_text_is_read():
    text = _bvh()
    h = read_bvh_header(text)
    assert h.names == ["mixamorig:Hips", "A", "B"] and h.parents.tolist() == [-1, 0, 0] and h.order == "zyx" and h.channels == 3
    assert h.offsets.tolist() == [[0.0, 1.5, -2.0], [1.0, 2.0, 3.0], [4.0, 5.0, 6.0]]          # the End Site's 9 9 9 is dropped
    assert h.frames == 2 and h.frametime == 0.016667 and text[h.motion_begin:].startswith(b"0 0 0 1")
    crlf = read_bvh_header(text.replace(b"\n", b"\r\n").replace(b"\t", b"  "))
    assert crlf.names == h.names and crlf.frames == 2 and crlf.offsets.tolist() == h.offsets.tolist()
    six = "CHANNELS 6 Xposition Yposition Zposition Xrotation Yrotation Zrotation"
    h6 = read_bvh_header(_bvh(root_channels=six, a=six, b=six))
    assert h6.channels == 6 and h6.order == "xyz"


REFUSED = {
    "nine channels": dict(a="CHANNELS 9 Xposition Yposition Zposition Zrotation Yrotation Xrotation Xscale Yscale Zscale"),
    "positions out of order": dict(root_channels="CHANNELS 6 Yposition Xposition Zposition Zrotation Yrotation Xrotation"),
    "rotation order disagrees": dict(b="CHANNELS 3 Xrotation Yrotation Zrotation"),
    "channel count disagrees": dict(b="CHANNELS 6 Xposition Yposition Zposition Zrotation Yrotation Xrotation"),
    "root with three channels": dict(root_channels="CHANNELS 3 Zrotation Yrotation Xrotation"),
    "no MOTION": dict(motion=""),
    "no Frames": dict(frames=""),
    "no Frame Time": dict(frametime=""),
    "brace missing": dict(close=""),
    "brace too many": dict(close="}\n}\n"),
    "too many joints": dict(extra="".join("\t\tJOINT X%d\n\t\t{\n\t\t\tOFFSET 0 0 0\n\t\t\tCHANNELS 3 Zrotation Yrotation Xrotation\n\t\t}\n" % i
                                          for i in range(254))),
}


@pytest.mark.parametrize("what", sorted(REFUSED))
def test_refusals(what):
    text = _bvh(**REFUSED[what])
    with pytest.raises(ValueError, match="byte") as e:
        read_bvh_header(text)
    at = int(str(e.value).rsplit("byte ", 1)[1].rstrip(")"))
    assert 0 <= at <= len(text) and (at == len(text) or at == 0 or text[at - 1:at] == b"\n")          # the first byte of a line
    if what == "nine channels":
        assert text[at:].lstrip().startswith(b"CHANNELS 9")
    if what == "too many joints":
        assert text[at:].lstrip().startswith(b"JOINT X253")
    if what == "rotation order disagrees":
        assert text[at:].lstrip().startswith(b"CHANNELS 3 Xrotation")


def test_256_joints_are_read():
    kw = dict(REFUSED["too many joints"])
    kw["extra"] = kw["extra"][: kw["extra"].index("\t\tJOINT X253")]
    h = read_bvh_header(_bvh(**kw).replace(b"7 8 9\n", b"7 8 9" + b" 0" * (3 * 253) + b"\n"))
    assert len(h.names) == 256 and h.parents[-1] == 2


def test_text_that_ends_inside_the_hierarchy():
    text = _bvh()
    for cut in (text.index(b"JOINT B"), text.index(b"End Site") + 12, text.index(b"MOTION") - 2):
        with pytest.raises(ValueError):
            read_bvh_header(text[:cut])


def test_header_parser_under_sanitizers(tmp_path):
    """The parser and a driver with its own main, compiled by g++ with the address and undefined-behaviour sanitizers linked statically,
    run once as a child process: nothing is loaded into Python."""
    exe = str(tmp_path / "bvh_header_main")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan",
           "-static-libubsan", os.path.join(HERE, "bvh_header_main.cpp"), os.path.join(ROOT, "mocha_sigasia2023_amd", "csrc", "bvh_header.cpp"),
           "-o", exe]
    built = subprocess.run(cmd, capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
    run = subprocess.run([exe] + FILES, capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.count("prefixes accepted") == len(FILES) and "ERROR" not in run.stderr, run.stdout + run.stderr
