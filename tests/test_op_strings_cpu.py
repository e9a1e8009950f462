"""Every op string of lrhip_unary_create goes through one reader (luaradio_amd/csrc/op_string.h).  The corpus of tests/helpers/op_string_corpus.py
- per head a well-formed string with and without its optional keys and one string per single defect - is held to what the library answered
BEFORE that reader existed, recorded in tests/golden/op_strings_before.json: a string refused then is refused now, in front of the device, with
the same message up to the quoted op string; a string accepted then is accepted now.  tools/host_op_string_check.cpp walks the same corpus and
every prefix of it through the reader alone."""
import os
import shutil
import subprocess

import pytest

from luaradio_amd import _lib
from tests.helpers import op_string_corpus as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CORPUS = C.corpus()


@pytest.fixture(scope="module")
def before():
    return C.before()


def test_the_record_covers_the_corpus(before):
    assert [C.key(op) for op in CORPUS] == list(before) and len(CORPUS) > 600
    heads = {op.split(":")[0] for op in CORPUS}
    assert set(C.HEADS) | set(C.PLAIN) | set(C.ELEMENTWISE) | {"nosuchoperation"} <= heads and len(C.HEADS) + len(C.PLAIN) + len(C.ELEMENTWISE) == 32
    # per head: a string the readers accepted, and each kind of refusal they share
    for head, keys in C.HEADS.items():
        mine = [m for k, (_, m) in before.items() if k.split(":")[0] == head]
        assert any(C.accepted(m) for m in mine), head
        for fragment in ("malformed parameter", "unknown parameter \"bogus\"", "given twice", "missing parameter \"%s\"" % keys[0][0]):
            assert any(fragment in m for m in mine), (head, fragment)
    for head in C.PLAIN:
        assert C.accepted(before[head][1]) and "takes no parameters" in before[head + ":x=1"][1]
    assert "unknown operation" in before["nosuchoperation"][1] and "unknown operation" in before["nosuchoperation:x=1"][1]


@pytest.mark.parametrize("head", list(C.HEADS) + ["parameterless", "other"])
def test_every_string_is_answered_as_before(before, head):
    L = _lib.load()
    mine = [op for op in CORPUS if (op.split(":")[0] == head if head in C.HEADS else
                                    op.split(":")[0] in C.PLAIN if head == "parameterless" else op.split(":")[0] not in list(C.HEADS) + C.PLAIN)]
    assert mine
    for op in mine:
        _, was = before[C.key(op)]
        rejected, message = C.ask(L, op)
        if C.accepted(was):
            # a stage came back (and was destroyed), or, without a device, the message is not one of the reader's or the stage's own rules
            assert not rejected or C.accepted(message), (op[:200], message)
        else:
            assert rejected and C.normalised(message) == C.normalised(was), (op[:200], was, message)


def test_reader_alone_on_every_prefix(tmp_path):
    """tools/host_op_string_check.cpp: nothing behind the terminator is read, and a refusal always leaves a message"""
    cxx = shutil.which("g++") or shutil.which("c++")
    if not cxx:
        pytest.skip("no C++ compiler")
    exe, listing = str(tmp_path / "host_op_string_check"), str(tmp_path / "corpus.txt")
    with open(listing, "w") as f:
        f.write("\n".join(CORPUS) + "\n")
    r = subprocess.run([cxx, "-O1", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "luaradio_amd", "csrc"), "-o", exe,
                        os.path.join(ROOT, "tools", "host_op_string_check.cpp")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([exe, listing], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip().endswith("OK"), r.stdout + r.stderr


def test_one_reader_in_the_sources():
    """the walk over the fields exists once"""
    csrc = os.path.join(ROOT, "luaradio_amd", "csrc")
    hits = [f for f in sorted(os.listdir(csrc)) if "strchr(k, '=')" in open(os.path.join(csrc, f)).read()]
    assert hits == ["op_string.h"]
