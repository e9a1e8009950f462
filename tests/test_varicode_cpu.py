"""VaricodeDecoderBlock without a GPU: the models (tests/helpers/varicode_model.py) against the reference's golden vectors, the window-function
automaton the device runs against the literal loop, the codes of 10 bits, the bound, the passes of luaradio_amd/csrc/varicode_plan.h played on
the CPU (tools/host_varicode_check.hip), and the Python mirror."""
import itertools
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import luaradio_amd as lr
from luaradio_amd import types
from tests import golden_util
from tests.helpers import varicode_model as vm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TILE = 4096                                              # DG_TILE


def text_of(y):
    return bytes(np.asarray(y, np.uint8))


@pytest.mark.parametrize("cls", [vm.VaricodeLiteral, vm.VaricodeWindow])
def test_golden_varicodedecoder_models(cls):
    vectors = golden_util.load("varicodedecoder_spec")["vectors"]
    assert [len(v["outputs"][0]) for v in vectors] == [11, 11, 0]
    for v in vectors:
        x, want = np.asarray(v["inputs"][0], np.uint8), np.asarray(v["outputs"][0], np.uint8)
        whole, samplewise = golden_util.run_whole_and_samplewise(cls, x)
        assert np.array_equal(whole, want) and np.array_equal(samplewise, want)
    assert text_of(vectors[0]["outputs"][0]) == b"Hello World"


def test_window_automaton_equals_literal_loop_exhaustively():
    """every input over {0, 1, 2} up to length 10, whole and cut in two at every place: the 21 states plus the bytes read back from the stream
    give the literal loop's characters and leave its state"""
    checked = 0
    for n in range(0, 11):
        for x in itertools.product((0, 1, 2), repeat=n):
            x = np.array(x, np.uint8)
            lit, win = vm.VaricodeLiteral(), vm.VaricodeWindow()
            assert np.array_equal(win.process(x), lit.process(x)) and win.carried == lit.state, x
            checked += 1
    assert checked == (3 ** 11 - 1) // 2
    rng = np.random.default_rng(7)
    for case in range(300):
        n = int(rng.integers(1, 200))
        x = rng.choice(np.array([0, 1, 2, 255], np.uint8), n, p=[0.45, 0.45, 0.05, 0.05])
        edges = [0] + sorted(int(c) for c in rng.integers(0, n + 1, int(rng.integers(0, 8)))) + [n]
        lit, win, whole = vm.VaricodeLiteral(), vm.VaricodeWindow(), vm.VaricodeLiteral()
        chars, at = whole.process(x), np.array(whole.positions, np.int64)
        for a, b in zip(edges[:-1], edges[1:]):
            want = lit.process(x[a:b])
            assert np.array_equal(win.process(x[a:b]), want) and win.carried == lit.state, (case, a, b)
            assert np.array_equal(want, chars[np.searchsorted(at, a):np.searchsorted(at, b)])      # the loop does not see the cuts


def test_codes_of_ten_bits_are_never_decoded():
    assert len(vm.CODE) == 128 and len(set(vm.CODE)) == 128 and len(vm.TEN_BIT) == 40
    assert set(b"%&?@Z^`{}~") <= set(vm.TEN_BIT) and not set(range(32, 127)) & set(vm.TEN_BIT) - set(b"%&?@Z^`{}~")
    for c in range(128):
        got = text_of(vm.VaricodeLiteral().process(vm.encode([c, ord("e")], lead=2)))
        if c in vm.TEN_BIT:
            assert bytes([c]) not in got or c == ord("e"), c
            assert got == b"e", (c, got)                 # a short code behind it survives
        else:
            assert got == bytes([c]) + b"e", (c, got)
    # the reset leaves the code's first delimiter zero behind: a 9-bit code right behind a lost character is lost too
    assert text_of(vm.VaricodeLiteral().process(vm.encode("!Zx"))) == b"!x"
    assert text_of(vm.VaricodeLiteral().process(vm.encode("Z!x"))) == b"x"
    assert text_of(vm.VaricodeLiteral().process(vm.encode("CQ de Zulu?"))) == b"CQ de ulu"
    assert text_of(vm.VaricodeWindow().process(vm.encode("CQ de Zulu?"))) == b"CQ de ulu"


def test_bound_holds_under_random_cuts():
    rng = np.random.default_rng(3)
    assert [vm.max_output(n) for n in (0, 1, 2, 3, 4, 5, 6, 100)] == [0, 1, 2, 3, 4, 5, 5, 36]
    worst = 0.0
    for case in range(200):
        n = int(rng.integers(1, 600))
        x = (rng.random(n) < (0.3, 0.5, 0.7)[case % 3]).astype(np.uint8)
        if case % 4 == 0:                                # the densest stream there is: 1 0 0 1 0 0 ...
            x = np.tile(np.array([1, 0, 0], np.uint8), n // 3 + 1)[:n]
        edges = [0] + sorted(int(c) for c in rng.integers(0, n + 1, int(rng.integers(0, 40)))) + [n]
        _, counts = vm.run_cuts(vm.VaricodeLiteral(), x, edges)
        for (a, b), c in zip(zip(edges[:-1], edges[1:]), counts):
            assert c <= vm.max_output(b - a), (case, a, b, c)
            if b - a >= 30:
                worst = max(worst, c / vm.max_output(b - a))
    assert worst > 0.9                                   # and it is not slack: the dense stream comes close to it


def test_random_streams_are_not_empty():
    """the floor the GPU test asserts (n / 20 characters) holds for both of its one-probabilities"""
    for p1, seed in ((0.5, 1), (0.3, 2)):
        x = (np.random.default_rng(seed).random(1 << 16) < p1).astype(np.uint8)
        assert len(vm.VaricodeLiteral().process(x)) >= len(x) // 10


def test_runs_of_ones_both_emit_and_lose_the_character():
    """R ones in front of the character `e`, then `t`: the ones left over from the last reset join the code, so what comes out depends on R
    modulo 11 - the entry states do not converge on a run of ones.  Over R the `e` is both emitted as it is and lost altogether."""
    fate = []
    for R in range(24):
        x = np.concatenate([np.zeros(2, np.uint8), np.ones(R, np.uint8), vm.encode("e", lead=0), vm.encode("t", lead=0)])
        fate.append(text_of(vm.VaricodeLiteral().process(x)))
        assert fate[-1].endswith(b"t") and len(fate[-1]) <= 2, (R, fate[-1])
    assert fate[0] == b"et" and fate.count(b"et") == 3 and fate.count(b"t") == 4
    assert fate[:13] == fate[11:]                        # periodic in R with the reset's period of 11


def test_block_mirror():
    """the CPU test that needs the feature: the block, its signature and its op, without the library"""
    blk = lr.VaricodeDecoderBlock()
    assert types.Byte.name == "Byte" and types.Byte.dtype == np.uint8 and types.Byte.size == 1 and types.Byte is not types.Bit
    assert types.type_of(np.zeros(1, np.uint8)) is types.Bit
    assert len(blk.type_signatures) == 1
    blk.differentiate([types.Bit])
    assert blk.get_input_type() is types.Bit and blk.get_output_type() is types.Byte
    assert blk.op() == "varicodedecoder"
    with pytest.raises(TypeError):
        blk.differentiate([types.Byte])
    with pytest.raises(TypeError):
        lr.VaricodeDecoderBlock(1)


def test_alphabet_equals_the_reference_table():
    ref = os.environ.get("LUARADIO_REFERENCE", "/root/reference")
    path = os.path.join(ref, "radio", "blocks", "protocol", "varicodedecoder.lua")
    if not os.path.exists(path):
        pytest.skip("no reference tree")
    with open(path) as f:
        pairs = re.findall(r"\[0x([0-9a-fA-F]+)\]\s*=\s*0x([0-9a-fA-F]+)", f.read())
    assert len(pairs) == 128
    assert {int(v, 16): int(k, 16) for k, v in pairs} == dict(enumerate(vm.CODE))


def test_varicode_passes_on_the_cpu(tmp_path):
    """per-thread maps over 16-byte chunks, their composition per tile and over tiles, the replay from the composed entry states: the functions
    the kernels call, driven by host loops, against a plain copy of the literal loop (characters and final state)"""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    exe = str(tmp_path / "host_varicode_check")
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O1", "-std=c++17", "-Wno-unused-function", "-I", os.path.join(ROOT, "luaradio_amd", "csrc"),
                        "-I", os.path.join(ROOT, "include"), "-o", exe, os.path.join(ROOT, "tools", "host_varicode_check.hip")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("OK"), r.stdout[-4000:] + r.stderr[-2000:]
