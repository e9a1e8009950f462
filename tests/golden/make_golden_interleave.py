#!/usr/bin/env python3
"""Golden vectors of InterleaveBlock, DeinterleaveBlock and WAVFileSource, converted from the reference's committed ``*.gen.lua`` with
make_golden.py's parser, and the expected headers of the reference's WAVFileSink spec.

Run in the build container (needs the reference tree, LUARADIO_REFERENCE):

    python tests/golden/make_golden_interleave.py

interleave_spec, deinterleave_spec, wavfilesource_spec: the schema of make_golden.py.  The source's first argument is an in-memory file
(``require('tests.buffer').open("\\x..")``), kept as ``{"type": "bytes", "hex": ...}`` as in iqfile_spec.

wavfilesink_headers: ``{"kind": "raw", "values": {"<bits>_<channels>": {"type": "bytes", "hex": ...}}}`` - the six 44-byte headers the sink
spec (tests/blocks/sinks/wavfile_spec.lua, hand-written, not generated) expects after 256 samples per channel at 44100 Hz.
"""
import gzip
import json
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_golden import HERE, REF, parse_block_spec  # noqa: E402

SPECS = [
    ("blocks/signal/interleave_spec", "interleave_spec"),
    ("blocks/signal/deinterleave_spec", "deinterleave_spec"),
    ("blocks/sources/wavfile_spec", "wavfilesource_spec"),
]
SINK_SPEC = "blocks/sinks/wavfile_spec.lua"


def write(doc, name):
    out = os.path.join(HERE, name + ".json.gz")
    with gzip.GzipFile(out, "wb", mtime=0) as f:       # mtime=0: byte-stable across regenerations
        f.write(json.dumps(doc, separators=(",", ":")).encode())
    n = len(doc["vectors"]) if doc["kind"] == "block" else len(doc["values"])
    print("%-55s -> %s (%d entries)" % (doc["source"], os.path.basename(out), n))


def sink_headers(text):
    """the `headers` table of the sink spec: [bits] = { [channels] = "\\x52\\x49..." }"""
    body = text[text.index("local headers = {"):text.index("local test_vectors")]
    values = {}
    for bits, inner in re.findall(r"\[(\d+)\]\s*=\s*\{(.*?)\n\s*\},", body, re.S):
        for channels, esc in re.findall(r"\[(\d+)\]\s*=\s*\"((?:\\x[0-9a-fA-F]{2})+)\"", inner):
            raw = bytes(int(h, 16) for h in re.findall(r"\\x([0-9a-fA-F]{2})", esc))
            assert len(raw) == 44, (bits, channels, len(raw))
            values["%s_%s" % (bits, channels)] = {"type": "bytes", "hex": raw.hex()}
    assert len(values) == 6, sorted(values)
    return values


def main():
    for spec, name in SPECS:
        with open(os.path.join(REF, "tests", spec + ".gen.lua")) as f:
            doc = parse_block_spec(f.read())
        doc["source"] = "tests/" + spec + ".gen.lua"
        write(doc, name)
    with open(os.path.join(REF, "tests", SINK_SPEC)) as f:
        values = sink_headers(f.read())
    write({"kind": "raw", "values": values, "source": "tests/" + SINK_SPEC}, "wavfilesink_headers")


if __name__ == "__main__":
    sys.exit(main())
