#!/usr/bin/env python3
"""Golden vectors of SignalSource, converted from the reference's committed ``tests/blocks/sources/signal_spec.gen.lua`` with make_golden.py's
parser.  (UniformRandomSource has no spec in the reference: its values are LuaJIT's math.random.)

Run in the build container (needs the reference tree, LUARADIO_REFERENCE):

    python tests/golden/make_golden_sources.py

signalsource_spec: the schema of make_golden.py; every vector has no inputs, the arguments (signal, frequency, rate, {amplitude, offset, phase})
and one output of 256 samples.
"""
import gzip
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_golden import HERE, REF, parse_block_spec  # noqa: E402

SPECS = [
    ("blocks/sources/signal_spec", "signalsource_spec"),
]


def write(doc, name):
    out = os.path.join(HERE, name + ".json.gz")
    with gzip.GzipFile(out, "wb", mtime=0) as f:       # mtime=0: byte-stable across regenerations
        f.write(json.dumps(doc, separators=(",", ":")).encode())
    print("%-55s -> %s (%d entries)" % (doc["source"], os.path.basename(out), len(doc["vectors"])))


def main():
    for spec, name in SPECS:
        with open(os.path.join(REF, "tests", spec + ".gen.lua")) as f:
            doc = parse_block_spec(f.read())
        doc["source"] = "tests/" + spec + ".gen.lua"
        write(doc, name)


if __name__ == "__main__":
    sys.exit(main())
