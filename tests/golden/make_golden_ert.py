#!/usr/bin/env python3
"""Golden vectors of PreambleSamplerBlock and ManchesterDecoderBlock, converted from the reference's committed ``*.gen.lua`` with
make_golden.py's parser.

Run in the build container (needs the reference tree, LUARADIO_REFERENCE):

    python tests/golden/make_golden_ert.py

Same schema as make_golden.py; Bit vectors (the preamble argument included) come out as {"type": "Bit", "data": [0, 1, ...]}.
"""
import gzip
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_golden import HERE, REF, parse_block_spec  # noqa: E402

SPECS = [
    "blocks/signal/preamblesampler_spec",
    "blocks/signal/manchesterdecoder_spec",
]


def main():
    for spec in SPECS:
        with open(os.path.join(REF, "tests", spec + ".gen.lua")) as f:
            doc = parse_block_spec(f.read())
        doc["source"] = "tests/" + spec + ".gen.lua"
        out = os.path.join(HERE, os.path.basename(spec) + ".json.gz")
        with gzip.GzipFile(out, "wb", mtime=0) as f:       # mtime=0: byte-stable across regenerations
            f.write(json.dumps(doc, separators=(",", ":")).encode())
        print("%-55s -> %s (%d entries)" % (doc["source"], os.path.basename(out), len(doc["vectors"])))


if __name__ == "__main__":
    sys.exit(main())
