#!/usr/bin/env python3
"""Golden vectors of RDSFramerBlock, converted from the reference's committed ``tests/blocks/protocol/rdsframer_spec.gen.lua`` with
make_golden.py's parser.

Run in the build container (needs the reference tree, LUARADIO_REFERENCE):

    python tests/golden/make_golden_rds.py

Same schema as make_golden.py.  The spec writes its outputs as ``require('radio.blocks.protocol.rdsframer').RDSFrameType.vector_from_array(
{{{{0x3aab, ...}}}, ...})`` with hexadecimal words, neither of which make_golden.py's parser reads: both are rewritten to the forms it knows
before parsing (no arithmetic happens here), and each frame's ``{{{a, b, c, d}}}`` (the struct, its blocks field, the array) comes out as
{"type": "RDSFrameType", "data": [[a, b, c, d], ...]}.
"""
import gzip
import json
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_golden import HERE, REF, parse_block_spec  # noqa: E402

SPEC = "blocks/protocol/rdsframer_spec"


def main():
    with open(os.path.join(REF, "tests", SPEC + ".gen.lua")) as f:
        text = f.read()
    text = text.replace("require('radio.blocks.protocol.rdsframer').RDSFrameType.vector_from_array", "radio.types.RDSFrameType.vector_from_array")
    text = re.sub(r"0x([0-9a-fA-F]+)", lambda m: str(int(m.group(1), 16)), text)
    doc = parse_block_spec(text)
    for v in doc["vectors"]:
        for out in v["outputs"]:
            assert out["type"] == "RDSFrameType"
            out["data"] = [frame[0][0] for frame in out["data"]]
            assert all(len(words) == 4 for words in out["data"])
    doc["source"] = "tests/" + SPEC + ".gen.lua"
    out = os.path.join(HERE, os.path.basename(SPEC) + ".json.gz")
    with gzip.GzipFile(out, "wb", mtime=0) as f:           # mtime=0: byte-stable across regenerations
        f.write(json.dumps(doc, separators=(",", ":")).encode())
    print("%-55s -> %s (%d entries)" % (doc["source"], os.path.basename(out), len(doc["vectors"])))


if __name__ == "__main__":
    sys.exit(main())
