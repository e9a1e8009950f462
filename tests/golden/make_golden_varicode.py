#!/usr/bin/env python3
"""Golden vectors of VaricodeDecoderBlock, converted from the reference's committed ``tests/blocks/protocol/varicodedecoder_spec.gen.lua`` with
make_golden.py's parser.

Run in the build container (needs the reference tree, LUARADIO_REFERENCE):

    python tests/golden/make_golden_varicode.py

Same schema as make_golden.py.  The spec writes its output bytes in hexadecimal (``0x48``), which make_golden.py's parser does not read: they
are rewritten to decimal before parsing (no arithmetic happens here).  Three vectors: "Hello World", the same with an extra leading 0 bit,
and 40 zeros, which give nothing.
"""
import gzip
import json
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_golden import HERE, REF, parse_block_spec  # noqa: E402

SPEC = "blocks/protocol/varicodedecoder_spec"


def main():
    with open(os.path.join(REF, "tests", SPEC + ".gen.lua")) as f:
        text = f.read()
    text = re.sub(r"0x([0-9a-fA-F]+)", lambda m: str(int(m.group(1), 16)), text)
    doc = parse_block_spec(text)
    assert len(doc["vectors"]) == 3
    for v in doc["vectors"]:
        assert [a["type"] for a in v["inputs"]] == ["Bit"] and [a["type"] for a in v["outputs"]] == ["Byte"]
    doc["source"] = "tests/" + SPEC + ".gen.lua"
    out = os.path.join(HERE, os.path.basename(SPEC) + ".json.gz")
    with gzip.GzipFile(out, "wb", mtime=0) as f:           # mtime=0: byte-stable across regenerations
        f.write(json.dumps(doc, separators=(",", ":")).encode())
    print("%-55s -> %s (%d entries)" % (doc["source"], os.path.basename(out), len(doc["vectors"])))


if __name__ == "__main__":
    sys.exit(main())
