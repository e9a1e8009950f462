#!/usr/bin/env python3
"""Golden vectors of AX25FramerBlock and POCSAGFramerBlock, converted from the reference's committed
``tests/blocks/protocol/{ax25,pocsag}framer_spec.gen.lua`` with make_golden.py's parser.

Run in the build container (needs the reference tree, LUARADIO_REFERENCE):

    python tests/golden/make_golden_packet_framers.py

Same schema as make_golden.py.  The specs write their outputs as ``require('radio.blocks.protocol.ax25framer').AX25FrameType.vector_from_array(
{{field, ...}, ...})`` with hexadecimal numbers: the constructor name and the numbers are rewritten to forms make_golden.py's parser knows
before parsing (no arithmetic happens here).  Each output is {"type": name, "frames": [frame, ...]}, a frame being the list of the frame
type's constructor arguments in the constructor's order:
  AX25FrameType     addresses [{"callsign": str, "ssid": int}, ...], control, pid, payload (str)
  POCSAGFrameType   address, func, data [word, ...]
"""
import gzip
import json
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_golden import HERE, REF, parse_block_spec  # noqa: E402

SPECS = (("blocks/protocol/ax25framer_spec", "ax25framer", "AX25FrameType", 4, 5),
         ("blocks/protocol/pocsagframer_spec", "pocsagframer", "POCSAGFrameType", 3, 6))


def main():
    for spec, module, type_name, nfields, nvectors in SPECS:
        with open(os.path.join(REF, "tests", spec + ".gen.lua")) as f:
            text = f.read()
        text = text.replace("require('radio.blocks.protocol.%s').%s.vector_from_array" % (module, type_name),
                            "radio.types.%s.vector_from_array" % type_name)
        text = re.sub(r"0x([0-9a-fA-F]+)", lambda m: str(int(m.group(1), 16)), text)
        doc = parse_block_spec(text)
        assert len(doc["vectors"]) == nvectors
        for v in doc["vectors"]:
            for out in v["outputs"]:
                assert out["type"] == type_name
                out["frames"] = out.pop("data")       # not "data": the frames are ragged lists, which golden_util.load() must leave alone
                assert all(len(frame) == nfields for frame in out["frames"])
        doc["source"] = "tests/" + spec + ".gen.lua"
        out = os.path.join(HERE, os.path.basename(spec) + ".json.gz")
        with gzip.GzipFile(out, "wb", mtime=0) as f:           # mtime=0: byte-stable across regenerations
            f.write(json.dumps(doc, separators=(",", ":")).encode())
        print("%-55s -> %s (%d entries)" % (doc["source"], os.path.basename(out), len(doc["vectors"])))


if __name__ == "__main__":
    sys.exit(main())
