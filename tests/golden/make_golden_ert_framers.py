#!/usr/bin/env python3
"""Golden vectors of SCMFramerBlock, SCMPlusFramerBlock and IDMFramerBlock, converted from the reference's committed
``tests/blocks/protocol/{scm,scmplus,idm}framer_spec.gen.lua`` with make_golden.py's parser.

Run in the build container (needs the reference tree, LUARADIO_REFERENCE):

    python tests/golden/make_golden_ert_framers.py

Same schema as make_golden.py.  The specs write their outputs as ``require('radio.blocks.protocol.scmframer').SCMFrameType.vector_from_array(
{{field, ...}, ...})`` with hexadecimal numbers, and IDM's byte-string fields as "\\x02\\x00...": the constructor name, the numbers and the
strings are rewritten to forms make_golden.py's parser knows before parsing (a string becomes the table of its byte values; no arithmetic
happens here).  Each output is {"type": name, "frames": [frame, ...]}, a frame being the list of the frame type's constructor arguments in the
constructor's order:
  SCMFrameType      ert_type, ert_id, consumption, physical_tamper, encoder_tamper, reserved, crc
  SCMPlusFrameType  protocol_id, ert_type, ert_id, consumption, tamper, crc
  IDMFrameType      application_version, ert_type, ert_id, consumption_interval_count, module_programming_state, tamper_count[6], async_count[2],
                    power_outage_flags[6], last_consumption_count, differential_consumption_intervals[53], transmit_time_offset, serial_crc,
                    packet_crc
"""
import gzip
import json
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_golden import HERE, REF, parse_block_spec  # noqa: E402

SPECS = (("blocks/protocol/scmframer_spec", "scmframer", "SCMFrameType", 7),
         ("blocks/protocol/scmplusframer_spec", "scmplusframer", "SCMPlusFrameType", 6),
         ("blocks/protocol/idmframer_spec", "idmframer", "IDMFrameType", 13))


def _string_to_table(m):
    body = m.group(1)
    values = re.findall(r"\\x([0-9a-fA-F]{2})", body)
    assert "".join("\\x" + v for v in values) == body, body
    return "{" + ", ".join(str(int(v, 16)) for v in values) + "}"


def main():
    for spec, module, type_name, nfields in SPECS:
        with open(os.path.join(REF, "tests", spec + ".gen.lua")) as f:
            text = f.read()
        text = text.replace("require('radio.blocks.protocol.%s').%s.vector_from_array" % (module, type_name),
                            "radio.types.%s.vector_from_array" % type_name)
        text = re.sub(r'"((?:\\x[0-9a-fA-F]{2})+)"', _string_to_table, text)
        text = re.sub(r"0x([0-9a-fA-F]+)", lambda m: str(int(m.group(1), 16)), text)
        doc = parse_block_spec(text)
        for v in doc["vectors"]:
            for out in v["outputs"]:
                assert out["type"] == type_name
                out["frames"] = out.pop("data")       # not "data": IDM's frames are ragged lists, which golden_util.load() must leave alone
                assert all(len(frame) == nfields for frame in out["frames"])
        doc["source"] = "tests/" + spec + ".gen.lua"
        out = os.path.join(HERE, os.path.basename(spec) + ".json.gz")
        with gzip.GzipFile(out, "wb", mtime=0) as f:           # mtime=0: byte-stable across regenerations
            f.write(json.dumps(doc, separators=(",", ":")).encode())
        print("%-55s -> %s (%d entries)" % (doc["source"], os.path.basename(out), len(doc["vectors"])))


if __name__ == "__main__":
    sys.exit(main())
