#!/usr/bin/env python3
"""Golden vectors of PulseAmplitudeModulatorBlock and QuadratureAmplitudeModulatorBlock, converted from the reference's committed
``*.gen.lua`` with make_golden.py's parser.

Run in the build container (needs the reference tree, LUARADIO_REFERENCE):

    python tests/golden/make_golden_modulators.py

Same schema as make_golden.py.  The option argument of these blocks is a Lua table constructor in the reference
(``{amplitudes = {[0] = -2, ...}}``, ``{constellation = {[0] = radio.types.ComplexFloat32(-1, -1), ...}}``, ``{msb_first = false}``); the
fixture holds it as plain data: ``{"amplitudes": [a0, a1, ...]}`` and ``{"constellation": [[re0, im0], ...]}`` indexed by symbol value,
``{"msb_first": false}``.
"""
import gzip
import json
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_golden import HERE, REF, LuaLiteralParser  # noqa: E402

SPECS = [
    "blocks/signal/pulseamplitudemodulator_spec",
    "blocks/signal/quadratureamplitudemodulator_spec",
]


class IndexedTableParser(LuaLiteralParser):
    """... plus tables with integer keys, ``{[0] = v, [1] = w}``: a list in key order (the keys must be 0 .. n - 1)"""

    assert "[{}(),=]" in LuaLiteralParser.TOKEN.pattern           # the punctuation class this subclass widens by the two brackets
    TOKEN = re.compile(LuaLiteralParser.TOKEN.pattern.replace("[{}(),=]", r"[{}(),=\[\]]"))

    def table(self):
        if self.peek()[1] != "[":
            return LuaLiteralParser.table(self)
        entries = {}
        while self.peek()[1] != "}":
            self.take("[")
            key = self.value()
            self.take("]")
            self.take("=")
            entries[key] = self.value()
            if self.peek()[1] == ",":
                self.take(",")
        self.take("}")
        if sorted(entries) != list(range(len(entries))):
            raise ValueError("integer-keyed table with keys %r" % sorted(entries))
        return [entries[k] for k in range(len(entries))]


def plain(value):
    """ComplexFloat32 scalars inside an option table -> [re, im]"""
    if isinstance(value, dict) and "scalar" in value:
        return [float(v) for v in value["scalar"]]
    if isinstance(value, dict):
        return {k: plain(v) for k, v in value.items()}
    if isinstance(value, list):
        return [plain(v) for v in value]
    return value


def parse_spec(text):
    m = re.search(r"jigs\.TestBlock\(radio\.(\w+),\s*", text)
    p = IndexedTableParser(text, m.end())
    p.take("{")
    vectors = p.table()
    eps = re.search(r"\{epsilon = (.*)\}\)\s*$", text[p.pos:], re.S).group(1).strip()
    for v in vectors:
        v["args"] = [plain(a) if isinstance(a, dict) and "type" not in a else a for a in v["args"]]
    return {"kind": "block", "block": m.group(1), "epsilon": eps, "vectors": vectors}


def main():
    for spec in SPECS:
        with open(os.path.join(REF, "tests", spec + ".gen.lua")) as f:
            doc = parse_spec(f.read())
        doc["source"] = "tests/" + spec + ".gen.lua"
        out = os.path.join(HERE, os.path.basename(spec) + ".json.gz")
        with gzip.GzipFile(out, "wb", mtime=0) as f:       # mtime=0: byte-stable across regenerations
            f.write(json.dumps(doc, separators=(",", ":")).encode())
        print("%-55s -> %s (%d entries)" % (doc["source"], os.path.basename(out), len(doc["vectors"])))


if __name__ == "__main__":
    sys.exit(main())
