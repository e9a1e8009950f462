"""The corpus of op strings behind tests/test_op_strings_cpu.py and tools/host_op_string_check.cpp: for every head lrhip_unary_create knows, and
one it does not, a well-formed string with every optional key, one with none, and one string per single defect - a field without '=', an empty key,
an empty value, an unknown key, each required key missing, each key twice, and for each typed field the values of the wrong kind.

What the library answered for each string at the commit BEFORE the op strings got one reader (luaradio_amd/csrc/op_string.h) is recorded in
tests/golden/op_strings_before.json: {key(op): [rejected, message]}.  The record was made on a machine without a device, so a string the readers
accept is "rejected" there too, with the message of the device initialisation; ACCEPTED tells the two apart.  To record a library again:

    LRHIP_LIB_PATH=/path/to/liblrhip.so python -m tests.helpers.op_string_corpus > tests/golden/op_strings_before.json
"""
import hashlib
import json
import os
import re

GOLDEN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "golden", "op_strings_before.json")

# the fragments by which a message of the readers is told from any other (the device's, out of memory)
PARSER_FRAGMENTS = ("malformed parameter", "unknown parameter", "given twice", "missing parameter", "bad value for", "bad tap", "bad table entry",
                    "with a comma", "takes no parameters", "unknown operation", "must be", "must not", "Unsupported", "unsupported", "is empty",
                    "the table has", "needs a buffer", "0 .. 255")

JUNK = ["1x", "1e999", "x"]
NUM = JUNK + ["nan", "inf", "-inf"]                       # a double: the last three pass strtod, whether they pass the stage is its own rule
FIN = NUM                                                 # a finite double
FLAG = JUNK + ["2", "-1", "0.5", "nan"]
SEED = ["-1", "1.5", "18446744073709551616", "0x10", "+1", " 1", "1e3"]
LIST = ["1,,2", "1,2,", "1,2x", ",1", "1,2;3"]
BITS = ["0121", "01 01", "2"]
LONG_ENDS = ["-9223372036854775809", "9223372036854775808"]


def ints(lo, hi):
    """a decimal integer in [lo, hi]: the wrong kinds and one outside each end"""
    return JUNK + ["1.5", "0x10", str(lo - 1), str(hi + 1)]


# head -> [(key, required, good value, wrong values)]; wrong values that the stage's own rules refuse (a period of 0) stand next to the reader's
HEADS = {
    "zerocrossingclockrecovery": [("period", True, "8.5", NUM + ["0", "-1"]), ("threshold", True, "0.25", NUM)],
    "clocksampler": [("period", True, "8.5", NUM + ["0", "-1"]), ("threshold", True, "0.25", NUM)],
    "slicer": [("threshold", True, "0.5", NUM)],
    "differentialdecoder": [("invert", True, "1", FLAG)],
    "manchesterdecoder": [("invert", True, "1", FLAG)],
    "binaryphasecorrector": [("num_samples", True, "16", NUM + ["0", "16777217", "1.5"]), ("sample_interval", False, "8", NUM + ["0", "2147483649", "1.5"])],
    "pll": [("alpha", True, "0.1", NUM), ("beta", True, "0.01", NUM), ("fmin", True, "-0.5", NUM), ("fmax", True, "0.5", NUM), ("mult", False, "2", NUM),
            ("port", False, "error", ["bogus", "OUT", "1"]), ("segment", False, "256", NUM + ["0", "1073741825", "1.5"]),
            ("warmup", False, "64", NUM + ["0", "1073741825", "1.5"]), ("speculate", False, "0", FLAG)],
    "preamblesampler": [("period", True, "4", ints(-0x7fffffff, 0x7fffffff) + ["1"]), ("num_samples", True, "8", ints(-0x7fffffff, 0x7fffffff) + ["1"]),
                        ("preamble", True, "0101", BITS)],
    "pam": [("period", True, "4", JUNK + ["1.5", "0x10", "0", "1073741824"] + LONG_ENDS), ("bits", True, "1", JUNK + ["1.5", "0", "17"] + LONG_ENDS),
            ("msb", True, "1", JUNK + ["1.5", "2", "-1"] + LONG_ENDS), ("table", True, "1,-0x1p+0", LIST + ["1", "1,2,3"])],
    "qam": [("period", True, "1", JUNK + ["1.5", "0x10", "0", "1073741824"] + LONG_ENDS), ("bits", True, "1", JUNK + ["1.5", "0", "17"] + LONG_ENDS),
            ("msb", True, "0", JUNK + ["1.5", "2", "-1"] + LONG_ENDS), ("table", True, "1,0,-1,0.5", LIST + ["1,2"])],
    "pfbsynthesizer": [("channels", True, "8", ints(0, 1000000) + ["7", "0"]), ("oversample", True, "2", ints(0, 1000000) + ["3", "0"]),
                       ("taps", True, "1,2,3,4,5,6,7,0x1p-1,9", LIST + ["1,2,3", ",".join(["0.5"] * 65538), ",".join(["0.5"] * 65538) + ","])],
    "interleave": [("channels", True, "2", NUM + ["1", "1.5", "33"]), ("size", True, "8", NUM + ["5", "16"])],
    "deinterleave": [("channels", True, "3", NUM + ["1", "1.5", "33"]), ("size", True, "4", NUM + ["5", "16"])],
    "wavpack": [("channels", True, "1", NUM + ["0", "1.5", "33"]), ("bits", True, "16", NUM + ["12", "4"])],
    "wavunpack": [("channels", True, "2", NUM + ["0", "1.5", "33"]), ("bits", True, "8", NUM + ["12", "64"])],
    "signalsource": [("signal", True, "sine", ["noise", "Sine"]), ("frequency", True, "1", FIN), ("rate", True, "2", FIN + ["0", "-1"]),
                     ("amplitude", True, "1.5", FIN), ("phase", True, "0.25", FIN), ("offset", True, "-0.5", FIN)],
    "uniformrandomsource": [("type", True, "byte", ["f64", "Byte"]), ("lo", True, "65", FIN + ["-1", "0.5", "91"]), ("hi", True, "90", FIN + ["256", "64"]),
                            ("seed", True, "18446744073709551615", SEED)],
}
PLAIN = ["rdsframer", "scmframer", "scmplusframer", "idmframer", "ax25framer", "pocsagframer", "varicodedecoder"]
ELEMENTWISE = ["complexmagnitude", "complexphase", "complextoreal", "complextoimag", "complexconjugate", "realtocomplex", "absolutevalue", "addconstant"]


def join(head, fields):
    return ":".join([head] + ["%s=%s" % kv for kv in fields])


def corpus():
    """the op strings, each once, in a fixed order"""
    ops = []
    for head, keys in HEADS.items():
        full = [(k, good) for k, _, good, _ in keys]
        ops.append(join(head, full))
        ops.append(join(head, [(k, good) for k, req, good, _ in keys if req]))
        ops.append(join(head, full[::-1]))                                     # the order of the fields is free
        ops.append(join(head, full) + ":" + keys[0][0])                        # no '='
        ops.append(join(head, full) + ":")
        ops.append(head + ":" + keys[0][0] + ":" + join("", full)[1:])         # the '=' of the first field lies behind the next ':'
        ops.append(join(head, full) + ":=1")                                   # empty key
        ops.append(join(head, full) + ":bogus=1")                              # unknown key
        ops.append(join(head, full) + ":" + keys[0][0].upper() + "=1")
        ops.append(head)                                                       # every key missing
        for i, (k, req, good, wrong) in enumerate(keys):
            ops.append(join(head, full[:i] + full[i + 1:]))                    # this key missing
            ops.append(join(head, full) + ":%s=%s" % (k, good))                # this key twice
            for w in [""] + wrong:
                ops.append(join(head, full[:i] + [(k, w)] + full[i + 1:]))
    for head in PLAIN:
        ops += [head, head + ":x=1", head + ":", head + ":x"]
    for head in ELEMENTWISE + ["nosuchoperation", ""]:
        ops += [head + ":x=1", head + ":"]
    ops += ["nosuchoperation", "slicer2:threshold=1", "slice:threshold=1"]
    return list(dict.fromkeys(ops))


def key(op):
    """the name an op string goes by in the record: itself, or its head and a digest if it is long"""
    return op if len(op) <= 200 else op[:60] + "...#" + hashlib.sha1(op.encode()).hexdigest()[:16]


def accepted(message):
    """the readers let the string through: the message, if any, is not one of theirs"""
    return not any(f in message for f in PARSER_FRAGMENTS)


def normalised(message):
    """a message without the quoted op string, which the readers may cut at another length, or leave out behind a missing key"""
    return re.sub(r' in ".*?"(?= \(|$)', "", message)


def ask(L, op):
    """(rejected, message) of lrhip_unary_create(op); a stage that comes back is destroyed"""
    stage = L.lrhip_unary_create(op.encode(), 0.0, 0.0, 0, 0)
    if stage:
        L.lrhip_stage_destroy(stage)
        return False, ""
    return True, L.lrhip_strerror().decode()


def before():
    with open(GOLDEN) as f:
        return json.load(f)


if __name__ == "__main__":
    from luaradio_amd import _lib
    L = _lib.load()
    print(json.dumps({key(op): list(ask(L, op)) for op in corpus()}, indent=0))
