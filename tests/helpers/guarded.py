"""One device call inside guard words (tests/test_gpu_bounds.py; the checks alone, on numpy arrays: tests/test_guarded_cpu.py).

Every buffer is one allocation laid out as [G guard | offset | payload | G guard].  The whole output allocation, payload included, is filled with the
sentinel 0xFFC0DE5A (a quiet-NaN payload no kernel computes) before each call; the input guards, the offset bytes and the payload behind the call's
n samples are filled once with a hostile pattern (the sentinel for sample streams, 0xFF for Bit / Byte streams and raw records) and once with finite
data (random floats, 0x00, 0x7F).  A stream is sent as consecutive calls on one object, each starting at the same address.

Checks per call (each reports the first offending 32-bit word, or byte for outputs narrower than a word, relative to `out`):
  (a) no byte before `out` changed              (b) no byte at or after out + count * out_size changed
  (c) no word of [0, count) still holds the sentinel and every float there is finite
  (d) the input allocations are byte-identical before and after
and per stream: (e) the hostile and the finite run give the same bytes, (f) the outputs meet the caller's oracle.

The memory and the call are arguments, so the same code runs a numpy fake on the CPU and liblrhip.so on the GPU."""
import numpy as np

SENT = np.uint32(0xFFC0DE5A)
SENT_BYTES = np.frombuffer(np.array([SENT], "<u4").tobytes(), np.uint8)
G_WORDS = 4096
G = 4 * G_WORDS                      # guard bytes per side

# input kinds -> (hostile fill, finite fill); "float" fills words, the others bytes
FILLS = {"float": (None, None), "bits": (0xFF, 0x00), "raw": (0xFF, 0x7F)}


class GuardViolation(AssertionError):
    pass


def sentinel_fill(nbytes):
    assert nbytes % 4 == 0
    return np.tile(SENT_BYTES, nbytes // 4)


def _first(mask):
    return int(np.argmax(mask)) if mask.any() else None


def _where(byte_index, lo):
    """a byte index of the allocation as an offset from `out` (the allocation's byte lo): whole words, rounded towards minus infinity"""
    return "word %d (byte %d) relative to the pointer" % ((byte_index - lo) // 4, byte_index - lo)


def check_before(alloc, lo, what="out"):
    """(a) alloc[:lo] is still the sentinel"""
    i = _first(alloc[:lo] != sentinel_fill(len(alloc))[:lo])
    if i is not None:
        raise GuardViolation("(a) write before %s: %s" % (what, _where(i, lo)))


def check_after(alloc, lo, nbytes, what="out"):
    """(b) alloc[lo + nbytes:] is still the sentinel (the words between the count and the capacity included)"""
    hi = lo + nbytes
    i = _first(alloc[hi:] != sentinel_fill(len(alloc))[hi:])
    if i is not None:
        raise GuardViolation("(b) write at or after the count of %d bytes of %s: %s" % (nbytes, what, _where(hi + i, lo)))


def check_written(alloc, lo, nbytes, out_size, floats, what="out"):
    """(c) every sample of [0, count) was written: no 32-bit word of it is the sentinel (a sample of 4 bytes or more: each of its words, at
    whatever alignment the pointer has; narrower samples: each aligned word of the allocation that lies inside), and every float is finite"""
    got = alloc[lo:lo + nbytes]
    if out_size % 4 == 0:
        w = np.frombuffer(got.tobytes(), "<u4")
        phase = lo % 4                                # the sentinel as seen through a pointer that is not word-aligned
        pat = np.frombuffer(np.roll(SENT_BYTES, -phase).tobytes(), "<u4")[0]
        i = _first(w == pat)
        if i is not None:
            raise GuardViolation("(c) unwritten sample %d of %s: word %d relative to the pointer" % (4 * i // out_size, what, i))
        if floats:
            i = _first(~np.isfinite(np.frombuffer(got.tobytes(), floats)))
            if i is not None:
                raise GuardViolation("(c) non-finite float %d of %s" % (i, what))
    else:
        a, b = -(-lo // 4) * 4, (lo + nbytes) // 4 * 4
        if b > a:
            i = _first(np.frombuffer(alloc[a:b].tobytes(), "<u4") == SENT)
            if i is not None:
                raise GuardViolation("(c) unwritten bytes of %s: %s" % (what, _where(a + 4 * i, lo)))


def check_input_untouched(before, after, lo, what="in"):
    """(d) the input allocation is byte-identical"""
    i = _first(before != after)
    if i is not None:
        raise GuardViolation("(d) %s modified: %s" % (what, _where(i, lo)))


def check_same(hostile, finite):
    """(e) per call, the bytes of a run with hostile guards equal those of a run with finite guards"""
    assert len(hostile) == len(finite)
    for c, (h, f) in enumerate(zip(hostile, finite)):
        if len(h) != len(f):
            raise GuardViolation("(e) call %d: %d bytes with hostile guards, %d with finite ones" % (c, len(h), len(f)))
        i = _first(h != f)
        if i is not None:
            raise GuardViolation("(e) call %d depends on bytes outside its input: first differing output word %d (byte %d)" % (c, i // 4, i))


class NumpyMemory:
    """host arrays: a handle is the array, an address is (array, byte offset)"""

    def alloc(self, nbytes):
        return np.zeros(nbytes, np.uint8)

    def write(self, h, data):
        h[:] = data

    def read(self, h):
        return h.copy()

    def addr(self, h, off):
        return (h, off)

    def sync(self):
        pass


class Buffer:
    """[G | offset | payload | G] of one stream edge"""

    def __init__(self, mem, off, payload):
        self.mem, self.off = mem, off
        self.lo = G + off
        self.size = (self.lo + payload + 3) // 4 * 4 + G
        self.h = mem.alloc(self.size)

    def addr(self):
        return self.mem.addr(self.h, self.lo)


def _input_image(size, lo, data, kind, hostile, rng):
    if kind == "float":
        img = sentinel_fill(size).copy() if hostile else np.frombuffer(rng.uniform(-1, 1, size // 4).astype("<f4").tobytes(), np.uint8).copy()
    else:
        img = np.full(size, FILLS[kind][0 if hostile else 1], np.uint8)
    img[lo:lo + len(data)] = data
    return img


def run_guarded(factory, inputs, lens, in_offset=0, out_offset=0, *, mem, call, max_output, in_kind="float", out_dtype=np.float32,
                out_floats=True, check=None, offsets_in_bytes=False, seed=0, outputs=1):
    """factory() -> a fresh block or chain; inputs: one array per input port (the whole stream); lens: the call lengths, consecutive pieces of the
    stream; in_offset / out_offset: samples (bytes with offsets_in_bytes) between the 16-byte aligned start and the pointer.
    call(obj, [input addresses], n, [output addresses], capacity) -> count runs one call (asynchronous is fine: mem.sync() follows);
    max_output(obj, n) -> capacity.  check(c, got) receives call c's outputs (one array of out_dtype per output port) for (f).
    Returns the per-call outputs of the hostile run."""
    inputs = [np.ascontiguousarray(x) for x in inputs]
    out_dtype = np.dtype(out_dtype)
    in_sizes = [x.dtype.itemsize for x in inputs]
    assert sum(lens) <= min(len(x) for x in inputs)
    runs = {}
    for hostile in (True, False):
        rng = np.random.default_rng(seed + 977)
        obj = factory()
        caps = [max_output(obj, n) for n in lens]
        ins = [Buffer(mem, in_offset * (1 if offsets_in_bytes else s), max(lens) * s) for s in in_sizes]
        outs = [Buffer(mem, out_offset * (1 if offsets_in_bytes else out_dtype.itemsize), max(caps) * out_dtype.itemsize) for _ in range(outputs)]
        per_call, pos = [], 0
        for c, (n, cap) in enumerate(zip(lens, caps)):
            images = [_input_image(b.size, b.lo, np.frombuffer(x[pos:pos + n].tobytes(), np.uint8), in_kind, hostile, rng) for b, x in zip(ins, inputs)]
            for b, img in zip(ins, images):
                mem.write(b.h, img)
            for b in outs:
                mem.write(b.h, sentinel_fill(b.size))
            mem.sync()
            count = call(obj, [b.addr() for b in ins], n, [b.addr() for b in outs], cap)
            mem.sync()
            tag = "call %d (n = %d, %s guards)" % (c, n, "hostile" if hostile else "finite")
            assert 0 <= count <= cap, (tag, count, cap)
            got = []
            try:
                for p, b in enumerate(outs):
                    y = mem.read(b.h)
                    nbytes = count * out_dtype.itemsize
                    check_before(y, b.lo, "out%d" % p)
                    check_after(y, b.lo, nbytes, "out%d" % p)
                    floats = {"f": out_dtype.str, "c": "<f%d" % (out_dtype.itemsize // 2)}.get(out_dtype.kind) if out_floats else None
                    check_written(y, b.lo, nbytes, out_dtype.itemsize, floats, "out%d" % p)
                    got.append(y[b.lo:b.lo + nbytes].copy())
                for p, (b, img) in enumerate(zip(ins, images)):
                    check_input_untouched(img, mem.read(b.h), b.lo, "in%d" % p)
            except GuardViolation as e:
                raise GuardViolation("%s: %s" % (tag, e)) from None
            per_call.append(got)
            pos += n
        runs[hostile] = per_call
    check_same([np.concatenate(g) for g in runs[True]], [np.concatenate(g) for g in runs[False]])
    result = [[np.frombuffer(g.tobytes(), out_dtype) for g in got] for got in runs[True]]
    if check is not None:
        for c, got in enumerate(result):
            check(c, got if outputs > 1 else got[0])
    return [got if outputs > 1 else got[0] for got in result]
