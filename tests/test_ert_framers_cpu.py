"""The models of the three ERT framers (tests/helpers/ert_framer_model.py) against the reference's golden vectors, the encoders against the
models, the persistent-correction finding (a rejected window's in-place correction changes what a later window holds), and the layouts of the
three frame types.  No GPU."""
import numpy as np
import pytest

from luaradio_amd import types
from tests import golden_util
from tests.helpers import ert_framer_model as M


@pytest.mark.parametrize("name", sorted(M.PROTOCOLS))
def test_literal_models_reproduce_the_goldens_whole_and_bit_by_bit(name):
    P = M.PROTOCOLS[name]
    for desc, x, want in M.golden_cases(name):
        assert len(want) >= 1
        whole, bitwise = golden_util.run_whole_and_samplewise(lambda: M.FramerLiteral(P), x)
        assert whole.dtype == P.dtype and M.same_records(whole, want) and M.pads_are_zero(whole), desc
        assert M.same_records(bitwise, want), desc


def test_check_matrices():
    for P in M.PROTOCOLS.values():
        assert len(set(P.rows)) == P.cw_len and 0 not in P.rows                   # a syndrome names at most one bit
        assert P.rows[-16:] == [1 << (15 - i) for i in range(16)]                # the check bits are the identity
    assert M.SCM.rows[0] == 0x6d9c and M.SCM.rows[58] == 0x6f63                  # scmframer.lua:54, :68
    assert M.SCM_PLUS.rows[0] == 0xaaa1 and M.SCM_PLUS.rows[95] == 0x1021        # scmplusframer.lua:52, :75
    # of the 65 536 syndromes, 1 + 112 leave an SCM+ window correctable
    assert 1 + len(M.SCM_PLUS.correct) == 113


@pytest.mark.parametrize("name", sorted(M.PROTOCOLS))
def test_encoders_round_trip(name):
    P = M.PROTOCOLS[name]
    rng = np.random.default_rng(3)
    for trial in range(8):
        sent = P.random_fields(rng)
        bits, want = M.encode(P, **sent)
        assert len(bits) == P.L and P.syndrome(bytearray(bits.tobytes())) == 0
        for k, v in sent.items():
            assert want[k] == v
        pad = rng.integers(0, 2, 50).astype(np.uint8)
        got = M.FramerLiteral(P).process(np.concatenate([pad, bits, pad]))
        assert M.same_records(got, P.record(want))
        # one error anywhere in the codeword is corrected, in the message and in the check bits
        for k in (P.cw_off + trial, P.L - 1 - trial):
            y = bits.copy()
            y[k] ^= 1
            assert M.same_records(M.FramerLiteral(P).process(np.concatenate([pad, y, pad])), P.record(want))
        # two errors are not
        a, b = M.uncorrectable_pair(P, 20, 40)
        y = bits.copy()
        y[P.cw_off + a] ^= 1
        y[P.cw_off + b] ^= 1
        assert len(M.FramerLiteral(P).process(y)) == 0


def test_idm_crc_byte_semantics():
    """idm_compute_crc reads byte values: a 2 is neither a one nor a zero"""
    bits = np.random.default_rng(4).integers(0, 2, 32).astype(np.uint8)
    twos = np.where(bits == 0, 2, bits).astype(np.uint8)
    assert M.idm_crc(bits, 0, 32) != M.idm_crc(twos, 0, 32)
    assert M.tonumber(bits, 0, 32) == M.tonumber(twos, 0, 32)


@pytest.mark.parametrize("name", ["scm+", "idm"])
@pytest.mark.parametrize("chain", [1, 2])
def test_a_rejected_windows_correction_persists(name, chain):
    """the finding: the literal model emits the frame, a walk over the raw windows does not"""
    P = M.PROTOCOLS[name]
    stream, want, flips = M.persistent_case(P, chain)
    assert len(flips) == chain + 1
    got = M.FramerLiteral(P).process(stream)
    assert M.same_records(got, P.record(want))
    assert len(M.pure_window_walk(P, stream)) == 0
    # cut anywhere, the literal model says the same
    blk = M.FramerLiteral(P)
    parts = [blk.process(stream[a:a + 37]) for a in range(0, len(stream), 37)]
    assert M.same_records(np.concatenate(parts), got)


def test_scm_has_no_mutating_reject():
    with pytest.raises(AssertionError):
        M.persistent_case(M.SCM)


def test_pure_walk_equals_the_literal_model_on_plain_streams():
    rng = np.random.default_rng(6)
    for P in M.PROTOCOLS.values():
        frames = [M.random_frame(P, rng) for _ in range(3)]
        x = np.concatenate([np.concatenate([rng.integers(0, 2, 70).astype(np.uint8), bits]) for bits, _ in frames])
        want = P.records([w for _, w in frames])
        assert M.same_records(M.FramerLiteral(P).process(x), want)
        assert M.same_records(M.pure_window_walk(P, x), want)


def test_frame_type_layouts():
    def layout(t):
        return {k: (v[1], v[0].itemsize, v[0].shape) for k, v in t.dtype.fields.items()}
    assert (types.SCMFrameType.size, types.SCMFrameType.dtype.itemsize) == (16, 16)
    assert layout(types.SCMFrameType) == {"ert_id": (0, 4, ()), "consumption": (4, 4, ()), "crc": (8, 2, ()), "ert_type": (10, 1, ()),
                                          "physical_tamper": (11, 1, ()), "encoder_tamper": (12, 1, ()), "reserved": (13, 1, ())}
    assert (types.SCMPlusFrameType.size, types.SCMPlusFrameType.dtype.itemsize) == (16, 16)
    assert layout(types.SCMPlusFrameType) == {"ert_id": (0, 4, ()), "consumption": (4, 4, ()), "tamper": (8, 2, ()), "crc": (10, 2, ()),
                                              "protocol_id": (12, 1, ()), "ert_type": (13, 1, ())}
    assert (types.IDMFrameType.size, types.IDMFrameType.dtype.itemsize) == (88, 88)
    assert layout(types.IDMFrameType) == {
        "ert_id": (0, 4, ()), "last_consumption_count": (4, 4, ()), "transmit_time_offset": (8, 2, ()), "serial_crc": (10, 2, ()),
        "packet_crc": (12, 2, ()), "application_version": (14, 1, ()), "ert_type": (15, 1, ()), "consumption_interval_count": (16, 1, ()),
        "module_programming_state": (17, 1, ()), "tamper_count": (18, 6, (6,)), "async_count": (24, 2, (2,)),
        "power_outage_flags": (26, 6, (6,)), "differential_consumption_intervals": (32, 53, (53,))}
    for t in (types.SCMFrameType, types.SCMPlusFrameType, types.IDMFrameType):
        assert all(t.dtype[k].byteorder in ("<", "=", "|") for k in t.dtype.names)
        assert t.vector(3).shape == (3,) and t.vector(3).dtype == t.dtype


@pytest.mark.parametrize("name", sorted(M.PROTOCOLS))
def test_overlapping_valid_windows(name):
    """a valid frame that starts inside an accepted one is not emitted; with the first broken, it is"""
    P = M.PROTOCOLS[name]
    rng = np.random.default_rng(8)
    for d in (P.pre_bits + 24, P.L - 1):
        x, first, second = M.overlap_stream(P, d, rng)
        assert M.same_records(M.FramerLiteral(P).process(x), P.record(first))
        a, b = M.uncorrectable_pair(P, 0, min(d - P.cw_off, 40))
        x[P.cw_off + a] ^= 1
        x[P.cw_off + b] ^= 1
        assert M.same_records(M.FramerLiteral(P).process(x), P.record(second))
