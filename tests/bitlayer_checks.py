"""The bit layer's decode kernels against the oracle, field by field: the corpora (make_cases / make_ida_cases and the
long frames of test_oracle_bitlayer), the comparisons and the coverage the packed kernels' share of them must reach.
Shared by the emulation tests (test_kernels_emul.py) and the -m gpu tests (test_gpu_bitlayer.py)."""
import ctypes as C

import numpy as np

import orc
from test_oracle_bitlayer import (decode_with, ida_decode_with, make_cases, make_ida_cases, make_long_frame_cases,
                                  make_long_ida_cases)

IDA_FIELDS = ("ok", "ft", "lcw_ft", "lcw_code", "ec_lcw", "lcw3_val", "da_ctr", "da_len", "cont", "crc_ok", "stored_crc",
              "computed_crc", "fixederrs", "payload_len", "bch_len")
FRAME_FIELDS = ("type", "sat_id", "beam_id", "n_pages", "timeslot", "sv_blocking", "bc_type", "iri_time", "bch_len")


def ida_corpus(seed):
    """[(bits, llr or None, direction)]: make_ida_cases and the long IDA frames, at most kMaxBits long"""
    old = [(b, l, d) for b, l, d in make_ida_cases(seed, n=160)]
    return [c for c in old + [(b, l, d) for b, l, d, _ in make_long_ida_cases(seed)] if len(c[0]) <= orc.MAX_BITS]


def frame_corpus(seed):
    """[(bits, llr or None)]: make_cases and the long IRA / IBC frames, at most kMaxBits long"""
    old = make_cases(seed, n=180)
    return [c for c in old + [(b, l) for b, l, _ in make_long_frame_cases(seed)] if len(c[0]) <= orc.MAX_BITS]


def oracle_ida(bits, llr, direction):
    L = orc.lib()
    L.orc_ida_decode.restype = C.c_int
    return ida_decode_with(L.orc_ida_decode, bits, llr, direction)[1]


def oracle_frame(bits, llr):
    L = orc.lib()
    L.orc_frame_decode.restype = C.c_int
    return decode_with(L.orc_frame_decode, bits, llr)[1]


def same_ida(g, o, k):
    """an IdaOut / irdm_ida_t against the oracle's record"""
    for f in IDA_FIELDS:
        assert getattr(g, f) == getattr(o, f), (k, f, getattr(g, f), getattr(o, f))
    assert bytes(g.payload) == bytes(o.payload), k
    assert bytes(g.bch_stream) == bytes(o.bch_stream), k


def same_ida_packed(g, o, k):
    """an irdm_ida_packed_t against the oracle's record: bch_stream 8 bits per byte, its first min(bch_len, 256) bits"""
    for f in IDA_FIELDS:
        assert getattr(g, f) == getattr(o, f), (k, f, getattr(g, f), getattr(o, f))
    assert bytes(g.payload) == bytes(o.payload), k
    bits = np.unpackbits(np.frombuffer(bytes(g.bch_stream), np.uint8))
    n = min(o.bch_len, 256)
    assert bytes(bits[:n]) == bytes(o.bch_stream)[:n] and not bits[n:].any(), k


def same_frame(g, o, k, pages_beyond=False):
    """a DecodedOut / irdm_decoded_t against the oracle's record (pages up to n_pages; all of them with pages_beyond)"""
    for f in FRAME_FIELDS:
        assert getattr(g, f) == getattr(o, f), (k, f, getattr(g, f), getattr(o, f))
    assert tuple(g.pos_xyz) == tuple(o.pos_xyz), k
    n = 12 if pages_beyond else o.n_pages
    assert tuple(g.page_tmsi)[:n] == tuple(o.page_tmsi)[:n] and tuple(g.page_msc)[:n] == tuple(o.page_msc)[:n], k


def same_frame_packed(g, o, k):
    same_frame(g, o, k, pages_beyond=True)
    if not o.type:
        assert bytes(g) == bytes(len(bytes(g))), k                   # every field 0 for a frame not taken


def _tied(llr):
    return llr is not None and len(np.unique(llr)) < len(llr) // 2


def assert_packed_ida_coverage(sel):
    """the packed kernel's share of ida_corpus (even lengths): long streams, the cap, uplink, Chase, ties"""
    c = dict(ok=0, over256=0, cap=0, uplink=0, chase=0, tied=0, crc_ok=0, crc_bad=0)
    for b, l, d in sel:
        o = oracle_ida(b, l, d)
        if not o.ok:
            continue
        c["ok"] += 1
        c["over256"] += o.bch_len > 256
        c["cap"] += o.bch_len >= 480
        c["uplink"] += d == 2
        c["chase"] += o.fixederrs >= 2
        c["tied"] += _tied(l)
        c["crc_ok" if o.crc_ok else "crc_bad"] += o.da_len > 0
    assert c["ok"] >= 60 and c["over256"] >= 20 and c["cap"] >= 4 and c["uplink"] >= 15, c
    assert c["chase"] >= 20 and c["tied"] >= 15 and c["crc_ok"] >= 10 and c["crc_bad"] >= 10, c


def assert_packed_frame_coverage(sel):
    c = dict(ira=0, ibc=0, cap=0, pages5=0, ibc_max=0, tied=0)
    for b, l in sel:
        o = oracle_frame(b, l)
        c["ira"] += o.type == 1
        c["ibc"] += o.type == 2
        c["cap"] += o.type == 1 and o.bch_len == 63 + 10 * 42
        c["pages5"] += o.type == 1 and o.n_pages >= 5
        c["ibc_max"] += o.type == 2 and o.bch_len == 8 * 21
        c["tied"] += o.type != 0 and _tied(l)
    assert c["ira"] >= 50 and c["ibc"] >= 30 and c["cap"] >= 5 and c["pages5"] >= 15 and c["ibc_max"] >= 5, c
    assert c["tied"] >= 15, c
