"""-m gpu: the post-demod bit layer kernel (bitlayer.hip, frame_decode.c) through the C-ABI against the oracle:
the stage alone on encoded IRA / IBC frames with injected errors (hard-decision and Chase paths), and behind the whole
pipeline on a scene whose bursts carry IRA / IBC frames, some of them weak enough for bit errors."""
import ctypes as C

import numpy as np
import pytest

import bitlayer as bl
import irdm
import orc
import parity
import siggen
from test_oracle_bitlayer import Decoded as OrcDecoded, decode_with, make_cases

pytestmark = pytest.mark.gpu

FIELDS = ("type", "sat_id", "beam_id", "pos_xyz", "alt", "n_pages", "lat", "lon", "page_tmsi", "page_msc",
          "timeslot", "sv_blocking", "bc_type", "iri_time", "bch_len")


def same(g, o):
    for f in FIELDS:
        a, b = getattr(g, f), getattr(o, f)
        if f in ("lat", "lon"):
            a, b = np.float64(a).view(np.uint64), np.float64(b).view(np.uint64)
        elif hasattr(a, "__len__"):
            a, b = tuple(a), tuple(b)
        assert a == b, (f, a, b)


def to_demod(bits, llr, k):
    d = irdm.Demod()
    d.id, d.timestamp, d.center_frequency = 10 * k, 1700000000 * 10**9 + k, 1.6262e9 + k
    d.n_bits = len(bits)
    d.n_symbols = len(bits) // 2
    d.ok = 1
    for i, b in enumerate(bits):
        d.bits[i] = int(b)
    if llr is not None:
        for i, v in enumerate(llr):
            d.llr[i] = float(v)
    return d


@pytest.mark.parametrize("seed", (0, 1))
def test_frame_decode_batch_matches_oracle(seed):
    L = orc.lib()
    L.orc_frame_decode.restype = C.c_int
    cases = [c for c in make_cases(seed, n=180) if len(c[0]) <= irdm.MAX_BITS]
    p = irdm.Pipeline(2_000_000, max_chunk_samples=32768, max_bursts_per_chunk=256)
    try:
        for use_llr in (True, False):
            sel = [(b, l) for b, l in cases if (l is not None) == use_llr]
            got = p.frame_decode_batch([to_demod(b, l, k) for k, (b, l) in enumerate(sel)], use_llr=use_llr)
            types = {0: 0, 1: 0, 2: 0}
            for k, ((b, l), g) in enumerate(zip(sel, got)):
                r, o = decode_with(L.orc_frame_decode, b, l)
                same(g, o)
                assert (g.type != 0) == bool(r) and g.id == 10 * k
                types[g.type] += 1
            assert types[1] and types[2] and types[0], types
    finally:
        p.close()


def _frame_scene(seed=31):
    fs = 2_000_000
    rng = np.random.default_rng(seed)
    n = int(2.2 * fs) // 32768 * 32768
    first = 530 * 2048
    bursts, truth = [], []
    for k in range(10):
        if k % 2 == 0:
            pages = [(int(rng.integers(0, 2**32)), int(rng.integers(0, 32))) for _ in range(2 + k % 3)]
            st = bl.ira_stream(int(rng.integers(0, 128)), int(rng.integers(0, 64)), int(rng.integers(-2047, 2048)),
                               int(rng.integers(-2047, 2048)), int(rng.integers(-2047, 2048)), pages, rng)
            st = st[:63 + 4 * 42]
            bits = bl.ira_frame(st)
            truth.append(1)
        else:
            st = bl.ibc_stream(int(rng.integers(0, 128)), int(rng.integers(0, 64)), int(rng.integers(0, 2)),
                               int(rng.integers(0, 2)), int(rng.integers(0, 2**32)), rng, n_blocks=4)
            bits = bl.ibc_frame(int(rng.integers(0, 4)), st)
            truth.append(2)
        bits = bits + [int(b) for b in rng.integers(0, 2, 290 - len(bits))] if len(bits) < 290 else bits
        if len(bits) % 2:
            bits.append(0)
        amp = 0.05 if k < 6 else (0.0075, 0.0065, 0.006, 0.0055)[k - 6]      # the last four: bit errors likely
        bursts.append(dict(start=first + 3000 + 190_000 * k, freq_hz=siggen.channel_freq(int(rng.integers(-20, 21)) or 3),
                           quads=[0] * 16 + siggen.bits_to_quadrants("".join(str(b) for b in bits)), amp=amp))
    return fs, siggen.make_stream(fs, n, bursts, seed=seed)[0], truth


def test_pipeline_decodes_ira_and_ibc_frames_like_the_oracle():
    fs, iq, truth = _frame_scene()
    ref = orc.run_stream(iq, fs)
    L = orc.lib()
    L.orc_frame_decode.restype = C.c_int
    p = irdm.Pipeline(fs, max_chunk_samples=len(iq), max_bursts_per_chunk=1024, pipeline_depth=1)
    p.set_option("decode_frames", 1)
    p.set_option("keep_frame_samples", 1)
    try:
        half = len(iq) // 2 // 32768 * 32768
        p.feed_host(iq[:half])
        p.feed_host(iq[half:])
        p.flush()
        infos, samples = p.poll_frames()
        got = dict(bursts=p.poll_bursts(), infos=infos, samples=samples, demods=p.poll_demods(), tagged=p.tagged)
        dec = p.poll_decoded()
    finally:
        p.close()
    parity.compare(got, ref)
    assert len(dec) == len(got["demods"]) == len(ref.demods) >= 8
    n_ok = {1: 0, 2: 0}
    for g, dm, rd in zip(dec, got["demods"], ref.demods):
        bits = np.ctypeslib.as_array(rd.bits)[:rd.n_bits]
        llr = np.ctypeslib.as_array(rd.llr)[:rd.n_bits]
        r, o = decode_with(L.orc_frame_decode, bits, llr)
        same(g, o)
        assert g.id == dm.id and g.timestamp == dm.timestamp and g.frequency == dm.center_frequency
        if g.type:
            n_ok[g.type] += 1
    # the strong bursts decode; an IRA frame may be claimed by the IBC branch first (frame_decode.c tries IBC before IRA and
    # the Chase decoder accepts many random blocks) -- whatever the reference's logic says is what must come out
    assert n_ok[1] >= 2 and n_ok[2] >= 3, n_ok


# ------------------------------------------------------------------ IDA (ida_decode.c) ----
from test_oracle_bitlayer import ida_decode_with, ida_tuple, make_ida_cases

IDA_FIELDS = ("ok", "ft", "lcw_ft", "lcw_code", "ec_lcw", "lcw3_val", "da_ctr", "da_len", "cont", "crc_ok", "stored_crc",
              "computed_crc", "fixederrs", "payload_len", "bch_len")


def same_ida(g, o):
    for f in IDA_FIELDS:
        assert getattr(g, f) == getattr(o, f), (f, getattr(g, f), getattr(o, f))
    assert bytes(g.payload) == bytes(o.payload) and bytes(g.bch_stream) == bytes(o.bch_stream)
    assert g.lcw_header == o.lcw_header, (g.lcw_header, o.lcw_header)


@pytest.mark.parametrize("seed", (0, 1))
def test_ida_decode_batch_matches_oracle(seed):
    L = orc.lib()
    L.orc_ida_decode.restype = C.c_int
    cases = make_ida_cases(seed, n=160)
    p = irdm.Pipeline(2_000_000, max_chunk_samples=32768, max_bursts_per_chunk=256)
    try:
        n_ok = 0
        for use_llr in (True, False):
            sel = [(b, l, d) for b, l, d in cases if (l is not None) == use_llr]
            dem = []
            for k, (b, l, d) in enumerate(sel):
                r = to_demod(b, l, k)
                r.direction = d
                dem.append(r)
            got = p.ida_decode_batch(dem, use_llr=use_llr)
            for k, ((b, l, d), g) in enumerate(zip(sel, got)):
                r, o = ida_decode_with(L.orc_ida_decode, b, l, d)
                same_ida(g, o)
                assert g.id == 10 * k and (not g.ok or g.direction == d)
                n_ok += g.ok
        assert n_ok >= 40
        # every LCW header form through the product's host formatter
        rng = np.random.default_rng(3)
        dem, want = [], []
        for d5 in range(32):
            for rep in range(3):
                st = bl.ida_stream(1, 20, 0, [0] * 20, rng)
                bits = bl.ida_frame(bl.lcw_bits(2, d5, int(rng.integers(0, 1 << 21))), st, rng)
                r = to_demod(bits, None, len(dem))
                r.direction = 1
                dem.append(r)
                want.append(ida_decode_with(L.orc_ida_decode, bits, None, 1)[1])
        for g, o in zip(p.ida_decode_batch(dem, use_llr=False), want):
            same_ida(g, o)
    finally:
        p.close()


def test_pipeline_decodes_ida_bursts_like_the_oracle():
    fs = 2_000_000
    rng = np.random.default_rng(41)
    n = int(2.0 * fs) // 32768 * 32768
    first = 530 * 2048
    bursts = []
    for k in range(8):
        st = bl.ida_stream(k % 8, 20 if k % 3 else 11, k & 1, [int(b) for b in rng.integers(0, 256, 20)], rng,
                           good_crc=bool(k != 5))
        bits = bl.ida_frame(bl.lcw_bits(2, int(rng.integers(0, 32)), int(rng.integers(0, 1 << 21))), st, rng)
        amp = 0.05 if k < 6 else 0.0065
        bursts.append(dict(start=first + 3000 + 200_000 * k, freq_hz=siggen.channel_freq(int(rng.integers(-20, 21)) or 4),
                           quads=[0] * 16 + siggen.bits_to_quadrants("".join(str(b) for b in bits)), amp=amp))
    iq = siggen.make_stream(fs, n, bursts, seed=41)[0]
    ref = orc.run_stream(iq, fs)
    L = orc.lib()
    L.orc_ida_decode.restype = C.c_int
    p = irdm.Pipeline(fs, max_chunk_samples=len(iq), max_bursts_per_chunk=1024, pipeline_depth=1)
    p.set_option("decode_ida", 1)
    p.set_option("decode_frames", 1)
    try:
        half = len(iq) // 2 // 32768 * 32768
        p.feed_host(iq[:half])
        p.feed_host(iq[half:])
        p.flush()
        demods, ida, dec = p.poll_demods(), p.poll_ida(), p.poll_decoded()
    finally:
        p.close()
    assert len(ida) == len(dec) == len(demods) == len(ref.demods) >= 6
    n_ok = n_crc = 0
    for g, dm, rd in zip(ida, demods, ref.demods):
        bits = np.ctypeslib.as_array(rd.bits)[:rd.n_bits]
        llr = np.ctypeslib.as_array(rd.llr)[:rd.n_bits]
        r, o = ida_decode_with(L.orc_ida_decode, bits, llr, rd.direction)
        same_ida(g, o)
        assert g.id == dm.id
        if g.ok:
            assert (g.timestamp, g.frequency, g.direction, g.confidence, g.n_symbols) == \
                   (dm.timestamp, dm.center_frequency, dm.direction, dm.confidence, dm.n_payload_symbols)
            n_ok += 1
            n_crc += g.crc_ok
    assert n_ok >= 6 and n_crc >= 5, (n_ok, n_crc)


# ------------------------------------------- all four decode kernels on the corpora, packed records and unpacking ----
import bitlayer_checks as BC                                                # noqa: E402


def _demods(sel):
    out = []
    for k, (b, l, d) in enumerate(sel):
        r = to_demod(b, l, k)
        r.direction = d
        r.magnitude, r.noise, r.level, r.confidence, r.n_payload_symbols = 1.5 + k, -3.0, 0.25 * k, k % 100, k % 400
        out.append(r)
    return out


def _packed_of(dm):
    f = irdm.DemodPacked()
    for name in ("id", "timestamp", "center_frequency", "direction", "magnitude", "noise", "confidence", "level",
                 "n_symbols", "n_payload_symbols", "n_bits", "ok"):
        setattr(f, name, getattr(dm, name))
    return f


CAP = 32                                                                    # burst_cap: every corpus takes several launches


@pytest.mark.parametrize("seed", (0, 1))
def test_ida_kernels_on_the_corpora(seed):
    """ida_decode_kernel and ida_packed_kernel on make_ida_cases and the long IDA frames against the oracle; every packed
    record unpacked equals ida_decode_kernel's record of the same frame with LLRs"""
    cases = BC.ida_corpus(seed)
    p = irdm.Pipeline(2_000_000, max_chunk_samples=32768, max_bursts_per_chunk=CAP)
    try:
        for use_llr in (True, False):
            sel = [c for c in cases if (c[1] is not None) == use_llr]
            assert len(sel) > CAP
            got = p.ida_decode_batch(_demods(sel), use_llr=use_llr)
            for k, ((b, l, d), g) in enumerate(zip(sel, got)):
                BC.same_ida(g, BC.oracle_ida(b, l, d), k)
                assert g.id == 10 * k
        sel = [(b, l if l is not None else np.zeros(len(b), np.float32), d) for b, l, d in cases if len(b) % 2 == 0]
        assert len(sel) > CAP
        dem = _demods(sel)
        packed = p.ida_packed_batch(dem)
        full = p.ida_decode_batch(dem, use_llr=True)
        for k, ((b, l, d), g, fu, dm) in enumerate(zip(sel, packed, full, dem)):
            BC.same_ida_packed(g, BC.oracle_ida(b, l, d), k)
            u = irdm.ida_unpack(g, _packed_of(dm))
            BC.same_ida(u, fu, k)
            for f in ("lcw_header", "id", "timestamp", "frequency", "direction", "magnitude", "noise", "level", "confidence",
                      "n_symbols"):
                assert getattr(u, f) == getattr(fu, f), (k, f, getattr(u, f), getattr(fu, f))
        BC.assert_packed_ida_coverage(sel)
        odd = _demods([(bl.ACCESS_DL + [0] * 301, None, 1)])
        with pytest.raises(RuntimeError):
            p.ida_packed_batch(odd)                                         # the packed kernels take 2 * n_symbols bits
    finally:
        p.close()


@pytest.mark.parametrize("seed", (0, 1))
def test_frame_kernels_on_the_corpora(seed):
    """frame_decode_kernel and frame_packed_kernel on make_cases and the long IRA / IBC frames against the oracle (lat /
    lon bit for bit); every packed record unpacked equals frame_decode_kernel's record of the same frame with LLRs"""
    cases = [(b, l, 0) for b, l in BC.frame_corpus(seed)]
    p = irdm.Pipeline(2_000_000, max_chunk_samples=32768, max_bursts_per_chunk=CAP)
    try:
        L = orc.lib()
        L.orc_frame_decode.restype = C.c_int
        for use_llr in (True, False):
            sel = [c for c in cases if (c[1] is not None) == use_llr]
            assert len(sel) > CAP
            got = p.frame_decode_batch(_demods(sel), use_llr=use_llr)
            for k, ((b, l, _), g) in enumerate(zip(sel, got)):
                same(g, decode_with(L.orc_frame_decode, b, l)[1])
                assert g.id == 10 * k
        sel = [(b, l if l is not None else np.zeros(len(b), np.float32), 0) for b, l, _ in cases if len(b) % 2 == 0]
        assert len(sel) > CAP
        dem = _demods(sel)
        packed = p.frame_packed_batch(dem)
        full = p.frame_decode_batch(dem, use_llr=True)
        for k, ((b, l, _), g, fu, dm) in enumerate(zip(sel, packed, full, dem)):
            BC.same_frame_packed(g, BC.oracle_frame(b, l), k)
            u = irdm.frame_unpack(g, _packed_of(dm))
            same(u, fu)
            assert (u.id, u.timestamp, u.frequency) == (fu.id, fu.timestamp, fu.frequency), k
        BC.assert_packed_frame_coverage([(b, l) for b, l, _ in sel])
        with pytest.raises(RuntimeError):
            p.frame_packed_batch(_demods([(bl.ACCESS_DL + [0] * 301, None, 1)]))
    finally:
        p.close()
