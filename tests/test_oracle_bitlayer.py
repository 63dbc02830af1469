"""Post-demod bit layer: the oracle's orc_frame_decode against the reference's frame_decode.c compiled
in place (oracle/_ref), on encoded IRA / IBC frames with known answers, bit errors inside and beyond the BCH and Chase
correction radius, truncated frames, and garbage."""
import ctypes as C

import numpy as np
import pytest

import bitlayer as bl
import orc
from refpins import refpins  # noqa: F401  (fixture)


class Decoded(C.Structure):
    _fields_ = [("type", C.c_int32), ("sat_id", C.c_int32), ("beam_id", C.c_int32), ("pos_xyz", C.c_int32 * 3),
                ("alt", C.c_int32), ("n_pages", C.c_int32), ("lat", C.c_double), ("lon", C.c_double),
                ("page_tmsi", C.c_uint32 * 12), ("page_msc", C.c_int32 * 12), ("timeslot", C.c_int32),
                ("sv_blocking", C.c_int32), ("bc_type", C.c_int32), ("iri_time", C.c_uint32),
                ("bch_len", C.c_int32), ("pad", C.c_int32)]


FIELDS = [f for f, _ in Decoded._fields_ if f not in ("bch_len", "pad")]


def as_tuple(d):
    out = []
    for f in FIELDS:
        v = getattr(d, f)
        if f in ("lat", "lon"):
            v = int(np.float64(v).view(np.uint64))       # bit-identical doubles
        elif hasattr(v, "__len__"):
            v = tuple(v)
        out.append(v)
    return tuple(out)


def decode_with(fn, bits, llr):
    b = np.ascontiguousarray(bits, np.uint8)
    d = Decoded()
    lp = None if llr is None else np.ascontiguousarray(llr, np.float32).ctypes.data_as(C.POINTER(C.c_float))
    r = fn(b.ctypes.data_as(C.POINTER(C.c_uint8)), lp, len(b), C.byref(d))
    return r, d


def make_cases(seed, n=120):
    rng = np.random.default_rng(seed)
    cases = []
    for k in range(n):
        kind = k % 6
        if kind in (0, 1, 2):                            # IRA
            pages = [(int(rng.integers(0, 2**32)), int(rng.integers(0, 32))) for _ in range(int(rng.integers(0, 5)))]
            st = bl.ira_stream(int(rng.integers(0, 128)), int(rng.integers(0, 64)), int(rng.integers(-2047, 2048)),
                               int(rng.integers(-2047, 2048)), int(rng.integers(-2047, 2048)), pages, rng,
                               terminate=bool(rng.integers(0, 2)))
            if len(st) % 42 != 21:                       # 63 + 42k always is; keep the pairing of the tail blocks
                st = st[:63 + (len(st) - 63) // 42 * 42]
            bits = bl.ira_frame(st, uplink=bool(kind == 2))
        elif kind in (3, 4):                             # IBC
            st = bl.ibc_stream(int(rng.integers(0, 128)), int(rng.integers(0, 64)), int(rng.integers(0, 2)),
                               int(rng.integers(0, 2)), int(rng.integers(0, 2**32)) if kind == 3 else None, rng,
                               n_blocks=int(rng.integers(1, 5)))
            bits = bl.ibc_frame(int(rng.integers(0, 4)), st)
        else:                                            # garbage behind a valid access code / no access code
            bits = list(bl.ACCESS_DL if rng.integers(0, 2) else rng.integers(0, 2, 24)) + \
                   [int(b) for b in rng.integers(0, 2, int(rng.integers(0, 400)))]
        bits += [int(b) for b in rng.integers(0, 2, int(rng.integers(0, 70)))]      # trailing payload noise
        n_err = int(rng.choice([0, 0, 1, 2, 3, 5, 8, 14, 30]))
        bits, llr = bl.corrupt(bits, rng, n_err, mark=bool(rng.integers(0, 4)), extra_weak=int(rng.integers(0, 6)))
        if rng.integers(0, 8) == 0:
            cut = int(rng.integers(0, len(bits)))
            bits, llr = bits[:cut], llr[:cut]
        cases.append((bits, None if rng.integers(0, 6) == 0 else llr))
    return cases


def test_encoder_round_trip_through_the_oracle(oracle):
    """clean frames decode to exactly the fields that were encoded"""
    oracle.orc_frame_decode.restype = C.c_int
    rng = np.random.default_rng(5)
    st = bl.ira_stream(77, 33, -1234, 987, 2000, [(0xDEADBEEF, 17), (12345, 3)], rng)
    r, d = decode_with(oracle.orc_frame_decode, bl.ira_frame(st), None)
    assert r == 1 and d.type == 1 and (d.sat_id, d.beam_id, tuple(d.pos_xyz)) == (77, 33, (-1234, 987, 2000))
    assert d.n_pages == 2 and d.page_tmsi[0] == 0xDEADBEEF and d.page_msc[0] == 17 and d.page_msc[1] == 3
    assert d.alt == int(np.sqrt(1234.0**2 + 987.0**2 + 2000.0**2) * 4.0) - 6378 + 23
    st = bl.ibc_stream(99, 12, 1, 0, 0xCAFEF00D, rng, n_blocks=3)
    r, d = decode_with(oracle.orc_frame_decode, bl.ibc_frame(2, st), None)
    assert r == 1 and d.type == 2 and (d.sat_id, d.beam_id, d.timeslot, d.sv_blocking, d.bc_type) == (99, 12, 1, 0, 2)
    assert d.iri_time == 0xCAFEF00D and d.bch_len == 3 * 42


@pytest.mark.parametrize("seed", range(4))
def test_oracle_matches_frame_decode_c(oracle, refpins, seed):
    R = refpins.lib
    oracle.orc_frame_decode.restype = C.c_int
    kinds = {0: 0, 1: 0, 2: 0}
    ours, theirs = [], []
    for bits, llr in make_cases(seed):
        ro, do = decode_with(oracle.orc_frame_decode, bits, llr)
        ours.append((ro, as_tuple(do)))
        if R:
            R.ref_frame_decode.restype = C.c_int
            rr, dr = decode_with(R.ref_frame_decode, bits, llr)
            assert ro == rr and as_tuple(do) == as_tuple(dr), (ro, rr, as_tuple(do), as_tuple(dr))
            theirs.append((rr, as_tuple(dr)))
        kinds[do.type] += 1
    refpins.same("frame_decode/%d" % seed, ours, theirs)
    assert kinds[1] >= 20 and kinds[2] >= 10 and kinds[0] >= 20, kinds      # IRA, IBC and rejected frames all occur


class Ida(C.Structure):
    _fields_ = [("ok", C.c_int32), ("ft", C.c_int32), ("lcw_ft", C.c_int32), ("lcw_code", C.c_int32),
                ("ec_lcw", C.c_int32), ("lcw3_val", C.c_uint32), ("da_ctr", C.c_int32), ("da_len", C.c_int32),
                ("cont", C.c_int32), ("crc_ok", C.c_int32), ("stored_crc", C.c_uint32), ("computed_crc", C.c_uint32),
                ("fixederrs", C.c_int32), ("payload_len", C.c_int32), ("bch_len", C.c_int32), ("pad", C.c_int32),
                ("payload", C.c_uint8 * 32), ("bch_stream", C.c_uint8 * 256), ("lcw_header", C.c_char * 128)]


def ida_decode_with(fn, bits, llr, direction):
    b = np.ascontiguousarray(bits, np.uint8)
    d = Ida()
    lp = None if llr is None else np.ascontiguousarray(llr, np.float32).ctypes.data_as(C.POINTER(C.c_float))
    r = fn(b.ctypes.data_as(C.POINTER(C.c_uint8)), lp, len(b), direction, C.byref(d))
    return r, d


def make_ida_cases(seed, n=120):
    rng = np.random.default_rng(1000 + seed)
    cases = []
    for k in range(n):
        ft = 2 if k % 8 else int(rng.integers(0, 8))                    # mostly IDA (ft == 2)
        lcw = bl.lcw_bits(ft, int(rng.integers(0, 32)), int(rng.integers(0, 1 << 21)))
        da_len = int(rng.integers(0, 21)) if k % 9 else int(rng.integers(21, 32))
        st = bl.ida_stream(int(rng.integers(0, 8)), da_len, int(rng.integers(0, 2)),
                           [int(b) for b in rng.integers(0, 256, 20)], rng, good_crc=bool(k % 5))
        if k % 11 == 0:
            st[17 + int(rng.integers(0, 3))] = 1                          # the "zero" field set -> rejected
        bits = bl.ida_frame(lcw, st, rng, uplink=bool(k % 3 == 0))
        n_err = int(rng.choice([0, 0, 1, 2, 4, 7, 12, 25]))
        bits, llr = bl.corrupt(bits, rng, n_err, mark=bool(rng.integers(0, 4)), extra_weak=int(rng.integers(0, 6)))
        if rng.integers(0, 10) == 0:
            cut = int(rng.integers(150, len(bits)))
            bits, llr = bits[:cut], llr[:cut]
        direction = 2 if k % 3 == 0 else (1 if k % 13 else 0)            # direction 0 = undefined -> rejected
        cases.append((bits, None if rng.integers(0, 6) == 0 else llr, direction))
    return cases


def ida_tuple(d):
    return (d.ok, d.ft, d.lcw_ft, d.lcw_code, d.ec_lcw, d.lcw3_val, d.da_ctr, d.da_len, d.cont, d.crc_ok, d.stored_crc,
            d.computed_crc, d.fixederrs, d.payload_len, d.bch_len, bytes(d.payload), bytes(d.bch_stream), d.lcw_header)


def test_ida_encoder_round_trip_through_the_oracle(oracle):
    oracle.orc_ida_decode.restype = C.c_int
    rng = np.random.default_rng(9)
    payload = list(range(100, 120))
    st = bl.ida_stream(5, 17, 1, payload, rng)
    r, d = ida_decode_with(oracle.orc_ida_decode, bl.ida_frame(bl.lcw_bits(2, 0b00011, 0x12345), st, rng), None, 1)
    assert r == 1 and (d.ft, d.da_ctr, d.da_len, d.cont, d.crc_ok, d.bch_len, d.fixederrs) == (2, 5, 17, 1, 1, 200, 0)
    assert list(d.payload[:17]) == payload[:17] and d.lcw3_val == 0x12345 and d.ec_lcw == 0
    assert d.lcw_header.decode().startswith("LCW(2,T:maint,C:") and len(d.lcw_header.decode()) == 111


@pytest.mark.parametrize("seed", range(4))
def test_oracle_matches_ida_decode_c(oracle, refpins, seed):
    R = refpins.lib
    oracle.orc_ida_decode.restype = C.c_int
    n_ok = n_crc = n_rej = 0
    ours, theirs = [], []
    for bits, llr, direction in make_ida_cases(seed):
        ro, do = ida_decode_with(oracle.orc_ida_decode, bits, llr, direction)
        ours.append((ro, ida_tuple(do)))
        if R:
            R.ref_ida_decode.restype = C.c_int
            rr, dr = ida_decode_with(R.ref_ida_decode, bits, llr, direction)
            assert ro == rr and ida_tuple(do) == ida_tuple(dr), (ida_tuple(do)[:16], ida_tuple(dr)[:16])
            theirs.append((rr, ida_tuple(dr)))
        n_ok += ro
        n_crc += do.crc_ok
        n_rej += 1 - ro
    refpins.same("ida_decode/%d" % seed, ours, theirs)
    assert n_ok >= 30 and n_crc >= 10 and n_rej >= 20, (n_ok, n_crc, n_rej)


def test_lcw_header_text_for_every_type_and_code(oracle, refpins):
    """format_lcw_header's switch (ida_decode.c:405-539): every (lcw_ft, lcw_code) pair with random lcw3 values, through
    whole frames so the reference's own formatter runs"""
    R = refpins.lib
    oracle.orc_ida_decode.restype = C.c_int
    rng = np.random.default_rng(77)
    seen = set()
    ours, theirs = [], []
    for d5 in range(32):
        for rep in range(6):
            lcw3 = int(rng.integers(0, 1 << 21))
            st = bl.ida_stream(1, 20, 0, [0] * 20, rng)
            bits = bl.ida_frame(bl.lcw_bits(2, d5, lcw3), st, rng)
            ro, do = ida_decode_with(oracle.orc_ida_decode, bits, None, 1)
            assert ro == 1
            ours.append(do.lcw_header)
            if R:
                R.ref_ida_decode.restype = C.c_int
                rr, dr = ida_decode_with(R.ref_ida_decode, bits, None, 1)
                assert ro == rr == 1 and do.lcw_header == dr.lcw_header, (d5, do.lcw_header, dr.lcw_header)
                theirs.append(dr.lcw_header)
            seen.add((do.lcw_ft, do.lcw_code))
    refpins.same("lcw_header", ours, theirs)
    assert len(seen) == 32          # the 5 encodable data bits reach 32 of the 64 (type, code) pairs


# ------------------------------------------------ long frames: the 512-bit stream cap, tails, multi-chunk Chase, ties ----
LLR_MODES = ("float", "quarter", "two", "equal", "zero", "none")


def ida_lengths():
    """every block boundary and every tail chunk boundary (4 tail bits, 1, 2 and 3 chunks) +-1 and +-2 bits, up to kMaxBits"""
    out = set()
    for n_full in range(1, 7):
        for r in (0, 4, 34, 64, 96):
            for d in (-2, -1, 0, 1, 2):
                n = 70 + 124 * n_full + r + d
                if n <= orc.MAX_BITS:
                    out.add(n)
    return sorted(out | {orc.MAX_BITS - 1, orc.MAX_BITS})


def _plan(bits, llr, pos, k, rng, ftab=(bl.POLY_DA, 2048)):
    """the k-th error plan over the frame's BCH blocks (pos: the frame indices of their 31 codeword bits, in stream order;
    ftab: their code's generator and syndrome table size); returns its name"""
    n = len(pos)
    plan = k % 6
    if plan == 1:
        for i in rng.choice(np.arange(24, len(bits)), size=int(rng.integers(1, 12)), replace=False):
            bits[i] ^= 1
            if rng.integers(0, 3):
                llr[i] = 0.05 * float(rng.random())
        return "random"
    if plan in (2, 3):                           # several blocks that need Chase; (3) then one that fails
        m = n - 1 if plan == 3 else n
        sel = sorted(int(i) for i in rng.choice(m, size=min(m, int(rng.integers(2, 5))), replace=False))
        for i in sel:
            bl.plant_errors(bits, llr, pos[i], 3, rng)
        if plan == 3:                            # behind the tenth chunk where there is one: the frame stays decodable
            fail = pos[int(rng.integers(min(max(sel[-1] + 1, 10), n - 1), n))]
            if ftab[0] == bl.POLY_DA:               # (Chase finds a BCH(31,20) codeword near almost any word)
                bl.plant_failure(bits, llr, fail)
            else:                                   # (BCH(31,21) + parity: seven errors fail the parity check)
                bl.plant_errors(bits, llr, fail, 7, rng, weak=0)
            return "chase_fail"
        return "chase"
    if plan == 4:                                # one weak error, weak decoys: several flip masks decode
        i = int(rng.integers(0, n))
        bl.plant_errors(bits, llr, pos[i], 3, rng, weak=1)
        for j in rng.choice([q for q in pos[i] if q is not None], size=3, replace=False):
            llr[int(j)] = 0.05 * float(rng.random())
        return "multi_mask"
    if plan == 5:
        for i in rng.choice(n, size=min(n, 2), replace=False):
            bl.plant_errors(bits, llr, pos[int(i)], 3, rng, weak=2, tie_fifth=True)
        return "tie_fifth"
    return "clean"


def _llr_mode(k, plan):
    return "float" if plan == "tie_fifth" else LLR_MODES[(k // 6) % len(LLR_MODES)]


def make_long_ida_cases(seed, reps=3):
    """IDA frames of 1 to 6 full blocks and 0 to 3 tail chunks at every length of ida_lengths(), both directions, every
    da_len, good and bad CRCs, with the error plans of _plan and the tied reliabilities of bl.tie_llr.
    Returns [(bits, llr or None, direction, info)], info = (plan, llr mode, positions of the chunks)."""
    rng = np.random.default_rng(5000 + seed)
    cases = []
    k = 0
    for _ in range(reps):
        for n_bits in ida_lengths():
            n_full, remain = (n_bits - 70) // 124, (n_bits - 70) % 124
            ns = remain // 2
            n_ch = 4 * n_full + bl.ida_tail_chunks(ns)
            good = bool(k % 2)
            st = bl.ida_stream(int(rng.integers(0, 8)), k % 32, int(rng.integers(0, 2)),
                               [int(b) for b in rng.integers(0, 256, 20)], rng, good_crc=good)
            st += [int(b) for b in rng.integers(0, 2, max(0, 20 * n_ch - 200))]
            if good:                             # the CRC covers the stream up to bch_len - 4: zeros keep it 0
                st[196:] = [0] * (len(st) - 196)
            chunks = [bl.da_block31(st[i:i + 20]) for i in range(0, 20 * n_ch, 20)]
            uplink = k % 3 == 0
            lcw = bl.lcw_bits(2, int(rng.integers(0, 32)), int(rng.integers(0, 1 << 21)))
            bits = bl.ida_long_frame(lcw, chunks, n_full, ns, bl.bits_from(rng), uplink)
            pos = bl.block_positions(lambda lab: bl.ida_long_frame(lcw, lab, n_full, ns, bl.labels(), uplink), chunks, 31)
            if remain % 2:
                bits.append(int(rng.integers(0, 2)))
            assert len(bits) == n_bits
            llr = np.full(n_bits, 1.0, np.float32) + rng.random(n_bits).astype(np.float32) * 0.1
            plan = _plan(bits, llr, pos, k, rng)
            mode = _llr_mode(k, plan)
            llr = None if mode == "none" else bl.tie_llr(llr, mode, rng)
            cases.append((bits, llr, 2 if uplink else 1, (plan, mode, pos)))
            k += 1
    return cases


def ida_coverage(cases, decode):
    """what the corpus exercises, from the frames and their decodes: decode(bits, llr, direction) -> (r, orc_ida_t)"""
    c = dict(ok=0, crc_ok=0, crc_bad=0, long=0, over256=0, cap=0, cap_cut=0, odd=0, uplink=0, tail=0, odd_tail=0, da_len=set(),
             chase_frames=0, prefix=0, multi_mask=0, tie_fifth=0, tied_llr=0)
    for bits, llr, direction, (plan, mode, pos) in cases:
        r, d = decode(bits, llr, direction)
        c["odd"] += len(bits) % 2
        c["uplink"] += direction == 2
        c["tied_llr"] += mode in ("quarter", "two", "equal", "zero")
        ns = (len(bits) - 70) % 124 // 2
        n_chase = 0
        for p in pos:
            if llr is None or None in p:
                continue
            kind, hits, tie = bl.chase_model([bits[i] for i in p], [llr[i] for i in p])
            n_chase += kind == "chase"
            c["multi_mask"] += kind == "chase" and len(set(hits)) > 1
            c["tie_fifth"] += kind == "chase" and tie
        if not r:
            continue
        c["ok"] += 1
        c["da_len"].add(d.da_len)
        c["crc_ok" if d.crc_ok else "crc_bad"] += d.da_len > 0
        c["long"] += len(bits) > 382
        c["over256"] += d.bch_len > 256
        c["cap"] += d.bch_len + 20 > 512                 # 6 full blocks: the next chunk would pass 512 bits
        c["cap_cut"] += d.bch_len == 480 and len(pos) > 24 and plan in ("clean", "multi_mask", "tie_fifth")
        c["tail"] += d.bch_len > 80 * ((len(bits) - 70) // 124)
        c["odd_tail"] += ns % 2 == 1 and d.bch_len > 80 * ((len(bits) - 70) // 124)
        c["chase_frames"] += n_chase >= 2
        c["prefix"] += plan == "chase_fail" and d.bch_len < 20 * len(pos)
    return c


def assert_ida_coverage(c):
    assert c["ok"] >= 60 and c["crc_ok"] >= 10 and c["crc_bad"] >= 10, c
    assert c["long"] >= 30 and c["over256"] >= 20 and c["cap"] >= 2 and c["cap_cut"] >= 2, c
    assert c["odd"] >= 20 and c["uplink"] >= 20 and c["tail"] >= 20 and c["odd_tail"] >= 5, c
    assert c["chase_frames"] >= 10 and c["prefix"] >= 3 and c["multi_mask"] >= 5 and c["tie_fifth"] >= 5, c
    assert c["tied_llr"] >= 40 and c["da_len"] >= set(range(21)), c


def make_long_frame_cases(seed, n=150):
    """IRA frames of 5 to 12 pages (past the 512-bit stream cap from 11 on), IBC frames with the most blocks frame_decode()
    takes (and one more), both directions, with the error plans of _plan and tied reliabilities.
    Returns [(bits, llr or None, info)], info = (kind, plan, llr mode, positions of the BCH blocks)."""
    rng = np.random.default_rng(7000 + seed)
    cases = []
    for k in range(n):
        uplink = k % 3 == 0
        if k % 4 != 3:                                   # IRA
            pages = [(int(rng.integers(0, 2**32)), int(rng.integers(0, 32))) for _ in range(5 + k % 8)]
            st = bl.ira_stream(int(rng.integers(0, 128)), int(rng.integers(0, 64)), int(rng.integers(-2047, 2048)),
                               int(rng.integers(-2047, 2048)), int(rng.integers(-2047, 2048)), pages, rng,
                               terminate=bool(rng.integers(0, 2)))
            st = st[:63 + 12 * 42]                       # 24 + 96 + 12 * 64 = 888 bits <= kMaxBits
            blocks = [bl.bch_block32(st[i:i + 21]) for i in range(0, len(st), 21)]
            bits = bl.ira_frame_blocks(blocks, uplink)
            pos = bl.block_positions(bl.ira_frame_blocks, blocks, 32, uplink)
            kind = "ira"
        else:                                            # IBC: 4 block pairs (ibc_max = 262), sometimes a fifth
            st = bl.ibc_stream(int(rng.integers(0, 128)), int(rng.integers(0, 64)), int(rng.integers(0, 2)),
                               int(rng.integers(0, 2)), int(rng.integers(0, 2**32)), rng, n_blocks=4 + k % 2)
            bc = int(rng.integers(0, 4))
            hv = bl.to_bits((bc << 4) | bl.gf2_rem(bl.POLY_HDR, bc << 4), 6)
            blocks = [bl.bch_block32(st[i:i + 21]) for i in range(0, len(st), 21)]
            bits = bl.ibc_frame_blocks(hv, blocks, uplink)
            pos = bl.block_positions(lambda lab: bl.ibc_frame_blocks(hv, lab, uplink), blocks, 32)
            kind = "ibc"
        bits += [int(b) for b in rng.integers(0, 2, int(rng.integers(0, max(1, orc.MAX_BITS - len(bits)))))]
        if k % 5 == 4 and len(bits) < orc.MAX_BITS:
            bits.append(int(rng.integers(0, 2)))         # odd lengths
        llr = np.full(len(bits), 1.0, np.float32) + rng.random(len(bits)).astype(np.float32) * 0.1
        plan = _plan(bits, llr, [p[:31] for p in pos], k, rng, (bl.POLY_RA, 1024))
        mode = _llr_mode(k, plan)
        llr = None if mode == "none" else bl.tie_llr(llr, mode, rng)
        cases.append((bits, llr, (kind, plan, mode, pos)))
    return cases


def frame_coverage(cases, decode):
    c = dict(ira=0, ibc=0, pages5=0, cap=0, ibc_max=0, uplink=0, odd=0, chase_frames=0, prefix=0, multi_mask=0,
             tie_fifth=0, tied_llr=0)
    for bits, llr, (kind, plan, mode, pos) in cases:
        r, d = decode(bits, llr)
        c["odd"] += len(bits) % 2
        c["uplink"] += bits[:24] == bl.ACCESS_UL
        c["tied_llr"] += mode in ("quarter", "two", "equal", "zero")
        n_chase = 0
        for p in pos:
            if llr is None:
                continue
            k, hits, tie = bl.chase_model([bits[i] for i in p[:31]], [llr[i] for i in p[:31]], bl.POLY_RA, 1024)
            n_chase += k == "chase"
            c["multi_mask"] += k == "chase" and len(set(hits)) > 1
            c["tie_fifth"] += k == "chase" and tie
        if not r:
            continue
        c["ira"] += d.type == 1
        c["ibc"] += d.type == 2
        c["pages5"] += d.type == 1 and d.n_pages >= 5
        c["cap"] += d.type == 1 and d.bch_len == 63 + 10 * 42
        c["ibc_max"] += d.type == 2 and d.bch_len == 8 * 21
        c["chase_frames"] += n_chase >= 2
        c["prefix"] += plan == "chase_fail" and d.bch_len < 21 * len(pos)
    return c


def assert_frame_coverage(c):
    assert c["ira"] >= 60 and c["ibc"] >= 15 and c["pages5"] >= 30 and c["cap"] >= 8 and c["ibc_max"] >= 5, c
    assert c["uplink"] >= 30 and c["odd"] >= 10 and c["tied_llr"] >= 40, c
    assert c["chase_frames"] >= 10 and c["prefix"] >= 3 and c["multi_mask"] >= 5 and c["tie_fifth"] >= 5, c


@pytest.mark.parametrize("seed", range(2))
def test_oracle_matches_ida_decode_c_on_long_frames(oracle, refpins, seed):
    R = refpins.lib
    oracle.orc_ida_decode.restype = C.c_int
    cases = make_long_ida_cases(seed)
    ours, theirs = [], []
    for bits, llr, direction, _ in cases:
        ro, do = ida_decode_with(oracle.orc_ida_decode, bits, llr, direction)
        ours.append((ro, ida_tuple(do)))
        if R:
            R.ref_ida_decode.restype = C.c_int
            rr, dr = ida_decode_with(R.ref_ida_decode, bits, llr, direction)
            assert (ro, ida_tuple(do)) == (rr, ida_tuple(dr)), (len(bits), ida_tuple(do)[:15], ida_tuple(dr)[:15])
            theirs.append((rr, ida_tuple(dr)))
    refpins.same("ida_decode_long/%d" % seed, ours, theirs)
    assert_ida_coverage(ida_coverage(cases, lambda b, l, d: ida_decode_with(oracle.orc_ida_decode, b, l, d)))


@pytest.mark.parametrize("seed", range(2))
def test_oracle_matches_frame_decode_c_on_long_frames(oracle, refpins, seed):
    R = refpins.lib
    oracle.orc_frame_decode.restype = C.c_int
    cases = make_long_frame_cases(seed)
    ours, theirs = [], []
    for bits, llr, _ in cases:
        ro, do = decode_with(oracle.orc_frame_decode, bits, llr)
        ours.append((ro, as_tuple(do)))
        if R:
            R.ref_frame_decode.restype = C.c_int
            rr, dr = decode_with(R.ref_frame_decode, bits, llr)
            assert ro == rr and as_tuple(do) == as_tuple(dr), (len(bits), as_tuple(do), as_tuple(dr))
            theirs.append((rr, as_tuple(dr)))
    refpins.same("frame_decode_long/%d" % seed, ours, theirs)
    assert_frame_coverage(frame_coverage(cases, lambda b, l: decode_with(oracle.orc_frame_decode, b, l)))
