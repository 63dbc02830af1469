"""Test-side ENCODER for the frames frame_decode() (frame_decode.c) recognises: BCH(31,21) + parity blocks,
the Iridium 2-way / 3-way symbol interleavers, IRA (ring alert) and IBC (broadcast) layouts, access codes.
Independent of the decoder under test: it is the inverse written from the bit layout, used to build inputs with known
answers, with controlled bit errors and reliabilities for the Chase decoder."""
import numpy as np

ACCESS_DL = [0, 0, 1, 1, 0, 0, 0, 0, 0, 0, 1, 1, 0, 0, 0, 0, 1, 1, 1, 1, 0, 0, 1, 1]
ACCESS_UL = [1, 1, 0, 0, 1, 1, 0, 0, 0, 0, 1, 1, 1, 1, 0, 0, 1, 1, 1, 1, 1, 1, 0, 0]
POLY_RA, POLY_HDR = 1207, 29


def gf2_rem(poly, val):
    pb = poly.bit_length()
    for i in range(31, pb - 2, -1):
        if val & (1 << i):
            val ^= poly << (i - pb + 1)
    return val


def to_bits(v, n):
    return [(v >> (n - 1 - i)) & 1 for i in range(n)]


def bch_block32(data21):
    """21 data bits -> 32-bit block: data | 10 check bits | overall parity (even weight)"""
    v = 0
    for b in data21:
        v = (v << 1) | int(b)
    cw = (v << 10) | gf2_rem(POLY_RA, v << 10)
    bits = to_bits(cw, 31)
    return bits + [sum(bits) & 1]


def interleave2(b1, b2):
    """inverse of de_interleave: 2 x 32 bits -> 64 bits"""
    out = [0] * 64
    for p in range(16):
        s = 31 - 2 * p
        out[2 * s], out[2 * s + 1] = b1[2 * p], b1[2 * p + 1]
        s = 30 - 2 * p
        out[2 * s], out[2 * s + 1] = b2[2 * p], b2[2 * p + 1]
    return out


def interleave3(b1, b2, b3):
    out = [0] * 96
    for p in range(16):
        for blk, base in ((b1, 47), (b2, 46), (b3, 45)):
            s = base - 3 * p
            out[2 * s], out[2 * s + 1] = blk[2 * p], blk[2 * p + 1]
    return out


def s12(v):
    """12-bit field of extract_signed12: sign bit + 11 bits, value = mag - 2048 when the sign bit is set"""
    return [1] + to_bits(v + 2048, 11) if v < 0 else [0] + to_bits(v, 11)


def ira_stream(sat, beam, x, y, z, pages, rng, terminate=True):
    hdr = to_bits(sat, 7) + to_bits(beam, 6) + s12(x) + s12(y) + s12(z) + [int(b) for b in rng.integers(0, 2, 14)]
    assert len(hdr) == 63
    st = list(hdr)
    for tmsi, msc in pages:
        st += to_bits(tmsi, 32) + [int(b) for b in rng.integers(0, 2, 2)] + to_bits(msc, 5) + \
              [int(b) for b in rng.integers(0, 2, 3)]
    if terminate:
        st += [1] * 42
    return st


def ira_frame(stream, uplink=False):
    """data stream (multiple of 21 bits; 63 header + 42 per page) -> frame bits incl. access code"""
    assert len(stream) % 21 == 0 and len(stream) >= 63
    return ira_frame_blocks([bch_block32(stream[i:i + 21]) for i in range(0, len(stream), 21)], uplink)


def ira_frame_blocks(blocks, uplink=False):
    """3 head blocks + pairs of 32-element blocks -> frame; the elements may be labels (block_positions)"""
    bits = list(ACCESS_UL if uplink else ACCESS_DL) + interleave3(*blocks[:3])
    rest = blocks[3:]
    for i in range(0, len(rest) - 1, 2):
        bits += interleave2(rest[i], rest[i + 1])
    return bits


def ibc_frame(bc_type, stream, uplink=False):
    """bc_type 0..3 (what 6 header bits can carry), stream = multiple of 42 data bits"""
    assert len(stream) % 42 == 0 and len(stream) >= 42
    hv = (bc_type << 4) | gf2_rem(POLY_HDR, bc_type << 4)
    return ibc_frame_blocks(to_bits(hv, 6), [bch_block32(stream[i:i + 21]) for i in range(0, len(stream), 21)], uplink)


def ibc_frame_blocks(hdr6, blocks, uplink=False):
    bits = list(ACCESS_UL if uplink else ACCESS_DL) + list(hdr6)
    for i in range(0, len(blocks), 2):
        bits += interleave2(blocks[i], blocks[i + 1])
    return bits


def ibc_stream(sat, beam, timeslot, sv_blocking, iri_time, rng, n_blocks=2):
    b1 = to_bits(sat, 7) + to_bits(beam, 6) + [int(rng.integers(0, 2))] + [timeslot, sv_blocking] + \
         [int(b) for b in rng.integers(0, 2, 26)]
    st = list(b1)
    if n_blocks >= 2:
        typ = 1 if iri_time is not None else int(rng.integers(2, 64))
        st += to_bits(typ, 6) + [int(b) for b in rng.integers(0, 2, 4)] + to_bits(iri_time or 0, 32)
    for _ in range(n_blocks - 2):
        st += [int(b) for b in rng.integers(0, 2, 42)]
    return st


def corrupt(bits, rng, n_errors, first=24, reliable=1.0, weak=0.05, mark=True, extra_weak=0):
    """flip n_errors random bits after the access code; LLRs: `reliable` everywhere, `weak` on the flipped bits when
    mark (so the Chase decoder can find them), plus extra_weak decoys"""
    bits = list(bits)
    llr = np.full(len(bits), reliable, np.float32) + rng.random(len(bits)).astype(np.float32) * 0.1
    idx = rng.choice(np.arange(first, len(bits)), size=min(n_errors, len(bits) - first), replace=False)
    for i in idx:
        bits[i] ^= 1
        if mark:
            llr[i] = weak * float(rng.random())
    for i in rng.choice(np.arange(first, len(bits)), size=min(extra_weak, len(bits) - first), replace=False):
        llr[i] = weak * float(rng.random())
    return bits, llr


# ---------------------------------------------------------------- IDA (ida_decode.c) ----
POLY_DA, POLY_LCW2, POLY_LCW3 = 3545, 465, 41
LCW_PERM = [40, 39, 36, 35, 32, 31, 28, 27, 24, 23, 20, 19, 16, 15, 12, 11, 8, 7, 4, 3,
            41, 38, 37, 34, 33, 30, 29, 26, 25, 22, 21, 18, 17, 14, 13, 10, 9, 6, 5, 2,
            1, 46, 45, 44, 43, 42]


def lcw_bits(ft, d5, lcw3):
    """46 on-air LCW bits: lcw1 = BCH(7,3) of ft, lcw2 = 13-bit codeword of 5 data bits (generator 465; the decoder reads
    its top 6 bits as lcw_ft (2) + lcw_code (4)), lcw3 = BCH(26,21) of lcw3; permuted and pair-swapped as the air
    interface does (inverse of decode_lcw's two steps)"""
    v1 = (ft << 4) | gf2_rem(POLY_HDR, ft << 4)
    v2 = (d5 << 8) | gf2_rem(POLY_LCW2, d5 << 8)
    v3 = (lcw3 << 5) | gf2_rem(POLY_LCW3, lcw3 << 5)
    lb = to_bits(v1, 7) + to_bits(v2, 13) + to_bits(v3, 26)
    swapped = [0] * 46
    for i in range(46):
        swapped[LCW_PERM[i] - 1] = lb[i]
    data = [0] * 46
    for i in range(0, 46, 2):
        data[i + 1], data[i] = swapped[i], swapped[i + 1]
    return data


def crc_ccitt(data):
    crc = 0xFFFF
    for b in data:
        crc ^= b << 8
        for _ in range(8):
            crc = ((crc << 1) ^ 0x1021) & 0xFFFF if crc & 0x8000 else (crc << 1) & 0xFFFF
    return crc


def ida_stream(da_ctr, da_len, cont, payload20, rng, good_crc=True):
    """200 decoded bits: header (cont @3, ctr @5-7, len @11-15, zero @17-19), 20 payload bytes, CRC-CCITT, 4 spare"""
    hdr = [int(b) for b in rng.integers(0, 2, 20)]
    hdr[3] = cont
    hdr[5:8] = to_bits(da_ctr, 3)
    hdr[11:16] = to_bits(da_len, 5)
    hdr[17:20] = [0, 0, 0]
    pl = []
    for by in payload20:
        pl += to_bits(by, 8)
    msg_bits = hdr + [0] * 12 + pl
    msg = [int("".join(map(str, msg_bits[i:i + 8])), 2) for i in range(0, len(msg_bits), 8)]
    crc = crc_ccitt(msg)
    if not good_crc:
        crc ^= 0x0101
    return hdr + pl + to_bits(crc, 16) + [int(b) for b in rng.integers(0, 2, 4)]


def da_block31(data20):
    v = int("".join(map(str, data20)), 2)
    return to_bits((v << 11) | gf2_rem(POLY_DA, v << 11), 31)


def interleave_n(h1, h2, n_sym):
    """inverse of de_interleave_n: h1 <- symbols n-1, n-3, ..; h2 <- symbols n-2, n-4, .."""
    out = [0] * (2 * n_sym)
    p = 0
    for s in range(n_sym - 1, 0, -2):
        out[2 * s], out[2 * s + 1] = h1[p], h1[p + 1]
        p += 2
    p = 0
    for s in range(n_sym - 2, -1, -2):
        out[2 * s], out[2 * s + 1] = h2[p], h2[p + 1]
        p += 2
    return out


def ida_frame(lcw, stream200, rng, uplink=False):
    """access code + LCW + two 124-bit blocks (chunks in air order 3,1,2,0) + the 64-bit tail block = 382 bits"""
    assert len(stream200) == 200
    ch = [da_block31(stream200[i:i + 20]) for i in range(0, 200, 20)]
    bits = list(ACCESS_UL if uplink else ACCESS_DL) + list(lcw)
    for blk in range(2):
        s = ch[4 * blk:4 * blk + 4]
        comb = s[3] + s[1] + s[2] + s[0]
        bits += interleave_n(comb[:62], comb[62:], 62)
    h2 = [int(rng.integers(0, 2))] + ch[8]
    h1 = [int(rng.integers(0, 2))] + ch[9]
    bits += interleave_n(h1, h2, 32)
    assert len(bits) == 382
    return bits


# ------------------------------------------------ long frames, error placement, tied LLRs ----
IDA_MAX_CHUNKS = 28        # 6 full 124-bit blocks of 4 chunks (kMaxBits = 896) + at most 3 tail chunks; 25 fit the 512-bit stream


def ida_tail_chunks(ns):
    """31-bit chunks the tail of ns symbols holds: its halves without their first bits, 2 * (ns - 1) bits"""
    return min(3, 2 * (ns - 1) // 31) if ns > 1 else 0


def ida_long_frame(lcw, chunks, n_full, ns, fill, uplink=False):
    """access code + LCW + n_full 124-bit blocks (chunks 4b..4b+3, air order 3,1,2,0) + a tail of ns symbols whose halves,
    without their first bits, (h2[1..] then h1[1..]) begin with the remaining chunks.  `fill` yields every other element:
    the halves' first bits, what follows the chunks, and symbol 0 of an odd tail (de_interleave_n reads neither half from
    it).  The elements may be labels (block_positions)."""
    assert 4 * n_full <= len(chunks) <= 4 * n_full + ida_tail_chunks(ns)
    out = list(ACCESS_UL if uplink else ACCESS_DL) + list(lcw)
    for blk in range(n_full):
        s = chunks[4 * blk:4 * blk + 4]
        comb = list(s[3]) + list(s[1]) + list(s[2]) + list(s[0])
        out += interleave_n(comb[:62], comb[62:], 62)
    if ns:
        comb = [x for c in chunks[4 * n_full:] for x in c]
        comb += [next(fill) for _ in range(max(0, 2 * (ns - 1) - len(comb)))]
        h2 = [next(fill)] + comb[:ns - 1]
        h1 = [next(fill)] + comb[ns - 1:]
        t = interleave_n(h1, h2, ns)
        if ns % 2:
            t[0], t[1] = next(fill), next(fill)
        out += t
    return out


def block_positions(build, blocks, width, *args, **kw):
    """frame bit index of every element of every block: `build` run on labels instead of bits"""
    lab = [[("b", i, k) for k in range(width)] for i in range(len(blocks))]
    frame = build(lab, *args, **kw)
    pos = [[None] * width for _ in blocks]
    for j, x in enumerate(frame):
        if isinstance(x, tuple) and x[0] == "b":
            pos[x[1]][x[2]] = j
    return pos


def labels():
    k = 0
    while True:
        yield ("f", k)
        k += 1


def bits_from(rng):
    while True:
        yield int(rng.integers(0, 2))


def syndrome_table(poly, nbits, max_err, size):
    """remainder -> error pattern of every 1- and 2-bit pattern, the first one found winning (build_syndrome_table)"""
    t = {}
    for b1 in range(nbits):
        r = gf2_rem(poly, 1 << b1)
        if r < size:
            t[r] = 1 << b1
    if max_err >= 2:
        for b1 in range(nbits):
            for b2 in range(b1 + 1, nbits):
                r = gf2_rem(poly, (1 << b1) | (1 << b2))
                if r < size and r not in t:
                    t[r] = (1 << b1) | (1 << b2)
    return t


_SYN = {}


def chase_model(cw_bits, llr31, poly=POLY_DA, size=2048):
    """chase_bch_da / chase_bch_decode_p's BCH part on a 31-bit codeword (bits in air order), for coverage counts:
    ('table' | 'chase' | 'fail', the codewords every flip mask 1..31 decodes to in mask order, whether the fifth and sixth
    smallest LLRs are equal -- a tie the selection sort's swaps decide)"""
    if poly not in _SYN:
        _SYN[poly] = syndrome_table(poly, 31, 2, size)
    tab = _SYN[poly]
    cw = int("".join(str(int(b)) for b in cw_bits), 2)
    syn = gf2_rem(poly, cw)
    if syn == 0 or syn in tab:
        return "table", [], False
    pos = list(range(31))
    for i in range(5):
        mi = i
        for j in range(i + 1, 31):
            if llr31[pos[j]] < llr31[pos[mi]]:
                mi = j
        pos[i], pos[mi] = pos[mi], pos[i]
    srt = sorted(float(v) for v in llr31)
    hits = []
    for mask in range(1, 32):
        f = cw
        for k in range(5):
            if mask & (1 << k):
                f ^= 1 << (30 - pos[k])
        syn = gf2_rem(poly, f)
        if syn == 0 or syn in tab:
            hits.append(f ^ tab.get(syn, 0))
    return ("chase" if hits else "fail"), hits, srt[4] == srt[5]


def tie_llr(llr, mode, rng):
    """reliabilities with ties: 'quarter' (rounded to multiples of 1/4), 'two' (two values), 'equal' (one value off the
    weak bits), 'zero' (all zero), anything else unchanged"""
    llr = np.asarray(llr, np.float32)
    if mode == "quarter":
        return np.round(llr * 4.0).astype(np.float32) / 4.0
    if mode == "two":
        return np.where(llr < 0.5, 0.25, 1.0).astype(np.float32)
    if mode == "equal":
        return np.where(llr < 0.5, llr, 1.0).astype(np.float32)
    if mode == "zero":
        return np.zeros_like(llr)
    return llr


def plant_errors(bits, llr, positions, n, rng, weak=None, tie_fifth=False):
    """flip n of a block's bits (positions: its frame indices); weak: how many of the flipped bits get a low LLR (all of
    them by default).  tie_fifth: the block's five lowest LLRs end in a tie -- positions 5 and 6 of the sorted order
    carry the same value, so the selection sort's swaps decide which of the two is flipped.  A position of None (the
    element an odd IDA tail does not carry) is left alone"""
    positions = [q for q in positions if q is not None]
    idx = [int(i) for i in rng.choice(len(positions), size=n, replace=False)]
    weak = n if weak is None else weak
    for j, i in enumerate(idx):
        bits[positions[i]] ^= 1
        if j < weak:
            llr[positions[i]] = 0.05 * float(rng.random())
    if tie_fifth:
        rest = [i for i in range(len(positions)) if i not in idx]
        order = [int(i) for i in rng.permutation(rest)]
        k = 0
        for j in range(weak, 4):            # four distinct low values below the tie, then the tie
            llr[positions[order[k]]] = 0.06 + 0.01 * j
            k += 1
        for i in order[k:k + 2]:
            llr[positions[i]] = 0.2
    return idx


_PROOF = {}


def chase_proof(poly=POLY_DA, size=2048):
    """(five positions W, syndrome s) such that no flip of a subset of W turns a word of syndrome s into one the table or
    a zero syndrome accepts: a block whose five least reliable bits are W and whose syndrome is s fails Chase decoding.
    Found by a seeded search (rare for BCH(31,20): about one 5-set in 200 has such an s)."""
    if poly not in _PROOF:
        bad = np.zeros(size, bool)
        bad[0] = True
        bad[list(syndrome_table(poly, 31, 2, size))] = True
        rng = np.random.default_rng(12345)
        while poly not in _PROOF:
            W = sorted(int(w) for w in rng.choice(31, 5, replace=False))
            T = np.array([gf2_rem(poly, sum(1 << (30 - W[k]) for k in range(5) if m >> k & 1)) for m in range(32)])
            ok = ~bad[np.bitwise_xor.outer(np.arange(size), T)].any(axis=1)
            if ok.any():
                _PROOF[poly] = (W, int(np.flatnonzero(ok)[0]))
    return _PROOF[poly]


def plant_failure(bits, llr, positions, poly=POLY_DA, size=2048):
    """make a block (positions: the frame indices of its 31 codeword bits) fail Chase decoding: its five least reliable
    bits are chase_proof's W and the error pattern is the proof's syndrome itself (bits 30 - b for every bit b of s)"""
    W, s = chase_proof(poly, size)
    for k, q in enumerate(positions):
        if q is None:
            continue
        llr[q] = 0.01 + 0.01 * W.index(k) if k in W else max(float(llr[q]), 1.0)
    for b in range(11):
        if s >> b & 1 and positions[30 - b] is not None:
            bits[positions[30 - b]] ^= 1
