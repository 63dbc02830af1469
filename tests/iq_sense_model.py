"""TEST INFRASTRUCTURE: the model of option iq_sense (iq_sense_kernel, csrc/bitlayer.hip): the three predicates of
include/irdm_hip.h in numpy / plain Python over tests/bitlayer.py's polynomials, the IDA predicate through the CPU oracle's
orc_ida_decode, each in the recorded and in the exchanged sense; and the numpy model of the exchange kernel."""
import numpy as np

import bitlayer as bl
import bitlayer_checks as bc
import irdm

ACCESS = (0x3030F3, 0xCC3CFC)
IRA, IBC, IDA = 1, 2, 4


def exchange(bits, llr):
    """b'[2i] = b[2i+1], b'[2i+1] = b[2i] over the whole dibits of the frame, the LLRs following their bits"""
    n = len(bits) & ~1
    idx = np.arange(n) ^ 1
    b = np.asarray(bits, np.uint8)[:n][idx]
    return b, (None if llr is None else np.asarray(llr, np.float32)[:n][idx])


def _word(bits):
    v = 0
    for b in bits:
        v = (v << 1) | int(b)
    return v


def clean_block(data, first_sym, stride):
    """a de-interleaved 32-bit block (symbols first_sym, first_sym - stride, ...): zero BCH(31,21) remainder over its first 31
    bits and even weight over all 32, nothing corrected"""
    blk = []
    for p in range(16):
        s = first_sym - stride * p
        blk += [int(data[2 * s]), int(data[2 * s + 1])]
    return bl.gf2_rem(bl.POLY_RA, _word(blk[:31])) == 0 and sum(blk) % 2 == 0


def predicates(bits, llr, direction):
    """the mask of the predicates that hold on an even number of bits (llr: an array, never None)"""
    n = len(bits)
    m = 0
    if n < 24:
        return 0
    if _word(bits[:24]) in ACCESS:
        data = bits[24:]
        if n - 24 >= 96 and all(clean_block(data, f, 3) for f in (47, 46, 45)):
            m |= IRA
        if n - 24 >= 6 + 64 and bl.gf2_rem(bl.POLY_HDR, _word(data[:6])) == 0 and \
                clean_block(data[6:], 31, 2) and clean_block(data[6:], 30, 2):
            m |= IBC
    o = bc.oracle_ida(bits, llr, direction)
    if o.ok and o.da_len > 0 and o.crc_ok:
        m |= IDA
    return m


def vote(bits, llr, direction):
    """(recorded, exchanged, n_bits) of one frame as the kernel reports them; llr None: all-zero LLRs, as a Demod record
    carries them"""
    n = len(bits) & ~1
    b = np.asarray(bits, np.uint8)[:n]
    l = np.zeros(n, np.float32) if llr is None else np.asarray(llr, np.float32)[:n]
    xb, xl = exchange(b, l)
    return predicates(b, l, direction), predicates(xb, xl, direction), n


def decides(rec, exch):
    """'recorded' / 'exchanged' / 'both' / None"""
    if rec and exch:
        return "both"
    return "recorded" if rec else ("exchanged" if exch else None)


def verdict(n_rec, n_exch):
    d = n_rec + n_exch
    if d < 5:
        return irdm.IQ_TOO_FEW
    if 10 * n_rec >= 9 * d:
        return irdm.IQ_AS_RECORDED
    return irdm.IQ_EXCHANGED if 10 * n_exch >= 9 * d else irdm.IQ_MIXED


def swap_bytes(raw, width):
    """the exchange kernel on a byte array of whole samples: the two `width`-byte components of every sample exchanged"""
    a = np.asarray(raw, np.uint8).reshape(-1, 2, width)
    return np.ascontiguousarray(a[:, ::-1, :]).reshape(-1)


def swap_complex(iq):
    return (iq.imag + 1j * iq.real).astype(np.complex64)
