// bitlayer_emul.cpp -- TEST INFRASTRUCTURE: csrc/bitlayer.hip's four decode kernels -- frame_decode_kernel and
// frame_packed_kernel (frame_decode.c:414-598: access-code check, de-interleave, BCH by syndrome tables, Chase decoding on
// the LLRs, IRA / IBC field extraction), ida_decode_kernel and ida_packed_kernel (ida_decode.c:543-660: LCW, payload
// descramble, BCH(31,20) + Chase, CRC-CCITT) -- on the CPU emulation of tests/hip_emul/hip/hip_runtime.h, with the
// syndrome tables built as csrc/create.cpp builds them (frame_decode.c:95-129, ida_decode.c:96-102), against the oracle's
// frame_decode / ida_decode (themselves pinned to the reference's object code).
#include <hip/hip_runtime.h>
#include <vector>

#include "bitlayer_emul.inc"

using namespace irdm;

namespace {

unsigned poly_rem(unsigned poly, unsigned v)
{
    if (!v) return 0u;
    const int pb = 32 - __builtin_clz(poly);
    for (int i = 31; i >= pb - 1; i--)
        if (v & (1u << i)) v ^= poly << (i - pb + 1);
    return v;
}

// remainder of every 1- and 2-bit error pattern -> (number of errors, pattern); csrc/create.cpp irdm_create
std::vector<int2> syndrome_table(unsigned poly, int nbits, int max_err, int size)
{
    std::vector<int2> t((size_t)size, make_int2(-1, 0));
    for (int b1 = 0; b1 < nbits; b1++) {
        const unsigned v = 1u << b1, r = poly_rem(poly, v);
        if (r < (unsigned)size) t[r] = make_int2(1, (int)v);
    }
    if (max_err >= 2)
        for (int b1 = 0; b1 < nbits; b1++)
            for (int b2 = b1 + 1; b2 < nbits; b2++) {
                const unsigned v = (1u << b1) | (1u << b2), r = poly_rem(poly, v);
                if (r < (unsigned)size && t[r].x < 0) t[r] = make_int2(2, (int)v);
            }
    return t;
}

// ida_decode_init (ida_decode.c:96-102), as csrc/create.cpp builds the tables
void ida_tables(std::vector<int2> &da, std::vector<int2> &l1, std::vector<int2> &l2, std::vector<int2> &l3)
{
    da = syndrome_table(3545u, 31, 2, 2048);
    l1 = syndrome_table(29u, 7, 1, 16);
    l2 = syndrome_table(465u, 14, 1, 256);
    l3 = syndrome_table(41u, 26, 2, 32);
}

// bits: [n][kMaxBits] hard bits, llr: [n][kMaxBits] or nullptr, n_bits[n], direction[n] or nullptr -> DemodOut records
std::vector<DemodOut> records(const uint8_t *bits, const float *llr, const int *n_bits, const int *direction, int n)
{
    std::vector<DemodOut> frames(n);
    for (int i = 0; i < n; i++) {
        memset(&frames[i], 0, sizeof(DemodOut));
        frames[i].ok = 1;
        frames[i].n_symbols = n_bits[i] / 2;
        frames[i].direction = direction ? direction[i] : 0;
        memcpy(frames[i].bits, bits + (size_t)i * kMaxBits, kMaxBits);
        if (llr) memcpy(frames[i].llr, llr + (size_t)i * kMaxBits, sizeof(float) * kMaxBits);
    }
    return frames;
}

}  // namespace

extern "C" {

// bits: [n][kMaxBits] hard bits, llr: [n][kMaxBits] (ignored unless use_llr), n_bits[n]; out: n DecodedOut
int bitlayer_emul_frame_decode(const uint8_t *bits, const float *llr, const int *n_bits, int n, int use_llr, DecodedOut *out)
{
    std::vector<DemodOut> frames = records(bits, llr, n_bits, nullptr, n);
    std::vector<int2> ra = syndrome_table(1207u, 31, 2, 1024), hdr = syndrome_table(29u, 7, 1, 16);
    memset(out, 0, sizeof(DecodedOut) * n);
    return launch_frame_decode(frames.data(), n, ra.data(), hdr.data(), use_llr, n_bits, out, nullptr);
}

// the same frames through the packed kernels, which read n_bits = 2 * n_symbols (n_bits[i] must be even), the direction
// and the LLRs from the record: out n FramePacked
int bitlayer_emul_frame_packed(const uint8_t *bits, const float *llr, const int *n_bits, int n, FramePacked *out)
{
    std::vector<DemodOut> frames = records(bits, llr, n_bits, nullptr, n);
    std::vector<int2> ra = syndrome_table(1207u, 31, 2, 1024), hdr = syndrome_table(29u, 7, 1, 16);
    memset(out, 0xA5, sizeof(FramePacked) * n);          // every word must be written
    return launch_frame_packed(frames.data(), n, ra.data(), hdr.data(), out, nullptr);
}

// direction[n]; out n IdaOut (ida_decode_kernel, n_bits and direction from the arrays, LLRs when use_llr)
int bitlayer_emul_ida_decode(const uint8_t *bits, const float *llr, const int *n_bits, const int *direction, int n,
                             int use_llr, IdaOut *out)
{
    std::vector<DemodOut> frames = records(bits, llr, n_bits, direction, n);
    std::vector<int2> da, l1, l2, l3;
    ida_tables(da, l1, l2, l3);
    memset(out, 0, sizeof(IdaOut) * n);
    return launch_ida_decode(frames.data(), n, da.data(), l1.data(), l2.data(), l3.data(), use_llr, n_bits, direction, out,
                             nullptr);
}

// out n IdaPacked (ida_packed_kernel: n_bits[i] even, direction and LLRs from the record)
int bitlayer_emul_ida_packed(const uint8_t *bits, const float *llr, const int *n_bits, const int *direction, int n,
                             IdaPacked *out)
{
    std::vector<DemodOut> frames = records(bits, llr, n_bits, direction, n);
    std::vector<int2> da, l1, l2, l3;
    ida_tables(da, l1, l2, l3);
    memset(out, 0xA5, sizeof(IdaPacked) * n);
    return launch_ida_packed(frames.data(), n, da.data(), l1.data(), l2.data(), l3.data(), out, nullptr);
}

int bitlayer_emul_sizes(int *decoded_bytes, int *max_bits)
{
    *decoded_bytes = (int)sizeof(DecodedOut);
    *max_bits = kMaxBits;
    return 0;
}

int bitlayer_emul_record_sizes(int *ida_bytes, int *ida_packed_bytes, int *frame_packed_bytes)
{
    *ida_bytes = (int)sizeof(IdaOut);
    *ida_packed_bytes = (int)sizeof(IdaPacked);
    *frame_packed_bytes = (int)sizeof(FramePacked);
    return 0;
}

}
