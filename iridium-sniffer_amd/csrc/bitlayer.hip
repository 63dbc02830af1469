// bitlayer.hip -- post-demod bit layer on gfx950: frame_decode() (frame_decode.c:414-598), SURVEY 8f row 3.
//
//   access code check (:428-431) -> IBC: BCH(7,3) header (:441-452), 2-way de-interleave (:156-176), BCH(31,21)
//   with Chase decoding on the LLRs (:224-295), parity (:399-407), field extraction (:368-393)
//   -> IRA: 3-way de-interleave (:178-199), three header blocks, paging blocks (:317-366).
//
// Integer / bitwise work, independent per frame: one lane per frame.  Codewords live in 32-bit registers (bit 30 =
// first bit, as bits_to_uint builds them); the de-interleavers are address arithmetic on the frame's bit array.  The
// only floats are the LLR comparisons of the Chase decoder's selection of the five least reliable positions (first
// minimum wins, :256-266) -- ordering only, so the result is exact.  lat / lon / alt (double atan2 / sqrt, :336-342) are
// finished on the host with the host libm from the integer position this kernel returns.
#include "common.hpp"
#include "types.hpp"
#include "kernels.hpp"

namespace irdm {

namespace {

constexpr unsigned kPolyRa = 1207u;   // BCH(31,21), frame_decode.c:36
constexpr unsigned kPolyHdr = 29u;    // BCH(7,3),   frame_decode.c:37
constexpr int kChase = 5;             // frame_decode.c:48

__device__ __forceinline__ unsigned gf2_rem(unsigned poly, int poly_bits, unsigned val)      // :82-91
{
    for (int i = 31; i >= poly_bits - 1; i--)
        if (val & (1u << i)) val ^= poly << (i - poly_bits + 1);
    return val;
}

// one de-interleaved 32-bit block: symbols first, first-stride, ... (16 of them), two bits each
struct Block {
    unsigned cw;        // bits 0..30 of the block, first bit at position 30 (bits_to_uint(block32, 31))
    unsigned parity;    // bit 31 of the block
};

__device__ __forceinline__ Block gather_block(const uint8_t *__restrict__ in, int first_sym, int stride)
{
    unsigned w = 0;
#pragma unroll
    for (int p = 0; p < 16; p++) {
        const int s = first_sym - stride * p;
        w = (w << 2) | ((unsigned)(in[2 * s] & 1) << 1) | (unsigned)(in[2 * s + 1] & 1);
    }
    Block b;
    b.cw = w >> 1;
    b.parity = w & 1u;
    return b;
}

// LLR of block position k (0..30) of the same gather
__device__ __forceinline__ float block_llr(const float *__restrict__ llr, int first_sym, int stride, int k)
{
    const int s = first_sym - stride * (k >> 1);
    return llr[2 * s + (k & 1)];
}

// chase_bch_decode_p (:224-295): corrected codeword in *out (data = out >> 10, check = out & 0x3ff); returns the error
// count or -1
__device__ int chase_bch(const Block &b, const float *__restrict__ llr, int first_sym, int stride,
                         const int2 *__restrict__ syn_ra, unsigned *out)
{
    unsigned val = b.cw;
    unsigned syn = gf2_rem(kPolyRa, 11, val);
    if (syn == 0) { *out = val; return 0; }
    if (syn < 1024 && syn_ra[syn].x >= 0) { *out = val ^ (unsigned)syn_ra[syn].y; return syn_ra[syn].x; }
    if (!llr) return -1;
    // the five least reliable positions, partial selection sort with "first minimum wins" (:256-266): equivalent to
    // five passes of strict-less arg-min over the positions not yet taken, in the permuted order the swaps produce.
    // The permutation matters for ties only through the order of comparison; it is reproduced literally.
    int pos[31];
    for (int i = 0; i < 31; i++) pos[i] = i;
    for (int i = 0; i < kChase; i++) {
        int mi = i;
        float mv = block_llr(llr, first_sym, stride, pos[i]);
        for (int j = i + 1; j < 31; j++) {
            const float v = block_llr(llr, first_sym, stride, pos[j]);
            if (v < mv) { mv = v; mi = j; }
        }
        const int t = pos[i]; pos[i] = pos[mi]; pos[mi] = t;
    }
    unsigned fm[kChase];
    for (int i = 0; i < kChase; i++) fm[i] = 1u << (30 - pos[i]);
    for (int mask = 1; mask < (1 << kChase); mask++) {
        unsigned f = b.cw;
        for (int k = 0; k < kChase; k++)
            if (mask & (1 << k)) f ^= fm[k];
        syn = gf2_rem(kPolyRa, 11, f);
        if (syn == 0) { *out = f; return 0; }
        if (syn < 1024 && syn_ra[syn].x >= 0) { *out = f ^ (unsigned)syn_ra[syn].y; return syn_ra[syn].x; }
    }
    return -1;
}

// check_parity32 (:399-407): data + check + parity bit have even weight
__device__ __forceinline__ bool parity_ok(unsigned corrected, unsigned parity_bit)
{
    return ((__popc(corrected & 0x7fffffffu) + (int)parity_bit) & 1) == 0;
}

// the decoded data bits, 21 per block, packed MSB-first into 32-bit words of `stream`
__device__ __forceinline__ void append21(unsigned *stream, int &len, unsigned corrected)
{
    const unsigned d = (corrected >> 10) & 0x1fffffu;
    for (int i = 0; i < 21; i++) {
        const unsigned bit = (d >> (20 - i)) & 1u;
        const int k = len + i;
        stream[k >> 5] |= bit << (31 - (k & 31));
    }
    len += 21;
}

__device__ __forceinline__ unsigned sbit(const unsigned *stream, int k) { return (stream[k >> 5] >> (31 - (k & 31))) & 1u; }

__device__ __forceinline__ unsigned sfield(const unsigned *stream, int k, int n)             // extract_uint, :309-315
{
    unsigned v = 0;
    for (int i = 0; i < n; i++) v = (v << 1) | sbit(stream, k + i);
    return v;
}

__device__ __forceinline__ int ssigned12(const unsigned *stream, int k)                      // extract_signed12, :299-307
{
    const int mag = (int)sfield(stream, k + 1, 11);
    return sbit(stream, k) ? mag - (1 << 11) : mag;
}

// remaining 64-bit blocks (:478-497, :569-588)
__device__ void more_blocks(const uint8_t *data, const float *llr, int offset, int limit, const int2 *syn_ra,
                            unsigned *stream, int cap_bits, int &len)
{
    while (offset + 64 <= limit && len + 42 <= cap_bits) {
        const Block b1 = gather_block(data + offset, 31, 2), b2 = gather_block(data + offset, 30, 2);
        unsigned c1, c2;
        const int ea = chase_bch(b1, llr ? llr + offset : nullptr, 31, 2, syn_ra, &c1);
        const int eb = chase_bch(b2, llr ? llr + offset : nullptr, 30, 2, syn_ra, &c2);
        if (ea < 0 || eb < 0) break;
        if (!parity_ok(c1, b1.parity)) break;
        if (!parity_ok(c2, b2.parity)) break;
        append21(stream, len, c1);
        append21(stream, len, c2);
        offset += 64;
    }
}

}  // namespace

__global__ __launch_bounds__(64) void frame_decode_kernel(const DemodOut *__restrict__ frames, int n_frames,
                                                          const int2 *__restrict__ syn_ra,
                                                          const int2 *__restrict__ syn_hdr, int use_llr,
                                                          const int *__restrict__ n_bits_in,
                                                          DecodedOut *__restrict__ out)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_frames) return;
    const DemodOut &f = frames[i];
    DecodedOut o;
    memset(&o, 0, sizeof(o));
    // demod_frame_t.n_bits is 2 * n_symbols (qpsk_demod.c:478); the stage-alone entry passes arbitrary lengths
    const int n_bits = n_bits_in ? n_bits_in[i] : (f.ok ? 2 * f.n_symbols : 0);
    const uint8_t *bits = f.bits;
    // access codes (:51-56) as 24-bit words, first bit most significant
    unsigned acc = 0;
    if (n_bits >= 24)
        for (int k = 0; k < 24; k++) acc = (acc << 1) | (unsigned)(bits[k] & 1);
    const bool is_dl = acc == 0x3030F3u, is_ul = acc == 0xCC3CFCu;
    if (n_bits < 24 || (!is_dl && !is_ul)) { out[i] = o; return; }
    const uint8_t *data = bits + 24;
    const float *llr = use_llr ? f.llr + 24 : nullptr;
    const int data_len = n_bits - 24;

    if (data_len >= 6 + 64) {                                           // ---- IBC (:441-505)
        unsigned hv = 0;
        for (int k = 0; k < 6; k++) hv = (hv << 1) | (unsigned)(data[k] & 1);
        const unsigned hs = gf2_rem(kPolyHdr, 5, hv);
        bool hdr_ok = false;
        if (hs == 0) hdr_ok = true;
        else if (hs < 16 && syn_hdr[hs].x >= 0) { hv ^= (unsigned)syn_hdr[hs].y; hdr_ok = true; }
        if (hdr_ok) {
            const Block b1 = gather_block(data + 6, 31, 2), b2 = gather_block(data + 6, 30, 2);
            unsigned c1, c2;
            const int e1 = chase_bch(b1, llr ? llr + 6 : nullptr, 31, 2, syn_ra, &c1);
            const int e2 = chase_bch(b2, llr ? llr + 6 : nullptr, 30, 2, syn_ra, &c2);
            if (e1 >= 0 && e2 >= 0 && parity_ok(c1, b1.parity) && parity_ok(c2, b2.parity)) {
                unsigned stream[8];                                     // 256 bits (:466)
                for (int k = 0; k < 8; k++) stream[k] = 0;
                int len = 0;
                append21(stream, len, c1);
                append21(stream, len, c2);
                const int ibc_max = data_len < 262 ? data_len : 262;
                more_blocks(data, llr, 6 + 64, ibc_max, syn_ra, stream, 256, len);
                o.type = 2;
                o.bch_len = len;
                o.bc_type = (int)((hv >> 4) & 7u);
                if (len >= 42) {                                        // parse_ibc (:368-393)
                    o.sat_id = (int)sfield(stream, 0, 7);
                    o.beam_id = (int)sfield(stream, 7, 6);
                    o.timeslot = (int)sbit(stream, 14);
                    o.sv_blocking = (int)sbit(stream, 15);
                    if (len >= 84 && sfield(stream, 42, 6) == 1u) o.iri_time = sfield(stream, 52, 32);
                }
                out[i] = o;
                return;
            }
        }
    }

    if (data_len >= 96) {                                               // ---- IRA (:514-595)
        const Block b1 = gather_block(data, 47, 3), b2 = gather_block(data, 46, 3), b3 = gather_block(data, 45, 3);
        unsigned c1, c2, c3;
        const int e1 = chase_bch(b1, llr, 47, 3, syn_ra, &c1);
        const int e2 = chase_bch(b2, llr, 46, 3, syn_ra, &c2);
        const int e3 = chase_bch(b3, llr, 45, 3, syn_ra, &c3);
        if (e1 >= 0 && e2 >= 0 && e3 >= 0 && parity_ok(c1, b1.parity) && parity_ok(c2, b2.parity) &&
            parity_ok(c3, b3.parity)) {
            unsigned stream[16];                                        // 512 bits (:545)
            for (int k = 0; k < 16; k++) stream[k] = 0;
            int len = 0;
            append21(stream, len, c1);
            append21(stream, len, c2);
            append21(stream, len, c3);
            more_blocks(data, llr, 96, data_len, syn_ra, stream, 512, len);
            o.type = 1;
            o.bch_len = len;
            if (len >= 63) {                                            // parse_ira (:317-366)
                o.sat_id = (int)sfield(stream, 0, 7);
                o.beam_id = (int)sfield(stream, 7, 6);
                o.pos_xyz[0] = ssigned12(stream, 13);
                o.pos_xyz[1] = ssigned12(stream, 25);
                o.pos_xyz[2] = ssigned12(stream, 37);
                int off = 63;
                while (off + 42 <= len && o.n_pages < 12) {
                    bool all1 = true;
                    for (int k = 0; k < 42; k++)
                        if (!sbit(stream, off + k)) { all1 = false; break; }
                    if (all1) break;
                    o.page_tmsi[o.n_pages] = sfield(stream, off, 32);
                    o.page_msc[o.n_pages] = (int)sfield(stream, off + 34, 5);
                    o.n_pages++;
                    off += 42;
                }
            }
        }
    }
    out[i] = o;
}

// ---------------------------------------------------------------------------
// ida_decode() (ida_decode.c:543-665): Link Control Word (46 bits behind a pair swap and a permutation, three BCH
// codes, :193-252), payload descramble (124-bit blocks = 62 symbols de-interleaved into two halves, four 31-bit
// BCH(31,20) chunks in the order 3,1,2,0, then the short tail block with the first bit of each half dropped,
// :276-377), Chase decoding on the LLRs (:107-172), IDA header fields and CRC-CCITT (:580-637).
// One lane per frame; a chunk's 31 bits / LLRs are gathered through the index maps into registers / scratch.
// ---------------------------------------------------------------------------
namespace {

__constant__ int c_lcw_perm[46] = {                                     // ida_decode.c:54-60
    40, 39, 36, 35, 32, 31, 28, 27, 24, 23, 20, 19, 16, 15, 12, 11, 8, 7, 4, 3,
    41, 38, 37, 34, 33, 30, 29, 26, 25, 22, 21, 18, 17, 14, 13, 10, 9, 6, 5, 2,
    1, 46, 45, 44, 43, 42
};

// chase_bch_da (:107-172) on a gathered chunk: cw = 31 bits (first bit at position 30), l = its LLRs or nullptr
__device__ int chase_da(unsigned cw, const float *l, const int2 *__restrict__ syn_da, unsigned *out, int *fixed)
{
    unsigned syn = gf2_rem(3545u, 12, cw);
    if (syn == 0) { *out = cw; *fixed = 0; return 0; }
    if (syn < 2048 && syn_da[syn].x >= 0) { *out = cw ^ (unsigned)syn_da[syn].y; *fixed = 1; return syn_da[syn].x; }
    if (!l) return -1;
    int pos[31];
    for (int i = 0; i < 31; i++) pos[i] = i;
    for (int i = 0; i < kChase; i++) {
        int mi = i;
        float mv = l[pos[i]];
        for (int j = i + 1; j < 31; j++) {
            const float v = l[pos[j]];
            if (v < mv) { mv = v; mi = j; }
        }
        const int t = pos[i]; pos[i] = pos[mi]; pos[mi] = t;
    }
    unsigned fm[kChase];
    for (int i = 0; i < kChase; i++) fm[i] = 1u << (30 - pos[i]);
    for (int mask = 1; mask < (1 << kChase); mask++) {
        unsigned f = cw;
        for (int k = 0; k < kChase; k++)
            if (mask & (1 << k)) f ^= fm[k];
        syn = gf2_rem(3545u, 12, f);
        if (syn == 0) { *out = f; *fixed = 1; return 0; }
        if (syn < 2048 && syn_da[syn].x >= 0) { *out = f ^ (unsigned)syn_da[syn].y; *fixed = 1; return syn_da[syn].x; }
    }
    return -1;
}

// position j of de_interleave_n's out1 (half == 0) / out2 (half == 1) -> input bit index (:259-272)
__device__ __forceinline__ int deint_index(int n_sym, int half, int j)
{
    const int s = (n_sym - 1 - half) - 2 * (j >> 1);
    return 2 * s + (j & 1);
}

// position t of the tail's combined stream (h2[1..] then h1[1..], each half ns - 1 = hl bits) -> input bit index from the
// tail's start.  An odd ns leaves h2[ns - 1] unwritten by de_interleave_n (t = hl - 1); the reference's build reads there
// what its last full block's de-interleave left in the same storage: that block's half2[ns - 1], 124 bits back.
// (h1[ns - 1], t = 2 hl - 1, is in no chunk for an odd ns.)
__device__ __forceinline__ int tail_index(int ns, int hl, int t)
{
    if (t < hl) return (ns & 1) && t == hl - 1 ? deint_index(62, 1, ns - 1) - 124 : deint_index(ns, 1, t + 1);
    return deint_index(ns, 0, t - hl + 1);
}

__device__ __forceinline__ void put20(uint8_t *stream, int &len, unsigned corrected)
{
    const unsigned d = (corrected >> 11) & 0xfffffu;
    for (int i = 0; i < 20; i++) stream[len + i] = (uint8_t)((d >> (19 - i)) & 1u);
    len += 20;
}

}  // namespace

__global__ __launch_bounds__(64) void ida_decode_kernel(const DemodOut *__restrict__ frames, int n_frames,
                                                        const int2 *__restrict__ syn_da,
                                                        const int2 *__restrict__ syn_l1, const int2 *__restrict__ syn_l2,
                                                        const int2 *__restrict__ syn_l3, int use_llr,
                                                        const int *__restrict__ n_bits_in,
                                                        const int *__restrict__ direction_in,
                                                        IdaOut *__restrict__ out)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_frames) return;
    const DemodOut &f = frames[i];
    IdaOut &o = out[i];
    o.ok = 0;
    const int n_bits = n_bits_in ? n_bits_in[i] : (f.ok ? 2 * f.n_symbols : 0);
    const int direction = direction_in ? direction_in[i] : f.direction;
    if (n_bits < 24 + 46 + 124) return;                                 // :547-548
    if (direction != 1 && direction != 2) return;                       // :551-552
    const uint8_t *data = f.bits + 24;
    const float *llr = use_llr ? f.llr + 24 : nullptr;
    const int data_len = n_bits - 24;

    // ---- decode_lcw (:193-252): lcw_bits[i] = swapped[perm[i] - 1], swapped[k] = data[k ^ 1]
    unsigned v1 = 0, v2 = 0, v3 = 0;
    for (int k = 0; k < 46; k++) {
        const unsigned b = (unsigned)(data[(c_lcw_perm[k] - 1) ^ 1] & 1);
        if (k < 7) v1 = (v1 << 1) | b;
        else if (k < 20) v2 = (v2 << 1) | b;
        else v3 = (v3 << 1) | b;
    }
    v2 <<= 1;                                                           // 13 bits + trailing zero (:222)
    const unsigned s1 = gf2_rem(29u, 5, v1), s2 = gf2_rem(465u, 9, v2), s3 = gf2_rem(41u, 6, v3);
    if (s1 != 0) { if (s1 >= 16 || syn_l1[s1].x < 0) return; v1 ^= (unsigned)syn_l1[s1].y; }
    if (s2 != 0) { if (s2 >= 256 || syn_l2[s2].x < 0) return; v2 ^= (unsigned)syn_l2[s2].y; }
    if (s3 != 0) { if (s3 >= 32 || syn_l3[s3].x < 0) return; v3 ^= (unsigned)syn_l3[s3].y; }
    const int ft = (int)(v1 >> 4) & 7;
    if (ft != 2) return;                                                // :563-564
    const int d2 = (int)(v2 >> 8) & 0x3F;
    const int payload_len = data_len - 46;
    if (payload_len < 124) return;
    const uint8_t *pd = data + 46;
    const float *pl = llr ? llr + 46 : nullptr;

    // ---- descramble_payload (:276-377)
    uint8_t st[512];                                                    // the reference's bch_stream[512] (:571); the record keeps 256
    int len = 0, fixederrs = 0;
    const int max_bch = 512;
    const int n_full = payload_len / 124, remain = payload_len % 124;
    bool failed = false;
    for (int blk = 0; blk < n_full && !failed; blk++) {
        const uint8_t *b = pd + blk * 124;
        const float *bl = pl ? pl + blk * 124 : nullptr;
        for (int c = 0; c < 4; c++) {
            if (len + 20 > max_bch) break;
            const int off = (c == 0 ? 3 : c == 1 ? 1 : c == 2 ? 2 : 0) * 31;
            unsigned cw = 0;
            float l[31];
            for (int k = 0; k < 31; k++) {
                const int j = off + k;
                const int idx = j < 62 ? deint_index(62, 0, j) : deint_index(62, 1, j - 62);
                cw = (cw << 1) | (unsigned)(b[idx] & 1);
                l[k] = bl ? bl[idx] : 0.0f;
            }
            unsigned cor;
            int fixed = 0;
            if (chase_da(cw, bl ? l : nullptr, syn_da, &cor, &fixed) < 0) { failed = true; break; }
            fixederrs += fixed;
            put20(st, len, cor);
        }
    }
    if (!failed && remain >= 4 && len + 2 * (remain / 2 - 1) <= max_bch) {
        const int ns = remain / 2;
        const uint8_t *b = pd + n_full * 124;
        const float *bl = pl ? pl + n_full * 124 : nullptr;
        if (ns > 1 && len + 20 <= max_bch) {
            const int hl = ns - 1;                                      // each half without its first bit
            int clen = 2 * hl;
            if (clen > 128) clen = 128;
            int pos = 0;
            while (pos + 31 <= clen && len + 20 <= max_bch) {
                unsigned cw = 0;
                float l[31];
                for (int k = 0; k < 31; k++) {
                    const int idx = tail_index(ns, hl, pos + k);        // combined = h2[1..] then h1[1..]
                    cw = (cw << 1) | (unsigned)(b[idx] & 1);
                    l[k] = bl ? bl[idx] : 0.0f;
                }
                unsigned cor;
                int fixed = 0;
                if (chase_da(cw, bl ? l : nullptr, syn_da, &cor, &fixed) < 0) break;
                fixederrs += fixed;
                put20(st, len, cor);
                pos += 31;
            }
        }
    }
    if (len < 196) return;                                              // :577-578

    const int cont = st[3];
    const int da_ctr = (st[5] << 2) | (st[6] << 1) | st[7];
    const int da_len = (st[11] << 4) | (st[12] << 3) | (st[13] << 2) | (st[14] << 1) | st[15];
    if (((st[17] << 2) | (st[18] << 1) | st[19]) != 0) return;
    if (da_len > 20) return;
    for (int k = 0; k < 32; k++) o.payload[k] = 0;
    const int plen = da_len > 0 ? da_len : 20;
    for (int k = 0; k < plen; k++) {
        unsigned by = 0;
        for (int b = 0; b < 8; b++) by = (by << 1) | st[20 + k * 8 + b];
        o.payload[k] = (uint8_t)by;
    }
    int crc_ok = 0;
    unsigned stored = 0, computed = 0;
    if (da_len > 0) {                                                   // CRC-CCITT-FALSE over the re-packed bits (:606-637)
        for (int k = 0; k < 16; k++) stored = (stored << 1) | st[9 * 20 + k];
        const int crc_bits = 20 + 12 + (len - 20 - 4);
        if ((crc_bits + 7) / 8 <= 64) {
            unsigned crc = 0xFFFFu;
            int nb = 0;
            unsigned cur = 0;
            // bit-serial: feed the message bits MSB-first, byte-wise zero padding at the end as the packed buffer has
            const int total_bits = ((crc_bits + 7) / 8) * 8;
            for (int bp = 0; bp < total_bits; bp++) {
                unsigned bit = 0;
                if (bp < 20) bit = st[bp];
                else if (bp >= 32 && bp < crc_bits) bit = st[20 + (bp - 32)];
                cur = (cur << 1) | bit;
                if (++nb == 8) {
                    crc ^= (cur & 0xffu) << 8;
                    for (int j = 0; j < 8; j++) crc = (crc & 0x8000u) ? ((crc << 1) ^ 0x1021u) & 0xffffu : (crc << 1) & 0xffffu;
                    nb = 0;
                    cur = 0;
                }
            }
            computed = crc;
            crc_ok = computed == 0;
        }
    }
    for (int k = 0; k < 256; k++) o.bch_stream[k] = k < len ? st[k] : (uint8_t)0;
    o.ft = ft;
    o.lcw_ft = (d2 >> 4) & 3;
    o.lcw_code = d2 & 0xF;
    o.lcw3_val = v3 >> 5;
    o.ec_lcw = (s1 != 0) + (s2 != 0) + (s3 != 0);
    o.da_ctr = da_ctr;
    o.da_len = da_len;
    o.cont = cont;
    o.crc_ok = crc_ok;
    o.stored_crc = stored;
    o.computed_crc = computed;
    o.fixederrs = fixederrs;
    o.payload_len = plen;
    o.bch_len = len;
    o.ok = 1;
}

// ---------------------------------------------------------------------------
// ida_decode() on the packed record path (option parsed_records): the same decode as ida_decode_kernel, with LLRs, ONE
// WAVEFRONT PER FRAME, its IdaPacked record written straight into pinned host memory.
//   * LCW: lane k < 46 fetches LCW bit k, one ballot makes the three words; the three small BCH codes are wavefront-uniform.
//   * payload: one 31-bit chunk per lane (at most 6 full 124-bit blocks of four chunks + 3 tail chunks), in the
//     reference's order: the algebraic decode of every chunk at once; then the chunks that need Chase, in stream order,
//     each with its 31 candidate flip masks on lanes 1..31 and the lowest mask that decodes winning (the serial loop's
//     first success).  The five least reliable positions are chosen by the chunk's own lane, the serial partial
//     selection sort literally (its swaps decide ties), over the chunk's LLRs in LDS.
//   * the stream: which chunks the serial loop would have accepted (a prefix: it stops at the first failure or the
//     512-bit cap) is wavefront-uniform arithmetic on a ballot; the accepted chunks' 20 data bits go to LDS, the header
//     fields, payload bytes, CRC-CCITT (byte-wise table, the same remainder as the bit-serial form) and the packed
//     stream come from there.
// The frame's bits and LLRs are the DemodOut demod_par_kernel wrote on the device (keep_bits).  The record is complete in
// pinned memory, behind a system-scope fence, when the stream reaches the host's synchronisation -- as demod_export's.
// ---------------------------------------------------------------------------
namespace {

constexpr int kIdaChunks = 28;                                          // 4 * (826 / 124) + the tail's (<= 3)

struct Crc16Tab { uint16_t v[256]; };
constexpr Crc16Tab make_crc16_tab()
{
    Crc16Tab t{};
    for (int i = 0; i < 256; i++) {
        unsigned c = (unsigned)i << 8;
        for (int j = 0; j < 8; j++) c = (c & 0x8000u) ? ((c << 1) ^ 0x1021u) & 0xffffu : (c << 1) & 0xffffu;
        t.v[i] = (uint16_t)c;
    }
    return t;
}
__constant__ Crc16Tab c_crc16 = make_crc16_tab();

__device__ __forceinline__ bool da_table_ok(unsigned syn, const int2 *__restrict__ syn_da)
{
    return syn == 0 || (syn < 2048 && syn_da[syn].x >= 0);
}

}  // namespace

__global__ __launch_bounds__(64) void ida_packed_kernel(const DemodOut *__restrict__ frames, int n_frames,
                                                        const int2 *__restrict__ syn_da,
                                                        const int2 *__restrict__ syn_l1, const int2 *__restrict__ syn_l2,
                                                        const int2 *__restrict__ syn_l3, IdaPacked *__restrict__ hp_ida)
{
    __shared__ uint8_t s_bits[kMaxBits - 70];              // the payload's hard bits (behind access code and LCW)
    __shared__ float s_llr[kMaxBits - 70];
    __shared__ float s_cl[kIdaChunks][32];                  // a chunk's 31 LLRs in codeword order
    __shared__ uint8_t s_pos[kIdaChunks][32];               // its selection sort's permutation
    __shared__ uint8_t s_st[512];                           // the reference's bch_stream, one bit per byte
    __shared__ uint8_t s_msg[64];                           // the CRC's message bytes
    __shared__ __attribute__((aligned(4))) IdaPacked s_rec;
    const int b = blockIdx.x;
    const int lane = threadIdx.x;
    if (b >= n_frames) return;
    if (lane < 22) reinterpret_cast<uint32_t *>(&s_rec)[lane] = 0;
    const DemodOut &f = frames[b];
    const int ok_in = f.ok, ns_in = f.n_symbols, direction = f.direction;
    const int n_bits = ok_in ? 2 * ns_in : 0;
    // the record: ok = 0 for every frame ida_decode() rejects
    auto emit = [&]() {
        __syncthreads();
        if (lane < 22) reinterpret_cast<uint32_t *>(hp_ida + b)[lane] = reinterpret_cast<const uint32_t *>(&s_rec)[lane];
        __threadfence_system();
    };
    if (n_bits < 24 + 46 + 124 || n_bits > kMaxBits || (direction != 1 && direction != 2)) { emit(); return; }
    const uint8_t *data = f.bits + 24;
    const int data_len = n_bits - 24;

    // ---- decode_lcw (:193-252)
    const unsigned long long lm =
        __builtin_amdgcn_ballot_w64(lane < 46 && (data[(c_lcw_perm[lane < 46 ? lane : 0] - 1) ^ 1] & 1));
    unsigned v1 = 0, v2 = 0, v3 = 0;
    for (int k = 0; k < 46; k++) {
        const unsigned bk = (unsigned)(lm >> k) & 1u;
        if (k < 7) v1 = (v1 << 1) | bk;
        else if (k < 20) v2 = (v2 << 1) | bk;
        else v3 = (v3 << 1) | bk;
    }
    v2 <<= 1;
    const unsigned s1 = gf2_rem(29u, 5, v1), s2 = gf2_rem(465u, 9, v2), s3 = gf2_rem(41u, 6, v3);
    bool lcw_ok = true;
    if (s1 != 0) { if (s1 >= 16 || syn_l1[s1].x < 0) lcw_ok = false; else v1 ^= (unsigned)syn_l1[s1].y; }
    if (lcw_ok && s2 != 0) { if (s2 >= 256 || syn_l2[s2].x < 0) lcw_ok = false; else v2 ^= (unsigned)syn_l2[s2].y; }
    if (lcw_ok && s3 != 0) { if (s3 >= 32 || syn_l3[s3].x < 0) lcw_ok = false; else v3 ^= (unsigned)syn_l3[s3].y; }
    const int ft = (int)(v1 >> 4) & 7;
    const int payload_len = data_len - 46;
    if (!lcw_ok || ft != 2 || payload_len < 124) { emit(); return; }
    const int d2 = (int)(v2 >> 8) & 0x3F;

    // ---- the payload's bits and LLRs into LDS
    for (int i = lane; i < payload_len; i += 64) {
        s_bits[i] = data[46 + i] & 1;
        s_llr[i] = f.llr[24 + 46 + i];
    }
    const int n_full = payload_len / 124, remain = payload_len % 124;
    const int ns = remain / 2, hl = ns - 1;
    const int clen = 2 * hl > 128 ? 128 : 2 * hl;
    const int n_tail = remain >= 4 && ns > 1 ? clen / 31 : 0;
    const int n_chunks = 4 * n_full + n_tail;
    __syncthreads();

    // ---- descramble_payload (:276-377): every chunk's algebraic decode at once
    const bool mine = lane < n_chunks;
    unsigned cw = 0, cor = 0;
    bool good = false, need = false;
    int fixed = 0;
    if (mine) {
        const bool tail = lane >= 4 * n_full;
        const int c = lane & 3, blk = lane >> 2;
        const int off = (c == 0 ? 3 : c == 1 ? 1 : c == 2 ? 2 : 0) * 31;
        const int base = tail ? n_full * 124 : blk * 124;
        const int tpos = (lane - 4 * n_full) * 31;
        for (int k = 0; k < 31; k++) {
            int idx;
            if (!tail) {
                const int j = off + k;
                idx = j < 62 ? deint_index(62, 0, j) : deint_index(62, 1, j - 62);
            } else {
                idx = tail_index(ns, hl, tpos + k);                     // >= -124: inside the last full block
            }
            cw = (cw << 1) | (unsigned)s_bits[base + idx];
            s_cl[lane][k] = s_llr[base + idx];
        }
        const unsigned syn = gf2_rem(3545u, 12, cw);
        if (syn == 0) { cor = cw; good = true; }
        else if (syn < 2048 && syn_da[syn].x >= 0) { cor = cw ^ (unsigned)syn_da[syn].y; good = true; fixed = 1; }
        else need = true;
    }
    // Chase (:107-172): the five least reliable positions, by the chunk's lane
    unsigned fm[kChase] = { 0, 0, 0, 0, 0 };
    if (need) {
        for (int i = 0; i < 31; i++) s_pos[lane][i] = (uint8_t)i;
        for (int i = 0; i < kChase; i++) {
            int mi = i;
            float mv = s_cl[lane][s_pos[lane][i]];
            for (int j = i + 1; j < 31; j++) {
                const float v = s_cl[lane][s_pos[lane][j]];
                if (v < mv) { mv = v; mi = j; }
            }
            const uint8_t t = s_pos[lane][i]; s_pos[lane][i] = s_pos[lane][mi]; s_pos[lane][mi] = t;
        }
#pragma unroll
        for (int i = 0; i < kChase; i++) fm[i] = 1u << (30 - s_pos[lane][i]);
    }
    // ... and its 31 candidates across the wavefront, chunk after chunk in stream order (behind the first chunk that
    // fails, nothing is accepted: the loop stops there)
    unsigned long long pend = __builtin_amdgcn_ballot_w64(need);
    while (pend) {
        const int c = __builtin_ctzll(pend);
        pend &= pend - 1;
        const unsigned cwc = (unsigned)__shfl((int)cw, c);
        unsigned fl = cwc;
#pragma unroll
        for (int k = 0; k < kChase; k++) {
            const unsigned fk = (unsigned)__shfl((int)fm[k], c);
            if (lane & (1 << k)) fl ^= fk;
        }
        const unsigned syn = gf2_rem(3545u, 12, fl);
        const bool hit = lane >= 1 && lane < 32 && da_table_ok(syn, syn_da);
        const unsigned long long hits = __builtin_amdgcn_ballot_w64(hit);
        if (!hits) break;
        const int m = __builtin_ctzll(hits);
        const unsigned res = (unsigned)__shfl((int)(syn == 0 ? fl : fl ^ (unsigned)syn_da[hit ? syn : 0].y), m);
        if (lane == c) { cor = res; good = true; fixed = 1; }
    }
    // the chunks the serial loop accepts
    const unsigned long long gm = __builtin_amdgcn_ballot_w64(mine && good);
    const int max_bch = 512;
    int len = 0;
    bool failed = false;
    for (int blk = 0; blk < n_full && !failed; blk++)
        for (int c = 0; c < 4; c++) {
            if (len + 20 > max_bch) break;
            if (!((gm >> (4 * blk + c)) & 1)) { failed = true; break; }
            len += 20;
        }
    if (!failed && remain >= 4 && len + 2 * (remain / 2 - 1) <= max_bch && ns > 1 && len + 20 <= max_bch)
        for (int t = 0; t < n_tail && len + 20 <= max_bch; t++) {
            if (!((gm >> (4 * n_full + t)) & 1)) break;
            len += 20;
        }
    const int n_acc = len / 20;
    const unsigned long long acc = n_acc >= 64 ? ~0ull : (1ull << n_acc) - 1;
    const int fixederrs = __popcll(__builtin_amdgcn_ballot_w64(fixed != 0) & acc);
    if (len < 196) { emit(); return; }                                  // :577-578
    if (lane < n_acc) {
        const unsigned d = (cor >> 11) & 0xfffffu;
        for (int i = 0; i < 20; i++) s_st[20 * lane + i] = (uint8_t)((d >> (19 - i)) & 1u);
    }
    __syncthreads();

    // ---- the IDA header (:580-637)
    const int cont = s_st[3];
    const int da_ctr = (s_st[5] << 2) | (s_st[6] << 1) | s_st[7];
    const int da_len = (s_st[11] << 4) | (s_st[12] << 3) | (s_st[13] << 2) | (s_st[14] << 1) | s_st[15];
    if (((s_st[17] << 2) | (s_st[18] << 1) | s_st[19]) != 0 || da_len > 20) { emit(); return; }
    const int plen = da_len > 0 ? da_len : 20;
    if (lane < 32) {
        unsigned by = 0, bs = 0;
        for (int k = 0; k < 8; k++) {
            by = (by << 1) | (lane < plen ? s_st[20 + lane * 8 + k] : 0u);
            bs = (bs << 1) | (8 * lane + k < len ? s_st[8 * lane + k] : 0u);
        }
        s_rec.payload[lane] = (uint8_t)by;
        s_rec.bch_stream[lane] = (uint8_t)bs;
    }
    int crc_ok = 0;
    unsigned stored = 0, computed = 0;
    if (da_len > 0) {
        for (int k = 0; k < 16; k++) stored = (stored << 1) | s_st[9 * 20 + k];
        const int crc_bits = 20 + 12 + (len - 20 - 4);
        const int n_bytes = (crc_bits + 7) / 8;
        if (n_bytes <= 64) {
            // message bit bp: the stream's first 20 bits, 12 zero bits, the stream from bit 20 on; zero padding
            if (lane < n_bytes) {
                unsigned by = 0;
                for (int k = 0; k < 8; k++) {
                    const int bp = 8 * lane + k;
                    unsigned bit = 0;
                    if (bp < 20) bit = s_st[bp];
                    else if (bp >= 32 && bp < crc_bits) bit = s_st[20 + (bp - 32)];
                    by = (by << 1) | bit;
                }
                s_msg[lane] = (uint8_t)by;
            }
            __syncthreads();
            unsigned crc = 0xFFFFu;
            for (int k = 0; k < n_bytes; k++) crc = ((crc << 8) ^ c_crc16.v[((crc >> 8) ^ s_msg[k]) & 0xffu]) & 0xffffu;
            computed = crc;
            crc_ok = computed == 0;
        }
    }
    if (lane == 0) {
        s_rec.ok = 1;
        s_rec.lcw3_val = v3 >> 5;
        s_rec.ft = (uint8_t)ft;
        s_rec.lcw_ft = (uint8_t)((d2 >> 4) & 3);
        s_rec.lcw_code = (uint8_t)(d2 & 0xF);
        s_rec.ec_lcw = (uint8_t)((s1 != 0) + (s2 != 0) + (s3 != 0));
        s_rec.da_ctr = (uint8_t)da_ctr;
        s_rec.da_len = (uint8_t)da_len;
        s_rec.cont = (uint8_t)cont;
        s_rec.crc_ok = (uint8_t)crc_ok;
        s_rec.stored_crc = (uint16_t)stored;
        s_rec.computed_crc = (uint16_t)computed;
        s_rec.fixederrs = (uint8_t)fixederrs;
        s_rec.payload_len = (uint8_t)plen;
        s_rec.bch_len = (uint16_t)len;
    }
    emit();
}

// ---------------------------------------------------------------------------
// frame_decode() on the packed record path (option frame_records): the same decode as frame_decode_kernel, ONE WAVEFRONT
// PER FRAME, its FramePacked record written straight into pinned host memory.
//   * the access code: lanes 0..23 and one ballot; the frame's bits and LLRs behind it are staged in LDS.
//   * IBC (header BCH(7,3) wavefront-uniform), then IRA: one lane per BCH(31,21) block -- the IBC head's two, the IRA
//     head's three, and the two of every more_blocks pair the stream's length and cap allow -- all decoded at once.
//     frame_decode() stops at the first block that fails (decode or parity) and keeps whole pairs before it: what it
//     accepts is a prefix, wavefront-uniform arithmetic on one ballot.
//   * Chase (:224-295): the blocks that need it, in block order, each with its 31 flip masks on lanes 1..31 and the
//     lowest mask that decodes winning (the serial loop's first success); the five least reliable positions are chosen
//     by the block's own lane, the serial partial selection sort literally (its swaps decide ties), over the block's
//     LLRs in LDS.  Blocks behind the first failure are never needed and not tried.
//   * the accepted blocks' 21 data bits go to LDS; parse_ibc / parse_ira read them there, one lane per paging block.
// The frame's bits and LLRs are the DemodOut demod_par_kernel wrote on the device (keep_bits).  The record is complete in
// pinned memory, behind a system-scope fence, when the stream reaches the host's synchronisation -- as demod_export's.
// ---------------------------------------------------------------------------
namespace {

constexpr int kFrameBlocks = 23;      // IRA: 3 head blocks + 10 more_blocks pairs (63 + 10 * 42 <= 512 bits); IBC: <= 8

// where a block's 32 bits lie among the data bits: gather_block(data + base, first, stride)
struct BlockAt {
    int base, first, stride;
};

__device__ __forceinline__ int block_bit(const BlockAt &g, int k)           // data bit of block position k (0..31)
{
    return g.base + 2 * (g.first - g.stride * (k >> 1)) + (k & 1);
}

__device__ __forceinline__ bool ra_table_ok(unsigned syn, const int2 *__restrict__ syn_ra)
{
    return syn == 0 || (syn < 1024 && syn_ra[syn].x >= 0);
}

// chase_bch_decode_p + check_parity32 of blocks 0..n-1 (lane j: block j at g): the ballot of the blocks that pass, in
// block order up to the first one that does not (bits behind it are not meaningful); lane j's corrected codeword in *cor_out
__device__ __forceinline__ unsigned long long decode_blocks(int lane, int n, const BlockAt &g, const uint8_t *s_bits,
                                                            const float *s_llr, float (*s_cl)[32], uint8_t (*s_pos)[32],
                                                            const int2 *__restrict__ syn_ra, unsigned *cor_out)
{
    const bool mine = lane < n;
    unsigned cw = 0, par = 0, cor = 0;
    bool good = false, need = false;
    if (mine) {
        for (int k = 0; k < 31; k++) {
            const int idx = block_bit(g, k);
            cw = (cw << 1) | (unsigned)s_bits[idx];
            s_cl[lane][k] = s_llr[idx];
        }
        par = s_bits[block_bit(g, 31)];
        const unsigned syn = gf2_rem(kPolyRa, 11, cw);
        if (syn == 0) { cor = cw; good = true; }
        else if (syn < 1024 && syn_ra[syn].x >= 0) { cor = cw ^ (unsigned)syn_ra[syn].y; good = true; }
        else need = true;
    }
    // blocks behind one that decodes but fails its parity are never looked at
    const unsigned long long bad = __builtin_amdgcn_ballot_w64(mine && good && !parity_ok(cor, par));
    const unsigned long long before = bad ? (1ull << __builtin_ctzll(bad)) - 1 : ~0ull;
    need = need && ((before >> lane) & 1);
    unsigned fm[kChase] = { 0, 0, 0, 0, 0 };
    if (need) {
        for (int i = 0; i < 31; i++) s_pos[lane][i] = (uint8_t)i;
        for (int i = 0; i < kChase; i++) {
            int mi = i;
            float mv = s_cl[lane][s_pos[lane][i]];
            for (int j = i + 1; j < 31; j++) {
                const float v = s_cl[lane][s_pos[lane][j]];
                if (v < mv) { mv = v; mi = j; }
            }
            const uint8_t t = s_pos[lane][i]; s_pos[lane][i] = s_pos[lane][mi]; s_pos[lane][mi] = t;
        }
#pragma unroll
        for (int i = 0; i < kChase; i++) fm[i] = 1u << (30 - s_pos[lane][i]);
    }
    unsigned long long pend = __builtin_amdgcn_ballot_w64(need);
    while (pend) {
        const int c = __builtin_ctzll(pend);
        pend &= pend - 1;
        unsigned fl = (unsigned)__shfl((int)cw, c);
#pragma unroll
        for (int k = 0; k < kChase; k++) {
            const unsigned fk = (unsigned)__shfl((int)fm[k], c);
            if (lane & (1 << k)) fl ^= fk;
        }
        const unsigned syn = gf2_rem(kPolyRa, 11, fl);
        const bool hit = lane >= 1 && lane < 32 && ra_table_ok(syn, syn_ra);
        const unsigned long long hits = __builtin_amdgcn_ballot_w64(hit);
        if (!hits) break;
        const int m = __builtin_ctzll(hits);
        const unsigned res = (unsigned)__shfl((int)(syn == 0 ? fl : fl ^ (unsigned)syn_ra[hit ? syn : 0].y), m);
        if (lane == c) { cor = res; good = true; }
        if (!parity_ok(res, (unsigned)__shfl((int)par, c))) break;
    }
    *cor_out = cor;
    return __builtin_amdgcn_ballot_w64(mine && good && parity_ok(cor, par));
}

// the 21 data bits of a corrected block into the stream (append21), one bit per byte
__device__ __forceinline__ void put21(uint8_t *s_st, int at, unsigned corrected)
{
    const unsigned d = (corrected >> 10) & 0x1fffffu;
    for (int i = 0; i < 21; i++) s_st[at + i] = (uint8_t)((d >> (20 - i)) & 1u);
}

__device__ __forceinline__ unsigned lfield(const uint8_t *s_st, int k, int n)                   // extract_uint
{
    unsigned v = 0;
    for (int i = 0; i < n; i++) v = (v << 1) | s_st[k + i];
    return v;
}

}  // namespace

__global__ __launch_bounds__(64) void frame_packed_kernel(const DemodOut *__restrict__ frames, int n_frames,
                                                          const int2 *__restrict__ syn_ra, const int2 *__restrict__ syn_hdr,
                                                          FramePacked *__restrict__ hp_frame)
{
    __shared__ uint8_t s_bits[kMaxBits];                    // the hard bits behind the access code
    __shared__ float s_llr[kMaxBits];
    __shared__ float s_cl[kFrameBlocks][32];                // a block's 31 LLRs in codeword order
    __shared__ uint8_t s_pos[kFrameBlocks][32];             // its selection sort's permutation
    __shared__ uint8_t s_st[512];                           // the decoded stream, one bit per byte (:466, :545)
    __shared__ __attribute__((aligned(4))) FramePacked s_rec;
    const int b = blockIdx.x;
    const int lane = threadIdx.x;
    if (b >= n_frames) return;
    if (lane < 20) reinterpret_cast<uint32_t *>(&s_rec)[lane] = 0;
    const DemodOut &f = frames[b];
    const int n_bits = f.ok ? 2 * f.n_symbols : 0;
    // the record: type 0 (FRAME_UNKNOWN) for every frame frame_decode() does not take
    auto emit = [&]() {
        __syncthreads();
        if (lane < 20) reinterpret_cast<uint32_t *>(hp_frame + b)[lane] = reinterpret_cast<const uint32_t *>(&s_rec)[lane];
        __threadfence_system();
    };
    if (n_bits < 24 || n_bits > kMaxBits) { emit(); return; }
    // ---- access codes (:428-431)
    const unsigned long long am = __builtin_amdgcn_ballot_w64(lane < 24 && (f.bits[lane < 24 ? lane : 0] & 1));
    unsigned acc = 0;
    for (int k = 0; k < 24; k++) acc = (acc << 1) | ((unsigned)(am >> k) & 1u);
    if (acc != 0x3030F3u && acc != 0xCC3CFCu) { emit(); return; }
    const int data_len = n_bits - 24;
    for (int i = lane; i < data_len; i += 64) {
        s_bits[i] = f.bits[24 + i] & 1;
        s_llr[i] = f.llr[24 + i];
    }
    __syncthreads();
    unsigned cor;

    if (data_len >= 6 + 64) {                                           // ---- IBC (:441-505)
        unsigned hv = 0;
        for (int k = 0; k < 6; k++) hv = (hv << 1) | (unsigned)s_bits[k];
        const unsigned hs = gf2_rem(kPolyHdr, 5, hv);
        bool hdr_ok = hs == 0;
        if (!hdr_ok && hs < 16 && syn_hdr[hs].x >= 0) { hv ^= (unsigned)syn_hdr[hs].y; hdr_ok = true; }
        if (hdr_ok) {
            // the head pair, and the more_blocks pairs the 262-bit limit and the 256-bit stream allow
            const int ibc_max = data_len < 262 ? data_len : 262;
            int n_pairs = 1;
            while (6 + 64 * n_pairs + 64 <= ibc_max && 42 * n_pairs + 42 <= 256) n_pairs++;
            const BlockAt g{ 6 + 64 * (lane >> 1), 31 - (lane & 1), 2 };
            const unsigned long long ok = decode_blocks(lane, 2 * n_pairs, g, s_bits, s_llr, s_cl, s_pos, syn_ra, &cor);
            if ((ok & 3u) == 3u) {
                int n_acc = 1;
                while (n_acc < n_pairs && ((ok >> (2 * n_acc)) & 3u) == 3u) n_acc++;
                if (lane < 2 * n_acc) put21(s_st, 21 * lane, cor);
                __syncthreads();
                if (lane == 0) {                                        // parse_ibc (:368-393); len >= 42
                    const int len = 42 * n_acc;
                    s_rec.type = 2;
                    s_rec.bch_len = (uint16_t)len;
                    s_rec.bc_type = (uint8_t)((hv >> 4) & 7u);
                    s_rec.sat_id = (uint8_t)lfield(s_st, 0, 7);
                    s_rec.beam_id = (uint8_t)lfield(s_st, 7, 6);
                    s_rec.timeslot = s_st[14];
                    s_rec.sv_blocking = s_st[15];
                    if (len >= 84 && lfield(s_st, 42, 6) == 1u) s_rec.iri_time = lfield(s_st, 52, 32);
                }
                emit();
                return;
            }
        }
    }

    if (data_len >= 96) {                                               // ---- IRA (:514-595)
        int n_pairs = 0;
        while (96 + 64 * n_pairs + 64 <= data_len && 63 + 42 * n_pairs + 42 <= 512) n_pairs++;
        const BlockAt g = lane < 3 ? BlockAt{ 0, 47 - lane, 3 } : BlockAt{ 96 + 64 * ((lane - 3) >> 1), 31 - ((lane - 3) & 1), 2 };
        const unsigned long long ok = decode_blocks(lane, 3 + 2 * n_pairs, g, s_bits, s_llr, s_cl, s_pos, syn_ra, &cor);
        if ((ok & 7u) == 7u) {
            int n_acc = 0;
            while (n_acc < n_pairs && ((ok >> (3 + 2 * n_acc)) & 3u) == 3u) n_acc++;
            const int len = 63 + 42 * n_acc;
            if (lane < 3 + 2 * n_acc) put21(s_st, 21 * lane, cor);
            __syncthreads();
            // parse_ira (:317-366): paging block p on lane p; the list ends at the first all-ones block
            const int off = 63 + 42 * lane;
            const bool page = lane < 12 && off + 42 <= len;
            bool all1 = true;
            unsigned tmsi = 0, msc = 0;
            if (page) {
                for (int k = 0; k < 42; k++) all1 = all1 && s_st[off + k];
                tmsi = lfield(s_st, off, 32);
                msc = lfield(s_st, off + 34, 5);
            }
            const int n_pages = __builtin_ctzll(~__builtin_amdgcn_ballot_w64(page && !all1));
            if (lane < n_pages) {
                s_rec.page_tmsi[lane] = tmsi;
                s_rec.page_msc[lane] = (uint8_t)msc;
            }
            if (lane == 0) {
                s_rec.type = 1;
                s_rec.bch_len = (uint16_t)len;
                s_rec.sat_id = (uint8_t)lfield(s_st, 0, 7);
                s_rec.beam_id = (uint8_t)lfield(s_st, 7, 6);
                for (int k = 0; k < 3; k++) {                           // extract_signed12
                    const int mag = (int)lfield(s_st, 13 + 12 * k + 1, 11);
                    s_rec.pos_xyz[k] = (int16_t)(s_st[13 + 12 * k] ? mag - (1 << 11) : mag);
                }
                s_rec.n_pages = (uint8_t)n_pages;
            }
        }
    }
    emit();
}

// ---------------------------------------------------------------------------
// option "iq_sense": which way round a frame's I and Q were.  A recording with its components exchanged demodulates with
// ok = 1 and full confidence (preamble and unique words use the DQPSK states 0 and 2 alone, and conjugation maps that
// diagonal onto itself), but the two bits of every dibit arrive exchanged.  Three predicates that chance does not
// satisfy, each evaluated on the bits as they are (X = 0, "recorded") and with every pair exchanged (X = 1: bit and LLR
// index ^ 1 -- every offset below is even, so the exchange commutes with them):
//   IRA  access code, >= 24 + 96 bits, the three header blocks of the 3-way de-interleave (frame_decode.c:178-199) have a
//        zero BCH(31,21) remainder and the parity bit of check_parity32 (:399-407), nothing corrected;
//   IBC  access code, >= 24 + 6 + 64 bits, zero BCH(7,3) remainder of the header, the first two blocks of the 2-way
//        de-interleave clean in the same way;
//   IDA  ida_decode() as ida_decode_kernel runs it, Chase decoding on the LLRs included, ends with da_len > 0 and a CRC
//        that holds.
// One lane per frame, its SenseRec written straight into pinned host memory (bit 0 IRA, bit 1 IBC, bit 2 IDA per sense).
// The helpers the four decode kernels use are not touched: the exchanged reads live in helpers of their own.
// ---------------------------------------------------------------------------
namespace {

template <int X>
__device__ __forceinline__ bool strict_block(const uint8_t *__restrict__ in, int first_sym, int stride)
{
    unsigned w = 0;
#pragma unroll
    for (int p = 0; p < 16; p++) {
        const int s = first_sym - stride * p;
        w = (w << 2) | ((unsigned)(in[(2 * s) ^ X] & 1) << 1) | (unsigned)(in[(2 * s + 1) ^ X] & 1);
    }
    return gf2_rem(kPolyRa, 11, w >> 1) == 0 && (__popc(w) & 1) == 0;
}

// ida_decode_kernel's decode with the reads at index ^ X, down to the two facts the predicate needs
template <int X>
__device__ bool ida_holds(const uint8_t *__restrict__ bits, const float *__restrict__ llr_all, int n_bits, int direction,
                          const int2 *__restrict__ syn_da, const int2 *__restrict__ syn_l1,
                          const int2 *__restrict__ syn_l2, const int2 *__restrict__ syn_l3)
{
    if (n_bits < 24 + 46 + 124) return false;
    if (direction != 1 && direction != 2) return false;
    const uint8_t *data = bits + 24;
    const float *llr = llr_all + 24;
    const int data_len = n_bits - 24;
    unsigned v1 = 0, v2 = 0, v3 = 0;
    for (int k = 0; k < 46; k++) {
        const unsigned b = (unsigned)(data[((c_lcw_perm[k] - 1) ^ 1) ^ X] & 1);
        if (k < 7) v1 = (v1 << 1) | b;
        else if (k < 20) v2 = (v2 << 1) | b;
        else v3 = (v3 << 1) | b;
    }
    v2 <<= 1;
    const unsigned s1 = gf2_rem(29u, 5, v1), s2 = gf2_rem(465u, 9, v2), s3 = gf2_rem(41u, 6, v3);
    if (s1 != 0) { if (s1 >= 16 || syn_l1[s1].x < 0) return false; v1 ^= (unsigned)syn_l1[s1].y; }
    if (s2 != 0 && (s2 >= 256 || syn_l2[s2].x < 0)) return false;
    if (s3 != 0 && (s3 >= 32 || syn_l3[s3].x < 0)) return false;
    if (((int)(v1 >> 4) & 7) != 2) return false;
    const int payload_len = data_len - 46;
    if (payload_len < 124) return false;
    const uint8_t *pd = data + 46;
    const float *pl = llr + 46;

    uint8_t st[512];
    int len = 0;
    const int max_bch = 512;
    const int n_full = payload_len / 124, remain = payload_len % 124;
    bool failed = false;
    for (int blk = 0; blk < n_full && !failed; blk++) {
        const uint8_t *b = pd + blk * 124;
        const float *bl = pl + blk * 124;
        for (int c = 0; c < 4; c++) {
            if (len + 20 > max_bch) break;
            const int off = (c == 0 ? 3 : c == 1 ? 1 : c == 2 ? 2 : 0) * 31;
            unsigned cw = 0;
            float l[31];
            for (int k = 0; k < 31; k++) {
                const int j = off + k;
                const int idx = (j < 62 ? deint_index(62, 0, j) : deint_index(62, 1, j - 62)) ^ X;
                cw = (cw << 1) | (unsigned)(b[idx] & 1);
                l[k] = bl[idx];
            }
            unsigned cor;
            int fixed = 0;
            if (chase_da(cw, l, syn_da, &cor, &fixed) < 0) { failed = true; break; }
            put20(st, len, cor);
        }
    }
    if (!failed && remain >= 4 && len + 2 * (remain / 2 - 1) <= max_bch) {
        const int ns = remain / 2;
        const uint8_t *b = pd + n_full * 124;
        const float *bl = pl + n_full * 124;
        if (ns > 1 && len + 20 <= max_bch) {
            const int hl = ns - 1;
            int clen = 2 * hl;
            if (clen > 128) clen = 128;
            int pos = 0;
            while (pos + 31 <= clen && len + 20 <= max_bch) {
                unsigned cw = 0;
                float l[31];
                for (int k = 0; k < 31; k++) {
                    const int idx = tail_index(ns, hl, pos + k) ^ X;    // (>= -124: b is an even number of bits into the frame)
                    cw = (cw << 1) | (unsigned)(b[idx] & 1);
                    l[k] = bl[idx];
                }
                unsigned cor;
                int fixed = 0;
                if (chase_da(cw, l, syn_da, &cor, &fixed) < 0) break;
                put20(st, len, cor);
                pos += 31;
            }
        }
    }
    if (len < 196) return false;
    const int da_len = (st[11] << 4) | (st[12] << 3) | (st[13] << 2) | (st[14] << 1) | st[15];
    if (((st[17] << 2) | (st[18] << 1) | st[19]) != 0) return false;
    if (da_len > 20 || da_len == 0) return false;
    // CRC-CCITT-FALSE over the re-packed bits (:606-637), bit-serial as in ida_decode_kernel
    const int crc_bits = 20 + 12 + (len - 20 - 4);
    if ((crc_bits + 7) / 8 > 64) return false;
    unsigned crc = 0xFFFFu, cur = 0;
    int nb = 0;
    const int total_bits = ((crc_bits + 7) / 8) * 8;
    for (int bp = 0; bp < total_bits; bp++) {
        unsigned bit = 0;
        if (bp < 20) bit = st[bp];
        else if (bp >= 32 && bp < crc_bits) bit = st[20 + (bp - 32)];
        cur = (cur << 1) | bit;
        if (++nb == 8) {
            crc ^= (cur & 0xffu) << 8;
            for (int j = 0; j < 8; j++) crc = (crc & 0x8000u) ? ((crc << 1) ^ 0x1021u) & 0xffffu : (crc << 1) & 0xffffu;
            nb = 0;
            cur = 0;
        }
    }
    return crc == 0;
}

template <int X>
__device__ unsigned iq_sense_of(const DemodOut &f, int n_bits, const int2 *__restrict__ syn_da,
                                const int2 *__restrict__ syn_l1, const int2 *__restrict__ syn_l2,
                                const int2 *__restrict__ syn_l3)
{
    unsigned m = 0;
    unsigned acc = 0;
    for (int k = 0; k < 24; k++) acc = (acc << 1) | (unsigned)(f.bits[k ^ X] & 1);
    if (acc == 0x3030F3u || acc == 0xCC3CFCu) {
        const uint8_t *data = f.bits + 24;
        const int data_len = n_bits - 24;
        if (data_len >= 96 && strict_block<X>(data, 47, 3) && strict_block<X>(data, 46, 3) && strict_block<X>(data, 45, 3))
            m |= 1u;
        if (data_len >= 6 + 64) {
            unsigned hv = 0;
            for (int k = 0; k < 6; k++) hv = (hv << 1) | (unsigned)(data[k ^ X] & 1);
            if (gf2_rem(kPolyHdr, 5, hv) == 0 && strict_block<X>(data + 6, 31, 2) && strict_block<X>(data + 6, 30, 2)) m |= 2u;
        }
    }
    if (ida_holds<X>(f.bits, f.llr, n_bits, f.direction, syn_da, syn_l1, syn_l2, syn_l3)) m |= 4u;
    return m;
}

}  // namespace

__global__ __launch_bounds__(64) void iq_sense_kernel(const DemodOut *__restrict__ frames, int n_frames,
                                                      const int2 *__restrict__ syn_da, const int2 *__restrict__ syn_l1,
                                                      const int2 *__restrict__ syn_l2, const int2 *__restrict__ syn_l3,
                                                      SenseRec *__restrict__ hp_sense)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_frames) return;
    const DemodOut &f = frames[i];
    SenseRec r;
    r.recorded = r.exchanged = 0;
    r.pad = 0;
    const int n_bits = f.ok && f.n_symbols > 0 ? 2 * f.n_symbols : 0;
    r.n_bits = (uint32_t)n_bits;
    if (n_bits >= 24 && n_bits <= kMaxBits) {
        r.recorded = (uint8_t)iq_sense_of<0>(f, n_bits, syn_da, syn_l1, syn_l2, syn_l3);
        r.exchanged = (uint8_t)iq_sense_of<1>(f, n_bits, syn_da, syn_l1, syn_l2, syn_l3);
    }
    hp_sense[i] = r;
    __threadfence_system();
}

int launch_iq_sense(const DemodOut *frames, int n_frames, const int2 *syn_da, const int2 *syn_l1, const int2 *syn_l2,
                    const int2 *syn_l3, SenseRec *hp_sense, hipStream_t stream)
{
    if (n_frames <= 0) return 0;
    hipLaunchKernelGGL(iq_sense_kernel, dim3((n_frames + 63) / 64), dim3(64), 0, stream, frames, n_frames, syn_da, syn_l1,
                       syn_l2, syn_l3, hp_sense);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

int launch_frame_packed(const DemodOut *frames, int n_frames, const int2 *syn_ra, const int2 *syn_hdr, FramePacked *hp_frame,
                        hipStream_t stream)
{
    if (n_frames <= 0) return 0;
    hipLaunchKernelGGL(frame_packed_kernel, dim3(n_frames), dim3(64), 0, stream, frames, n_frames, syn_ra, syn_hdr, hp_frame);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

int launch_ida_packed(const DemodOut *frames, int n_frames, const int2 *syn_da, const int2 *syn_l1, const int2 *syn_l2,
                      const int2 *syn_l3, IdaPacked *hp_ida, hipStream_t stream)
{
    if (n_frames <= 0) return 0;
    hipLaunchKernelGGL(ida_packed_kernel, dim3(n_frames), dim3(64), 0, stream, frames, n_frames, syn_da, syn_l1, syn_l2,
                       syn_l3, hp_ida);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

int launch_ida_decode(const DemodOut *frames, int n_frames, const int2 *syn_da, const int2 *syn_l1, const int2 *syn_l2,
                      const int2 *syn_l3, int use_llr, const int *n_bits, const int *direction, IdaOut *out,
                      hipStream_t stream)
{
    if (n_frames <= 0) return 0;
    hipLaunchKernelGGL(ida_decode_kernel, dim3((n_frames + 63) / 64), dim3(64), 0, stream, frames, n_frames, syn_da,
                       syn_l1, syn_l2, syn_l3, use_llr, n_bits, direction, out);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

int launch_frame_decode(const DemodOut *frames, int n_frames, const int2 *syn_ra, const int2 *syn_hdr, int use_llr,
                        const int *n_bits, DecodedOut *out, hipStream_t stream)
{
    if (n_frames <= 0) return 0;
    hipLaunchKernelGGL(frame_decode_kernel, dim3((n_frames + 63) / 64), dim3(64), 0, stream, frames, n_frames,
                       syn_ra, syn_hdr, use_llr, n_bits, out);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace irdm
