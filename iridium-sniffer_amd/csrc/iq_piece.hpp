// iq_piece.hpp -- the samples of one 16-byte piece (or of one sample's bytes) of a device format as the two float bit
// patterns load_iq<FMT> (common.hpp) gives, for the passes that read a chunk with 16-byte loads (iq_moments.hpp,
// iq_balance.hpp).  Bit patterns, not floats: a cf32 component travels untouched, a signalling NaN included.
#pragma once
#include "common.hpp"

namespace irdm {

// the launch geometry those passes share: `head` samples up to the first 16-byte boundary of d_in (at most 16 / bps - 1,
// at most n), nvec 16-byte pieces, the rest (at most 16 / bps - 1); the workgroups of nt threads under max_grid
static inline int iq_piece_grid(int fmt, const void *d_in, size_t n, int nt, int max_grid, long long *head_out, long long *nvec_out)
{
    const int bps = fmt_bytes(fmt), spv = 16 / bps;
    const size_t mis = (size_t)(reinterpret_cast<uintptr_t>(d_in) & 15u);
    long long head = (long long)(((16 - mis) & 15u) / (size_t)bps);
    if (head > (long long)n) head = (long long)n;
    const long long nvec = ((long long)n - head) / spv;
    *head_out = head;
    *nvec_out = nvec;
    const long long want = (nvec + nt - 1) / nt;
    return (int)(want < 1 ? 1 : (want > max_grid ? max_grid : want));
}

// one component from its code, as load_iq<FMT> converts it
template <int FMT>
__device__ __forceinline__ unsigned iq_code_bits(int code)
{
    if (FMT == 0) return __float_as_uint((float)code / 128.0f);
    if (FMT == 1) return __float_as_uint((float)(code >> 8) / 128.0f);
    if (FMT == 3) return __float_as_uint(i16_full<3>(code));
    if (FMT == 4) return __float_as_uint(i16_full<4>(code));
    if (FMT == 6) return __float_as_uint(cu8_f(code));
    if (FMT == 8) return __float_as_uint(i32_f<8>(code));
    return __float_as_uint(i32_f<9>(code));
}

// one 32-bit word of a 2- or 4-byte-per-sample format: two samples (o[0..3]) or one (o[0..1])
template <int FMT>
__device__ __forceinline__ void iq_word_bits(unsigned w, unsigned *o)
{
    if (FMT == 0) {
        o[0] = iq_code_bits<FMT>((int)(signed char)(w & 0xff));
        o[1] = iq_code_bits<FMT>((int)(signed char)((w >> 8) & 0xff));
        o[2] = iq_code_bits<FMT>((int)(signed char)((w >> 16) & 0xff));
        o[3] = iq_code_bits<FMT>((int)(signed char)(w >> 24));
    } else if (FMT == 6) {
        o[0] = iq_code_bits<FMT>((int)(w & 0xff));
        o[1] = iq_code_bits<FMT>((int)((w >> 8) & 0xff));
        o[2] = iq_code_bits<FMT>((int)((w >> 16) & 0xff));
        o[3] = iq_code_bits<FMT>((int)(w >> 24));
    } else {
        o[0] = iq_code_bits<FMT>((int)(short)(w & 0xffff));
        o[1] = iq_code_bits<FMT>((int)(short)(w >> 16));
    }
}

// a 16-byte piece: 16 / bytes-per-sample samples, o[2 k] = I, o[2 k + 1] = Q of sample k
template <int FMT>
__device__ __forceinline__ void iq_piece_bits(const uint4 v, unsigned *o)
{
    constexpr int BPS = kFmtBytes<FMT>;
    if (FMT == 2) {
        o[0] = v.x; o[1] = v.y; o[2] = v.z; o[3] = v.w;
    } else if (BPS == 8) {
        o[0] = iq_code_bits<FMT>((int)v.x); o[1] = iq_code_bits<FMT>((int)v.y);
        o[2] = iq_code_bits<FMT>((int)v.z); o[3] = iq_code_bits<FMT>((int)v.w);
    } else {
        constexpr int PW = BPS == 2 ? 4 : 2;                // floats per word
        iq_word_bits<FMT>(v.x, o);
        iq_word_bits<FMT>(v.y, o + PW);
        iq_word_bits<FMT>(v.z, o + 2 * PW);
        iq_word_bits<FMT>(v.w, o + 3 * PW);
    }
}

// the sample at p (aligned to a sample only)
template <int FMT>
__device__ __forceinline__ void iq_sample_bits(const unsigned char *p, unsigned *o)
{
    constexpr int BPS = kFmtBytes<FMT>;
    if (FMT == 2) {
        const unsigned *w = reinterpret_cast<const unsigned *>(p);
        o[0] = w[0]; o[1] = w[1];
    } else if (BPS == 8) {
        const int *w = reinterpret_cast<const int *>(p);
        o[0] = iq_code_bits<FMT>(w[0]); o[1] = iq_code_bits<FMT>(w[1]);
    } else if (BPS == 4) {
        iq_word_bits<FMT>(*reinterpret_cast<const unsigned *>(p), o);
    } else {
        const unsigned w = *reinterpret_cast<const unsigned short *>(p);
        if (FMT == 0) {
            o[0] = iq_code_bits<FMT>((int)(signed char)(w & 0xff));
            o[1] = iq_code_bits<FMT>((int)(signed char)(w >> 8));
        } else {
            o[0] = iq_code_bits<FMT>((int)(w & 0xff));
            o[1] = iq_code_bits<FMT>((int)(w >> 8));
        }
    }
}

}  // namespace irdm
