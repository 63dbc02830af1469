// iq_piece.hpp -- one 16-byte piece (or one sample's bytes) of a device format taken apart: the byte layout of the eight
// formats beside load_iq<FMT> (common.hpp), written once for the passes that read a chunk with 16-byte loads
// (chunk_span.hpp).  Two views:
//   * codes: f(k, code) for every component in memory order, k = 0 for I and 1 for Q; the code is the file's integer, for
//     cf32 the raw word (input_stats.hpp counts and sums codes);
//   * bits: the float bit patterns load_iq<FMT> gives (iq_moments.hpp, iq_balance.hpp).  Bit patterns, not floats: a cf32
//     component travels untouched, a signalling NaN included.
// Everything is inlined into the caller's lane loop: the functor is a lambda over the lane's accumulators.
#pragma once
#include "common.hpp"

namespace irdm {

// one 32-bit word of a 2- or 4-byte-per-sample format: two samples or one
template <int FMT, typename F>
__device__ __forceinline__ void iq_word_codes(unsigned w, F &&f)
{
    if (FMT == 0) {
        f(0, (int)(signed char)(w & 0xff));
        f(1, (int)(signed char)((w >> 8) & 0xff));
        f(0, (int)(signed char)((w >> 16) & 0xff));
        f(1, (int)(signed char)(w >> 24));
    } else if (FMT == 6) {
        f(0, (int)(w & 0xff));
        f(1, (int)((w >> 8) & 0xff));
        f(0, (int)((w >> 16) & 0xff));
        f(1, (int)(w >> 24));
    } else {
        f(0, (int)(short)(w & 0xffff));
        f(1, (int)(short)(w >> 16));
    }
}

// a 16-byte piece: 16 / bytes-per-sample samples
template <int FMT, typename F>
__device__ __forceinline__ void iq_piece_codes(const uint4 v, F &&f)
{
    if (kFmtBytes<FMT> == 8) {
        f(0, (int)v.x);
        f(1, (int)v.y);
        f(0, (int)v.z);
        f(1, (int)v.w);
    } else {
        iq_word_codes<FMT>(v.x, f);
        iq_word_codes<FMT>(v.y, f);
        iq_word_codes<FMT>(v.z, f);
        iq_word_codes<FMT>(v.w, f);
    }
}

// the sample at p (aligned to a sample only)
template <int FMT, typename F>
__device__ __forceinline__ void iq_sample_codes(const unsigned char *p, F &&f)
{
    constexpr int BPS = kFmtBytes<FMT>;
    if (BPS == 8) {
        const int *w = reinterpret_cast<const int *>(p);
        f(0, w[0]);
        f(1, w[1]);
    } else if (BPS == 4) {
        iq_word_codes<FMT>(*reinterpret_cast<const unsigned *>(p), f);
    } else {
        const unsigned w = *reinterpret_cast<const unsigned short *>(p);
        f(0, FMT == 0 ? (int)(signed char)(w & 0xff) : (int)(w & 0xff));
        f(1, FMT == 0 ? (int)(signed char)(w >> 8) : (int)(w >> 8));
    }
}

// one component from its code, as load_iq<FMT> converts it
template <int FMT>
__device__ __forceinline__ unsigned iq_code_bits(int code)
{
    if (FMT == 2) return (unsigned)code;
    if (FMT == 0) return __float_as_uint((float)code / 128.0f);
    if (FMT == 1) return __float_as_uint((float)(code >> 8) / 128.0f);
    if (FMT == 3) return __float_as_uint(i16_full<3>(code));
    if (FMT == 4) return __float_as_uint(i16_full<4>(code));
    if (FMT == 6) return __float_as_uint(cu8_f(code));
    if (FMT == 8) return __float_as_uint(i32_f<8>(code));
    return __float_as_uint(i32_f<9>(code));
}

// o[2 k] = I, o[2 k + 1] = Q of sample k of the piece
template <int FMT>
__device__ __forceinline__ void iq_piece_bits(const uint4 v, unsigned *o)
{
    int j = 0;
    iq_piece_codes<FMT>(v, [&](int, int code) { o[j++] = iq_code_bits<FMT>(code); });
}

template <int FMT>
__device__ __forceinline__ void iq_sample_bits(const unsigned char *p, unsigned *o)
{
    iq_sample_codes<FMT>(p, [&](int k, int code) { o[k] = iq_code_bits<FMT>(code); });
}

}  // namespace irdm
