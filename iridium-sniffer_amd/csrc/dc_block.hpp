// dc_block.hpp -- irdm_dc_block / irdm_frontend_dc_block / irdm_dc_block_device (include/irdm_hip.h): a receiver's DC
// offset tracked block by block and subtracted.  n samples of any device format at `src` become cf32 at `dst`.
//
// The arithmetic (tests/dc_model.py restates it in numpy), one rule for all eight formats:
//   * a component c is the float load_iq<FMT> makes of the sample (iq_piece.hpp);
//   * q(c) = llrint(c' * 2^32) as int64, c' = c clamped to +-64, a NaN counting 0: float -> double and the product are
//     exact here, the rounding is to nearest, ties to even (|q| <= 2^38; dc_quant below computes it in integers), and the
//     clamp keeps one glitch of 1e30 from owning a block's mean;
//   * the stream is cut into blocks of B = 2^log2 samples (12 <= log2 <= 24) aligned to the stream position;
//     S_k = the int64 sum of q over block k, per arm (B * 2^38 <= 2^62: no overflow).  Integer addition is associative:
//     S_k depends neither on the launch geometry nor on the order the atomics arrive in nor on how feeds cut the block,
//     which float atomics could not promise;
//   * m_k = (float)((double)S_k / (B * 2^32)), per arm;
//   * a sample of block k >= 1 becomes (__fsub_rn(i, m_{k-1}.i), __fsub_rn(q, m_{k-1}.q)), block 0 uses the seed; a NaN
//     component leaves as its own bits with the quiet bit set (what the subtraction gives on this hardware and in numpy,
//     said here so that it does not depend on either).
//
// Three launches per chunk (or per piece of at most the ring's span) on the stream the chunk arrives on:
//   1. dc_sums_kernel<FMT> reads the chunk once in 16-byte pieces (the span geometry of chunk_span.hpp; the pieces are dealt
//      to the wavefronts in contiguous runs, so that a wavefront meets few blocks).  A lane keeps the int64 sums of the block
//      its wavefront's 64 pieces begin in and of the block behind it (64 pieces are at most 512 samples: they straddle at
//      most one edge, and a piece may itself straddle it: the block is decided per sample).  When the wavefront moves on to
//      another block it reduces the sums by shuffles (wave_reduce.hpp) and lane 0 issues one 64-bit integer atomic per arm
//      and block into the accumulator ring: slot = block mod slots, kDcCopies copies per slot, the wavefronts spread over
//      the copies (scrub.hpp has the measurement of what one address costs).  The slots a chunk opens are cleared on the
//      same stream in front of the launch.
//   2. dc_close_kernel, one wavefront, a lane per block: the copies of every block the chunk completed are added up, m_k goes
//      to the means ring (slot = block mod slots), and the device record takes the blocks complete, the first and last mean,
//      the minimum and maximum per arm and the sums of the block left open.
//   3. dc_sub_kernel<FMT> converts and subtracts.  Its shape is iq_balance_kernel's: a lane loads 16 bytes of src (8 / 4 / 2
//      samples), which become 64 / 32 / 16 bytes of dst in 16-byte stores where dst + head lies on a 16-byte boundary, in
//      8-byte stores otherwise; for the 2- and 4-byte formats the wavefront turns its 64 pieces through LDS so that each
//      store instruction writes 1 KiB of consecutive bytes.  In place (dst == src) for the 8-byte formats: a lane has read
//      its piece before it writes it and reads no other lane's.
// Bounds.  dc_sums_kernel reads the samples of src's span and adds to accumulator slots of the blocks
// [first >> log2, (first + n - 1) >> log2] alone, taken mod slots (the host refuses a launch that spans more blocks than the
// ring has slots).  dc_close_kernel reads those slots and writes means slots of the blocks it closes and the record.
// dc_sub_kernel reads the samples of src's span (chunk_span.hpp) and the means slots of the blocks
// [(first >> log2) - 1, ((first + n - 1) >> log2) - 1], and writes the same sample indices of dst: the vector part dst
// samples [head, head + nvec * spv), the scalar part [0, head) and [head + nvec * spv, n).
//
// Included by the translation units that launch it (feed.cpp: irdm_feed_host of a context and irdm_dc_block_device;
// frontend.cpp: the capture in front of K0 / K0r / K0w).
#pragma once
#include <math.h>
#include <string.h>
#include <algorithm>
#include "common.hpp"
#include "chunk_span.hpp"
#include "iq_piece.hpp"
#include "wave_reduce.hpp"
#include "../../include/irdm_hip.h"

#if !defined(__HIP__)
// (a host compiler: the CPU emulation of the tests.  One rounding, as the device intrinsic)
static inline float __fsub_rn(float a, float b) { volatile float d = a - b; return d; }
#endif

namespace irdm {

constexpr int kDcMinLog2 = 12, kDcMaxLog2 = 24, kDcDefaultLog2 = 20;
constexpr int kDcCopies = 32;                           // copies of a block's two sums (a power of two)
constexpr unsigned kDcClampBits = 0x42800000u;          // 64.0f
constexpr size_t kDcSlotWords = (size_t)kDcCopies * 2;  // 64-bit words of a slot of the accumulator ring
constexpr size_t kDcDevicePiece = (size_t)1 << 24;      // irdm_dc_block_device: samples per round of three launches
constexpr size_t kDcSpan = (size_t)1 << 26;             // a context's or a front end's: a longer chunk takes several rounds

// q(c) on the bits of c, in integers (as first written -- float to double, a double product, llrint -- the sums pass took
// 106 us per 64 Mi ci8 samples where a copy of the same bytes takes 19): |c| = M 2^(e - 150) with the 24-bit M, so
// |c| 2^32 = M 2^s, s = e - 118 <= 14; a negative s shifts right and rounds to nearest, ties to even.  A subnormal (e = 0)
// and everything below 2^-33 give 0.
__host__ __device__ __forceinline__ long long dc_quant(unsigned bits)
{
    const unsigned mag = bits & 0x7fffffffu;
    if (mag > 0x7f800000u) return 0;                    // a NaN
    long long q;
    if (mag >= kDcClampBits) q = 1ll << 38;             // beyond +-64, the infinities included
    else {
        const unsigned M = (mag & 0x7fffffu) | 0x800000u;
        const int s = (int)(mag >> 23) - 118;
        if (s >= 0) q = (long long)M << s;
        else if (s < -25) q = 0;
        else q = (long long)((M + ((1u << (-s - 1)) - 1u) + ((M >> -s) & 1u)) >> -s);
    }
    return (bits >> 31) ? -q : q;
}

// q of a component from its code: the 8- and 16-bit formats are a power of two times the code (|c| <= 16: no clamp)
template <int FMT>
__device__ __forceinline__ long long dc_quant_code(int code)
{
    if (FMT == 0) return (long long)code * (1ll << 25);                 // code / 128
    if (FMT == 1) return (long long)(code >> 8) * (1ll << 25);
    if (FMT == 3) return (long long)code * (1ll << 17);                 // code / 32768
    if (FMT == 4) return (long long)code * (1ll << 21);                 // code / 2048
    if (FMT == 6) return (long long)(2 * code - 255) * (1ll << 24);     // (2 u - 255) / 256
    return dc_quant(iq_code_bits<FMT>(code));
}

// m_k of one arm
__host__ __device__ __forceinline__ float dc_mean(long long sum, int log2)
{
    return (float)((double)sum / ((double)(1ull << log2) * 4294967296.0));
}

// c - m on the bits of c
__device__ __forceinline__ unsigned dc_sub_bits(unsigned bits, float m)
{
    if ((bits & 0x7fffffffu) > 0x7f800000u) return bits | 0x00400000u;
    return __float_as_uint(__fsub_rn(__uint_as_float(bits), m));
}

// the device record of a stream (or of one irdm_dc_block_device call)
struct DcRec {
    unsigned long long blocks;          // blocks closed so far
    float first[2], last[2], mn[2], mx[2];
    long long open[2];                  // the sums of the block left open by the launch that wrote the record last
};

// the stream position `first` of a launch's sample 0, the block length and the rings
struct DcGeom {
    unsigned long long first;
    int log2;
    unsigned mask;                      // slots - 1 (slots: a power of two)
};

template <typename T>
__device__ __forceinline__ T dc_wave_min(T v)
{
    for (int d = 32; d > 0; d >>= 1) {
        const T o = __shfl_down(v, d);
        v = o < v ? o : v;
    }
    return v;
}

__device__ __forceinline__ void dc_flush(unsigned long long *acc, const DcGeom g, unsigned long long kb, int copy, long long (&s)[4])
{
    unsigned long long t[4];
#pragma unroll
    for (int j = 0; j < 4; j++) t[j] = wave_sum((unsigned long long)s[j]);
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int j = 0; j < 4; j++)
            if (t[j]) atomicAdd(&acc[(((kb + (unsigned)(j >> 1)) & g.mask) * kDcCopies + (unsigned)copy) * 2 + (unsigned)(j & 1)], t[j]);
    }
#pragma unroll
    for (int j = 0; j < 4; j++) s[j] = 0;
}

// 1. the sums of the samples of FMT of span sp at `src` (aligned to a sample) into the accumulator ring
template <int FMT>
__global__ __launch_bounds__(kChunkNT) void dc_sums_kernel(const void *__restrict__ src, const ChunkSpan sp, const DcGeom g,
                                                           unsigned long long *__restrict__ acc)
{
    constexpr int BPS = kFmtBytes<FMT>, SPV = 16 / BPS;
    const ChunkLane cl = chunk_lane();
    const unsigned char *const bytes = static_cast<const unsigned char *>(src);
    const uint4 *const pieces = reinterpret_cast<const uint4 *>(bytes + sp.head * BPS);
    const int lane = threadIdx.x & 63;
    const long long wave = cl.gid >> 6, n_waves = cl.stride >> 6;
    const int copy = (int)(wave & (kDcCopies - 1));
    // the wavefront's run of pieces [b0, b1): whole rounds of 64, so every lane of it makes every trip and reaches every shuffle
    const long long per = ((sp.nvec + n_waves - 1) / n_waves + 63) & ~63ll;
    const long long b0 = wave * per, b1 = b0 + per < sp.nvec ? b0 + per : sp.nvec;
    long long s[4] = { 0, 0, 0, 0 };                    // I, Q of block kb; I, Q of block kb + 1
    unsigned long long kb = 0;
    bool open = false;
    for (long long b = b0; b < b1; b += 64) {
        const unsigned long long k = (g.first + (unsigned long long)(sp.head + b * SPV)) >> g.log2;
        if (open && k != kb) dc_flush(acc, g, kb, copy, s);
        kb = k;
        open = true;
        const long long i = b + lane;
        if (i < b1) {
            const unsigned long long pos = g.first + (unsigned long long)(sp.head + i * SPV);
            const uint4 v = pieces[i];
            if (((pos + (SPV - 1)) >> g.log2) == kb) {
                iq_piece_codes<FMT>(v, [&](int arm, int code) { s[arm] += dc_quant_code<FMT>(code); });
            } else {
                int j = 0;
                iq_piece_codes<FMT>(v, [&](int arm, int code) {
                    const int hi = ((pos + (unsigned)(j >> 1)) >> g.log2) != kb ? 2 : 0;
                    s[hi + arm] += dc_quant_code<FMT>(code);
                    j++;
                });
            }
        }
    }
    if (open) dc_flush(acc, g, kb, copy, s);
    // the scalar head and tail (the first workgroup's first threads): a sample each, straight into the ring
    const long long si = cl.scalar<SPV>(sp);
    if (si < 0) return;
    const unsigned long long ks = (g.first + (unsigned long long)si) >> g.log2;
    iq_sample_codes<FMT>(bytes + si * BPS, [&](int arm, int code) {
        const long long q = dc_quant_code<FMT>(code);
        if (q) atomicAdd(&acc[((ks & g.mask) * kDcCopies + (unsigned)copy) * 2 + (unsigned)arm], (unsigned long long)q);
    });
}

// 2. blocks [k_begin, k_end) closed: their means into the means ring, the record brought up to date (fresh: started over).
// open_valid: the slot of block k_end has been opened, its sums go to the record.  One wavefront.  (A template, as the other
// two: every translation unit that includes this header may hold it.)
template <int COPIES>
__global__ __launch_bounds__(64) void dc_close_kernel(const unsigned long long *__restrict__ acc, float2 *__restrict__ means,
                                                      DcRec *__restrict__ rec, const DcGeom g, unsigned long long k_begin,
                                                      unsigned long long k_end, int fresh, int open_valid)
{
    const int lane = threadIdx.x;
    float mn[2] = { INFINITY, INFINITY }, mx[2] = { -INFINITY, -INFINITY }, m_first[2] = { 0.0f, 0.0f }, m_last[2] = { 0.0f, 0.0f };
    for (unsigned long long k = k_begin + (unsigned)lane; k < k_end; k += 64) {
        const unsigned long long *slot = acc + (k & g.mask) * kDcSlotWords;
        unsigned long long t[2] = { 0, 0 };                 // (two's complement: the copies add up as the int64 they hold)
        for (int c = 0; c < COPIES; c++) {
            t[0] += slot[2 * c];
            t[1] += slot[2 * c + 1];
        }
        const float m[2] = { dc_mean((long long)t[0], g.log2), dc_mean((long long)t[1], g.log2) };
        means[k & g.mask] = make_float2(m[0], m[1]);
        for (int a = 0; a < 2; a++) {
            mn[a] = m[a] < mn[a] ? m[a] : mn[a];
            mx[a] = m[a] > mx[a] ? m[a] : mx[a];
            if (k == k_begin) m_first[a] = m[a];
            m_last[a] = m[a];
        }
    }
    long long t_open[2] = { 0, 0 };
    if (open_valid && lane < kDcCopies) {
        const unsigned long long *slot = acc + (k_end & g.mask) * kDcSlotWords;
        t_open[0] = (long long)slot[2 * lane];
        t_open[1] = (long long)slot[2 * lane + 1];
    }
    const int owner = k_end > k_begin ? (int)((k_end - 1 - k_begin) & 63) : 0;
    float r_mn[2], r_mx[2], r_last[2];
    long long r_open[2];
    for (int a = 0; a < 2; a++) {
        r_mn[a] = dc_wave_min(mn[a]);
        r_mx[a] = wave_max(mx[a]);
        r_last[a] = __shfl(m_last[a], owner);
        r_open[a] = (long long)wave_sum((unsigned long long)t_open[a]);
    }
    if (lane != 0) return;
    const bool any = k_end > k_begin;
    if (fresh) {
        rec->blocks = 0;
        for (int a = 0; a < 2; a++) rec->first[a] = rec->last[a] = rec->mn[a] = rec->mx[a] = 0.0f;
    }
    for (int a = 0; a < 2; a++) {
        if (any) {
            const bool none = rec->blocks == 0;
            if (none) rec->first[a] = m_first[a];
            rec->last[a] = r_last[a];
            rec->mn[a] = none || r_mn[a] < rec->mn[a] ? r_mn[a] : rec->mn[a];
            rec->mx[a] = none || r_mx[a] > rec->mx[a] ? r_mx[a] : rec->mx[a];
        }
        rec->open[a] = r_open[a];
    }
    rec->blocks += k_end - k_begin;
}

// the mean in front of the block that holds stream position pos: m0 for block k0, the means ring's otherwise
struct DcPrev {
    unsigned long long k0;
    float m0_i, m0_q;
};
__device__ __forceinline__ float2 dc_prev(const float2 *__restrict__ means, const DcGeom &g, const DcPrev &pv, unsigned long long k)
{
    return k == pv.k0 ? make_float2(pv.m0_i, pv.m0_q) : means[(k - 1) & g.mask];
}

// SPV samples (o[2 k], o[2 k + 1]: the bits of I and Q) from stream position pos on
template <int SPV>
__device__ __forceinline__ void dc_sub_piece(unsigned *o, unsigned long long pos, const float2 *__restrict__ means, const DcGeom &g,
                                             const DcPrev &pv)
{
    const unsigned long long ka = pos >> g.log2, kz = (pos + (SPV - 1)) >> g.log2;
    const float2 ma = dc_prev(means, g, pv, ka), mz = kz == ka ? ma : dc_prev(means, g, pv, kz);
#pragma unroll
    for (int k = 0; k < SPV; k++) {
        const float2 m = ((pos + (unsigned)k) >> g.log2) == ka ? ma : mz;
        o[2 * k] = dc_sub_bits(o[2 * k], m.x);
        o[2 * k + 1] = dc_sub_bits(o[2 * k + 1], m.y);
    }
}

// 3. the samples of FMT of span sp at `src` (aligned to a sample) to cf32 at `dst` (aligned to 8 bytes), each less the mean
// of the block in front of its own.  dst16: dst + head samples lies on a 16-byte boundary.  (No __restrict__: dst may be src.)
template <int FMT>
__global__ __launch_bounds__(kChunkNT) void dc_sub_kernel(void *dst, const void *src, const ChunkSpan sp, const DcGeom g,
                                                          const float2 *means, const DcPrev pv, int dst16)
{
    constexpr int BPS = kFmtBytes<FMT>, SPV = 16 / BPS;
    const ChunkLane cl = chunk_lane();
    const long long gid = cl.gid, stride = cl.stride, head = sp.head, nvec = sp.nvec;
    const unsigned char *const bytes = static_cast<const unsigned char *>(src);
    const uint4 *const pieces = reinterpret_cast<const uint4 *>(bytes + head * BPS);
    unsigned *const out = static_cast<unsigned *>(dst);
    if constexpr (BPS < 8) {
        // (iq_balance_kernel's turn through LDS: store j of lane k writes piece 64 j + k of the wavefront's contiguous
        // 1024 QPL bytes; the trip count is the wavefront's, every lane reaches both wavefront barriers; slot s of lane k
        // sits at k QPL + (s ^ k % QPL))
        constexpr int QPL = SPV / 2;
        __shared__ uint4 sh[kChunkNT * QPL];
        const int lane = threadIdx.x & 63;
        uint4 *const mine = sh + (threadIdx.x >> 6) * 64 * QPL;
        for (long long b = gid - lane; dst16 && b < nvec; b += stride) {
            const long long i = b + lane;
            if (i < nvec) {
                unsigned o[2 * SPV];
                iq_piece_bits<FMT>(pieces[i], o);
                dc_sub_piece<SPV>(o, g.first + (unsigned long long)(head + i * SPV), means, g, pv);
#pragma unroll
                for (int s = 0; s < QPL; s++)
                    mine[lane * QPL + (s ^ (lane & (QPL - 1)))] = make_uint4(o[4 * s], o[4 * s + 1], o[4 * s + 2], o[4 * s + 3]);
            }
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            __builtin_amdgcn_wave_barrier();
            uint4 *const q = reinterpret_cast<uint4 *>(out + 2 * (head + b * SPV));
            const long long left = nvec - b;
            const int live = (int)(left < 64 ? left : 64) * QPL;            // 16-byte pieces of this block that exist
#pragma unroll
            for (int j = 0; j < QPL; j++) {
                const int idx = j * 64 + lane, k = idx / QPL, s = idx % QPL;
                if (idx < live) q[idx] = mine[k * QPL + (s ^ (k & (QPL - 1)))];
            }
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            __builtin_amdgcn_wave_barrier();
        }
    }
    for (long long i = gid; (BPS == 8 || !dst16) && i < nvec; i += stride) {
        unsigned o[2 * SPV];
        iq_piece_bits<FMT>(pieces[i], o);
        dc_sub_piece<SPV>(o, g.first + (unsigned long long)(head + i * SPV), means, g, pv);
        unsigned *q = out + 2 * (head + i * SPV);
        if (dst16) {
#pragma unroll
            for (int k = 0; k < SPV / 2; k++)
                reinterpret_cast<uint4 *>(q)[k] = make_uint4(o[4 * k], o[4 * k + 1], o[4 * k + 2], o[4 * k + 3]);
        } else {
#pragma unroll
            for (int k = 0; k < SPV; k++) reinterpret_cast<uint2 *>(q)[k] = uint2{ o[2 * k], o[2 * k + 1] };
        }
    }
    const long long si = cl.scalar<SPV>(sp);
    if (si < 0) return;
    unsigned o[2];
    iq_sample_bits<FMT>(bytes + si * BPS, o);
    dc_sub_piece<1>(o, g.first + (unsigned long long)si, means, g, pv);
    reinterpret_cast<uint2 *>(out)[si] = uint2{ o[0], o[1] };
}

// ---- host side ----

// The rings and the record on the device (cache: what they hold is told apart by the stream position the host keeps).
struct DcRings {
    unsigned long long *d_acc = nullptr;
    float2 *d_means = nullptr;
    DcRec *d_rec = nullptr;
    unsigned slots = 0;                 // a power of two

    // blocks of 2^log2 that `span` samples from any position touch, the one in front of them, and one to spare
    static unsigned slots_for(size_t span, int log2)
    {
        unsigned s = 4;
        while ((size_t)s < (span >> log2) + 4) s <<= 1;
        return s;
    }
    void free()
    {
        if (d_acc) (void)hipFree(d_acc);
        if (d_means) (void)hipFree(d_means);
        if (d_rec) (void)hipFree(d_rec);
        *this = DcRings{};
    }
    // rings for launches of at most `span` samples (the device is current; nothing of the pass is in flight)
    int alloc(size_t span, int log2)
    {
        const unsigned want = slots_for(span, log2);
        if (want <= slots) return 0;
        free();
        if (hipMalloc(reinterpret_cast<void **>(&d_acc), (size_t)want * kDcSlotWords * 8) != hipSuccess ||
            hipMalloc(reinterpret_cast<void **>(&d_means), (size_t)want * sizeof(float2)) != hipSuccess ||
            hipMalloc(reinterpret_cast<void **>(&d_rec), sizeof(DcRec)) != hipSuccess) {
            free();
            return -1;
        }
        slots = want;
        return 0;
    }
};

// the slots of blocks [a, b) cleared on `stream` (b - a <= slots)
static inline int dc_clear_slots(const DcRings &r, uint64_t a, uint64_t b, hipStream_t stream)
{
    while (a < b) {
        const uint64_t s0 = a & (r.slots - 1), run = std::min<uint64_t>(b - a, r.slots - s0);
        if (hipMemsetAsync(r.d_acc + s0 * kDcSlotWords, 0, run * kDcSlotWords * 8, stream) != hipSuccess) return -1;
        a += run;
    }
    return 0;
}

// n samples of fmt at d_in (aligned to a sample), which lie at stream position pos, to cf32 at d_out (aligned to 8 bytes;
// d_in itself for an 8-byte format, no other overlap) on `stream`: the three launches.  `opened`: the blocks whose slots
// have been opened so far (it moves on); block k0 is corrected by (m0_i, m0_q), every other block by the means ring.
// fresh: the record starts over when this call closes a block.  always_close: the close pass runs even when no block
// ends (irdm_dc_block_device reads the open sums from the record).  0, or -1: a span the rings are too small for, more
// than kChunkMaxLaunch samples, or a launch that failed; n == 0 launches nothing.
static inline int dc_enqueue(const DcRings &r, int log2, int fmt, void *d_out, const void *d_in, size_t n, uint64_t pos, uint64_t &opened,
                             uint64_t k0, float m0_i, float m0_q, bool fresh, bool always_close, hipStream_t stream)
{
    if (n == 0) return 0;
    const uint64_t kf = pos >> log2, kl = (pos + n - 1) >> log2, k_end = (pos + n) >> log2;
    if (!r.slots || kl - kf + 3 > r.slots || n > kChunkMaxLaunch || !fmt_valid(fmt)) return -1;
    const size_t bps = (size_t)fmt_bytes(fmt);
    if (opened < kf) opened = kf;
    if (dc_clear_slots(r, opened, kl + 1, stream) != 0) return -1;
    opened = kl + 1;
    int grid = 0;
    const ChunkSpan sp = chunk_span((int)bps, d_in, n, kChunkNT, kChunkMaxGrid, &grid);
    const DcGeom g{ (unsigned long long)pos, log2, r.slots - 1 };
    const DcPrev pv{ (unsigned long long)k0, m0_i, m0_q };
    const int dst16 = ((reinterpret_cast<uintptr_t>(d_out) + (uintptr_t)sp.head * 8u) & 15u) == 0 ? 1 : 0;
    fmt_dispatch(fmt, [&](auto f) {
        hipLaunchKernelGGL((dc_sums_kernel<decltype(f)::value>), dim3(grid), dim3(kChunkNT), 0, stream, d_in, sp, g, r.d_acc);
    });
    if (hipGetLastError() != hipSuccess) return -1;
    if (k_end > kf || always_close) {
        hipLaunchKernelGGL((dc_close_kernel<kDcCopies>), dim3(1), dim3(64), 0, stream, r.d_acc, r.d_means, r.d_rec, g, (unsigned long long)kf,
                           (unsigned long long)k_end, fresh ? 1 : 0, k_end < opened ? 1 : 0);
        if (hipGetLastError() != hipSuccess) return -1;
    }
    fmt_dispatch(fmt, [&](auto f) {
        hipLaunchKernelGGL((dc_sub_kernel<decltype(f)::value>), dim3(grid), dim3(kChunkNT), 0, stream, d_out, d_in, sp, g, r.d_means, pv, dst16);
    });
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

// irdm_dc_block / irdm_frontend_dc_block: the setting (configuration: it survives a reset) and the rings (cache);
// host_chain.hpp holds it and the staging buffer for a wire format other than cf32
struct DcBlock : DcRings {
    int on = 0, log2 = kDcDefaultLog2, wire_fmt = 2;
    float seed_i = 0.0f, seed_q = 0.0f;
    size_t span = 0;                    // samples per round of three launches (what the rings were made for)
};
// Stream state: the samples the pass has taken and the blocks whose slots it has opened.  The open block's sums, the means
// and the figures lie in the rings and the record on the device, which these two numbers give their meaning: a fresh
// DcStream makes the next feed open block 0 again and the next close pass start the record over.
struct DcStream {
    uint64_t pos = 0, opened = 0;
};

// a chunk of a context or a front end: n samples of the wire format at d_in to cf32 at d_out, in rounds of at most dc.span
// samples
static inline int dc_feed(const DcBlock &dc, DcStream &st, void *d_out, const void *d_in, size_t n, hipStream_t stream)
{
    const size_t bps = (size_t)fmt_bytes(dc.wire_fmt);
    for (size_t off = 0; off < n; off += dc.span) {
        const size_t piece = std::min(dc.span, n - off);
        if (dc_enqueue(dc, dc.log2, dc.wire_fmt, static_cast<char *>(d_out) + off * 8, static_cast<const char *>(d_in) + off * bps, piece,
                       st.pos, st.opened, 0, dc.seed_i, dc.seed_q, (st.pos >> dc.log2) == 0, false, stream) != 0)
            return -1;
        st.pos += piece;
    }
    return 0;
}

// the figures of a stream so far (`stream` has been waited for)
static inline int dc_result(const DcBlock &dc, const DcStream &st, irdm_dc_stats_t *out)
{
    memset(out, 0, sizeof(*out));
    out->n_samples = st.pos;
    out->n_blocks = st.pos >> dc.log2;
    out->block_log2 = dc.log2;
    out->wire_format = dc.wire_fmt;
    out->seed_i = dc.seed_i;
    out->seed_q = dc.seed_q;
    if (!out->n_blocks) return 0;
    DcRec rec;
    if (hipMemcpy(&rec, dc.d_rec, sizeof(rec), hipMemcpyDeviceToHost) != hipSuccess || rec.blocks != out->n_blocks) return -1;
    out->first_i = rec.first[0], out->first_q = rec.first[1];
    out->last_i = rec.last[0], out->last_q = rec.last[1];
    out->min_i = rec.mn[0], out->min_q = rec.mn[1];
    out->max_i = rec.mx[0], out->max_q = rec.mx[1];
    return 0;
}

// the setting taken: 0, or -1 for a block length outside 12 .. 24, an unknown wire format, a seed that is not finite or
// lies beyond +-64, or memory that could not be had.  max_chunk: the longest chunk a feed brings (0: any).  A negative log2
// switches the pass off (the cache stays).
static inline int dc_configure(DcBlock &dc, int wire_fmt, int log2, float seed_i, float seed_q, size_t max_chunk)
{
    if (log2 < 0) {
        dc.on = 0;
        return 0;
    }
    if (log2 < kDcMinLog2 || log2 > kDcMaxLog2 || !fmt_valid(wire_fmt) || !(fabsf(seed_i) <= 64.0f) || !(fabsf(seed_q) <= 64.0f)) return -1;
    if (log2 != dc.log2) dc.DcRings::free();
    const size_t span = max_chunk ? std::min(max_chunk, kDcSpan) : kDcSpan;
    if (span > dc.span) dc.DcRings::free();
    if (dc.alloc(span, log2) != 0) return -1;
    dc.span = std::max(span, dc.span);
    dc.on = 1;
    dc.log2 = log2;
    dc.wire_fmt = wire_fmt;
    dc.seed_i = seed_i;
    dc.seed_q = seed_q;
    return 0;
}

// ---- irdm_dc_mean_host: the same rule on host memory ----

// component `arm` of sample i of format fmt at p, as load_iq<fmt> converts it: its bits
static inline unsigned dc_host_bits(int fmt, const unsigned char *p, size_t i, int arm)
{
    float c = 0.0f;
    switch (fmt) {
    case 2: {
        unsigned w;
        memcpy(&w, p + i * 8 + (size_t)arm * 4, 4);
        return w;
    }
    case 0: c = (float)(signed char)p[i * 2 + (size_t)arm] / 128.0f; break;
    case 6: c = cu8_f((int)p[i * 2 + (size_t)arm]); break;
    case 1: case 3: case 4: {
        short v;
        memcpy(&v, p + i * 4 + (size_t)arm * 2, 2);
        c = fmt == 1 ? (float)(v >> 8) / 128.0f : (fmt == 3 ? i16_full<3>(v) : i16_full<4>(v));
        break;
    }
    default: {
        int v;
        memcpy(&v, p + i * 8 + (size_t)arm * 4, 4);
        c = fmt == 8 ? i32_f<8>(v) : i32_f<9>(v);
    }
    }
    unsigned w;
    memcpy(&w, &c, 4);
    return w;
}

// out = (float)((double)sum q / (n 2^32)) per arm over the n leading samples (n a power of two gives a block's m_k; any
// other n divides by n all the same); n == 0 gives zeros
static inline int dc_mean_host(int fmt, const void *h_iq, size_t n, float out[2])
{
    if (!fmt_valid(fmt) || (!h_iq && n) || !out || n > ((size_t)1 << kDcMaxLog2)) return -1;
    long long s[2] = { 0, 0 };
    const unsigned char *p = static_cast<const unsigned char *>(h_iq);
    for (size_t i = 0; i < n; i++) {
        s[0] += dc_quant(dc_host_bits(fmt, p, i, 0));
        s[1] += dc_quant(dc_host_bits(fmt, p, i, 1));
    }
    for (int a = 0; a < 2; a++) out[a] = n ? (float)((double)s[a] / ((double)n * 4294967296.0)) : 0.0f;
    return 0;
}

}  // namespace irdm
