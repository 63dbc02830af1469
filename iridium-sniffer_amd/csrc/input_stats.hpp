// input_stats.hpp -- option "input_stats" (irdm_input_stats_t, include/irdm_hip.h): DC offset, RMS, peak and the count of
// components at the converter's rails, reduced on the device over the raw samples of a context's or a front end's input.
//
// One memory-bound pass per chunk on a side stream, behind the chunk's arrival and beside K1; nothing of it is fused into
// K1 or the decimator.  The kernel reads b_in bytes per sample and writes nothing but its sums:
//   * the span geometry of chunk_span.hpp, the codes taken from a piece by iq_piece.hpp;
//   * integer formats: x = c * 2^-K with an integer c (ci8 c = v, K = 7; cu8 c = 2u - 255, K = 8; ci16 c = v >> 8, K = 7;
//     ci16-full c = v, K = 15; sc16q11 c = v, K = 11).  A lane sums c and c^2 of one 16-byte piece in 32 bits (int16: c^2
//     straight into 64 -- one square already needs 31), then adds to its 64-bit accumulators; rails and the extreme codes
//     are taken on the file's codes.  The int32 formats (ci32 c = v, K = 31; 24-bit in int32 c = v, K = 23): c^2 reaches
//     2^62, so 2^30 of them do not fit a 64-bit word -- a lane keeps the low and the high 32 bits of every square in two
//     64-bit sums (each below 2^62 per launch) and the host puts them together in 128 bits.  Wavefronts reduce by shuffles, the workgroup through LDS, then one 64-bit integer
//     atomic per quantity.  Integer sums do not depend on any order: the result is that of the stream, however it was cut.
//   * cf32: x and x^2 are exact doubles; a workgroup's partial sums go to its row of a slab the host folds in row order
//     (no floating-point atomics: the result is reproducible for a given cut of the stream); max |x| is an integer
//     maximum on the float's bits; NaN and Inf are counted and left out.
// The host adds the launches' 64-bit sums in 128 bits and forms sum / sum_sq with one rounding.
//
// Included by the translation units that launch it (feed.cpp: a context's input and irdm_input_stats_device;
// frontend.cpp: the capture in front of K0 / K0r).
#pragma once
#include <math.h>
#include <string.h>
#include <algorithm>
#include "common.hpp"
#include "chunk_span.hpp"
#include "iq_piece.hpp"
#include "pass_ring.hpp"
#include "wave_reduce.hpp"
#include "../../include/irdm_hip.h"

namespace irdm {

// samples of a launch, below kChunkMaxLaunch: a lane's 32-bit counts cannot overflow (two components per sample)
constexpr size_t kIsMaxLaunch = (size_t)1 << 30;

// one launch's sums on the device, all zero before the launch; cf32: [kChunkMaxGrid][4] doubles behind it
struct InputStatsAcc {
    unsigned long long rail_lo[2], rail_hi[2], nonfinite[2];
    unsigned long long sum_c[2];        // two's complement
    unsigned long long sum_c2[2];
    unsigned min_key[2];                // max of 2^31 - code (0: no component yet)
    unsigned max_key[2];                // max of 2^31 + code
    unsigned abs_bits[2];               // cf32: the largest bit pattern of |x| over finite x
    unsigned pad[2];
    unsigned long long sum_c2_hi[2];    // the int32 formats: the sum of c^2 >> 32 (sum_c2 then holds that of c^2 & 0xffffffff)
};
constexpr size_t kIsBlockBytes = sizeof(InputStatsAcc) + sizeof(double) * 4 * kChunkMaxGrid;

template <int FMT> struct IsFmt;
template <> struct IsFmt<0> { static constexpr int LO = -128, HI = 127, K = 7; };
template <> struct IsFmt<6> { static constexpr int LO = 0, HI = 255, K = 8; };
template <> struct IsFmt<1> { static constexpr int LO = -32768, HI = 32767, K = 7; };
template <> struct IsFmt<3> { static constexpr int LO = -32768, HI = 32767, K = 15; };
template <> struct IsFmt<4> { static constexpr int LO = -2048, HI = 2047, K = 11; };
template <> struct IsFmt<8> { static constexpr int LO = -0x7fffffff - 1, HI = 0x7fffffff, K = 31; };
template <> struct IsFmt<9> { static constexpr int LO = -(1 << 23), HI = (1 << 23) - 1, K = 23; };
constexpr bool is_fmt32(int fmt) { return fmt == 8 || fmt == 9; }
constexpr int is_fmt_k(int fmt) { return fmt == 0 || fmt == 1 ? 7 : (fmt == 6 ? 8 : (fmt == 3 ? 15 : (fmt == 4 ? 11 : (fmt == 8 ? 31 : 23)))); }

// the integer c of a file code: x = c * 2^-K is what load_iq gives
template <int FMT>
__host__ __device__ __forceinline__ int is_level(int code)
{
    return FMT == 6 ? 2 * code - 255 : (FMT == 1 ? code >> 8 : code);
}

// a lane's accumulators, integer formats; ls / ls2: the sums of the piece at hand
struct IsLane {
    unsigned lo[2], hi[2];
    int cmin[2], cmax[2];
    long long s[2];
    unsigned long long s2[2];
    unsigned long long s2h[2];          // (the int32 formats)
    int ls[2];
    unsigned ls2[2];
};

template <int FMT>
__device__ __forceinline__ void is_take(IsLane &a, int k, int code)
{
    a.lo[k] += code <= IsFmt<FMT>::LO ? 1u : 0u;
    a.hi[k] += code >= IsFmt<FMT>::HI ? 1u : 0u;
    a.cmin[k] = code < a.cmin[k] ? code : a.cmin[k];
    a.cmax[k] = code > a.cmax[k] ? code : a.cmax[k];
    const int c = is_level<FMT>(code);
    if (is_fmt32(FMT)) {                                                    // no 32-bit piece sums: one c already needs 32 bits
        const unsigned long long c2 = (unsigned long long)((long long)c * (long long)c);   // <= 2^62
        a.s[k] += (long long)c;
        a.s2[k] += c2 & 0xffffffffull;
        a.s2h[k] += c2 >> 32;
        return;
    }
    a.ls[k] += c;
    if (kFmtBytes<FMT> == 2) a.ls2[k] += (unsigned)(c * c);                 // at most 8 * 255^2 per piece
    else a.s2[k] += (unsigned long long)(unsigned)(c * c);                  // c^2 <= 2^30
}

__device__ __forceinline__ void is_piece_done(IsLane &a)
{
    for (int k = 0; k < 2; k++) {
        a.s[k] += (long long)a.ls[k];
        a.s2[k] += (unsigned long long)a.ls2[k];
        a.ls[k] = 0;
        a.ls2[k] = 0u;
    }
}

// a lane's accumulators, cf32
struct IsLaneF {
    unsigned lo[2], hi[2], nf[2], absb[2];
    double s[2], s2[2];
};

__device__ __forceinline__ void is_take_f(IsLaneF &a, int k, unsigned bits)
{
    const unsigned mag = bits & 0x7fffffffu;
    if (mag >= 0x7f800000u) {                           // NaN or Inf: counted, left out of everything else
        a.nf[k] += 1u;
        return;
    }
    const float x = __uint_as_float(bits);
    a.lo[k] += x <= -1.0f ? 1u : 0u;
    a.hi[k] += x >= 1.0f ? 1u : 0u;
    a.absb[k] = mag > a.absb[k] ? mag : a.absb[k];
    const double d = (double)x, q = d * d;              // both exact
    a.s[k] += d;
    a.s2[k] += q;
}

// The samples of span sp at `in` (aligned to a sample).  Every thread reaches every shuffle and barrier.
template <int FMT>
__global__ __launch_bounds__(kChunkNT) void input_stats_kernel(const void *__restrict__ in, const ChunkSpan sp,
                                                               InputStatsAcc *__restrict__ acc, double *__restrict__ slab)
{
    constexpr int BPS = kFmtBytes<FMT>, SPV = 16 / BPS, NW = kChunkNT / 64;
    const ChunkLane cl = chunk_lane();
    const long long si = cl.scalar<SPV>(sp);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const unsigned char *const bytes = static_cast<const unsigned char *>(in);
    const uint4 *const pieces = reinterpret_cast<const uint4 *>(bytes + sp.head * BPS);

    if constexpr (FMT == 2) {
        __shared__ double sh_d[NW][4];
        __shared__ unsigned sh_u[NW][8];
        IsLaneF a;
        for (int k = 0; k < 2; k++) {
            a.lo[k] = a.hi[k] = a.nf[k] = a.absb[k] = 0u;
            a.s[k] = a.s2[k] = 0.0;
        }
        const auto take = [&](int k, int code) { is_take_f(a, k, (unsigned)code); };
        if (si >= 0) iq_sample_codes<FMT>(bytes + si * BPS, take);
        for (long long i = cl.gid; i < sp.nvec; i += cl.stride) iq_piece_codes<FMT>(pieces[i], take);
        // the order of every sum is fixed by the launch geometry: a lane's pieces, the shuffle tree, the waves in turn
        unsigned u[8] = { a.lo[0], a.lo[1], a.hi[0], a.hi[1], a.nf[0], a.nf[1], a.absb[0], a.absb[1] };
        double d[4] = { a.s[0], a.s[1], a.s2[0], a.s2[1] };
        for (int j = 0; j < 6; j++) u[j] = wave_sum(u[j]);
        for (int j = 6; j < 8; j++) u[j] = wave_max(u[j]);
        for (int j = 0; j < 4; j++) d[j] = wave_sum(d[j]);
        if (lane == 0) {
            for (int j = 0; j < 8; j++) sh_u[wave][j] = u[j];
            for (int j = 0; j < 4; j++) sh_d[wave][j] = d[j];
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            for (int w = 1; w < NW; w++) {
                for (int j = 0; j < 6; j++) u[j] += sh_u[w][j];
                for (int j = 6; j < 8; j++) u[j] = sh_u[w][j] > u[j] ? sh_u[w][j] : u[j];
                for (int j = 0; j < 4; j++) d[j] += sh_d[w][j];
            }
            for (int k = 0; k < 2; k++) {
                if (u[k]) atomicAdd(&acc->rail_lo[k], (unsigned long long)u[k]);
                if (u[2 + k]) atomicAdd(&acc->rail_hi[k], (unsigned long long)u[2 + k]);
                if (u[4 + k]) atomicAdd(&acc->nonfinite[k], (unsigned long long)u[4 + k]);
                if (u[6 + k]) atomicMax(&acc->abs_bits[k], u[6 + k]);
            }
            for (int j = 0; j < 4; j++) slab[(size_t)blockIdx.x * 4 + j] = d[j];
        }
    } else {
        constexpr int NQ = is_fmt32(FMT) ? 10 : 8;
        __shared__ unsigned long long sh_q[NW][NQ];
        __shared__ int sh_m[NW][4];
        IsLane a;
        for (int k = 0; k < 2; k++) {
            a.lo[k] = a.hi[k] = 0u;
            a.cmin[k] = 0x7fffffff;
            a.cmax[k] = -0x7fffffff - 1;
            a.s[k] = 0;
            a.s2[k] = 0ull;
            a.s2h[k] = 0ull;
            a.ls[k] = 0;
            a.ls2[k] = 0u;
        }
        const auto take = [&](int k, int code) { is_take<FMT>(a, k, code); };
        if (si >= 0) {
            iq_sample_codes<FMT>(bytes + si * BPS, take);
            is_piece_done(a);
        }
        for (long long i = cl.gid; i < sp.nvec; i += cl.stride) {
            iq_piece_codes<FMT>(pieces[i], take);
            is_piece_done(a);               // (the int32 formats keep no piece sums: nothing to add)
        }
        unsigned long long q[10] = { a.lo[0], a.lo[1], a.hi[0], a.hi[1], (unsigned long long)a.s[0], (unsigned long long)a.s[1],
                                     a.s2[0], a.s2[1], a.s2h[0], a.s2h[1] };
        int m[4] = { a.cmin[0], a.cmin[1], a.cmax[0], a.cmax[1] };
        for (int j = 0; j < NQ; j++) q[j] = wave_sum(q[j]);
        for (int j = 0; j < 2; j++) m[j] = wave_min(m[j]);
        for (int j = 2; j < 4; j++) m[j] = wave_max(m[j]);
        if (lane == 0) {
            for (int j = 0; j < NQ; j++) sh_q[wave][j] = q[j];
            for (int j = 0; j < 4; j++) sh_m[wave][j] = m[j];
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            for (int w = 1; w < NW; w++) {
                for (int j = 0; j < NQ; j++) q[j] += sh_q[w][j];
                for (int j = 0; j < 2; j++) m[j] = sh_m[w][j] < m[j] ? sh_m[w][j] : m[j];
                for (int j = 2; j < 4; j++) m[j] = sh_m[w][j] > m[j] ? sh_m[w][j] : m[j];
            }
            for (int k = 0; k < 2; k++) {
                if (q[k]) atomicAdd(&acc->rail_lo[k], q[k]);
                if (q[2 + k]) atomicAdd(&acc->rail_hi[k], q[2 + k]);
                if (q[4 + k]) atomicAdd(&acc->sum_c[k], q[4 + k]);
                if (q[6 + k]) atomicAdd(&acc->sum_c2[k], q[6 + k]);
                if (is_fmt32(FMT) && q[8 + k]) atomicAdd(&acc->sum_c2_hi[k], q[8 + k]);
                if (m[k] <= m[2 + k]) {                 // the workgroup saw a component
                    // (the int32 formats: 2^31 - 1 - code, so that INT32_MIN has a key; 0 is then the key of INT32_MAX, and a
                    // launch that ran at all has seen a component)
                    atomicMax(&acc->min_key[k], (is_fmt32(FMT) ? 0x7fffffffu : 0x80000000u) - (unsigned)m[k]);
                    atomicMax(&acc->max_key[k], 0x80000000u + (unsigned)m[2 + k]);
                }
            }
        }
    }
}

// ---- host side ----

// the running totals of a stream
struct InputStatsRun {
    uint64_t n = 0;
    uint64_t lo[2] = { 0, 0 }, hi[2] = { 0, 0 }, nf[2] = { 0, 0 };
    __int128 sc[2] = { 0, 0 };
    unsigned __int128 sc2[2] = { 0, 0 };
    unsigned min_key[2] = { 0, 0 }, max_key[2] = { 0, 0 }, abs_bits[2] = { 0, 0 };
    double fs[2] = { 0.0, 0.0 }, fs2[2] = { 0.0, 0.0 };
};

// One launch over n <= kIsMaxLaunch samples (aligned to a sample of fmt) into d_block (kIsBlockBytes, zeroed here) on
// `stream`; returns the grid (the rows of the slab a cf32 launch wrote; 0: n == 0, nothing launched), -1 on error.
static inline int launch_input_stats(int fmt, const void *d_in, size_t n, void *d_block, hipStream_t stream)
{
    if (!fmt_valid(fmt) || n > kIsMaxLaunch || (reinterpret_cast<uintptr_t>(d_in) % (size_t)fmt_bytes(fmt)) != 0) return -1;
    if (n == 0) return 0;
    int grid = 0;
    const ChunkSpan sp = chunk_span(fmt_bytes(fmt), d_in, n, kChunkNT, kChunkMaxGrid, &grid);
    InputStatsAcc *acc = static_cast<InputStatsAcc *>(d_block);
    double *slab = reinterpret_cast<double *>(acc + 1);
    if (hipMemsetAsync(acc, 0, sizeof(InputStatsAcc), stream) != hipSuccess) return -1;
    fmt_dispatch(fmt, [&](auto f) {
        hipLaunchKernelGGL((input_stats_kernel<decltype(f)::value>), dim3(grid), dim3(kChunkNT), 0, stream, d_in, sp, acc, slab);
    });
    return hipGetLastError() == hipSuccess ? grid : -1;
}

// a finished launch's block (host copy) into the totals
static inline void input_stats_fold(InputStatsRun &t, int fmt, const void *h_block, int grid, size_t n)
{
    t.n += n;
    if (grid <= 0) return;
    const InputStatsAcc &a = *static_cast<const InputStatsAcc *>(h_block);
    const double *slab = reinterpret_cast<const double *>(&a + 1);
    for (int k = 0; k < 2; k++) {
        t.lo[k] += a.rail_lo[k];
        t.hi[k] += a.rail_hi[k];
        t.nf[k] += a.nonfinite[k];
        t.sc[k] += (__int128)(long long)a.sum_c[k];
        t.sc2[k] += (unsigned __int128)a.sum_c2[k] + ((unsigned __int128)a.sum_c2_hi[k] << 32);
        t.min_key[k] = std::max(t.min_key[k], a.min_key[k]);
        t.max_key[k] = std::max(t.max_key[k], a.max_key[k]);
        t.abs_bits[k] = std::max(t.abs_bits[k], a.abs_bits[k]);
    }
    if (fmt == IRDM_FMT_CF32)
        for (int g = 0; g < grid; g++)
            for (int k = 0; k < 2; k++) {
                t.fs[k] += slab[(size_t)g * 4 + k];
                t.fs2[k] += slab[(size_t)g * 4 + 2 + k];
            }
}

static inline void input_stats_result(const InputStatsRun &t, int fmt, irdm_input_stats_t *out)
{
    memset(out, 0, sizeof(*out));
    out->n_samples = t.n;
    const int K = is_fmt_k(fmt);
    const bool wide = is_fmt32(fmt);                     // (their keys: see the kernel)
    for (int k = 0; k < 2; k++) {
        out->n_rail_lo[k] = t.lo[k];
        out->n_rail_hi[k] = t.hi[k];
        out->n_nonfinite[k] = t.nf[k];
        if (fmt == IRDM_FMT_CF32) {
            out->sum[k] = t.fs[k];
            out->sum_sq[k] = t.fs2[k];
            memcpy(&out->abs_max[k], &t.abs_bits[k], sizeof(float));
            continue;
        }
        out->sum[k] = ldexp((double)t.sc[k], -K);                // one rounding: the conversion; the scaling is exact
        out->sum_sq[k] = ldexp((double)t.sc2[k], -2 * K);
        if (wide ? t.n != 0 : t.min_key[k] != 0) {
            out->code_min[k] = (int32_t)((wide ? 0x7fffffffu : 0x80000000u) - t.min_key[k]);
            out->code_max[k] = (int32_t)(t.max_key[k] - 0x80000000u);
            // the level is monotone in the code: max |x| is at one of the two extreme codes (|c| <= 2^15: exact floats; the
            // int32 formats: (float)|c| rounds as load_iq's (float)v does, and rounding keeps the order)
            auto level = [&](int code) {
                const long long c = fmt == 6 ? is_level<6>(code) : (fmt == 1 ? is_level<1>(code) : code);
                return ldexpf((float)(c < 0 ? -c : c), -K);
            };
            out->abs_max[k] = std::max(level(out->code_min[k]), level(out->code_max[k]));
        }
    }
}

// The pass of a context or a front end: its switch (configuration) and its ring on a side stream (cache; pass_ring.hpp).
struct InputStatsPass : PassRing {
    int on = 0;
};
// Stream state: the totals, and the launches in flight (an entry's meta: the launch's grid).
struct InputStatsStream : PassRingStream {
    InputStatsRun run;
};

static inline auto input_stats_folder(InputStatsStream &st, int fmt)
{
    return [&st, fmt](const void *h_block, const PassRingStream::Entry &e) { input_stats_fold(st.run, fmt, h_block, (int)e.meta, e.n); };
}

// launches up to and including tag `upto` are waited for and folded, oldest first
static inline int input_stats_settle(InputStatsPass &ps, InputStatsStream &st, int fmt, uint64_t upto)
{
    return ps.settle(st, upto, input_stats_folder(st, fmt));
}

// n samples at d_in, produced on `arrival` (nullptr: complete in memory): their pass on the side stream.  The launches
// carry `tag`; the caller orders whatever overwrites d_in behind ps.ev[st.last_slot] or settles the tag first.
static inline int input_stats_enqueue(InputStatsPass &ps, InputStatsStream &st, int fmt, const void *d_in, size_t n,
                                      hipStream_t arrival, uint64_t tag)
{
    if (n == 0) return 0;
    if (ps.follow(arrival) != 0) return -1;
    const size_t bps = (size_t)fmt_bytes(fmt);
    for (size_t off = 0; off < n; off += kIsMaxLaunch) {
        const size_t piece = std::min(kIsMaxLaunch, n - off);
        const int slot = ps.acquire(st, input_stats_folder(st, fmt));
        if (slot < 0) return -1;
        const int grid = launch_input_stats(fmt, static_cast<const char *>(d_in) + off * bps, piece, ps.d_block[slot], ps.stream);
        if (grid < 0) return -1;
        const size_t bytes = sizeof(InputStatsAcc) + (fmt == IRDM_FMT_CF32 ? sizeof(double) * 4 * (size_t)grid : 0);
        if (ps.commit(st, slot, bytes, ps.stream, (uint64_t)grid, piece, tag) != 0) return -1;
    }
    return 0;
}

}  // namespace irdm
