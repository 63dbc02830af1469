// input_stats.hpp -- option "input_stats" (irdm_input_stats_t, include/irdm_hip.h): DC offset, RMS, peak and the count of
// components at the converter's rails, reduced on the device over the raw samples of a context's or a front end's input.
//
// One memory-bound pass per chunk on a side stream, behind the chunk's arrival and beside K1; nothing of it is fused into
// K1 or the decimator.  The kernel reads b_in bytes per sample and writes nothing but its sums:
//   * 16-byte loads per lane (8 / 4 / 2 samples at 2 / 4 / 8 bytes per sample), a scalar head and tail for a base that is
//     aligned to a sample only;
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
#include <deque>
#include "common.hpp"
#include "../../include/irdm_hip.h"

namespace irdm {

constexpr int kIsNT = 256;                              // threads of a workgroup
constexpr int kIsMaxGrid = 2048;                        // workgroups of a launch (rows of the cf32 slab)
constexpr size_t kIsMaxLaunch = (size_t)1 << 30;        // samples of a launch: a lane's 32-bit counts cannot overflow
constexpr int kIsSlots = 4;                             // launches in flight per context

// one launch's sums on the device, all zero before the launch; cf32: [kIsMaxGrid][4] doubles behind it
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
constexpr size_t kIsBlockBytes = sizeof(InputStatsAcc) + sizeof(double) * 4 * kIsMaxGrid;

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

// one 32-bit word of the input: two samples (8-bit formats) or one (int16 formats)
template <int FMT>
__device__ __forceinline__ void is_word(IsLane &a, unsigned w)
{
    if (FMT == 0) {
        is_take<FMT>(a, 0, (int)(signed char)(w & 0xff));
        is_take<FMT>(a, 1, (int)(signed char)((w >> 8) & 0xff));
        is_take<FMT>(a, 0, (int)(signed char)((w >> 16) & 0xff));
        is_take<FMT>(a, 1, (int)(signed char)(w >> 24));
    } else if (FMT == 6) {
        is_take<FMT>(a, 0, (int)(w & 0xff));
        is_take<FMT>(a, 1, (int)((w >> 8) & 0xff));
        is_take<FMT>(a, 0, (int)((w >> 16) & 0xff));
        is_take<FMT>(a, 1, (int)(w >> 24));
    } else {
        is_take<FMT>(a, 0, (int)(short)(w & 0xffff));
        is_take<FMT>(a, 1, (int)(short)(w >> 16));
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

// a wavefront's reductions into lane 0: shuffles of 32-bit words (a 64-bit value travels as its two halves)
__device__ __forceinline__ unsigned long long is_down64(unsigned long long v, int d)
{
    const unsigned lo = __shfl_down((unsigned)v, d), hi = __shfl_down((unsigned)(v >> 32), d);
    return ((unsigned long long)hi << 32) | lo;
}
__device__ __forceinline__ unsigned is_wave_sum(unsigned v)
{
    for (int d = 32; d > 0; d >>= 1) v += __shfl_down(v, d);
    return v;
}
__device__ __forceinline__ unsigned long long is_wave_sum(unsigned long long v)
{
    for (int d = 32; d > 0; d >>= 1) v += is_down64(v, d);
    return v;
}
__device__ __forceinline__ double is_wave_sum(double v)
{
    for (int d = 32; d > 0; d >>= 1) v += __builtin_bit_cast(double, is_down64(__builtin_bit_cast(unsigned long long, v), d));
    return v;
}
__device__ __forceinline__ int is_wave_min(int v)
{
    for (int d = 32; d > 0; d >>= 1) {
        const int o = __shfl_down(v, d);
        v = o < v ? o : v;
    }
    return v;
}
template <typename T>
__device__ __forceinline__ T is_wave_max(T v)
{
    for (int d = 32; d > 0; d >>= 1) {
        const T o = __shfl_down(v, d);
        v = o > v ? o : v;
    }
    return v;
}

// n samples at `in` (aligned to a sample): `head` samples up to the first 16-byte boundary, nvec 16-byte pieces, the rest.
// Every thread reaches every shuffle and barrier.
template <int FMT>
__global__ __launch_bounds__(kIsNT) void input_stats_kernel(const void *__restrict__ in, long long n, long long head,
                                                            long long nvec, InputStatsAcc *__restrict__ acc,
                                                            double *__restrict__ slab)
{
    constexpr int BPS = kFmtBytes<FMT>, SPV = 16 / BPS, NW = kIsNT / 64;
    const long long gid = (long long)blockIdx.x * kIsNT + threadIdx.x, stride = (long long)gridDim.x * kIsNT;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const unsigned char *const bytes = static_cast<const unsigned char *>(in);
    const uint4 *const pieces = reinterpret_cast<const uint4 *>(bytes + head * BPS);
    // the scalar head and tail: at most SPV - 1 samples each, one per thread of the first workgroup
    const long long tail0 = head + nvec * SPV;
    long long si = -1;
    if (gid < head) si = gid;
    else if (gid - head < n - tail0) si = tail0 + (gid - head);

    if constexpr (FMT == 2) {
        __shared__ double sh_d[NW][4];
        __shared__ unsigned sh_u[NW][8];
        IsLaneF a;
        for (int k = 0; k < 2; k++) {
            a.lo[k] = a.hi[k] = a.nf[k] = a.absb[k] = 0u;
            a.s[k] = a.s2[k] = 0.0;
        }
        if (si >= 0) {
            const unsigned *w = reinterpret_cast<const unsigned *>(bytes + si * BPS);
            is_take_f(a, 0, w[0]);
            is_take_f(a, 1, w[1]);
        }
        for (long long i = gid; i < nvec; i += stride) {
            const uint4 v = pieces[i];
            is_take_f(a, 0, v.x);
            is_take_f(a, 1, v.y);
            is_take_f(a, 0, v.z);
            is_take_f(a, 1, v.w);
        }
        // the order of every sum is fixed by the launch geometry: a lane's pieces, the shuffle tree, the waves in turn
        unsigned u[8] = { a.lo[0], a.lo[1], a.hi[0], a.hi[1], a.nf[0], a.nf[1], a.absb[0], a.absb[1] };
        double d[4] = { a.s[0], a.s[1], a.s2[0], a.s2[1] };
        for (int j = 0; j < 6; j++) u[j] = is_wave_sum(u[j]);
        for (int j = 6; j < 8; j++) u[j] = is_wave_max(u[j]);
        for (int j = 0; j < 4; j++) d[j] = is_wave_sum(d[j]);
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
        if (si >= 0) {
            if (BPS == 8) {
                const int *w = reinterpret_cast<const int *>(bytes + si * BPS);
                is_take<FMT>(a, 0, w[0]);
                is_take<FMT>(a, 1, w[1]);
            } else if (BPS == 2) {
                const unsigned w = *reinterpret_cast<const unsigned short *>(bytes + si * BPS);
                if (FMT == 0) {
                    is_take<FMT>(a, 0, (int)(signed char)(w & 0xff));
                    is_take<FMT>(a, 1, (int)(signed char)(w >> 8));
                } else {
                    is_take<FMT>(a, 0, (int)(w & 0xff));
                    is_take<FMT>(a, 1, (int)(w >> 8));
                }
            } else {
                is_word<FMT>(a, *reinterpret_cast<const unsigned *>(bytes + si * BPS));
            }
            is_piece_done(a);
        }
        for (long long i = gid; i < nvec; i += stride) {
            const uint4 v = pieces[i];
            if (BPS == 8) {
                is_take<FMT>(a, 0, (int)v.x);
                is_take<FMT>(a, 1, (int)v.y);
                is_take<FMT>(a, 0, (int)v.z);
                is_take<FMT>(a, 1, (int)v.w);
            } else {
                is_word<FMT>(a, v.x);
                is_word<FMT>(a, v.y);
                is_word<FMT>(a, v.z);
                is_word<FMT>(a, v.w);
                is_piece_done(a);
            }
        }
        unsigned long long q[10] = { a.lo[0], a.lo[1], a.hi[0], a.hi[1], (unsigned long long)a.s[0], (unsigned long long)a.s[1],
                                     a.s2[0], a.s2[1], a.s2h[0], a.s2h[1] };
        int m[4] = { a.cmin[0], a.cmin[1], a.cmax[0], a.cmax[1] };
        for (int j = 0; j < NQ; j++) q[j] = is_wave_sum(q[j]);
        for (int j = 0; j < 2; j++) m[j] = is_wave_min(m[j]);
        for (int j = 2; j < 4; j++) m[j] = is_wave_max(m[j]);
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

// workgroups of the launch over n samples at d_in (0: nothing to launch)
static inline int input_stats_grid(int fmt, const void *d_in, size_t n, long long *head_out, long long *nvec_out)
{
    const int bps = fmt_bytes(fmt), spv = 16 / bps;
    const size_t mis = (size_t)(reinterpret_cast<uintptr_t>(d_in) & 15u);
    long long head = (long long)(((16 - mis) & 15u) / (size_t)bps);
    if (head > (long long)n) head = (long long)n;
    const long long nvec = ((long long)n - head) / spv;
    *head_out = head;
    *nvec_out = nvec;
    if (n == 0) return 0;
    const long long want = (nvec + kIsNT - 1) / kIsNT;
    return (int)(want < 1 ? 1 : (want > kIsMaxGrid ? kIsMaxGrid : want));
}

// One launch over n <= kIsMaxLaunch samples (aligned to a sample of fmt) into d_block (kIsBlockBytes, zeroed here) on
// `stream`; returns the grid (the rows of the slab a cf32 launch wrote), -1 on error.
static inline int launch_input_stats(int fmt, const void *d_in, size_t n, void *d_block, hipStream_t stream)
{
    if (!fmt_valid(fmt) || n > kIsMaxLaunch || (reinterpret_cast<uintptr_t>(d_in) % (size_t)fmt_bytes(fmt)) != 0) return -1;
    long long head = 0, nvec = 0;
    const int grid = input_stats_grid(fmt, d_in, n, &head, &nvec);
    if (grid == 0) return 0;
    InputStatsAcc *acc = static_cast<InputStatsAcc *>(d_block);
    double *slab = reinterpret_cast<double *>(acc + 1);
    if (hipMemsetAsync(acc, 0, sizeof(InputStatsAcc), stream) != hipSuccess) return -1;
#define IRDM_LAUNCH_IS(F)                                                                                               \
    hipLaunchKernelGGL((input_stats_kernel<F>), dim3(grid), dim3(kIsNT), 0, stream, d_in, (long long)n, head, nvec, acc, slab)
    switch (fmt) {
    case 0: IRDM_LAUNCH_IS(0); break;
    case 1: IRDM_LAUNCH_IS(1); break;
    case 2: IRDM_LAUNCH_IS(2); break;
    case 3: IRDM_LAUNCH_IS(3); break;
    case 4: IRDM_LAUNCH_IS(4); break;
    case 8: IRDM_LAUNCH_IS(8); break;
    case 9: IRDM_LAUNCH_IS(9); break;
    default: IRDM_LAUNCH_IS(6); break;
    }
#undef IRDM_LAUNCH_IS
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

// The pass of a context or a front end.  Cache: the side stream, kIsSlots blocks on the device with their pinned copies.
struct InputStatsPass {
    int on = 0;
    hipStream_t stream = nullptr;
    hipEvent_t ev_in = nullptr;
    void *d_block[kIsSlots] = {}, *h_block[kIsSlots] = {};
    hipEvent_t ev[kIsSlots] = {};
};
// Stream state: the totals, and the launches whose blocks have not been folded yet, oldest first.
struct InputStatsStream {
    InputStatsRun run;
    struct Pending { int slot, grid; size_t n; uint64_t tag; };
    std::deque<Pending> pending;
    uint64_t launches = 0;
    int last_slot = -1;                 // the slot of the launch enqueued last (-1: none since the stream began)
};

static inline void input_stats_pass_free(InputStatsPass &ps)
{
    if (ps.stream) (void)hipStreamSynchronize(ps.stream);
    for (int i = 0; i < kIsSlots; i++) {
        if (ps.d_block[i]) (void)hipFree(ps.d_block[i]);
        if (ps.h_block[i]) (void)hipHostFree(ps.h_block[i]);
        if (ps.ev[i]) (void)hipEventDestroy(ps.ev[i]);
    }
    if (ps.ev_in) (void)hipEventDestroy(ps.ev_in);
    if (ps.stream) (void)hipStreamDestroy(ps.stream);
    ps = InputStatsPass{};
}

// the buffers, when the option is first set (the device is current)
static inline int input_stats_pass_alloc(InputStatsPass &ps)
{
    if (ps.stream) return 0;
    bool ok = hipStreamCreateWithFlags(&ps.stream, hipStreamNonBlocking) == hipSuccess;
    ok = ok && hipEventCreateWithFlags(&ps.ev_in, hipEventDisableTiming) == hipSuccess;
    for (int i = 0; i < kIsSlots; i++) {
        ok = ok && hipMalloc(&ps.d_block[i], kIsBlockBytes) == hipSuccess;
        ok = ok && hipHostMalloc(&ps.h_block[i], kIsBlockBytes, hipHostMallocDefault) == hipSuccess;
        ok = ok && hipEventCreateWithFlags(&ps.ev[i], hipEventDisableTiming) == hipSuccess;
    }
    if (!ok) {
        input_stats_pass_free(ps);
        return -1;
    }
    return 0;
}

// launches up to and including tag `upto` are waited for and folded, oldest first
static inline int input_stats_settle(InputStatsPass &ps, InputStatsStream &st, int fmt, uint64_t upto)
{
    while (!st.pending.empty() && st.pending.front().tag <= upto) {
        const InputStatsStream::Pending e = st.pending.front();
        if (hipEventSynchronize(ps.ev[e.slot]) != hipSuccess) return -1;
        input_stats_fold(st.run, fmt, ps.h_block[e.slot], e.grid, e.n);
        st.pending.pop_front();
    }
    return 0;
}

// n samples at d_in, produced on `arrival` (nullptr: complete in memory): their pass on the side stream.  The launches
// carry `tag`; the caller orders whatever overwrites d_in behind ps.ev[st.last_slot] or settles the tag first.
static inline int input_stats_enqueue(InputStatsPass &ps, InputStatsStream &st, int fmt, const void *d_in, size_t n,
                                      hipStream_t arrival, uint64_t tag)
{
    if (n == 0) return 0;
    if (arrival) {
        if (hipEventRecord(ps.ev_in, arrival) != hipSuccess || hipStreamWaitEvent(ps.stream, ps.ev_in, 0) != hipSuccess) return -1;
    }
    const size_t bps = (size_t)fmt_bytes(fmt);
    for (size_t off = 0; off < n; off += kIsMaxLaunch) {
        const size_t piece = std::min(kIsMaxLaunch, n - off);
        const int slot = (int)(st.launches % kIsSlots);
        // the slot's previous launch (kIsSlots launches ago) leaves its pinned block first
        for (bool busy = true; busy;) {
            busy = false;
            for (const auto &e : st.pending) busy = busy || e.slot == slot;
            if (busy && input_stats_settle(ps, st, fmt, st.pending.front().tag) != 0) return -1;
        }
        const int grid = launch_input_stats(fmt, static_cast<const char *>(d_in) + off * bps, piece, ps.d_block[slot], ps.stream);
        if (grid < 0) return -1;
        const size_t bytes = sizeof(InputStatsAcc) + (fmt == IRDM_FMT_CF32 ? sizeof(double) * 4 * (size_t)grid : 0);
        if (hipMemcpyAsync(ps.h_block[slot], ps.d_block[slot], bytes, hipMemcpyDeviceToHost, ps.stream) != hipSuccess) return -1;
        if (hipEventRecord(ps.ev[slot], ps.stream) != hipSuccess) return -1;
        st.pending.push_back(InputStatsStream::Pending{ slot, grid, piece, tag });
        st.launches++;
        st.last_slot = slot;
    }
    return 0;
}

}  // namespace irdm
