// burst_resample.hpp -- option "burst_resample" (include/irdm_hip.h): the decimated row of every burst resampled to exactly
// 250 000 samples/s before the 25-tap low-pass, for streams whose rate is no multiple of 250 kHz.
//
// The decimator leaves a burst's row at fs / decim, decim = round(fs / 250000): 218.75 .. 291.67 kHz.  Everything behind it
// takes the row for 250 kHz -- ten samples per symbol, frequencies and times in units of it.  This stage makes that true:
// a rational polyphase filter at L / M = decim 250000 / fs in lowest terms (2.4 MHz: 25/24, 10.24 MHz: 1025/1024), L <= 4096.
//
//   output m of a row x[0 .. n) is the band-limited interpolation of x at input time m M / L:
//     q = floor(m M / L),  ph = (m M) mod L                                   (64-bit integers)
//     y[m] = sum_{k < T} taps[ph][k] x[q - T/2 + 1 + k],  x = 0 outside [0, n),  m < floor(n L / M)
//   taps[ph][k] = P[(k - T/2 + 1) L - ph]: P the prototype (host_design.cpp design_resample_taps: a windowed sinc designed in
//   binary64 at rate L f_in, centred on 0, so an impulse at input i is centred at output i L / M -- the stage adds no delay).
//   T = kBrTaps = 20 per phase: flat within 0.01 dB to 50 kHz and 80 dB down from 165 kHz at every ratio (16 taps reach
//   0.013 dB / 79 dB at best; tests/test_burst_resample_host.py holds the table to both).
//
// Arithmetic: per component ONE chain of float32 fused multiply-adds over k = 0 .. T-1, starting from 0.  A result depends
// on the row and the ratio alone -- not on the tile geometry or the lane -- and tests/burst_resample_model.py reproduces it
// bit for bit.
//
// One workgroup per (burst, tile of kBrTile consecutive outputs); a thread per output.  The tile's input span -- at most
// (kBrTile - 1) M / L + 1 + T samples, M / L <= 8/7 -- is staged through LDS once by 16-byte loads (rows start on 128-byte
// lines); a thread's T taps are five 16-byte loads from the phase-major table (at most 4096 x 20 floats = 320 KB: L2), its
// T samples 8-byte LDS reads at a stride of one sample between neighbouring lanes (M / L is near 1: no bank conflicts
// beyond the occasional repeated or skipped sample).  m M = q0 L + r0 is divided once per workgroup in 64 bits; a thread
// adds t M < 2^21 to r0 and divides in 32.
//
// Rows: work[b].dec_off is the row's offset in BOTH scratch buffers (the host spaces the rows for the longer of the two
// lengths), work[b].dec_len the decimated length.  burst_resample_commit_kernel, behind it on the stream, stores the new
// length into work[b].dec_len: the stages from post1 on read BurstWork as they always have.
//
// Launched by chain.cpp (the chain of a chunk) and state.cpp (irdm_burst_resample_batch).
#pragma once
#include <stdint.h>
#include "common.hpp"
#include "types.hpp"

namespace irdm {

constexpr int kBrTaps = 20;                 // taps per phase (a multiple of 4: 16-byte loads)
constexpr int kBrMaxL = 4096;
constexpr int kBrTile = 256;                // outputs per workgroup, one per thread
// staged samples per tile: 255 * 8/7 + 1 + kBrTaps + 1 (rounding the start down to a 16-byte pair) = 314 at most
constexpr int kBrSpan = 320;
static_assert(kBrTaps % 4 == 0 && kBrSpan % 2 == 0 && (kBrTile - 1) * 8 / 7 + 1 + kBrTaps + 2 <= kBrSpan,
              "a tile's input span fits the LDS stage");

// a ratio the kernel takes: lowest terms are the caller's business, 7/8 <= L / M <= 8/7, L <= kBrMaxL
static inline bool burst_resample_ratio_ok(long long L, long long M)
{
    return L >= 1 && M >= 1 && L <= kBrMaxL && 7 * M <= 8 * L && 7 * L <= 8 * M;
}

__host__ __device__ __forceinline__ int burst_resample_len(int n, int L, int M)
{
    return (int)((long long)n * L / M);
}

// (templates, as symbol_clock_kernel is: every translation unit of the host side sees this header, two instantiate them)
template <int T>
__global__ __launch_bounds__(kBrTile) void burst_resample_kernel(const BurstWork *__restrict__ work, const float2 *__restrict__ dec,
                                                                 float2 *__restrict__ res, const float *__restrict__ taps, int L, int M)
{
    static_assert(T == kBrTaps, "one instance");
    __shared__ float2 sh_x[kBrSpan];
    const BurstWork &w = work[blockIdx.y];
    const int n_in = w.dec_len;
    if (w.drop_reason != 0 || n_in <= 0) return;                                 // (the whole workgroup)
    const int n_out = burst_resample_len(n_in, L, M);
    const int m0 = (int)blockIdx.x * kBrTile;
    if (m0 >= n_out) return;                                                     // (the whole workgroup)
    const int tid = threadIdx.x;
    const long long t0 = (long long)m0 * M;
    const int q0 = (int)(t0 / L), r0 = (int)(t0 % L);
    // the stage holds inputs [lo, lo + kBrSpan): lo the first tap of the tile's first output, rounded down to an even index
    const int lo = (q0 - kBrTaps / 2 + 1) & ~1;
    const float2 *x = dec + (size_t)w.dec_off;
    if (tid < kBrSpan / 2) {
        const int i = lo + 2 * tid;
        float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (i >= 0 && i + 1 < n_in) {
            v = *reinterpret_cast<const float4 *>(x + i);
        } else {
            if (i >= 0 && i < n_in) { const float2 a = x[i]; v.x = a.x; v.y = a.y; }
            if (i + 1 >= 0 && i + 1 < n_in) { const float2 a = x[i + 1]; v.z = a.x; v.w = a.y; }
        }
        *reinterpret_cast<float4 *>(&sh_x[2 * tid]) = v;
    }
    __syncthreads();
    const int m = m0 + tid;
    if (m >= n_out) return;
    const unsigned u = (unsigned)r0 + (unsigned)tid * (unsigned)M;
    const int q = q0 + (int)(u / (unsigned)L), ph = (int)(u % (unsigned)L);
    float h[kBrTaps];
    const float4 *tp = reinterpret_cast<const float4 *>(taps + (size_t)ph * kBrTaps);
#pragma unroll
    for (int k = 0; k < kBrTaps / 4; k++) {
        const float4 t = tp[k];
        h[4 * k] = t.x; h[4 * k + 1] = t.y; h[4 * k + 2] = t.z; h[4 * k + 3] = t.w;
    }
    const float2 *s = sh_x + (q - kBrTaps / 2 + 1 - lo);
    float ar = 0.0f, ai = 0.0f;
#pragma unroll
    for (int k = 0; k < kBrTaps; k++) {
        const float2 v = s[k];
        ar = fmaf(h[k], v.x, ar);
        ai = fmaf(h[k], v.y, ai);
    }
    res[(size_t)w.dec_off + m] = make_float2(ar, ai);
}

// behind burst_resample_kernel on the stream: the rows' new lengths, where every later stage reads them
template <int T>
__global__ __launch_bounds__(256) void burst_resample_commit_kernel(BurstWork *__restrict__ work, int n_bursts, int L, int M)
{
    const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (i >= n_bursts) return;
    if (work[i].drop_reason == 0 && work[i].dec_len > 0) work[i].dec_len = burst_resample_len(work[i].dec_len, L, M);
}

// n_bursts rows of `dec` (work[b].dec_off / .dec_len; the longest max_dec_len) into the same offsets of `res` at L / M, and
// the new lengths into work[b].dec_len, on `stream`.  taps: the phase-major table of the ratio on the device.
static inline int launch_burst_resample(BurstWork *d_work, int n_bursts, int max_dec_len, const float2 *dec, float2 *res,
                                        const float *d_taps, int L, int M, hipStream_t stream)
{
    if (n_bursts <= 0 || max_dec_len <= 0) return 0;
    if (!burst_resample_ratio_ok(L, M) || !d_taps) return -1;
    const int max_out = burst_resample_len(max_dec_len, L, M);
    if (max_out > 0) {
        const dim3 grid((unsigned)((max_out + kBrTile - 1) / kBrTile), (unsigned)n_bursts);
        hipLaunchKernelGGL((burst_resample_kernel<kBrTaps>), grid, dim3(kBrTile), 0, stream, d_work, dec, res, d_taps, L, M);
    }
    hipLaunchKernelGGL((burst_resample_commit_kernel<kBrTaps>), dim3((unsigned)((n_bursts + 255) / 256)), dim3(256), 0, stream, d_work,
                       n_bursts, L, M);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace irdm
