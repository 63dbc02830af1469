// frontend.hip -- K0, the band-select front end: frequency shift + real low-pass + integer decimation of a wideband capture,
// in front of K1 (no reference counterpart: the reference is given a stream at the detector's rate).
//
//   y[m] = sum_k h[k] * r[m D + c - k],   r[n] = x[n] * T[(q n) mod 65536],   c = (ntaps - 1) / 2,   r[n] = 0 outside the stream
//
// Arithmetic contract (restated in plain C in tests/frontend_model.c):
//   x[n]   the sample converted exactly as load_iq converts it (common.hpp)
//   r[n]   = cmul(x[n], T[i]), i = (q n) mod 65536 from the 64-bit stream position: four rounded products, one rounded
//            difference, one rounded sum (common.hpp cmul).  Outside the stream r[n] is +0 + 0i, not a product.
//   y[m]   per component ONE accumulator, starting at +0, and ntaps fused multiply-adds in ASCENDING INPUT ORDER:
//            acc = fmaf(h[ntaps - 1 - j], r[m D - c + j], acc),  j = 0 .. ntaps - 1
//
// Shape.  A workgroup of NT lanes makes a tile of NT * 8 consecutive outputs.  Its (NT * 8 - 1) D + ntaps input samples are
// converted and rotated ONCE, by the load stage, into LDS (8 bytes per sample; every sample feeds ntaps / D ~ 44 outputs).
// A lane then owns 8 CONSECUTIVE outputs: an input sample read from LDS (one ds_read_b64) goes into up to 8 accumulator
// pairs (8 v_pk_fma_f32), so the tap loop is on the VALU side of the LDS port (128 B/clk per CU = one 64-lane ds_read_b64 in
// 4 clocks, the time of four packed FMAs on the four SIMDs).  Lane l's window starts 8 D samples behind lane l - 1's; a row
// of 8 D samples is followed by one pad sample so that the lane stride (8 D + 1) is odd and the 64 reads of an instruction
// fall into different banks.  In step i every lane multiplies by the SAME taps h'[i - r D], r = 0 .. 7: wavefront-uniform,
// read as one aligned 8-dword scalar load per step from a table the host lays out (G[i][r]); the (8 - 1) D steps at either
// end, where only some of the 8 outputs take part, are unrolled with their taps from the plain reversed array.
// Finished outputs go through LDS once more so that the global stores are consecutive 8-byte stores per lane.
//
// Bounds: every global read of the capture is the load stage's (fe_stage.hpp: zero for a position outside
// [tail | chunk]); every global write is guarded by m < m1.  LDS: (cnt + cnt / (8 D) + 1) samples, the host computes the
// same expression.
#include "common.hpp"
#include "types.hpp"
#include "kernels.hpp"
#include "fe_stage.hpp"

namespace irdm {

constexpr int kFeR = 8;               // outputs per lane

int frontend_threads(int D)
{
    // NT * 8 * D <= 8192 staged samples (64 KB) per tile
    return D <= 4 ? 256 : (D <= 8 ? 128 : 64);
}

// staged samples of a tile and their LDS footprint in samples (rows of 8 D + one pad each)
static inline long long fe_tile_samples(int D, int nt, int ntaps) { return (long long)(nt * kFeR - 1) * D + ntaps; }
size_t frontend_lds_bytes(int D, int ntaps)
{
    const long long cnt = fe_tile_samples(D, frontend_threads(D), ntaps);
    return (size_t)(cnt + cnt / (kFeR * D) + 1) * sizeof(float2);
}

// the pad samples in front of staged sample g: one behind every row of RD staged samples
template <int RD>
struct fe_pad {
    __device__ __forceinline__ int operator()(int g) const { return g / RD; }
};

template <int D, int NT>
__global__ __launch_bounds__(NT) void frontend_kernel(FrontendArgs a, const float *__restrict__ hr, const float *__restrict__ G,
                                                      const float2 *__restrict__ T, unsigned long long *__restrict__ kclk)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char fe_lds[];
    constexpr int R = kFeR, RD = R * D, TO = NT * R;
    fe_v2 *s = reinterpret_cast<fe_v2 *>(fe_lds);
    const int tid = threadIdx.x;
    const int ntaps = a.ntaps;
    kclk_enter(kclk);
    const long long mt = a.m0 + (long long)blockIdx.x * TO;              // the tile's first output
    const long long n_start = mt * D - (ntaps - 1) / 2;                 // ... and its first input sample
    const int cnt = (TO - 1) * D + ntaps;

    // ---- load stage: convert, rotate, into LDS ----
    fe_stage<NT>(a, n_start, cnt, T, s, tid, fe_pad<RD>{});
    __syncthreads();

    // ---- the taps: lane `tid` owns outputs mt + R tid + r; in step i it reads its sample i (input (mt + R tid) D - c + i) ----
    const fe_v2 *w = s + tid * (RD + 1);
    fe_v2 acc[R];
#pragma unroll
    for (int r = 0; r < R; r++) acc[r] = fe_v2{ 0.0f, 0.0f };
    // steps 0 .. (R - 1) D - 1: output r joins at step r D
#pragma unroll
    for (int b = 0; b < R - 1; b++) {
#pragma unroll
        for (int p = 0; p < D; p++) {
            const int i = b * D + p;
            const fe_v2 x = w[i + i / RD];
#pragma unroll
            for (int r = 0; r <= b; r++) acc[r] = fe_fma(hr[i - r * D], x, acc[r]);
        }
    }
    // steps (R - 1) D .. ntaps - 1: all R outputs, taps G[i - (R - 1) D][r] = hr[i - r D]
    // in blocks of U steps, the next block's taps (scalar loads) and samples (LDS reads) requested before the current
    // block's multiply-adds: neither latency is waited for while there is arithmetic to issue
    {
        constexpr int U = 4;
        const float *g = G;
        int i = (R - 1) * D;
        float tc[U * R];
        fe_v2 xc[U];
        auto fetch = [&](float (&t)[U * R], fe_v2 (&x)[U], const float *gp, int at) {
#pragma unroll
            for (int k = 0; k < U * R; k++) t[k] = gp[k];
#pragma unroll
            for (int u = 0; u < U; u++) x[u] = w[at + u + (at + u) / RD];
        };
        if (i + U <= ntaps) fetch(tc, xc, g, i);
#pragma unroll 1
        for (; i + U <= ntaps; i += U, g += U * R) {
            float tn[U * R];
            fe_v2 xn[U];
            const bool more = i + 2 * U <= ntaps;
            // (the last block fetches itself again: in bounds, unused)
            fetch(tn, xn, more ? g + U * R : g, more ? i + U : i);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int u = 0; u < U; u++)
#pragma unroll
                for (int r = 0; r < R; r++) acc[r] = fe_fma(tc[u * R + r], xc[u], acc[r]);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int k = 0; k < U * R; k++) tc[k] = tn[k];
#pragma unroll
            for (int u = 0; u < U; u++) xc[u] = xn[u];
        }
#pragma unroll 1
        for (; i < ntaps; i++, g += R) {
            const fe_v2 x = w[i + i / RD];
#pragma unroll
            for (int r = 0; r < R; r++) acc[r] = fe_fma(g[r], x, acc[r]);
        }
    }
    // steps ntaps .. ntaps + (R - 1) D - 1: output r has left after step r D + ntaps - 1
#pragma unroll
    for (int b = 0; b < R - 1; b++) {
#pragma unroll
        for (int p = 0; p < D; p++) {
            const int e = b * D + p, i = ntaps + e;
            const fe_v2 x = w[i + i / RD];
#pragma unroll
            for (int r = b + 1; r < R; r++) acc[r] = fe_fma(hr[i - r * D], x, acc[r]);
        }
    }
    __syncthreads();

    // ---- outputs through LDS (rows of R + 1), then consecutive stores ----
#pragma unroll
    for (int r = 0; r < R; r++) s[tid * (R + 1) + r] = acc[r];
    __syncthreads();
    for (int o = tid; o < TO; o += NT) {
        const long long m = mt + o;
        if (m < a.m1) {
            const fe_v2 y = s[(o / R) * (R + 1) + (o % R)];
            a.out[m - a.m0] = make_float2(y.x, y.y);
        }
    }
    kclk_leave(kclk);
}

template <int D>
static int launch_frontend_d(const FrontendArgs &a, const float *hr, const float *G, const float2 *T, hipStream_t stream,
                             unsigned long long *kclk)
{
    constexpr int NT = D <= 4 ? 256 : (D <= 8 ? 128 : 64);
    const long long n_out = a.m1 - a.m0;
    const long long tiles = (n_out + NT * kFeR - 1) / (NT * kFeR);
    if (tiles <= 0) return 0;
    if (tiles > 0x7fffffffll) return -1;
    const size_t lds = frontend_lds_bytes(D, a.ntaps);
    if (lds > 160 * 1024) return -1;
    if (hipFuncSetAttribute(reinterpret_cast<const void *>(&frontend_kernel<D, NT>), hipFuncAttributeMaxDynamicSharedMemorySize,
                            (int)lds) != hipSuccess)
        return -1;
    hipLaunchKernelGGL((frontend_kernel<D, NT>), dim3((unsigned)tiles), dim3(NT), lds, stream, a, hr, G, T, kclk);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

// outputs [a.m0, a.m1) of the front end into a.out; hr: the taps reversed (ntaps), G: the table of the full steps
// ((ntaps - 7 D) rows of 8), T: the 65536-entry rotation table
int launch_frontend(int D, const FrontendArgs &a, const float *hr, const float *G, const float2 *T, hipStream_t stream,
                    unsigned long long *kclk)
{
    if (a.ntaps < (kFeR - 1) * D + 1 || !fmt_valid(a.fmt) || a.m1 < a.m0 || a.pos0 < 0) return -1;
    switch (D) {
#define FE_CASE(d) case d: return launch_frontend_d<d>(a, hr, G, T, stream, kclk);
    FE_CASE(2) FE_CASE(3) FE_CASE(4) FE_CASE(5) FE_CASE(6) FE_CASE(7) FE_CASE(8) FE_CASE(9) FE_CASE(10) FE_CASE(11)
    FE_CASE(12) FE_CASE(13) FE_CASE(14) FE_CASE(15) FE_CASE(16)
#undef FE_CASE
    default: return -1;
    }
}

// The samples a later output still needs: new_tail[i] = [tail | chunk][from + i], raw bytes (bps per sample).
__global__ __launch_bounds__(256) void frontend_tail_kernel(const unsigned char *__restrict__ tail, long long n_tail,
                                                            const unsigned char *__restrict__ in, long long n_in, long long from,
                                                            int n_new, int bps, unsigned char *__restrict__ out)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n_new) return;
    const long long v = from + i;
    if (v < 0 || v >= n_tail + n_in) return;
    const unsigned char *src = v < n_tail ? tail + (size_t)v * bps : in + (size_t)(v - n_tail) * bps;
    for (int b = 0; b < bps; b++) out[(size_t)i * bps + b] = src[b];
}

int launch_frontend_tail(const void *tail, long long n_tail, const void *in, long long n_in, long long from, int n_new, int bps,
                         void *out, hipStream_t stream)
{
    if (n_new <= 0) return 0;
    hipLaunchKernelGGL(frontend_tail_kernel, dim3((unsigned)((n_new + 255) / 256)), dim3(256), 0, stream,
                       static_cast<const unsigned char *>(tail), n_tail, static_cast<const unsigned char *>(in), n_in, from, n_new,
                       bps, static_cast<unsigned char *>(out));
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

// ---- the requantiser: the cf32 band as a ci8 / ci16 recording (irdm_frontend_save, irdm_requantize_device) ----
//
// Arithmetic contract, per float component x, k = (float)gain * S (S = 128 / 32768) formed once by the host:
//   v = rintf(x * k)       one rounded product, rounded to nearest, ties to even
//   q = clamp(v, -S, S - 1);  NaN -> 0;  +-Inf -> the rail of its sign
// Statistics (three 64-bit words at `stats`, added to): [0] components, [1] clipped components (v outside [-S, S - 1], or
// NaN), [2] the largest bit pattern of |x * k| over the components with x finite (a non-negative float's pattern orders as
// the float does).  All three are independent of the order in which the workgroups arrive.
//
// Shape.  Memory-bound: 8 bytes in, 2 or 4 bytes out per sample.  A lane takes kRqV = 4 consecutive samples per step: two
// 16-byte loads (four 8-byte ones when the input is only 8-byte aligned) and one 8- or 16-byte store; the lanes of a
// wavefront are consecutive, the grid strides.  A piece may start at any sample: the `head` samples in front of the first
// output address that is aligned for the wide store, and the fewer than kRqV behind the last whole step, are done one per
// lane by workgroup 0.  The statistics are reduced per wavefront (shuffles), then per workgroup (LDS); lane 0 of the
// workgroup issues one atomic per statistic.
// Bounds: every index is below n (head <= n; quads * kRqV <= n - head); the launcher refuses a misaligned pointer.
constexpr int kRqThreads = 256, kRqV = 4, kRqMaxBlocks = 2048;

struct RqAcc { unsigned comps, clipped, peak; };

template <int S>
__device__ __forceinline__ int rq_one(float x, float k, RqAcc &a)
{
    const float p = x * k;
    const float v = rintf(p);
    if ((__float_as_uint(x) & 0x7fffffffu) < 0x7f800000u) a.peak = max(a.peak, __float_as_uint(p) & 0x7fffffffu);
    a.comps++;
    if (!(v >= (float)-S && v <= (float)(S - 1))) a.clipped++;            // (a NaN compares false: counted)
    if (v != v) return 0;
    return (int)fminf(fmaxf(v, (float)-S), (float)(S - 1));
}

template <int S, typename Q>
__global__ __launch_bounds__(kRqThreads) void requant_kernel(const float2 *__restrict__ in, long long n, int head, int in16,
                                                             float k, Q *__restrict__ out, unsigned long long *__restrict__ stats)
{
    __shared__ unsigned red[3 * (kRqThreads / 64)];
    RqAcc a{ 0u, 0u, 0u };
    const int tid = threadIdx.x;
    const long long quads = (n - head) / kRqV;
    const float2 *bin = in + head;
    Q *bout = out + 2 * head;
    for (long long g = (long long)blockIdx.x * kRqThreads + tid; g < quads; g += (long long)gridDim.x * kRqThreads) {
        float c[2 * kRqV];
        if (in16) {
            const float4 *p = reinterpret_cast<const float4 *>(bin + g * kRqV);
            const float4 u0 = p[0], u1 = p[1];
            c[0] = u0.x; c[1] = u0.y; c[2] = u0.z; c[3] = u0.w;
            c[4] = u1.x; c[5] = u1.y; c[6] = u1.z; c[7] = u1.w;
        } else {
            const float2 *p = bin + g * kRqV;
#pragma unroll
            for (int j = 0; j < kRqV; j++) {
                const float2 u = p[j];
                c[2 * j] = u.x;
                c[2 * j + 1] = u.y;
            }
        }
        unsigned q[2 * kRqV];
#pragma unroll
        for (int j = 0; j < 2 * kRqV; j++) q[j] = (unsigned)rq_one<S>(c[j], k, a);
        if constexpr (sizeof(Q) == 1) {
            uint2 w;
            w.x = (q[0] & 0xffu) | (q[1] & 0xffu) << 8 | (q[2] & 0xffu) << 16 | q[3] << 24;
            w.y = (q[4] & 0xffu) | (q[5] & 0xffu) << 8 | (q[6] & 0xffu) << 16 | q[7] << 24;
            *reinterpret_cast<uint2 *>(bout + g * (2 * kRqV)) = w;
        } else {
            *reinterpret_cast<uint4 *>(bout + g * (2 * kRqV)) =
                make_uint4((q[0] & 0xffffu) | q[1] << 16, (q[2] & 0xffffu) | q[3] << 16, (q[4] & 0xffffu) | q[5] << 16,
                           (q[6] & 0xffffu) | q[7] << 16);
        }
    }
    if (blockIdx.x == 0) {
        // the scalar head and tail: at most kRqV - 1 samples each
        const long long tail0 = head + quads * kRqV;
        const long long i = tid < head ? tid : (tail0 + (tid - head) < n ? tail0 + (tid - head) : -1);
        if (i >= 0) {
            const float2 x = in[i];
            out[2 * i] = (Q)rq_one<S>(x.x, k, a);
            out[2 * i + 1] = (Q)rq_one<S>(x.y, k, a);
        }
    }
    // the statistics: wavefront, workgroup, one atomic each
#pragma unroll
    for (int d = 32; d; d >>= 1) {
        a.comps += __shfl_xor(a.comps, d);
        a.clipped += __shfl_xor(a.clipped, d);
        a.peak = max(a.peak, __shfl_xor(a.peak, d));
    }
    if ((tid & 63) == 0) {
        red[3 * (tid >> 6)] = a.comps;
        red[3 * (tid >> 6) + 1] = a.clipped;
        red[3 * (tid >> 6) + 2] = a.peak;
    }
    __syncthreads();
    if (tid == 0) {
        unsigned long long comps = 0, clipped = 0, peak = 0;
        for (int w = 0; w < kRqThreads / 64; w++) {
            comps += red[3 * w];
            clipped += red[3 * w + 1];
            if (red[3 * w + 2] > peak) peak = red[3 * w + 2];
        }
        if (comps) atomicAdd(&stats[0], comps);
        if (clipped) atomicAdd(&stats[1], clipped);
        if (peak) atomicMax(&stats[2], peak);
    }
}

template <int S, typename Q>
static int launch_requant_q(const float2 *in, long long n, float k, Q *out, unsigned long long *stats, hipStream_t stream)
{
    // the samples in front of the first output address aligned for a lane's store of kRqV samples
    const uintptr_t A = (uintptr_t)(2 * kRqV) * sizeof(Q), sample = 2 * sizeof(Q);
    const uintptr_t o = reinterpret_cast<uintptr_t>(out);
    if (o % sample != 0 || reinterpret_cast<uintptr_t>(in) % sizeof(float2) != 0) return -1;
    const int head = (int)std::min<long long>((long long)(((A - o % A) % A) / sample), n);
    const long long quads = (n - head) / kRqV;
    const int in16 = reinterpret_cast<uintptr_t>(in + head) % 16 == 0 ? 1 : 0;
    const long long blocks = std::max<long long>(1, std::min<long long>((quads + kRqThreads - 1) / kRqThreads, kRqMaxBlocks));
    hipLaunchKernelGGL((requant_kernel<S, Q>), dim3((unsigned)blocks), dim3(kRqThreads), 0, stream, in, n, head, in16, k, out, stats);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

// n cf32 samples at `in` (8-byte aligned) -> interleaved int8 (bits 8; out 2-byte aligned) or int16 (bits 16; 4-byte aligned)
// pairs at `out`, k = (float)gain * S; the statistics are added to stats[0 .. 3).  n = 0 launches nothing.
int launch_requant(int bits, const void *in, long long n, float k, void *out, unsigned long long *stats, hipStream_t stream)
{
    if (n < 0 || (bits != 8 && bits != 16) || !(k > 0.0f) || k > 3.0e38f) return -1;
    if (n == 0) return 0;
    if (!in || !out || !stats) return -1;
    if (bits == 8) return launch_requant_q<128>(static_cast<const float2 *>(in), n, k, static_cast<signed char *>(out), stats, stream);
    return launch_requant_q<32768>(static_cast<const float2 *>(in), n, k, static_cast<short *>(out), stats, stream);
}

}  // namespace irdm
