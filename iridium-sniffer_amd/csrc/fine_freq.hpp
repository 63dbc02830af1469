// fine_freq.hpp -- option "fine_freq" (irdm_fine_freq_t / irdm_fine_freq_summary_t, include/irdm_hip.h): the carrier
// frequency of every downmixed frame, estimated on the device from the samples the demodulator is handed.
//
// The fourth power of a QPSK frame carries a spectral line at four times the frame's residual carrier offset.  The kernel
// looks for it on a fixed grid (tests/fine_freq_model.py states the same in numpy); f_o is the context's out_rate:
//   y[n] = x[n]^4:  a = re re - im im,  b = 2 re im,  y = (a a - b b) + i 2 a b
//   P(g) = |sum_n y[n] exp(-2 pi i g n / f_o)|^2
//   coarse: g_k = -1000 + 20 k Hz, k = 0 .. 100; k_c the first maximum; quality = P(g_kc) / mean_k P(g_k)
//   fine:   h_j = g_kc + 4 (j - 5), j = 0 .. 10; j* the first maximum; inside, the three-point parabola refines it
//   df = g* / 4
// Only a line within its main lobe of an edge shows there, so P is also taken at kFfGuard points of the coarse step beyond
// either edge (+-1020 .. +-1200 Hz): where one of them exceeds P(g_kc), or k_c is at an edge, the record is out of range
// and df is the edge of that side, +-250 Hz.  The guard points enter nothing else.  A frame more than +-300 Hz from the
// downmixer's value has its line beyond the guard points: the grid then shows the frame's modulation, and the check is blind.
// A linear drift over the frame leaves the line's centre at the frequency of the frame's middle.
//
// One workgroup per frame, 1024 threads, y staged once in LDS as doubles (71 KB of dynamic LDS beside 17 KB of partial sums:
// one workgroup of sixteen wavefronts to a CU).
//   coarse: thread (s, j), j < 121 of 128 lanes, sums point j over the s-th eighth of the frame; the eighths are added in
//           their order.  Every lane of a wavefront reads the same y[n] (a broadcast).
//   fine:   in the same launch, once thread 0 has found k_c: thread (s, j), j < 11 of 16 lanes, sums point j over the s-th
//           of 64 segments; the segments are added in their order.
// The sum over a segment is Goertzel's second-order recurrence on the real and the imaginary part of y (four binary64
// operations per sample and point), closed by exp(-i w) and turned by exp(-i w m) as symbol_clock_kernel does; the two
// phases come from g / f_o and from the FRACTION of g m / f_o through sc_sincos_turns (the polynomials of libm_port.hpp
// kept in double).  w is at most 0.03 rad, where the recurrence loses a factor 1 / sin w: over the 555 samples of an eighth
// its rounding error stays near 1e-11 of the sum, and a wrong tenth of a fine step on a 64-sample frame would take 2e-8.
// All arithmetic is binary64 with separately rounded products and sums, in an order fixed by the frame's length alone: a
// frame's record depends on its samples only, and the CPU emulation computes the same bits.  No scratch memory.
// Cost: 4 binary64 operations per sample and point on 132 points, where symbol_clock_kernel takes 2 on 221.
//
// Launched by chain.cpp (the chain of a chunk) and state.cpp (irdm_fine_freq_batch); the host side below it is the
// summary of a stream (pipeline.hpp: StreamState::fine).
#pragma once
#include <float.h>
#include <math.h>
#include <string.h>
#include <deque>
#include <vector>
#include "common.hpp"
#include "types.hpp"
#include "symbol_clock.hpp"
#include "../../include/irdm_hip.h"

namespace irdm {

constexpr int kFfCoarse = 101;                          // coarse grid points
constexpr int kFfGuard = 10;                            // points beyond either edge, for the out-of-range flag only
constexpr int kFfPoints = kFfCoarse + 2 * kFfGuard;     // point j is k = j - kFfGuard
constexpr int kFfLanes = 128;                           // threads of a coarse segment: two wavefronts, 7 lanes idle
constexpr int kFfSeg = 8;                               // coarse segments a frame is cut into
constexpr int kFfNT = kFfLanes * kFfSeg;                // threads of a workgroup
constexpr int kFfFine = 11;                             // fine grid points
constexpr int kFfFineLanes = 16;                        // threads of a fine segment
constexpr int kFfFineSeg = kFfNT / kFfFineLanes;        // fine segments
constexpr int kFfMinSamples = 64;
constexpr double kFfG0 = -1000.0, kFfStep = 20.0, kFfFineStep = 4.0, kFfEdge = 250.0;
constexpr size_t kFfLdsBytes = sizeof(double) * 2 * (size_t)kMaxFrameSamples;
// the summary's histogram of refined - PLL: 1 Hz bins over +-500 Hz
constexpr int kFfBins = 1001;
constexpr double kFfBin0 = -500.0;

// the kernel's record (the public one without the burst id and the absolute frequency)
struct FineRec {
    float df, quality;
    uint32_t flags, n;
};

// sum_{n in [n0, n1)} y[n] exp(-2 pi i f n), f in cycles per sample, |f| < 1/2, y as (re, im) pairs of doubles
__device__ __forceinline__ void ff_segment_sum(const double *y, int n0, int n1, double f, double *re_out, double *im_out)
{
    double es, ec;
    sc_sincos_turns(f, &es, &ec);                                                // exp(i w), w = 2 pi f
    const double c2 = 2.0 * ec;
    double r1 = 0.0, r2 = 0.0, i1 = 0.0, i2 = 0.0;
    // (four samples read ahead of the dependent steps that use them, as symbol_clock_kernel reads eight)
    int n = n0;
    for (; n + 4 <= n1; n += 4) {
        double v[8];
#pragma unroll
        for (int i = 0; i < 8; i++) v[i] = y[2 * n + i];
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const double r0 = __fma_rn(c2, r1, v[2 * i] - r2);
            const double i0 = __fma_rn(c2, i1, v[2 * i + 1] - i2);
            r2 = r1;
            r1 = r0;
            i2 = i1;
            i1 = i0;
        }
    }
    for (; n < n1; n++) {
        const double r0 = __fma_rn(c2, r1, y[2 * n] - r2);
        const double i0 = __fma_rn(c2, i1, y[2 * n + 1] - i2);
        r2 = r1;
        r1 = r0;
        i2 = i1;
        i1 = i0;
    }
    // behind the last sample m: s[m] - exp(-i w) s[m-1] = sum_n p[n] exp(i w (m - n)) for the real sequence p; y = p + i q
    const double pr = r1 - ec * r2, pi = es * r2;
    const double qr = i1 - ec * i2, qi = es * i2;
    const double yr = pr - qi, yi = pi + qr;
    const double t = f * (double)(n1 - 1);
    double zs, zc;
    sc_sincos_turns(t - rint(t), &zs, &zc);                                      // exp(i w m), the phase from the fraction of f m
    *re_out = yr * zc + yi * zs;
    *im_out = yi * zc - yr * zs;
}

// frames: n_frames rows of kMaxFrameSamples float2; work[i].num_samples / .drop_reason say what row i holds
// (a template, as symbol_clock_kernel is: every translation unit of the host side sees this header, two instantiate it)
template <int SEG>
__global__ __launch_bounds__(kFfNT) void fine_freq_kernel(const BurstWork *__restrict__ work, const float2 *__restrict__ frames,
                                                          double out_rate, FineRec *__restrict__ out)
{
#if defined(IRDM_HIP_EMULATED)
    unsigned char *ff_lds = hip_emul::dyn_lds();
#else
    extern __shared__ __attribute__((aligned(16))) unsigned char ff_lds[];
#endif
    static_assert(SEG * kFfLanes == kFfNT && kFfNT <= 1024 && kFfPoints <= kFfLanes, "a workgroup is SEG segments of kFfLanes threads");
    static_assert(kFfFineSeg * kFfFineLanes == kFfNT && kFfFine <= kFfFineLanes, "and kFfFineSeg segments of kFfFineLanes");
    double *sh_y = reinterpret_cast<double *>(ff_lds);                           // y[n] = (sh_y[2 n], sh_y[2 n + 1])
    __shared__ double sh_part[2][kFfNT];                                         // [re / im][segment][lane], both stages
    __shared__ double sh_P[kFfPoints];
    __shared__ double sh_Pf[kFfFineLanes];
    __shared__ int sh_bad, sh_kc;
    const int tid = threadIdx.x;
    const BurstWork &w = work[blockIdx.x];
    const int N = w.num_samples;
    if (w.drop_reason != 0 || N < kFfMinSamples || N > kMaxFrameSamples) {      // (the whole workgroup)
        if (tid == 0) out[blockIdx.x] = FineRec{ 0.0f, 0.0f, IRDM_FINE_FREQ_INVALID, w.drop_reason != 0 || N < 0 ? 0u : (uint32_t)N };
        return;
    }
    const float2 *x = frames + (size_t)blockIdx.x * kMaxFrameSamples;
    if (tid == 0) sh_bad = 0;
    __syncthreads();
    FineRec r = { 0.0f, 0.0f, IRDM_FINE_FREQ_INVALID, (uint32_t)N };               // (thread 0's)
    bool bad = false;
    for (int n = tid; n < N; n += kFfNT) {
        const float2 v = x[n];
        bad = bad || !(fabsf(v.x) <= FLT_MAX) || !(fabsf(v.y) <= FLT_MAX);
        const double re = (double)v.x, im = (double)v.y;
        const double a = re * re - im * im, b = 2.0 * (re * im);
        sh_y[2 * n] = a * a - b * b;
        sh_y[2 * n + 1] = 2.0 * (a * b);
    }
    if (bad) sh_bad = 1;
    __syncthreads();
    if (sh_bad) {                                                                // (the whole workgroup: a sample that is not finite)
        if (tid == 0) out[blockIdx.x] = FineRec{ 0.0f, 0.0f, IRDM_FINE_FREQ_INVALID, (uint32_t)N };
        return;
    }
    // coarse stage: thread (seg, j), point j over samples [seg L, (seg + 1) L)
    {
        const int j = tid % kFfLanes, seg = tid / kFfLanes;
        const int L = (N + SEG - 1) / SEG;
        const int n0 = seg * L, n1 = (seg + 1) * L < N ? (seg + 1) * L : N;
        double ar = 0.0, ai = 0.0;
        if (j < kFfPoints && n0 < n1) ff_segment_sum(sh_y, n0, n1, (kFfG0 + kFfStep * (double)(j - kFfGuard)) / out_rate, &ar, &ai);
        sh_part[0][tid] = ar;
        sh_part[1][tid] = ai;
    }
    __syncthreads();
    if (tid < kFfPoints) {
        double re = sh_part[0][tid], im = sh_part[1][tid];
        for (int g = 1; g < SEG; g++) {
            re += sh_part[0][g * kFfLanes + tid];
            im += sh_part[1][g * kFfLanes + tid];
        }
        sh_P[tid] = re * re + im * im;
    }
    __syncthreads();
    const double *P = sh_P + kFfGuard;                                           // P[k], k = -kFfGuard .. 100 + kFfGuard
    if (tid == 0) {
        int kc = 0;
        double pmax = P[0], psum = 0.0;
#pragma unroll 16
        for (int i = 0; i < kFfCoarse; i++) {                                    // (unrolled: sixteen reads in flight, not one)
            const double v = P[i];
            psum += v;
            if (v > pmax) {
                pmax = v;
                kc = i;
            }
        }
        int go = -1;                                                             // the fine stage's centre, or none
        if (pmax > 0.0 && psum <= 1.0e300) {                                     // (neither holds for a NaN)
            double lo = 0.0, hi = 0.0;                                           // the largest beyond either edge
#pragma unroll
            for (int i = 1; i <= kFfGuard; i++) {
                lo = fmax(lo, P[-i]);
                hi = fmax(hi, P[kFfCoarse - 1 + i]);
            }
            r.quality = (float)(pmax / (psum / (double)kFfCoarse));
            if (fmax(lo, hi) > pmax) {
                r.df = (float)(lo >= hi ? -kFfEdge : kFfEdge);
                r.flags = IRDM_FINE_FREQ_OUT_OF_RANGE;
            } else if (kc == 0 || kc == kFfCoarse - 1) {
                r.df = (float)(kc == 0 ? -kFfEdge : kFfEdge);
                r.flags = IRDM_FINE_FREQ_OUT_OF_RANGE;
            } else {
                r.flags = 0;
                go = kc;
            }
        }
        if (go < 0) out[blockIdx.x] = r;                                         // (else the fine stage completes it)
        sh_kc = go;
    }
    __syncthreads();
    const int kc = sh_kc;
    if (kc < 0) return;                                                          // (the whole workgroup)
    // fine stage: thread (seg, j), point j over samples [seg L, (seg + 1) L)
    {
        const int j = tid % kFfFineLanes, seg = tid / kFfFineLanes;
        const int L = (N + kFfFineSeg - 1) / kFfFineSeg;
        const int n0 = seg * L, n1 = (seg + 1) * L < N ? (seg + 1) * L : N;
        double ar = 0.0, ai = 0.0;
        if (j < kFfFine && n0 < n1)
            ff_segment_sum(sh_y, n0, n1, ((kFfG0 + kFfStep * (double)kc) + kFfFineStep * (double)(j - kFfFine / 2)) / out_rate, &ar, &ai);
        sh_part[0][tid] = ar;
        sh_part[1][tid] = ai;
    }
    __syncthreads();
    if (tid < kFfFine) {
        double re = sh_part[0][tid], im = sh_part[1][tid];
        for (int g = 1; g < kFfFineSeg; g++) {
            re += sh_part[0][g * kFfFineLanes + tid];
            im += sh_part[1][g * kFfFineLanes + tid];
        }
        sh_Pf[tid] = re * re + im * im;
    }
    __syncthreads();
    if (tid != 0) return;
    int js = 0;
    double fmax_ = sh_Pf[0];
#pragma unroll
    for (int i = 1; i < kFfFine; i++) {
        if (sh_Pf[i] > fmax_) {
            fmax_ = sh_Pf[i];
            js = i;
        }
    }
    double g = (kFfG0 + kFfStep * (double)kc) + kFfFineStep * (double)(js - kFfFine / 2);
    if (js > 0 && js < kFfFine - 1) {
        const double a = sh_Pf[js - 1], b = sh_Pf[js], c = sh_Pf[js + 1];
        g += kFfFineStep * (0.5 * (a - c) / (a - 2.0 * b + c));
    }
    r.df = (float)(g / 4.0);
    out[blockIdx.x] = r;
}

// n_frames frames at d_frames (pitch kMaxFrameSamples) with their work records: their records into `out` (device or
// pinned host memory) on `stream`
static inline int launch_fine_freq(const BurstWork *d_work, int n_frames, const float2 *d_frames, double out_rate, FineRec *out,
                                   hipStream_t stream)
{
    if (n_frames <= 0) return 0;
    // (the kernel may be given more than 64 KB of dynamic LDS: once per device)
    static bool raised[64];
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return -1;
    if (!raised[dev]) {
        if (hipFuncSetAttribute(reinterpret_cast<const void *>(&fine_freq_kernel<kFfSeg>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)kFfLdsBytes) != hipSuccess)
            return -1;
        raised[dev] = true;
    }
    hipLaunchKernelGGL((fine_freq_kernel<kFfSeg>), dim3(n_frames), dim3(kFfNT), kFfLdsBytes, stream, d_work, d_frames, out_rate, out);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

// ---- host side: the summary of a stream ----

// Stream state: the per-frame records until they are polled, and the histogram of refined - PLL the summary is read from
// (bin centres: the quartiles do not depend on how the stream was cut)
struct FineFreqStream {
    std::deque<irdm_fine_freq_t> q;
    std::vector<uint64_t> hist;         // kFfBins counts, allocated with the first frame
    uint64_t seen = 0, applied = 0, not_ok = 0, out_of_range = 0, invalid = 0;
};

static inline int fine_freq_bin(double d)
{
    const double k = floor(d - kFfBin0 + 0.5);
    return !(k >= 0.0) ? 0 : (k >= (double)kFfBins ? kFfBins - 1 : (int)k);
}

// One frame that reached the demodulator: its record, the downmixer's frequency of the frame, whether the unique word
// passed, and the frequency the PLL's arithmetic gives a frame that passed.  Returns the centre frequency of the frame's
// demodulator record: the refined one, or the PLL's where the record is flagged.
static inline double fine_freq_fold(FineFreqStream &st, uint64_t id, const FineRec &r, double cfreq, bool ok, double pll)
{
    irdm_fine_freq_t o;
    o.id = id;
    o.freq_hz = cfreq + (double)r.df;
    o.df_hz = r.df;
    o.quality = r.quality;
    o.flags = r.flags | (ok ? 0u : (uint32_t)IRDM_FINE_FREQ_NOT_OK);
    o.n = r.n;
    st.q.push_back(o);
    st.seen++;
    if (!ok) st.not_ok++;
    else if (r.flags & IRDM_FINE_FREQ_INVALID) st.invalid++;
    else if (r.flags & IRDM_FINE_FREQ_OUT_OF_RANGE) st.out_of_range++;
    else {
        if (st.hist.empty()) st.hist.assign((size_t)kFfBins, 0);
        st.hist[(size_t)fine_freq_bin(o.freq_hz - pll)]++;
        st.applied++;
        return o.freq_hz;
    }
    return pll;
}

// the centre of the bin that holds the ceil(q applied)-th smallest difference
static inline double fine_freq_quantile(const FineFreqStream &st, double q)
{
    if (st.applied == 0) return 0.0;
    uint64_t want = (uint64_t)ceil(q * (double)st.applied), run = 0;
    if (want < 1) want = 1;
    for (int k = 0; k < kFfBins; k++) {
        run += st.hist[(size_t)k];
        if (run >= want) return kFfBin0 + (double)k;
    }
    return kFfBin0 + (double)(kFfBins - 1);
}

static inline void fine_freq_result(const FineFreqStream &st, irdm_fine_freq_summary_t *out)
{
    memset(out, 0, sizeof(*out));
    out->frames_seen = st.seen;
    out->frames_applied = st.applied;
    out->frames_not_ok = st.not_ok;
    out->frames_out_of_range = st.out_of_range;
    out->frames_invalid = st.invalid;
    out->median = fine_freq_quantile(st, 0.5);
    out->q25 = fine_freq_quantile(st, 0.25);
    out->q75 = fine_freq_quantile(st, 0.75);
}

}  // namespace irdm
