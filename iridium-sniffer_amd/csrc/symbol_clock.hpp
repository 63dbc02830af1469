// symbol_clock.hpp -- option "symbol_clock" (irdm_clock_est_t / irdm_symbol_clock_t, include/irdm_hip.h): the symbol clock
// error of every downmixed frame, estimated on the device from the samples the demodulator is handed.
//
// |x|^2 of a frame carries a spectral line at the symbol rate.  At a nominal sps samples per symbol and a clock error eps the
// line sits at 1 / (sps (1 + eps)) cycles per sample; the kernel looks for it on the fixed grid eps_k = -0.08 + 0.001 k,
// k = 0 .. 160 (tests/clock_model.py states the same in numpy):
//   p[n] = re^2 + im^2,  p' = p - mean(p),  P[k] = |sum_n p'[n] exp(-2 pi i f_k n)|^2,  f_k = 1 / (sps (1 + eps_k))
//   k* the first maximum; inside the grid the three-point parabola refines it, at an edge the record is flagged out of range;
//   quality = P[k*] / mean_k P[k].
// Only a line within its main lobe (1 / n cycles per sample) of an edge shows there: a line further out leaves the grid
// to the frame's own modulation, whose maximum says nothing (its quality is that of a frame without a line, 2 .. 7 against
// 12 and more).  So P is also taken at kScGuard points of the same step beyond either edge (eps = -11 % .. -8.1 % and
// +8.1 % .. +11 %): where one of them exceeds P[k*] the record is out of range too, with eps the edge of that side.  The
// guard points enter nothing else -- k*, the quality and the eps of a record that is not flagged come from the 161.
//
// One workgroup per frame, kScSeg x 256 threads: thread (s, j) sums point j of the 221 over the s-th quarter of the frame,
// the quarters are added in their order.  p' is staged once in LDS as doubles (35.5 KB of 62 KB); every lane of a wavefront reads the same
// p'[n] (a broadcast).  All arithmetic is binary64 with separately rounded products and sums, in an order fixed by the
// frame's length alone: a frame's record depends on its samples only, and the CPU emulation computes the same bits.  The
// sum over a quarter is Goertzel's second-order recurrence (two binary64 operations per sample and grid point where a
// phasor recurrence takes six with fused multiply-adds, ten without): in binary64 its rounding error over the 1110 samples of
// a quarter at w = 0.57 .. 0.71 rad stays near 1e-13 of the sum, where a tenth of a grid step on a 64-sample frame asks for
// 3e-6.  The two phases a thread needs -- exp(i w) and the quarter's closing exp(-i w m) -- come from f_k and from the
// FRACTION of f_k m through the polynomials of libm_port.hpp kept in double (the reduction to an octant is exact).
// Cost: 2 binary64 operations per sample and grid point -- a chunk of 667 bursts of 2000 samples 0.59 G of them, at four
// cycles a wavefront instruction per SIMD -- on 667 workgroups of sixteen wavefronts, two to a CU (the 32-wavefront limit):
// the launch is bound by the binary64 issue rate of the CUs it occupies, in two rounds of workgroups.
//
// Launched by chain.cpp (the chain of a chunk) and state.cpp (irdm_symbol_clock_batch); the host side below it is the
// summary of a stream (pipeline.hpp: StreamState::clock).
#pragma once
#include <math.h>
#include <string.h>
#include <deque>
#include <vector>
#include "common.hpp"
#include "types.hpp"
#include "libm_port.hpp"
#include "../../include/irdm_hip.h"

namespace irdm {

constexpr int kScFreqs = 161;                           // grid points
constexpr int kScGuard = 30;                            // points beyond either edge of the grid, for the out-of-range flag only
constexpr int kScPoints = kScFreqs + 2 * kScGuard;      // point j is k = j - kScGuard
constexpr int kScLanes = 256;                           // threads of a segment: four wavefronts, 35 lanes idle
constexpr int kScSeg = 4;                               // segments a frame is cut into
constexpr int kScNT = kScLanes * kScSeg;                // threads of a workgroup
constexpr int kScMinSamples = 64;
constexpr double kScEps0 = -0.08, kScStep = 0.001;
// the summary's histogram: 0.01 % bins over +-8 %
constexpr int kScBins = 1601;
constexpr double kScBin = 1e-4;

// the kernel's record (the public one without the burst id)
struct ClockRec {
    float eps, quality;
    uint32_t flags, n;
};

// (sin, cos) of 2 pi t for |t| <= 1/2: t = q / 4 + r with |r| <= 1/8 exactly, the polynomials on 2 pi r, the quadrant by
// exchange and sign
__host__ __device__ __forceinline__ void sc_sincos_turns(double t, double *s_out, double *c_out)
{
    const double q = rint(t * 4.0);
    const double x = (t - q * 0.25) * 6.283185307179586476925;
    double s, c;
    libm_sincosf_poly<false>(x, x * x, 0, &s, &c);
    const int qi = (int)q & 3;
    const double s1 = (qi & 1) ? c : s, c1 = (qi & 1) ? -s : c;
    *s_out = (qi & 2) ? -s1 : s1;
    *c_out = (qi & 2) ? -c1 : c1;
}

__host__ __device__ __forceinline__ double sc_grid_freq(int k, float sps)
{
    return 1.0 / ((double)sps * (1.0 + (kScEps0 + kScStep * (double)k)));
}

// frames: n_frames rows of kMaxFrameSamples float2; work[i].num_samples / .drop_reason say what row i holds
// (a template, as input_stats_kernel is: every translation unit of the host side sees this header, two instantiate it)
template <int SEG>
__global__ __launch_bounds__(kScNT) void symbol_clock_kernel(const BurstWork *__restrict__ work, const float2 *__restrict__ frames,
                                                             float sps, ClockRec *__restrict__ out)
{
    __shared__ double sh_p[kMaxFrameSamples];
    __shared__ double sh_red[kScNT];
    static_assert(SEG * kScLanes == kScNT && kScNT <= 1024, "a workgroup is SEG segments of kScLanes threads");
    __shared__ double sh_part[2][SEG][kScLanes];
    __shared__ double sh_P[kScPoints];
    __shared__ int sh_bad;
    const int tid = threadIdx.x;
    const BurstWork &w = work[blockIdx.x];
    const int N = w.num_samples;
    if (w.drop_reason != 0 || N < kScMinSamples || N > kMaxFrameSamples) {       // (the whole workgroup)
        if (tid == 0) out[blockIdx.x] = ClockRec{ 0.0f, 0.0f, IRDM_CLOCK_INVALID, w.drop_reason != 0 || N < 0 ? 0u : (uint32_t)N };
        return;
    }
    const float2 *x = frames + (size_t)blockIdx.x * kMaxFrameSamples;
    if (tid == 0) sh_bad = 0;
    __syncthreads();
    // p and its mean: a thread's samples in their order, then a tree over the threads
    double s = 0.0;
    bool bad = false;
    for (int n = tid; n < N; n += kScNT) {
        const float2 v = x[n];
        const double p = (double)v.x * (double)v.x + (double)v.y * (double)v.y;
        bad = bad || !(fabs(p) <= 1.0e300);
        sh_p[n] = p;
        s += p;
    }
    if (bad) sh_bad = 1;
    sh_red[tid] = s;
    __syncthreads();
    for (int d = 512; d > 0; d >>= 1) {
        if (tid < d && tid + d < kScNT) sh_red[tid] += sh_red[tid + d];
        __syncthreads();
    }
    if (sh_bad) {                                                                // (the whole workgroup: a sample that is not finite)
        if (tid == 0) out[blockIdx.x] = ClockRec{ 0.0f, 0.0f, IRDM_CLOCK_INVALID, (uint32_t)N };
        return;
    }
    const double mean = sh_red[0] / (double)N;
    for (int n = tid; n < N; n += kScNT) sh_p[n] -= mean;
    __syncthreads();
    // thread (seg, k): grid point k over samples [seg L, (seg + 1) L) by Goertzel's recurrence s[n] = p'[n] + 2 cos(w) s[n-1]
    // - s[n-2] (one subtraction and one fused multiply-add per sample); behind the last sample m of the segment
    // s[m] - exp(-i w) s[m-1] = sum_n p'[n] exp(i w (m - n)), which exp(-i w m) turns into the segment's share of the sum
    const int j = tid % kScLanes, seg = tid / kScLanes;
    const int L = (N + SEG - 1) / SEG;
    const int n_end = (seg + 1) * L < N ? (seg + 1) * L : N;
    double ar = 0.0, ai = 0.0;
    if (j < kScPoints && seg * L < n_end) {
        const double f = sc_grid_freq(j - kScGuard, sps);
        double es, ec;
        sc_sincos_turns(f - rint(f), &es, &ec);                                  // exp(i w), w = 2 pi f
        const double c2 = 2.0 * ec;
        double s1 = 0.0, s2 = 0.0;
        // (eight samples read ahead of the eight dependent steps that use them: a step is two instructions, an LDS read
        // waited for in every step is sixty cycles and more)
        int n = seg * L;
        for (; n + 8 <= n_end; n += 8) {
            double v[8];
#pragma unroll
            for (int i = 0; i < 8; i++) v[i] = sh_p[n + i];
#pragma unroll
            for (int i = 0; i < 8; i++) {
                const double s0 = __fma_rn(c2, s1, v[i] - s2);
                s2 = s1;
                s1 = s0;
            }
        }
        for (; n < n_end; n++) {
            const double s0 = __fma_rn(c2, s1, sh_p[n] - s2);
            s2 = s1;
            s1 = s0;
        }
        const double yr = s1 - ec * s2, yi = es * s2;
        const double t = f * (double)(n_end - 1);
        double zs, zc;
        sc_sincos_turns(t - rint(t), &zs, &zc);                                  // exp(i w m), the phase from the fraction of f m
        ar = yr * zc + yi * zs;
        ai = yi * zc - yr * zs;
    }
    sh_part[0][seg][j] = ar;
    sh_part[1][seg][j] = ai;
    __syncthreads();
    if (tid < kScPoints) {
        double re = sh_part[0][0][tid], im = sh_part[1][0][tid];
        for (int g = 1; g < SEG; g++) {
            re += sh_part[0][g][tid];
            im += sh_part[1][g][tid];
        }
        sh_P[tid] = re * re + im * im;
    }
    __syncthreads();
    if (tid != 0) return;
    const double *P = sh_P + kScGuard;                                           // P[k], k = -kScGuard .. 160 + kScGuard
    int ks = 0;
    double pmax = P[0], psum = 0.0;
#pragma unroll 16
    for (int i = 0; i < kScFreqs; i++) {                                        // (unrolled: sixteen reads in flight, not one)
        const double v = P[i];
        psum += v;
        if (v > pmax) {
            pmax = v;
            ks = i;
        }
    }
    ClockRec r = { 0.0f, 0.0f, IRDM_CLOCK_INVALID, (uint32_t)N };
    if (pmax > 0.0 && psum <= 1.0e300) {                                         // (neither holds for a NaN)
        double e = kScEps0 + kScStep * (double)ks;
        r.flags = IRDM_CLOCK_OUT_OF_RANGE;
        if (ks > 0 && ks < kScFreqs - 1) {
            const double a = P[ks - 1], b = P[ks], c = P[ks + 1];
            e = kScEps0 + ((double)ks + 0.5 * (a - c) / (a - 2.0 * b + c)) * kScStep;
            r.flags = 0;
        }
        double lo = 0.0, hi = 0.0;                                               // the largest beyond either edge
#pragma unroll
        for (int i = 1; i <= kScGuard; i++) {
            lo = fmax(lo, P[-i]);
            hi = fmax(hi, P[kScFreqs - 1 + i]);
        }
        if (fmax(lo, hi) > pmax) {
            e = lo >= hi ? kScEps0 : kScEps0 + kScStep * (double)(kScFreqs - 1);
            r.flags = IRDM_CLOCK_OUT_OF_RANGE;
        }
        r.eps = (float)e;
        r.quality = (float)(pmax / (psum / (double)kScFreqs));
    }
    out[blockIdx.x] = r;
}

// n_frames frames at d_frames (pitch kMaxFrameSamples) with their work records: their records into `out` (device or
// pinned host memory) on `stream`
static inline int launch_symbol_clock(const BurstWork *d_work, int n_frames, const float2 *d_frames, float sps, ClockRec *out,
                                      hipStream_t stream)
{
    if (n_frames <= 0) return 0;
    hipLaunchKernelGGL((symbol_clock_kernel<kScSeg>), dim3(n_frames), dim3(kScNT), 0, stream, d_work, d_frames, sps, out);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

// ---- host side: the summary of a stream ----

// Stream state: the per-frame records until they are polled, and the histogram the summary is read from (bin centres: the
// quartiles do not depend on how the stream was cut)
struct SymbolClockStream {
    std::deque<irdm_clock_est_t> q;
    std::vector<uint64_t> hist;         // kScBins counts, allocated with the first frame
    uint64_t used = 0, not_ok = 0, out_of_range = 0, invalid = 0;
};

static inline int symbol_clock_bin(float eps)
{
    const int k = (int)floor(((double)eps - kScEps0) / kScBin + 0.5);
    return k < 0 ? 0 : (k >= kScBins ? kScBins - 1 : k);
}

// one frame that reached the demodulator: its record, and whether the unique word passed
static inline void symbol_clock_fold(SymbolClockStream &st, uint64_t id, const ClockRec &r, bool ok)
{
    irdm_clock_est_t o;
    o.id = id;
    o.eps = r.eps;
    o.quality = r.quality;
    o.flags = r.flags | (ok ? 0u : (uint32_t)IRDM_CLOCK_NOT_OK);
    o.n = r.n;
    st.q.push_back(o);
    if (!ok) st.not_ok++;
    else if (r.flags & IRDM_CLOCK_INVALID) st.invalid++;
    else if (r.flags & IRDM_CLOCK_OUT_OF_RANGE) st.out_of_range++;
    else {
        if (st.hist.empty()) st.hist.assign((size_t)kScBins, 0);
        st.hist[(size_t)symbol_clock_bin(r.eps)]++;
        st.used++;
    }
}

// the centre of the bin that holds the ceil(q used)-th smallest estimate
static inline double symbol_clock_quantile(const SymbolClockStream &st, double q)
{
    if (st.used == 0) return 0.0;
    uint64_t want = (uint64_t)ceil(q * (double)st.used), run = 0;
    if (want < 1) want = 1;
    for (int k = 0; k < kScBins; k++) {
        run += st.hist[(size_t)k];
        if (run >= want) return kScEps0 + (double)k * kScBin;
    }
    return kScEps0 + (double)(kScBins - 1) * kScBin;
}

static inline void symbol_clock_result(const SymbolClockStream &st, int decim, irdm_symbol_clock_t *out)
{
    memset(out, 0, sizeof(*out));
    out->frames_used = st.used;
    out->frames_not_ok = st.not_ok;
    out->frames_out_of_range = st.out_of_range;
    out->frames_invalid = st.invalid;
    out->median = symbol_clock_quantile(st, 0.5);
    out->q25 = symbol_clock_quantile(st, 0.25);
    out->q75 = symbol_clock_quantile(st, 0.75);
    out->implied_rate_hz = 250000.0 * (double)decim * (1.0 + out->median);
}

}  // namespace irdm
