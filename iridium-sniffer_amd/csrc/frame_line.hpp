// frame_line.hpp -- the core of the per-frame line estimators: symbol_clock_kernel (symbol_clock.hpp: the place of the symbol
// rate's line in |x|^2), fine_freq_kernel (fine_freq.hpp: the carrier's line in x^4) and fine_time_kernel (fine_time.hpp: the
// phase of the symbol rate's line).  Each is a __global__ function of its own that stages its signal in LDS as doubles and
// composes the pieces below; every piece is resolved at compile time.
//
//   line_open / line_vote   a row that holds no usable frame, or a sample that is not finite: the INVALID record
//   line_segment_sum        sum_n y[n] exp(-2 pi i f n) over a segment by Goertzel's second-order recurrence
//   line_grid_power         a grid of frequencies: thread (segment, point) sums, the segments are added in their order
//   line_peak               the first maximum and the parabola's offset from it, the grid's sum, the largest guard points
//   line_launch             one workgroup per frame
//   LineStream              host side: the records of a stream until they are polled, and the histogram of its summary
//
// All arithmetic is binary64 with separately rounded products and sums (but the recurrence's explicit fused multiply-add),
// in an order fixed by the frame's length alone: a frame's record depends on its samples only, and the CPU emulation computes
// the same bits as the device (tests/golden/line_records.json holds them, tests/line_records.py compares).
//
// Goertzel: s[n] = y[n] + 2 cos(w) s[n-1] - s[n-2], one subtraction and one fused multiply-add per sample and real
// sequence; behind the last sample m of the segment s[m] - exp(-i w) s[m-1] = sum_n y[n] exp(i w (m - n)), which
// exp(-i w m) turns into the segment's share of the sum.  The two phases come from f and from the FRACTION of f m through
// the polynomials of libm_port.hpp kept in double (the reduction to an octant is exact).
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

constexpr int kLineMinSamples = 64;                     // a shorter frame has no estimate

// the flags of a record: the three public sets, value for value (fine_time's "ambiguous" is its "out of range": the line's
// place is further from the correlator's than a quarter of a symbol)
enum : uint32_t { kLineInvalid = 1u, kLineOutOfRange = 2u, kLineNotOk = 4u };
static_assert(IRDM_CLOCK_INVALID == kLineInvalid && IRDM_FINE_FREQ_INVALID == kLineInvalid && IRDM_FINE_TIME_INVALID == kLineInvalid,
              "one flag set for the three estimators");
static_assert(IRDM_CLOCK_OUT_OF_RANGE == kLineOutOfRange && IRDM_FINE_FREQ_OUT_OF_RANGE == kLineOutOfRange &&
              IRDM_FINE_TIME_AMBIGUOUS == kLineOutOfRange, "one flag set for the three estimators");
static_assert(IRDM_CLOCK_NOT_OK == kLineNotOk && IRDM_FINE_FREQ_NOT_OK == kLineNotOk && IRDM_FINE_TIME_NOT_OK == kLineNotOk,
              "one flag set for the three estimators");

// a kernel's record: the public one without the burst id (and what the context adds to it).  Every record type has
// invalid(n): the record of a row without an estimate
struct LineRec {
    float value, quality;               // eps (symbol_clock), df in Hz (fine_freq)
    uint32_t flags, n;
    __host__ __device__ static LineRec invalid(uint32_t n) { return LineRec{ 0.0f, 0.0f, kLineInvalid, n }; }
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

// The same to binary64's precision, for an estimator that reads the line's PHASE (fine_time.hpp): the polynomials above are
// sinf's and cosf's, good to 1e-9, which a power does not see and a phase does -- 1e-8 rad of the phase a segment's sum is
// turned by.  Taylor's polynomials to x^15 and x^16 in Horner's scheme on x^2, |x| <= pi / 4: the next terms are 5e-17 and
// 2e-18.  Products and sums are rounded separately, so the device and the CPU emulation give the same bits.
__host__ __device__ __forceinline__ void sc_sincos_turns_exact(double t, double *s_out, double *c_out)
{
    const double q = rint(t * 4.0);
    const double x = (t - q * 0.25) * 6.283185307179586476925;
    const double z = x * x;
    double ps = -1.0 / 1307674368000.0, pc = 1.0 / 20922789888000.0;             // -1 / 15!, 1 / 16!
    ps = ps * z + 1.0 / 6227020800.0;                                            // 1 / 13!
    pc = pc * z - 1.0 / 87178291200.0;                                           // -1 / 14!
    ps = ps * z - 1.0 / 39916800.0;
    pc = pc * z + 1.0 / 479001600.0;
    ps = ps * z + 1.0 / 362880.0;
    pc = pc * z - 1.0 / 3628800.0;
    ps = ps * z - 1.0 / 5040.0;
    pc = pc * z + 1.0 / 40320.0;
    ps = ps * z + 1.0 / 120.0;
    pc = pc * z - 1.0 / 720.0;
    ps = ps * z - 1.0 / 6.0;
    pc = pc * z + 1.0 / 24.0;
    pc = pc * z - 0.5;
    const double s = x + x * (z * ps), c = 1.0 + z * pc;
    const int qi = (int)q & 3;
    const double s1 = (qi & 1) ? c : s, c1 = (qi & 1) ? -s : c;
    *s_out = (qi & 2) ? -s1 : s1;
    *c_out = (qi & 2) ? -c1 : c1;
}

// The whole workgroup: true, with the INVALID record written, where row w holds no frame of a usable length; else the vote
// "a sample is not finite" is opened
template <typename Rec>
__device__ __forceinline__ bool line_open(const BurstWork &w, int *sh_bad, Rec *out)
{
    const int N = w.num_samples;
    if (w.drop_reason != 0 || N < kLineMinSamples || N > kMaxFrameSamples) {
        if (threadIdx.x == 0) *out = Rec::invalid(w.drop_reason != 0 || N < 0 ? 0u : (uint32_t)N);
        return true;
    }
    if (threadIdx.x == 0) *sh_bad = 0;
    __syncthreads();
    return false;
}

// The whole workgroup, behind the staging loop: true, with the INVALID record written, where a thread saw `bad`.  (Its barrier
// also stands behind whatever the threads wrote to LDS before it.)
template <typename Rec>
__device__ __forceinline__ bool line_vote(bool bad, int *sh_bad, int N, Rec *out)
{
    if (bad) *sh_bad = 1;
    __syncthreads();
    if (!*sh_bad) return false;
    if (threadIdx.x == 0) *out = Rec::invalid((uint32_t)N);
    return true;
}

// sum_{n in [n0, n1)} y[n] exp(-2 pi i f n), f in cycles per sample, |f| <= 1/2 (both grids lie far inside: 0.09 .. 0.12
// of the clock's at ten samples per symbol, 0.005 of the frequency's): y is CH interleaved real sequences of doubles, one
// (a real signal) or two (re, im).  AHEAD samples are read ahead of the dependent steps that use them: a step is two
// instructions per sequence, an LDS read waited for in every step is sixty cycles and more.  EXACT: the two phases by
// sc_sincos_turns_exact.
template <int CH, int AHEAD, bool EXACT = false>
__device__ __forceinline__ void line_segment_sum(const double *y, int n0, int n1, double f, double *re_out, double *im_out)
{
    static_assert(CH == 1 || CH == 2, "a real or a complex signal");
    double es, ec;
    if constexpr (EXACT) sc_sincos_turns_exact(f, &es, &ec);
    else sc_sincos_turns(f, &es, &ec);                                           // exp(i w), w = 2 pi f
    const double c2 = 2.0 * ec;
    double s1[CH] = {}, s2[CH] = {};
    int n = n0;
    for (; n + AHEAD <= n1; n += AHEAD) {
        double v[CH * AHEAD];
#pragma unroll
        for (int i = 0; i < CH * AHEAD; i++) v[i] = y[CH * n + i];
#pragma unroll
        for (int i = 0; i < CH * AHEAD; i++) {
            const double s0 = __fma_rn(c2, s1[i % CH], v[i] - s2[i % CH]);
            s2[i % CH] = s1[i % CH];
            s1[i % CH] = s0;
        }
    }
    for (; n < n1; n++) {
#pragma unroll
        for (int c = 0; c < CH; c++) {
            const double s0 = __fma_rn(c2, s1[c], y[CH * n + c] - s2[c]);
            s2[c] = s1[c];
            s1[c] = s0;
        }
    }
    double yr = s1[0] - ec * s2[0], yi = es * s2[0];
    if constexpr (CH == 2) {                                                     // y = p + i q
        const double qr = s1[1] - ec * s2[1], qi = es * s2[1];
        yr = yr - qi;
        yi = yi + qr;
    }
    const double t = f * (double)(n1 - 1);
    double zs, zc;
    if constexpr (EXACT) sc_sincos_turns_exact(t - rint(t), &zs, &zc);
    else sc_sincos_turns(t - rint(t), &zs, &zc);                                 // exp(i w m), the phase from the fraction of f m
    *re_out = yr * zc + yi * zs;
    *im_out = yi * zc - yr * zs;
}

// The whole workgroup of SEG * LANES threads: |sum_n y[n] exp(-2 pi i freq(j) n)|^2 of the N samples at y into sh_P[j],
// j < POINTS <= LANES.  Thread (seg, j) sums point j over samples [seg L, (seg + 1) L); the first POINTS threads add the
// segments in their order.  sh_part: 2 * SEG * LANES doubles; behind the call it still holds the segments' sums, real parts
// at [seg LANES + j], imaginary parts SEG LANES further on (fine_time_kernel reads its line's from there).  The LANES threads
// of a segment read the same y[n]: from 32 LANES on a broadcast within each 32-lane half of a wavefront, which is what an
// 8-byte LDS read is served by (fine_freq's fine stage, 16 lanes, reads two addresses per half).
template <int POINTS, int LANES, int SEG, int CH, int AHEAD, bool EXACT = false, typename Freq>
__device__ __forceinline__ void line_grid_power(const double *y, int N, double *sh_part, double *sh_P, Freq freq)
{
    static_assert(POINTS <= LANES && SEG * LANES <= 1024, "a workgroup is SEG segments of LANES threads");
    constexpr int NT = SEG * LANES;
    const int tid = threadIdx.x;
    const int j = tid % LANES, seg = tid / LANES;
    const int L = (N + SEG - 1) / SEG;
    const int n0 = seg * L, n1 = (seg + 1) * L < N ? (seg + 1) * L : N;
    double ar = 0.0, ai = 0.0;
    if (j < POINTS && n0 < n1) line_segment_sum<CH, AHEAD, EXACT>(y, n0, n1, freq(j), &ar, &ai);
    sh_part[tid] = ar;
    sh_part[NT + tid] = ai;
    __syncthreads();
    if (tid < POINTS) {
        double re = sh_part[tid], im = sh_part[NT + tid];
        for (int g = 1; g < SEG; g++) {
            re += sh_part[g * LANES + tid];
            im += sh_part[NT + g * LANES + tid];
        }
        sh_P[tid] = re * re + im * im;
    }
    __syncthreads();
}

// the three-point parabola's vertex about P[k], in grid steps
__device__ __forceinline__ double line_parabola(const double *P, int k)
{
    const double a = P[k - 1], b = P[k], c = P[k + 1];
    return 0.5 * (a - c) / (a - 2.0 * b + c);
}

// One thread: over P[0 .. FREQS) the first maximum, the parabola's offset from it (0 at an end) and the sum; over the GUARD
// points on either side of them (P[-GUARD .. 0) and P[FREQS .. FREQS + GUARD)) the largest.  The guard points enter nothing
// else.  Every field is computed for every caller: line_peak is inlined, and what a caller does not read (the coarse stage
// of fine_freq_kernel: off; its fine stage: psum, lo, hi) is dead code the compiler drops.
struct LinePeak {
    int k;
    double pmax, psum, off, lo, hi;
    __device__ bool usable() const { return pmax > 0.0 && psum <= 1.0e300; }     // (neither holds for a NaN)
    __device__ bool guarded() const { return fmax(lo, hi) > pmax; }              // the line is beyond the grid, on the side lo >= hi says
};

template <int FREQS, int GUARD>
__device__ __forceinline__ LinePeak line_peak(const double *P)
{
    LinePeak r = { 0, P[0], 0.0, 0.0, 0.0, 0.0 };
#pragma unroll 16
    for (int i = 0; i < FREQS; i++) {                                            // (unrolled: sixteen reads in flight, not one)
        const double v = P[i];
        r.psum += v;
        if (v > r.pmax) {
            r.pmax = v;
            r.k = i;
        }
    }
    if (r.k > 0 && r.k < FREQS - 1) r.off = line_parabola(P, r.k);
#pragma unroll
    for (int i = 1; i <= GUARD; i++) {
        r.lo = fmax(r.lo, P[-i]);
        r.hi = fmax(r.hi, P[FREQS - 1 + i]);
    }
    return r;
}

// n_frames workgroups of `threads` on `stream`, one per frame (none: nothing is launched)
template <typename Kernel, typename... Args>
static inline int line_launch(Kernel kernel, int n_frames, int threads, size_t lds_bytes, hipStream_t stream, Args... args)
{
    if (n_frames <= 0) return 0;
    hipLaunchKernelGGL(kernel, dim3(n_frames), dim3(threads), lds_bytes, stream, args...);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

// ---- host side: the summary of a stream ----

// the histogram's bins: bin k is centred on origin + k width; a value beyond either end, or none at all, falls into the end's
struct LineBins {
    double origin, width;
    int count;
    int bin(double v) const
    {
        const double k = floor((v - origin) / width + 0.5);
        return !(k >= 0.0) ? 0 : (k >= (double)count ? count - 1 : (int)k);
    }
    double centre(int k) const { return origin + (double)k * width; }
};

// Stream state: the per-frame public records until they are polled, and the histogram the summary is read from (bin
// centres: the quartiles do not depend on how the stream was cut)
template <typename PublicRec>
struct LineStream {
    LineBins bins;
    std::deque<PublicRec> q;
    std::vector<uint64_t> hist;         // bins.count counts, allocated with the first frame
    uint64_t used = 0, not_ok = 0, out_of_range = 0, invalid = 0;
};

// one frame that reached the demodulator: its public record, the kernel's flags, whether the unique word passed, and the
// value the histogram takes if the frame is used; says whether it is
template <typename PublicRec>
static inline bool line_fold(LineStream<PublicRec> &st, const PublicRec &o, uint32_t flags, bool ok, double value)
{
    st.q.push_back(o);
    if (!ok) st.not_ok++;
    else if (flags & kLineInvalid) st.invalid++;
    else if (flags & kLineOutOfRange) st.out_of_range++;
    else {
        if (st.hist.empty()) st.hist.assign((size_t)st.bins.count, 0);
        st.hist[(size_t)st.bins.bin(value)]++;
        st.used++;
        return true;
    }
    return false;
}

// the centre of the bin that holds the ceil(q used)-th smallest value
template <typename PublicRec>
static inline double line_quantile(const LineStream<PublicRec> &st, double q)
{
    if (st.used == 0) return 0.0;
    uint64_t want = (uint64_t)ceil(q * (double)st.used), run = 0;
    if (want < 1) want = 1;
    for (int k = 0; k < st.bins.count; k++) {
        run += st.hist[(size_t)k];
        if (run >= want) return st.bins.centre(k);
    }
    return st.bins.centre(st.bins.count - 1);
}

}  // namespace irdm
