// fine_time.hpp -- option "fine_time" (irdm_fine_time_t / irdm_fine_time_summary_t, include/irdm_hip.h): the arrival time of
// every downmixed frame's first symbol, refined on the device from the samples the demodulator is handed.  The third of the
// frame line estimators: the pieces, their arithmetic and the host side's histogram are frame_line.hpp's.
//
// Signal: |x|^2 of a frame carries a spectral line at the symbol rate, and the PHASE of that line is the symbol timing
// (Oerder and Meyr; tests/fine_time_model.py states the same in numpy).  At a nominal sps samples per symbol:
//   W = min(N, 131 sps), simplex min(N, 80 sps): the shortest frame there is, so the part that holds signal in every frame
//       (a sum over a whole 1910-sample frame takes in the ramp-down of a short burst and is biased by +0.2 us)
//   p[n] = re^2 + im^2,  p' = p - mean(p) over the window,  S(f) = sum_{n < W} p'[n] exp(-2 pi i f n),  f0 = 1 / sps
//   tau = -arg S(f0) / 2 pi * sps in [-sps / 2, sps / 2): from x[0] to the nearest symbol centre, in samples
//   floor = mean |S(f_j)|^2 over f_j = f0 (1 + 0.02 j), j = +-2 .. +-9 (the line's main lobe ends at j = +-0.8 for W = 1310)
// The kernel leaves (Re S(f0), Im S(f0), floor) in doubles; arg is taken on the HOST (fine_time_tau): the device library's
// atan2 is pinned neither between the CPU emulation and the device nor between ROCm releases, the sums are, bit for bit.
//
// Geometry: one workgroup per frame, kFtSeg x 32 threads = four wavefronts: thread (s, j) sums point j of the 17 over the
// s-th eighth of the window, 164 samples at the most.  A segment is one 32-lane half of a wavefront, the unit an 8-byte LDS
// read is served in, so each read is a broadcast.  p' is staged once in LDS as doubles (10.2 KB of 16.6 KB).  w = 0.51 ..
// 0.74 rad: the recurrence's rounding error stays near 1e-13 of the sum (symbol_clock.hpp), 1e-13 rad of the phase, and the
// sines and cosines a segment's sum is turned by are binary64's (sc_sincos_turns_exact: sinf's polynomials are off by
// 1e-8 rad, 2e-8 samples of tau, which the other two estimators' powers do not see).
// Cost: 2 binary64 operations per sample and point on 17 points and at most 1310 samples, against symbol_clock_kernel's 221
// points on up to 4440; eight workgroups to a CU.
//
// Launched by chain.cpp (the chain of a chunk) and state.cpp (irdm_fine_time_batch); the host side below it turns a record
// into the frame's time and keeps the summary of a stream (pipeline.hpp: StreamState::ftime).
#pragma once
#include "frame_line.hpp"

namespace irdm {

constexpr int kFtFloor = 16;                            // floor points: j = -9 .. -2 and 2 .. 9
constexpr int kFtPoints = 1 + kFtFloor;                 // point 0 is f0
constexpr int kFtLanes = 32;                            // threads of a segment: half a wavefront, 15 lanes idle
constexpr int kFtSeg = 8;                               // segments a window is cut into
constexpr int kFtNT = kFtLanes * kFtSeg;                // threads of a workgroup
constexpr int kFtWinNormal = 131, kFtWinSimplex = 80;   // symbols of the window: iridium.h's minimum frame lengths
constexpr int kFtMaxWin = kFtWinNormal * 10;            // samples of LDS: sps is 10 in every context (create.cpp)
constexpr double kFtFloorStep = 0.02;
// the summary's histogram of tau - c: 0.01-sample bins over +-2.5 samples (a record beyond them is ambiguous)
constexpr LineBins kFtHist = { -2.5, 0.01, 501 };

// the kernel's record: the line as a complex number, the floor, and LineRec's flags and n
struct TimeRec {
    double re, im, floor;
    uint32_t flags, n;
    __host__ __device__ static TimeRec invalid(uint32_t n) { return TimeRec{ 0.0, 0.0, 0.0, kLineInvalid, n }; }
};
static_assert(sizeof(TimeRec) == 32, "four 8-byte words, written by one thread");

__host__ __device__ __forceinline__ int ft_window(int N, int simplex, float sps)
{
    int W = (int)((float)(simplex ? kFtWinSimplex : kFtWinNormal) * sps);
    if (W > kFtMaxWin) W = kFtMaxWin;
    return N < W ? N : W;
}

// point j: f0 (j = 0), then f0 (1 + 0.02 jj) over jj = -9 .. -2, 2 .. 9
__host__ __device__ __forceinline__ double ft_freq(int j, float sps)
{
    const double f0 = 1.0 / (double)sps;
    if (j == 0) return f0;
    const int jj = j <= kFtFloor / 2 ? j - 1 - (kFtFloor / 2 + 1) : j - (kFtFloor / 2 - 1);
    return f0 * (1.0 + kFtFloorStep * (double)jj);
}

// frames: n_frames rows of kMaxFrameSamples float2; work[i].num_samples / .drop_reason / .simplex say what row i holds
// (a template, as symbol_clock_kernel is: every translation unit of the host side sees this header, two instantiate it)
template <int SEG>
__global__ __launch_bounds__(kFtNT) void fine_time_kernel(const BurstWork *__restrict__ work, const float2 *__restrict__ frames,
                                                          float sps, TimeRec *__restrict__ out)
{
    static_assert(SEG * kFtLanes == kFtNT && (kFtNT & (kFtNT - 1)) == 0, "a workgroup is SEG segments of kFtLanes threads; the tree halves it");
    __shared__ double sh_p[kFtMaxWin];
    __shared__ double sh_red[kFtNT];
    __shared__ double sh_part[2 * kFtNT];
    __shared__ double sh_P[kFtLanes];
    __shared__ int sh_bad;
    const int tid = threadIdx.x;
    const BurstWork &w = work[blockIdx.x];
    const int N = w.num_samples;
    if (line_open(w, &sh_bad, &out[blockIdx.x])) return;
    const int W = ft_window(N, w.simplex, sps);                                  // (64 <= W <= kFtMaxWin)
    const float2 *x = frames + (size_t)blockIdx.x * kMaxFrameSamples;
    // p over the window and its mean: a thread's samples in their order, then a tree over the threads; a sample that is not
    // finite anywhere in the frame, behind the window too, leaves no estimate
    double s = 0.0;
    bool bad = false;
    for (int n = tid; n < N; n += kFtNT) {
        const float2 v = x[n];
        const double p = (double)v.x * (double)v.x + (double)v.y * (double)v.y;
        bad = bad || !(fabs(p) <= 1.0e300);
        if (n < W) {
            sh_p[n] = p;
            s += p;
        }
    }
    sh_red[tid] = s;
    if (line_vote(bad, &sh_bad, N, &out[blockIdx.x])) return;
    for (int d = kFtNT / 2; d > 0; d >>= 1) {
        if (tid < d) sh_red[tid] += sh_red[tid + d];
        __syncthreads();
    }
    const double mean = sh_red[0] / (double)W;
    for (int n = tid; n < W; n += kFtNT) sh_p[n] -= mean;
    __syncthreads();
    line_grid_power<kFtPoints, kFtLanes, SEG, 1, 8, true>(sh_p, W, sh_part, sh_P, [sps](int j) { return ft_freq(j, sps); });
    if (tid != 0) return;
    // the line itself: point 0's segments once more, in the order line_grid_power added them
    double re = sh_part[0], im = sh_part[kFtNT];
    for (int g = 1; g < SEG; g++) {
        re += sh_part[g * kFtLanes];
        im += sh_part[kFtNT + g * kFtLanes];
    }
    double fsum = 0.0;
#pragma unroll
    for (int j = 1; j < kFtPoints; j++) fsum += sh_P[j];
    TimeRec r = TimeRec::invalid((uint32_t)N);
    if (sh_P[0] > 0.0 && fsum <= 1.0e300) r = TimeRec{ re, im, fsum / (double)kFtFloor, 0u, (uint32_t)N };   // (neither holds for a NaN)
    out[blockIdx.x] = r;
}

// n_frames frames at d_frames (pitch kMaxFrameSamples) with their work records: their records into `out` (device or
// pinned host memory) on `stream`
static inline int launch_fine_time(const BurstWork *d_work, int n_frames, const float2 *d_frames, float sps, TimeRec *out,
                                   hipStream_t stream)
{
    return line_launch(fine_time_kernel<kFtSeg>, n_frames, kFtNT, 0, stream, d_work, d_frames, sps, out);
}

// ---- host side: a record's time, and the summary of a stream (frame_line.hpp: LineStream over tau - c) ----

using FineTimeStream = LineStream<irdm_fine_time_t>;

// tau in [-sps / 2, sps / 2) of a record without a flag: atan2 is in [-pi, pi], -pi for an imaginary part of -0 alone
static inline double fine_time_tau(const TimeRec &r, float sps)
{
    const double tau = -atan2(r.im, r.re) / 6.283185307179586476925 * (double)sps;
    return tau >= 0.5 * (double)sps ? tau - (double)sps : tau;
}

// the public record of a kernel's record alone (irdm_fine_time_batch; the context adds id, corr, time_ns and its flags)
static inline void fine_time_public(const TimeRec &r, float sps, irdm_fine_time_t *o)
{
    memset(o, 0, sizeof(*o));
    o->s_re = r.re;
    o->s_im = r.im;
    o->floor = r.floor;
    o->flags = r.flags;
    o->n = r.n;
    if (r.flags & kLineInvalid) return;
    o->tau = fine_time_tau(r, sps);
    o->quality = (float)((r.re * r.re + r.im * r.im) / r.floor);
}

// One frame that reached the demodulator: its record, the correlator's peak (uw_start, in samples behind the downmixer's
// timestamp) and correction c = uw_corr, whether the unique word passed.  The frame's sample 0 is uw_start + delta samples
// behind the timestamp: delta = tau where the record carries no flag, else c -- an invalid record, and an ambiguous one
// (|tau - c| > sps / 4: the line names another symbol's centre, or nothing), keep the correlator's place, so that every
// timestamp of a run means the same.  Returns the time of the frame's demodulator record.
static inline uint64_t fine_time_fold(FineTimeStream &st, uint64_t id, const TimeRec &r, float sps, uint64_t timestamp, int uw_start,
                                      float uw_corr, double out_rate, bool ok)
{
    irdm_fine_time_t o;
    fine_time_public(r, sps, &o);
    const double c = (double)uw_corr;
    if (!(o.flags & kLineInvalid) && !(fabs(o.tau - c) <= (double)sps / 4.0)) o.flags |= kLineOutOfRange;
    const uint32_t kernel_flags = o.flags;
    const double delta = kernel_flags ? c : o.tau;
    o.id = id;
    o.corr = uw_corr;
    o.time_ns = timestamp + (uint64_t)llrint(((double)uw_start + delta) * 1e9 / out_rate);      // (a negative sum wraps back below timestamp)
    if (!ok) o.flags |= kLineNotOk;
    line_fold(st, o, kernel_flags, ok, o.tau - c);
    return o.time_ns;
}

static inline void fine_time_result(const FineTimeStream &st, irdm_fine_time_summary_t *out)
{
    memset(out, 0, sizeof(*out));
    out->frames_seen = st.used + st.not_ok + st.out_of_range + st.invalid;       // (every frame is one of the four)
    out->frames_applied = st.used;
    out->frames_not_ok = st.not_ok;
    out->frames_ambiguous = st.out_of_range;
    out->frames_invalid = st.invalid;
    out->median = line_quantile(st, 0.5);
    out->q25 = line_quantile(st, 0.25);
    out->q75 = line_quantile(st, 0.75);
}

}  // namespace irdm
