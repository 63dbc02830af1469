// symbol_clock.hpp -- option "symbol_clock" (irdm_clock_est_t / irdm_symbol_clock_t, include/irdm_hip.h): the symbol clock
// error of every downmixed frame, estimated on the device from the samples the demodulator is handed.  One of the two
// frame line estimators: the pieces, their arithmetic and the host side's histogram are frame_line.hpp's.
//
// Signal: |x|^2 of a frame carries a spectral line at the symbol rate.  At a nominal sps samples per symbol and a clock error
// eps the line sits at 1 / (sps (1 + eps)) cycles per sample (tests/clock_model.py states the same in numpy):
//   p[n] = re^2 + im^2,  p' = p - mean(p),  P[k] = |sum_n p'[n] exp(-2 pi i f_k n)|^2,  f_k = 1 / (sps (1 + eps_k))
// Grid: eps_k = -0.08 + 0.001 k, k = 0 .. 160; k* the first maximum; inside the grid the three-point parabola refines it, at
// an edge the record is flagged out of range; quality = P[k*] / mean_k P[k].
// Only a line within its main lobe (1 / n cycles per sample) of an edge shows there: a line further out leaves the grid
// to the frame's own modulation, whose maximum says nothing (its quality is that of a frame without a line, 2 .. 7 against
// 12 and more).  So P is also taken at kScGuard points of the same step beyond either edge (eps = -11 % .. -8.1 % and
// +8.1 % .. +11 %): where one of them exceeds P[k*] the record is out of range too, with eps the edge of that side.
//
// Geometry: one workgroup per frame, kScSeg x 256 threads: thread (s, j) sums point j of the 221 over the s-th quarter of
// the frame.  p' is staged once in LDS as doubles (35.5 KB of 62 KB).  Over the 1110 samples of a quarter at w = 0.57 ..
// 0.71 rad the recurrence's rounding error stays near 1e-13 of the sum, where a tenth of a grid step on a 64-sample frame
// asks for 3e-6.
// Cost: 2 binary64 operations per sample and grid point -- a chunk of 667 bursts of 2000 samples 0.59 G of them, at four
// cycles a wavefront instruction per SIMD -- on 667 workgroups of sixteen wavefronts, two to a CU (the 32-wavefront limit):
// the launch is bound by the binary64 issue rate of the CUs it occupies, in two rounds of workgroups.
//
// Launched by chain.cpp (the chain of a chunk) and state.cpp (irdm_symbol_clock_batch); the host side below it is the
// summary of a stream (pipeline.hpp: StreamState::clock).
#pragma once
#include "frame_line.hpp"

namespace irdm {

constexpr int kScFreqs = 161;                           // grid points
constexpr int kScGuard = 30;                            // points beyond either edge of the grid, for the out-of-range flag only
constexpr int kScPoints = kScFreqs + 2 * kScGuard;      // point j is k = j - kScGuard
constexpr int kScLanes = 256;                           // threads of a segment: four wavefronts, 35 lanes idle
constexpr int kScSeg = 4;                               // segments a frame is cut into
constexpr int kScNT = kScLanes * kScSeg;                // threads of a workgroup
constexpr double kScEps0 = -0.08, kScStep = 0.001;
// the summary's histogram: 0.01 % bins over +-8 %
constexpr int kScBins = 1601;
constexpr double kScBin = 1e-4;

__host__ __device__ __forceinline__ double sc_grid_freq(int k, float sps)
{
    return 1.0 / ((double)sps * (1.0 + (kScEps0 + kScStep * (double)k)));
}

// frames: n_frames rows of kMaxFrameSamples float2; work[i].num_samples / .drop_reason say what row i holds
// (a template, as input_stats_kernel is: every translation unit of the host side sees this header, two instantiate it)
template <int SEG>
__global__ __launch_bounds__(kScNT) void symbol_clock_kernel(const BurstWork *__restrict__ work, const float2 *__restrict__ frames,
                                                             float sps, LineRec *__restrict__ out)
{
    __shared__ double sh_p[kMaxFrameSamples];
    __shared__ double sh_red[kScNT];
    static_assert(SEG * kScLanes == kScNT, "a workgroup is SEG segments of kScLanes threads");
    __shared__ double sh_part[2 * kScNT];
    __shared__ double sh_P[kScPoints];
    __shared__ int sh_bad;
    const int tid = threadIdx.x;
    const BurstWork &w = work[blockIdx.x];
    const int N = w.num_samples;
    if (line_open(w, &sh_bad, &out[blockIdx.x])) return;
    const float2 *x = frames + (size_t)blockIdx.x * kMaxFrameSamples;
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
    sh_red[tid] = s;
    if (line_vote(bad, &sh_bad, N, &out[blockIdx.x])) return;
    for (int d = 512; d > 0; d >>= 1) {
        if (tid < d && tid + d < kScNT) sh_red[tid] += sh_red[tid + d];
        __syncthreads();
    }
    const double mean = sh_red[0] / (double)N;
    for (int n = tid; n < N; n += kScNT) sh_p[n] -= mean;
    __syncthreads();
    line_grid_power<kScPoints, kScLanes, SEG, 1, 8>(sh_p, N, sh_part, sh_P, [sps](int j) { return sc_grid_freq(j - kScGuard, sps); });
    if (tid != 0) return;
    const double *P = sh_P + kScGuard;                                           // P[k], k = -kScGuard .. 160 + kScGuard
    const LinePeak pk = line_peak<kScFreqs, kScGuard>(P);
    LineRec r = { 0.0f, 0.0f, kLineInvalid, (uint32_t)N };
    if (pk.usable()) {
        r.quality = (float)(pk.pmax / (pk.psum / (double)kScFreqs));
        r.flags = kLineOutOfRange;
        if (pk.guarded()) r.value = (float)(pk.lo >= pk.hi ? kScEps0 : kScEps0 + kScStep * (double)(kScFreqs - 1));
        else if (pk.k == 0 || pk.k == kScFreqs - 1) r.value = (float)(kScEps0 + kScStep * (double)pk.k);
        else {
            r.value = (float)(kScEps0 + ((double)pk.k + pk.off) * kScStep);
            r.flags = 0;
        }
    }
    out[blockIdx.x] = r;
}

// n_frames frames at d_frames (pitch kMaxFrameSamples) with their work records: their records into `out` (device or
// pinned host memory) on `stream`
static inline int launch_symbol_clock(const BurstWork *d_work, int n_frames, const float2 *d_frames, float sps, LineRec *out,
                                      hipStream_t stream)
{
    return line_launch(symbol_clock_kernel<kScSeg>, n_frames, kScNT, 0, stream, d_work, d_frames, sps, out);
}

// ---- host side: the summary of a stream (frame_line.hpp: LineStream over eps) ----

using SymbolClockStream = LineStream<irdm_clock_est_t>;
constexpr LineBins kScHist = { kScEps0, kScBin, kScBins };

// one frame that reached the demodulator: its record, and whether the unique word passed
static inline void symbol_clock_fold(SymbolClockStream &st, uint64_t id, const LineRec &r, bool ok)
{
    irdm_clock_est_t o;
    o.id = id;
    o.eps = r.value;
    o.quality = r.quality;
    o.flags = r.flags | (ok ? 0u : kLineNotOk);
    o.n = r.n;
    line_fold(st, o, r.flags, ok, (double)r.value);
}

static inline void symbol_clock_result(const SymbolClockStream &st, int decim, irdm_symbol_clock_t *out)
{
    memset(out, 0, sizeof(*out));
    out->frames_used = st.used;
    out->frames_not_ok = st.not_ok;
    out->frames_out_of_range = st.out_of_range;
    out->frames_invalid = st.invalid;
    out->median = line_quantile(st, 0.5);
    out->q25 = line_quantile(st, 0.25);
    out->q75 = line_quantile(st, 0.75);
    out->implied_rate_hz = 250000.0 * (double)decim * (1.0 + out->median);
}

}  // namespace irdm
