// fine_freq.hpp -- option "fine_freq" (irdm_fine_freq_t / irdm_fine_freq_summary_t, include/irdm_hip.h): the carrier
// frequency of every downmixed frame, estimated on the device from the samples the demodulator is handed.  One of the two
// frame line estimators: the pieces, their arithmetic and the host side's histogram are frame_line.hpp's.
//
// Signal: the fourth power of a QPSK frame carries a spectral line at four times the frame's residual carrier offset
// (tests/fine_freq_model.py states the same in numpy); f_o is the context's out_rate:
//   y[n] = x[n]^4:  a = re re - im im,  b = 2 re im,  y = (a a - b b) + i 2 a b
//   P(g) = |sum_n y[n] exp(-2 pi i g n / f_o)|^2
// Grid, in two stages of one launch:
//   coarse: g_k = -1000 + 20 k Hz, k = 0 .. 100; k_c the first maximum; quality = P(g_kc) / mean_k P(g_k)
//   fine:   h_j = g_kc + 4 (j - 5), j = 0 .. 10; j* the first maximum; inside, the three-point parabola refines it
//   df = g* / 4
// Only a line within its main lobe of an edge shows there, so P is also taken at kFfGuard points of the coarse step beyond
// either edge (+-1020 .. +-1200 Hz): where one of them exceeds P(g_kc), or k_c is at an edge, the record is out of range
// and df is the edge of that side, +-250 Hz.  A frame more than +-300 Hz from the downmixer's value has its line beyond the
// guard points: the grid then shows the frame's modulation, and the check is blind.  A linear drift over the frame leaves
// the line's centre at the frequency of the frame's middle.
//
// Geometry: one workgroup per frame, 1024 threads, y staged once in LDS as doubles (71 KB of dynamic LDS beside 17 KB of
// partial sums: one workgroup of sixteen wavefronts to a CU).
//   coarse: thread (s, j), j < 121 of 128 lanes, sums point j over the s-th eighth of the frame
//   fine:   once thread 0 has found k_c: thread (s, j), j < 11 of 16 lanes, sums point j over the s-th of 64 segments
// w is at most 0.03 rad, where the recurrence loses a factor 1 / sin w: over the 555 samples of an eighth its rounding error
// stays near 1e-11 of the sum, and a wrong tenth of a fine step on a 64-sample frame would take 2e-8.  No scratch memory.
// Cost: 4 binary64 operations per sample and point on 132 points, where symbol_clock_kernel takes 2 on 221.
//
// Launched by chain.cpp (the chain of a chunk) and state.cpp (irdm_fine_freq_batch); the host side below it is the
// summary of a stream (pipeline.hpp: StreamState::fine).
#pragma once
#include <float.h>
#include "frame_line.hpp"

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
constexpr double kFfG0 = -1000.0, kFfStep = 20.0, kFfFineStep = 4.0, kFfEdge = 250.0;
constexpr size_t kFfLdsBytes = sizeof(double) * 2 * (size_t)kMaxFrameSamples;
// the summary's histogram of refined - PLL: 1 Hz bins over +-500 Hz
constexpr LineBins kFfHist = { -500.0, 1.0, 1001 };

// frames: n_frames rows of kMaxFrameSamples float2; work[i].num_samples / .drop_reason say what row i holds
// (a template, as symbol_clock_kernel is: every translation unit of the host side sees this header, two instantiate it)
template <int SEG>
__global__ __launch_bounds__(kFfNT) void fine_freq_kernel(const BurstWork *__restrict__ work, const float2 *__restrict__ frames,
                                                          double out_rate, LineRec *__restrict__ out)
{
#if defined(IRDM_HIP_EMULATED)
    unsigned char *ff_lds = hip_emul::dyn_lds();
#else
    extern __shared__ __attribute__((aligned(16))) unsigned char ff_lds[];
#endif
    static_assert(SEG * kFfLanes == kFfNT && kFfFineSeg * kFfFineLanes == kFfNT, "both stages use the whole workgroup");
    double *sh_y = reinterpret_cast<double *>(ff_lds);                           // y[n] = (sh_y[2 n], sh_y[2 n + 1])
    __shared__ double sh_part[2 * kFfNT];                                        // both stages
    __shared__ double sh_P[kFfPoints];
    __shared__ double sh_Pf[kFfFineLanes];
    __shared__ int sh_bad, sh_kc;
    const int tid = threadIdx.x;
    const BurstWork &w = work[blockIdx.x];
    const int N = w.num_samples;
    if (line_open(w, &sh_bad, &out[blockIdx.x])) return;
    const float2 *x = frames + (size_t)blockIdx.x * kMaxFrameSamples;
    bool bad = false;
    for (int n = tid; n < N; n += kFfNT) {
        const float2 v = x[n];
        bad = bad || !(fabsf(v.x) <= FLT_MAX) || !(fabsf(v.y) <= FLT_MAX);
        const double re = (double)v.x, im = (double)v.y;
        const double a = re * re - im * im, b = 2.0 * (re * im);
        sh_y[2 * n] = a * a - b * b;
        sh_y[2 * n + 1] = 2.0 * (a * b);
    }
    if (line_vote(bad, &sh_bad, N, &out[blockIdx.x])) return;
    line_grid_power<kFfPoints, kFfLanes, SEG, 2, 4>(sh_y, N, sh_part, sh_P,
                                                    [out_rate](int j) { return (kFfG0 + kFfStep * (double)(j - kFfGuard)) / out_rate; });
    LineRec r = { 0.0f, 0.0f, kLineInvalid, (uint32_t)N };                       // (thread 0's)
    if (tid == 0) {
        const LinePeak pk = line_peak<kFfCoarse, kFfGuard>(sh_P + kFfGuard);     // P[k], k = -kFfGuard .. 100 + kFfGuard
        int go = -1;                                                             // the fine stage's centre, or none
        if (pk.usable()) {
            r.quality = (float)(pk.pmax / (pk.psum / (double)kFfCoarse));
            r.flags = kLineOutOfRange;
            if (pk.guarded()) r.value = (float)(pk.lo >= pk.hi ? -kFfEdge : kFfEdge);
            else if (pk.k == 0 || pk.k == kFfCoarse - 1) r.value = (float)(pk.k == 0 ? -kFfEdge : kFfEdge);
            else {
                r.flags = 0;
                go = pk.k;
            }
        }
        if (go < 0) out[blockIdx.x] = r;                                         // (else the fine stage completes it)
        sh_kc = go;
    }
    __syncthreads();
    const int kc = sh_kc;
    if (kc < 0) return;                                                          // (the whole workgroup)
    const auto h = [kc](int j) { return (kFfG0 + kFfStep * (double)kc) + kFfFineStep * (double)(j - kFfFine / 2); };
    line_grid_power<kFfFine, kFfFineLanes, kFfFineSeg, 2, 4>(sh_y, N, sh_part, sh_Pf, [=](int j) { return h(j) / out_rate; });
    if (tid != 0) return;
    const LinePeak pf = line_peak<kFfFine, 0>(sh_Pf);
    r.value = (float)((h(pf.k) + kFfFineStep * pf.off) / 4.0);                   // (off is 0 at an end of the fine grid; h is never -0)
    out[blockIdx.x] = r;
}

// n_frames frames at d_frames (pitch kMaxFrameSamples) with their work records: their records into `out` (device or
// pinned host memory) on `stream`
static inline int launch_fine_freq(const BurstWork *d_work, int n_frames, const float2 *d_frames, double out_rate, LineRec *out,
                                   hipStream_t stream)
{
    // (the kernel may be given more than 64 KB of dynamic LDS: once per device)
    static bool raised[64];
    int dev = 0;
    if (n_frames > 0) {
        if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return -1;
        if (!raised[dev] && hipFuncSetAttribute(reinterpret_cast<const void *>(&fine_freq_kernel<kFfSeg>),
                                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)kFfLdsBytes) != hipSuccess)
            return -1;
        raised[dev] = true;
    }
    return line_launch(fine_freq_kernel<kFfSeg>, n_frames, kFfNT, kFfLdsBytes, stream, d_work, d_frames, out_rate, out);
}

// ---- host side: the summary of a stream (frame_line.hpp: LineStream over refined - PLL) ----

using FineFreqStream = LineStream<irdm_fine_freq_t>;

// One frame that reached the demodulator: its record, the downmixer's frequency of the frame, whether the unique word
// passed, and the frequency the PLL's arithmetic gives a frame that passed.  Returns the centre frequency of the frame's
// demodulator record: the refined one, or the PLL's where the record is flagged.
static inline double fine_freq_fold(FineFreqStream &st, uint64_t id, const LineRec &r, double cfreq, bool ok, double pll)
{
    irdm_fine_freq_t o;
    o.id = id;
    o.freq_hz = cfreq + (double)r.value;
    o.df_hz = r.value;
    o.quality = r.quality;
    o.flags = r.flags | (ok ? 0u : kLineNotOk);
    o.n = r.n;
    return line_fold(st, o, r.flags, ok, o.freq_hz - pll) ? o.freq_hz : pll;
}

static inline void fine_freq_result(const FineFreqStream &st, irdm_fine_freq_summary_t *out)
{
    memset(out, 0, sizeof(*out));
    out->frames_seen = st.used + st.not_ok + st.out_of_range + st.invalid;       // (every frame is one of the four)
    out->frames_applied = st.used;
    out->frames_not_ok = st.not_ok;
    out->frames_out_of_range = st.out_of_range;
    out->frames_invalid = st.invalid;
    out->median = line_quantile(st, 0.5);
    out->q25 = line_quantile(st, 0.25);
    out->q75 = line_quantile(st, 0.75);
}

}  // namespace irdm
