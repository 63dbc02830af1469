// iq_moments.hpp -- option "iq_moments" / irdm_iq_moments_device (irdm_iq_moments_t, include/irdm_hip.h): the second
// moments of a stream's I and Q, from which the host derives the receiver's I/Q imbalance -- the gain of the Q arm over the
// I arm, the phase by which the two miss 90 degrees, and the level of the image at -f that every signal at +f leaves.
//
// One pass per chunk that reads b_in bytes per sample and writes nothing but its sums:
//   * the span geometry of chunk_span.hpp, at most kChunkMaxLaunch = 2^31 samples per launch (a lane's 32-bit count cannot
//     overflow);
//   * every sample converted as load_iq<FMT> converts it (iq_piece.hpp), then widened to binary64: i, q and the products
//     i i, q q, i q of two floats are exact doubles, so only the order of the additions is free (the products enter as
//     fma(i, q, sum): one rounding, that of the addition).  A cf32 sample with a component whose exponent field is all ones
//     is left out and not counted in n_used;
//   * a lane's five sums and its count are reduced over the wavefront by shuffles (wave_reduce.hpp), over the workgroup
//     through LDS, and the workgroup writes its row of a block that the host adds up in row order.  No atomics: the figures
//     of a launch depend on its geometry alone, two launches over one buffer give the same bytes.
// Bounds: it reads the span's samples (chunk_span.hpp); a workgroup writes rows[blockIdx.x], blockIdx.x < grid <= kChunkMaxGrid.
//
// Included by the translation units that launch it (feed.cpp: a context's stream and irdm_iq_moments_device;
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

// a workgroup's row: sum i, sum q, sum i i, sum q q, sum i q, and the samples that entered them
struct alignas(64) IqmRow {
    double s[5];
    unsigned long long used;
};
constexpr size_t kImBlockBytes = sizeof(IqmRow) * kChunkMaxGrid;

struct IqmLane {
    double s[5];
    unsigned used;
};

template <int FMT>
__device__ __forceinline__ void iqm_take(IqmLane &a, unsigned i_bits, unsigned q_bits)
{
    if (FMT == 2 && ((i_bits & 0x7f800000u) == 0x7f800000u || (q_bits & 0x7f800000u) == 0x7f800000u)) return;
    const double i = (double)__uint_as_float(i_bits), q = (double)__uint_as_float(q_bits);
    a.s[0] += i;
    a.s[1] += q;
    a.s[2] = __fma_rn(i, i, a.s[2]);                    // (the product is exact: the rounding is the addition's)
    a.s[3] = __fma_rn(q, q, a.s[3]);
    a.s[4] = __fma_rn(i, q, a.s[4]);
    a.used += 1u;
}

// The samples of span sp at `in` (aligned to a sample).  Every thread reaches every shuffle and the barrier.
template <int FMT>
__global__ __launch_bounds__(kChunkNT) void iq_moments_kernel(const void *__restrict__ in, const ChunkSpan sp, IqmRow *__restrict__ rows)
{
    constexpr int BPS = kFmtBytes<FMT>, SPV = 16 / BPS, NW = kChunkNT / 64;
    __shared__ double sh_d[NW][5];
    __shared__ unsigned sh_u[NW];
    const ChunkLane cl = chunk_lane();
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const unsigned char *const bytes = static_cast<const unsigned char *>(in);
    const uint4 *const pieces = reinterpret_cast<const uint4 *>(bytes + sp.head * BPS);
    IqmLane a;
    for (int j = 0; j < 5; j++) a.s[j] = 0.0;
    a.used = 0u;
    const long long si = cl.scalar<SPV>(sp);
    if (si >= 0) {
        unsigned o[2];
        iq_sample_bits<FMT>(bytes + si * BPS, o);
        iqm_take<FMT>(a, o[0], o[1]);
    }
    for (long long i = cl.gid; i < sp.nvec; i += cl.stride) {
        unsigned o[2 * SPV];
        iq_piece_bits<FMT>(pieces[i], o);
#pragma unroll
        for (int k = 0; k < SPV; k++) iqm_take<FMT>(a, o[2 * k], o[2 * k + 1]);
    }
    // the order of every sum is fixed by the launch geometry: a lane's pieces, the shuffle tree, the waves in turn
    double d[5];
    for (int j = 0; j < 5; j++) d[j] = wave_sum(a.s[j]);
    unsigned long long u = wave_sum(a.used);
    if (lane == 0) {
        for (int j = 0; j < 5; j++) sh_d[wave][j] = d[j];
        sh_u[wave] = (unsigned)u;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < NW; w++) {
            for (int j = 0; j < 5; j++) d[j] += sh_d[w][j];
            u += sh_u[w];
        }
        IqmRow r;
        for (int j = 0; j < 5; j++) r.s[j] = d[j];
        r.used = u;
        rows[blockIdx.x] = r;
    }
}

// ---- host side ----

// the running totals of a stream
struct IqmRun {
    uint64_t n = 0, used = 0;
    double s[5] = { 0.0, 0.0, 0.0, 0.0, 0.0 };
};

// One launch over n <= kChunkMaxLaunch samples (aligned to a sample of fmt) into d_rows (kImBlockBytes) on `stream`; returns
// the grid (the rows the launch wrote; 0: n == 0, nothing launched), -1 on error.
static inline int launch_iq_moments(int fmt, const void *d_in, size_t n, void *d_rows, hipStream_t stream)
{
    if (!fmt_valid(fmt) || n > kChunkMaxLaunch || (reinterpret_cast<uintptr_t>(d_in) % (size_t)fmt_bytes(fmt)) != 0) return -1;
    if (n == 0) return 0;
    int grid = 0;
    const ChunkSpan sp = chunk_span(fmt_bytes(fmt), d_in, n, kChunkNT, kChunkMaxGrid, &grid);
    IqmRow *rows = static_cast<IqmRow *>(d_rows);
    fmt_dispatch(fmt, [&](auto f) {
        hipLaunchKernelGGL((iq_moments_kernel<decltype(f)::value>), dim3(grid), dim3(kChunkNT), 0, stream, d_in, sp, rows);
    });
    return hipGetLastError() == hipSuccess ? grid : -1;
}

// a finished launch's rows (host copy) into the totals, in row order
static inline void iq_moments_fold(IqmRun &t, const void *h_rows, int grid, size_t n)
{
    t.n += n;
    const IqmRow *rows = static_cast<const IqmRow *>(h_rows);
    for (int g = 0; g < grid; g++) {
        for (int j = 0; j < 5; j++) t.s[j] += rows[g].s[j];
        t.used += rows[g].used;
    }
}

// the record: the sums, and gain, phase and image level derived from the central moments in binary64
static inline void iq_moments_result(const IqmRun &t, irdm_iq_moments_t *out)
{
    memset(out, 0, sizeof(*out));
    out->n_samples = t.n;
    out->n_used = t.used;
    out->sum_i = t.s[0];
    out->sum_q = t.s[1];
    out->sum_ii = t.s[2];
    out->sum_qq = t.s[3];
    out->sum_iq = t.s[4];
    if (t.used < 2) return;
    const double N = (double)t.used, mi = t.s[0] / N, mq = t.s[1] / N;
    const double cii = t.s[2] / N - mi * mi, cqq = t.s[3] / N - mq * mq, ciq = t.s[4] / N - mi * mq;
    if (!(cii > 0.0) || !(cqq > 0.0)) return;
    const double r = sqrt(cii * cqq);
    if (!(fabs(ciq) < r)) return;
    const double g = sqrt(cqq / cii), sp = ciq / r, cp = sqrt(1.0 - sp * sp);
    out->gain_db = 10.0 * log10(cqq / cii);
    out->phase_deg = asin(sp) * (180.0 / M_PI);
    // |1 - g e^{j phi}| / |1 + g e^{-j phi}|
    const double num = hypot(1.0 - g * cp, g * sp), den = hypot(1.0 + g * cp, g * sp);
    const double img = num > 0.0 ? 20.0 * log10(num / den) : -120.0;
    out->image_db = img < -120.0 ? -120.0 : img;
    out->valid = 1;
}

// The pass of a context or a front end: its switch (configuration) and its ring on a side stream (cache; pass_ring.hpp).
struct IqMomentsPass : PassRing {
    int on = 0;
};
// Stream state: the totals, and the launches in flight (an entry's meta: the launch's grid, the rows it wrote).
struct IqMomentsStream : PassRingStream {
    IqmRun run;
};

static inline auto iq_moments_folder(IqMomentsStream &st)
{
    return [&st](const void *h_rows, const PassRingStream::Entry &e) { iq_moments_fold(st.run, h_rows, (int)e.meta, e.n); };
}

// launches up to and including tag `upto` are waited for and folded, oldest first
static inline int iq_moments_settle(IqMomentsPass &ps, IqMomentsStream &st, uint64_t upto)
{
    return ps.settle(st, upto, iq_moments_folder(st));
}

// n samples at d_in, produced on `arrival` (nullptr: complete in memory): their pass on the side stream.  The launches
// carry `tag`; the caller orders whatever overwrites d_in behind ps.ev[st.last_slot] or settles the tag first.
static inline int iq_moments_enqueue(IqMomentsPass &ps, IqMomentsStream &st, int fmt, const void *d_in, size_t n,
                                     hipStream_t arrival, uint64_t tag)
{
    if (n == 0) return 0;
    if (ps.follow(arrival) != 0) return -1;
    const size_t bps = (size_t)fmt_bytes(fmt);
    for (size_t off = 0; off < n; off += kChunkMaxLaunch) {
        const size_t piece = std::min(kChunkMaxLaunch, n - off);
        const int slot = ps.acquire(st, iq_moments_folder(st));
        if (slot < 0) return -1;
        const int grid = launch_iq_moments(fmt, static_cast<const char *>(d_in) + off * bps, piece, ps.d_block[slot], ps.stream);
        if (grid < 0) return -1;
        if (ps.commit(st, slot, sizeof(IqmRow) * (size_t)grid, ps.stream, (uint64_t)grid, piece, tag) != 0) return -1;
    }
    return 0;
}

}  // namespace irdm
