// scrub.hpp -- option "scrub" / irdm_scrub_device (include/irdm_hip.h): every cf32 sample with a component that is not
// finite or lies outside +-2^e zeroed in place, for recordings with a ragged tail, a division by zero upstream or corrupt
// bytes.  One such sample puts a NaN or an Inf into the detector's baseline sums, which never recover.
//
// A component c is good iff fabsf(c) <= L, L = ldexpf(1, e), 0 <= e <= 127.  On the bits: (bits & 0x7fffffff) <= bits(L) --
// non-negative floats order as their bit patterns do, every Inf and NaN pattern lies above every finite one, and a
// subnormal is compared as it is whatever the denormal mode.  A sample with a component that is not good becomes +0, +0
// (all 64 bits zero); every other sample keeps its bits.
//
// One memory-bound pass, cf32 only (the integer formats hold no such value: nothing is launched for them):
//   * a lane loads 16 bytes (two samples) and stores them to the address it loaded from ONLY if it changed them: on a clean
//     recording the pass reads and writes nothing;
//   * the buffer need only be aligned to a sample: the span geometry of chunk_span.hpp (at 8 bytes per sample a head and a
//     tail of at most one sample each).
// Counting: a lane counts in registers; the counts are reduced over the wavefront by shuffles (wave_reduce.hpp) and lane 0 issues one atomic
// per non-zero count -- a file that is all NaN costs a few atomics per wavefront, not one per sample.  The wavefronts of a
// launch spread their atomics over kSbRows copies of the figures, 128 bytes apart, which the host adds up: with one copy
// the 8192 wavefronts of a full grid queue at one address, and a chunk with 1 % bad samples took 487 us where the pass
// without counting takes 129 (measured on the MI355X, 64 Mi samples).  The positions of the
// first and the last zeroed sample of a launch are two 32-bit maxima, 0xffffffff - index and index + 1 (0: none); the host
// adds the launch's base and cuts a buffer into launches of at most kChunkMaxLaunch = 2^31 samples, so an index fits.
// Every thread reaches every shuffle.
// Bounds: it reads and writes the span's samples (chunk_span.hpp) and, counting, its block of kSbRows figures.
//
// Launched by host_chain.hpp (the host feeds of a context and a front end) and by irdm_scrub_device (feed.cpp).
#pragma once
#include <string.h>
#include <algorithm>
#include "common.hpp"
#include "chunk_span.hpp"
#include "pass_ring.hpp"
#include "wave_reduce.hpp"
#include "../../include/irdm_hip.h"

namespace irdm {

constexpr int kSbRows = 64;                             // copies of a launch's figures (a power of two)
constexpr int kSbDefaultLog2 = 40;

// one of the kSbRows copies of a launch's figures on the device, all zero before the launch: a block is ScrubAcc[kSbRows]
struct alignas(128) ScrubAcc {
    unsigned long long n_zeroed, n_nonfinite, n_over;
    unsigned first_key;                 // max of 0xffffffff - index over the zeroed samples (0: none)
    unsigned last_key;                  // max of index + 1
};

constexpr size_t kSbBlockBytes = sizeof(ScrubAcc) * kSbRows;

// the bit pattern of 2^e
static inline unsigned scrub_limit_bits(int limit_log2) { return (unsigned)(limit_log2 + 127) << 23; }

// a lane's counts
struct SbLane {
    unsigned zeroed, nonfinite, over, first_key, last_key;
};

// one sample (its two words) at index idx of the launch: true if it is to be zeroed
__device__ __forceinline__ bool sb_take(SbLane &a, unsigned i_bits, unsigned q_bits, unsigned limit_bits, unsigned idx)
{
    const unsigned mi = i_bits & 0x7fffffffu, mq = q_bits & 0x7fffffffu;
    if (mi <= limit_bits && mq <= limit_bits) return false;
    a.nonfinite += (mi >= 0x7f800000u ? 1u : 0u) + (mq >= 0x7f800000u ? 1u : 0u);
    a.over += (mi > limit_bits && mi < 0x7f800000u ? 1u : 0u) + (mq > limit_bits && mq < 0x7f800000u ? 1u : 0u);
    a.zeroed += 1u;
    const unsigned fk = 0xffffffffu - idx, lk = idx + 1u;
    a.first_key = fk > a.first_key ? fk : a.first_key;
    a.last_key = lk > a.last_key ? lk : a.last_key;
    return true;
}

// The cf32 samples of span sp (at most 2^31) at `buf` (aligned to a sample).  COUNT false: nothing is counted, acc is not
// touched.
template <bool COUNT>
__global__ __launch_bounds__(kChunkNT) void scrub_kernel(void *__restrict__ buf, const ChunkSpan sp, unsigned limit_bits,
                                                         ScrubAcc *__restrict__ acc)
{
    const ChunkLane cl = chunk_lane();
    unsigned char *const bytes = static_cast<unsigned char *>(buf);
    uint4 *const pieces = reinterpret_cast<uint4 *>(bytes + sp.head * 8);
    SbLane a;
    a.zeroed = a.nonfinite = a.over = a.first_key = a.last_key = 0u;
    for (long long i = cl.gid; i < sp.nvec; i += cl.stride) {
        uint4 v = pieces[i];
        const unsigned idx = (unsigned)(sp.head + 2 * i);
        const bool b0 = sb_take(a, v.x, v.y, limit_bits, idx);
        const bool b1 = sb_take(a, v.z, v.w, limit_bits, idx + 1u);
        if (b0 || b1) {
            if (b0) v.x = v.y = 0u;
            if (b1) v.z = v.w = 0u;
            pieces[i] = v;
        }
    }
    const long long si = cl.scalar<2>(sp);
    if (si >= 0) {
        unsigned *q = reinterpret_cast<unsigned *>(bytes + si * 8);
        if (sb_take(a, q[0], q[1], limit_bits, (unsigned)si)) {
            q[0] = 0u;
            q[1] = 0u;
        }
    }
    if (!COUNT) return;
    const unsigned z = wave_sum(a.zeroed), nf = wave_sum(a.nonfinite), ov = wave_sum(a.over);
    const unsigned fk = wave_max(a.first_key), lk = wave_max(a.last_key);
    acc += (blockIdx.x * (kChunkNT / 64) + (threadIdx.x >> 6)) & (kSbRows - 1);
    if ((threadIdx.x & 63) == 0 && z) {
        atomicAdd(&acc->n_zeroed, (unsigned long long)z);
        if (nf) atomicAdd(&acc->n_nonfinite, (unsigned long long)nf);
        if (ov) atomicAdd(&acc->n_over, (unsigned long long)ov);
        atomicMax(&acc->first_key, fk);
        atomicMax(&acc->last_key, lk);
    }
}

// ---- host side ----

// One launch over n <= kChunkMaxLaunch cf32 samples at d_buf (aligned to a sample) on `stream`; the block d_acc (kSbBlockBytes,
// zero; or nullptr: no counting) takes the figures.  0, or -1 for a pointer that is not aligned to a sample, a limit outside 0 .. 127, too many
// samples or a launch that failed; n == 0 launches nothing.
static inline int launch_scrub(void *d_buf, size_t n, int limit_log2, ScrubAcc *d_acc, hipStream_t stream)
{
    if (limit_log2 < 0 || limit_log2 > 127 || n > kChunkMaxLaunch || (reinterpret_cast<uintptr_t>(d_buf) % 8u) != 0) return -1;
    if (n == 0) return 0;
    int grid = 0;
    const ChunkSpan sp = chunk_span(8, d_buf, n, kChunkNT, kChunkMaxGrid, &grid);
    if (d_acc)
        hipLaunchKernelGGL((scrub_kernel<true>), dim3(grid), dim3(kChunkNT), 0, stream, d_buf, sp, scrub_limit_bits(limit_log2), d_acc);
    else
        hipLaunchKernelGGL((scrub_kernel<false>), dim3(grid), dim3(kChunkNT), 0, stream, d_buf, sp, scrub_limit_bits(limit_log2), d_acc);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

// n cf32 samples at d_buf scrubbed on `stream` without figures, in launches of at most kChunkMaxLaunch
static inline int scrub_plain(void *d_buf, size_t n, int limit_log2, hipStream_t stream)
{
    for (size_t off = 0; off < n; off += kChunkMaxLaunch)
        if (launch_scrub(static_cast<char *>(d_buf) + off * 8, std::min(kChunkMaxLaunch, n - off), limit_log2, nullptr, stream) != 0) return -1;
    return 0;
}

// the running totals of a stream; first / last are stream positions, valid when zeroed > 0
struct ScrubRun {
    uint64_t n = 0, zeroed = 0, nonfinite = 0, over = 0, first = 0, last = 0;
};

// a finished launch's block (host copy) over the n samples from stream position `base` into the totals
static inline void scrub_fold(ScrubRun &t, const ScrubAcc *rows, uint64_t base, size_t n)
{
    t.n += n;
    ScrubAcc a{};
    for (int r = 0; r < kSbRows; r++) {
        a.n_zeroed += rows[r].n_zeroed;
        a.n_nonfinite += rows[r].n_nonfinite;
        a.n_over += rows[r].n_over;
        a.first_key = std::max(a.first_key, rows[r].first_key);
        a.last_key = std::max(a.last_key, rows[r].last_key);
    }
    if (!a.n_zeroed) return;
    const uint64_t first = base + (uint64_t)(0xffffffffu - a.first_key), last = base + (uint64_t)a.last_key - 1;
    if (!t.zeroed || first < t.first) t.first = first;
    if (!t.zeroed || last > t.last) t.last = last;
    t.zeroed += a.n_zeroed;
    t.nonfinite += a.n_nonfinite;
    t.over += a.n_over;
}

static inline void scrub_result(const ScrubRun &t, int limit_log2, int active, irdm_scrub_stats_t *out)
{
    memset(out, 0, sizeof(*out));
    out->n_samples = t.n;
    out->n_zeroed = t.zeroed;
    out->n_nonfinite = t.nonfinite;
    out->n_over = t.over;
    out->first = t.first;
    out->last = t.last;
    out->limit_log2 = limit_log2;
    out->active = active;
}

// The pass of a context or a front end: the switch and the limit (configuration) and its ring (cache; pass_ring.hpp),
// without a side stream -- the pass runs on the stream its chunk arrives on, in front of everything that reads the chunk.
struct ScrubPass : PassRing {
    int on = 0, limit_log2 = kSbDefaultLog2;
};
// Stream state: the totals, and the launches in flight (an entry's meta: the stream position of the launch's first sample).
struct ScrubStream : PassRingStream {
    ScrubRun run;
};

static inline auto scrub_folder(ScrubStream &st)
{
    return [&st](const void *h_acc, const PassRingStream::Entry &e) { scrub_fold(st.run, static_cast<const ScrubAcc *>(h_acc), e.meta, e.n); };
}

// every launch in flight is waited for and folded, oldest first
static inline int scrub_settle(ScrubPass &ps, ScrubStream &st) { return ps.settle(st, ~0ull, scrub_folder(st)); }

// The n cf32 samples at d_buf, which `stream` has produced, from stream position `base`: scrubbed on `stream`, the figures
// on their way to a pinned block.  (A launch's tag is its number: taking a slot again settles its previous launch alone.)
static inline int scrub_enqueue(ScrubPass &ps, ScrubStream &st, void *d_buf, size_t n, uint64_t base, hipStream_t stream)
{
    for (size_t off = 0; off < n; off += kChunkMaxLaunch) {
        const size_t piece = std::min(kChunkMaxLaunch, n - off);
        const int slot = ps.acquire(st, scrub_folder(st));
        if (slot < 0) return -1;
        ScrubAcc *d_acc = static_cast<ScrubAcc *>(ps.d_block[slot]);
        if (hipMemsetAsync(d_acc, 0, kSbBlockBytes, stream) != hipSuccess) return -1;
        if (launch_scrub(static_cast<char *>(d_buf) + off * 8, piece, ps.limit_log2, d_acc, stream) != 0) return -1;
        if (ps.commit(st, slot, kSbBlockBytes, stream, base + off, piece, st.launches) != 0) return -1;
    }
    return 0;
}

}  // namespace irdm
