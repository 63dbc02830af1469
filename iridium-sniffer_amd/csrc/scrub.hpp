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
//   * grid-stride loop, at most kSbMaxGrid workgroups of kSbNT threads;
//   * the buffer need only be aligned to a sample: the sample in front of the first 16-byte boundary and the one behind the
//     last are handled one per thread by the first threads of the grid (iq_swap.hpp's head and tail).
// Counting: a lane counts in registers; the counts are reduced over the wavefront by shuffles and lane 0 issues one atomic
// per non-zero count -- a file that is all NaN costs a few atomics per wavefront, not one per sample.  The wavefronts of a
// launch spread their atomics over kSbRows copies of the figures, 128 bytes apart, which the host adds up: with one copy
// the 8192 wavefronts of a full grid queue at one address, and a chunk with 1 % bad samples took 487 us where the pass
// without counting takes 129 (measured on the MI355X, 64 Mi samples).  The positions of the
// first and the last zeroed sample of a launch are two 32-bit maxima, 0xffffffff - index and index + 1 (0: none); the host
// adds the launch's base and cuts a buffer into launches of at most kSbMaxLaunch = 2^31 samples, so an index fits.
// Every thread reaches every shuffle.
// Bounds: the vector part covers bytes [head * 8, (head + 2 nvec) * 8), head + 2 nvec <= n; the scalar part the samples
// [0, head) and [head + 2 nvec, n).
//
// Included by the translation units that launch it (feed.cpp: irdm_feed_host of a context and irdm_scrub_device;
// frontend.cpp: the capture in front of K0 / K0r).
#pragma once
#include <string.h>
#include <algorithm>
#include <deque>
#include "common.hpp"
#include "../../include/irdm_hip.h"

namespace irdm {

constexpr int kSbNT = 256;                              // threads of a workgroup
constexpr int kSbMaxGrid = 2048;                        // workgroups of a launch
constexpr size_t kSbMaxLaunch = (size_t)1 << 31;        // samples of a launch: an index and a lane's counts fit 32 bits
constexpr int kSbSlots = 4;                             // launches in flight per context
constexpr int kSbRows = 64;                             // copies of a launch's figures (a power of two)
constexpr int kSbDefaultLog2 = 40;

// one of the kSbRows copies of a launch's figures on the device, all zero before the launch: a block is ScrubAcc[kSbRows]
struct alignas(128) ScrubAcc {
    unsigned long long n_zeroed, n_nonfinite, n_over;
    unsigned first_key;                 // max of 0xffffffff - index over the zeroed samples (0: none)
    unsigned last_key;                  // max of index + 1
};

// the bit pattern of 2^e
constexpr size_t kSbBlockBytes = sizeof(ScrubAcc) * kSbRows;

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

__device__ __forceinline__ unsigned sb_wave_sum(unsigned v)
{
    for (int d = 32; d > 0; d >>= 1) v += __shfl_down(v, d);
    return v;
}
__device__ __forceinline__ unsigned sb_wave_max(unsigned v)
{
    for (int d = 32; d > 0; d >>= 1) {
        const unsigned o = __shfl_down(v, d);
        v = o > v ? o : v;
    }
    return v;
}

// n <= 2^31 cf32 samples at `buf` (aligned to a sample): `head` samples up to the first 16-byte boundary, nvec 16-byte
// pieces, the rest.  COUNT false: nothing is counted, acc is not touched.
template <bool COUNT>
__global__ __launch_bounds__(kSbNT) void scrub_kernel(void *__restrict__ buf, long long n, long long head, long long nvec,
                                                      unsigned limit_bits, ScrubAcc *__restrict__ acc)
{
    const long long gid = (long long)blockIdx.x * kSbNT + threadIdx.x, stride = (long long)gridDim.x * kSbNT;
    unsigned char *const bytes = static_cast<unsigned char *>(buf);
    uint4 *const pieces = reinterpret_cast<uint4 *>(bytes + head * 8);
    SbLane a;
    a.zeroed = a.nonfinite = a.over = a.first_key = a.last_key = 0u;
    for (long long i = gid; i < nvec; i += stride) {
        uint4 v = pieces[i];
        const unsigned idx = (unsigned)(head + 2 * i);
        const bool b0 = sb_take(a, v.x, v.y, limit_bits, idx);
        const bool b1 = sb_take(a, v.z, v.w, limit_bits, idx + 1u);
        if (b0 || b1) {
            if (b0) v.x = v.y = 0u;
            if (b1) v.z = v.w = 0u;
            pieces[i] = v;
        }
    }
    // the scalar head and tail: at most one sample each, one per thread
    const long long tail0 = head + nvec * 2;
    long long si = -1;
    if (gid < head) si = gid;
    else if (gid - head < n - tail0) si = tail0 + (gid - head);
    if (si >= 0) {
        unsigned *q = reinterpret_cast<unsigned *>(bytes + si * 8);
        if (sb_take(a, q[0], q[1], limit_bits, (unsigned)si)) {
            q[0] = 0u;
            q[1] = 0u;
        }
    }
    if (!COUNT) return;
    const unsigned z = sb_wave_sum(a.zeroed), nf = sb_wave_sum(a.nonfinite), ov = sb_wave_sum(a.over);
    const unsigned fk = sb_wave_max(a.first_key), lk = sb_wave_max(a.last_key);
    acc += (blockIdx.x * (kSbNT / 64) + (threadIdx.x >> 6)) & (kSbRows - 1);
    if ((threadIdx.x & 63) == 0 && z) {
        atomicAdd(&acc->n_zeroed, (unsigned long long)z);
        if (nf) atomicAdd(&acc->n_nonfinite, (unsigned long long)nf);
        if (ov) atomicAdd(&acc->n_over, (unsigned long long)ov);
        atomicMax(&acc->first_key, fk);
        atomicMax(&acc->last_key, lk);
    }
}

// ---- host side ----

// One launch over n <= kSbMaxLaunch cf32 samples at d_buf (aligned to a sample) on `stream`; the block d_acc (kSbBlockBytes,
// zero; or nullptr: no counting) takes the figures.  0, or -1 for a pointer that is not aligned to a sample, a limit outside 0 .. 127, too many
// samples or a launch that failed; n == 0 launches nothing.
static inline int launch_scrub(void *d_buf, size_t n, int limit_log2, ScrubAcc *d_acc, hipStream_t stream)
{
    if (limit_log2 < 0 || limit_log2 > 127 || n > kSbMaxLaunch || (reinterpret_cast<uintptr_t>(d_buf) % 8u) != 0) return -1;
    if (n == 0) return 0;
    const size_t mis = (size_t)(reinterpret_cast<uintptr_t>(d_buf) & 15u);
    long long head = mis ? 1 : 0;
    if (head > (long long)n) head = (long long)n;
    const long long nvec = ((long long)n - head) / 2;
    const long long want = (nvec + kSbNT - 1) / kSbNT;
    const int grid = (int)(want < 1 ? 1 : (want > kSbMaxGrid ? kSbMaxGrid : want));
    static_assert(kSbNT >= 2, "the first workgroup holds the scalar head and tail");
    if (d_acc)
        hipLaunchKernelGGL((scrub_kernel<true>), dim3(grid), dim3(kSbNT), 0, stream, d_buf, (long long)n, head, nvec,
                           scrub_limit_bits(limit_log2), d_acc);
    else
        hipLaunchKernelGGL((scrub_kernel<false>), dim3(grid), dim3(kSbNT), 0, stream, d_buf, (long long)n, head, nvec,
                           scrub_limit_bits(limit_log2), d_acc);
    return hipGetLastError() == hipSuccess ? 0 : -1;
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

// The pass of a context or a front end.  Configuration: the switch and the limit.  Cache: kSbSlots blocks on the device
// with their pinned copies, allocated when the switch is first set.
struct ScrubPass {
    int on = 0, limit_log2 = kSbDefaultLog2;
    ScrubAcc *d_acc[kSbSlots] = {}, *h_acc[kSbSlots] = {};
    hipEvent_t ev[kSbSlots] = {};
};
// Stream state: the totals, and the launches whose figures have not been folded yet, oldest first.
struct ScrubStream {
    ScrubRun run;
    struct Pending { int slot; uint64_t base; size_t n; };
    std::deque<Pending> pending;
    uint64_t launches = 0;
};

static inline void scrub_pass_free(ScrubPass &ps)
{
    for (int i = 0; i < kSbSlots; i++) {
        if (ps.d_acc[i]) (void)hipFree(ps.d_acc[i]);
        if (ps.h_acc[i]) (void)hipHostFree(ps.h_acc[i]);
        if (ps.ev[i]) (void)hipEventDestroy(ps.ev[i]);
    }
    ps = ScrubPass{};
}

// the blocks, when the switch is first set (the device is current)
static inline int scrub_pass_alloc(ScrubPass &ps)
{
    if (ps.ev[0]) return 0;
    bool ok = true;
    for (int i = 0; i < kSbSlots; i++) {
        ok = ok && hipMalloc(reinterpret_cast<void **>(&ps.d_acc[i]), kSbBlockBytes) == hipSuccess;
        ok = ok && hipHostMalloc(reinterpret_cast<void **>(&ps.h_acc[i]), kSbBlockBytes, hipHostMallocDefault) == hipSuccess;
        ok = ok && hipEventCreateWithFlags(&ps.ev[i], hipEventDisableTiming) == hipSuccess;
    }
    if (!ok) {
        const int on = ps.on, lim = ps.limit_log2;
        scrub_pass_free(ps);
        ps.on = on;
        ps.limit_log2 = lim;
        return -1;
    }
    return 0;
}

// every launch in flight is waited for and folded, oldest first
static inline int scrub_settle(ScrubPass &ps, ScrubStream &st, size_t keep = 0)
{
    while (st.pending.size() > keep) {
        const ScrubStream::Pending e = st.pending.front();
        if (hipEventSynchronize(ps.ev[e.slot]) != hipSuccess) return -1;
        scrub_fold(st.run, ps.h_acc[e.slot], e.base, e.n);
        st.pending.pop_front();
    }
    return 0;
}

// The n cf32 samples at d_buf, which `stream` has produced, from stream position `base`: scrubbed on `stream`, the figures
// on their way to a pinned block.  (At most kSbSlots - 1 launches stay in flight: a slot is free when it is taken again.)
static inline int scrub_enqueue(ScrubPass &ps, ScrubStream &st, void *d_buf, size_t n, uint64_t base, hipStream_t stream)
{
    for (size_t off = 0; off < n; off += kSbMaxLaunch) {
        const size_t piece = std::min(kSbMaxLaunch, n - off);
        if (scrub_settle(ps, st, kSbSlots - 1) != 0) return -1;
        const int slot = (int)(st.launches % kSbSlots);
        if (hipMemsetAsync(ps.d_acc[slot], 0, kSbBlockBytes, stream) != hipSuccess) return -1;
        if (launch_scrub(static_cast<char *>(d_buf) + off * 8, piece, ps.limit_log2, ps.d_acc[slot], stream) != 0) return -1;
        if (hipMemcpyAsync(ps.h_acc[slot], ps.d_acc[slot], kSbBlockBytes, hipMemcpyDeviceToHost, stream) != hipSuccess) return -1;
        if (hipEventRecord(ps.ev[slot], stream) != hipSuccess) return -1;
        st.pending.push_back(ScrubStream::Pending{ slot, base + off, piece });
        st.launches++;
    }
    return 0;
}

}  // namespace irdm
