// chunk_span.hpp -- the geometry of a chunk pass: one memory-bound kernel over the n samples of a raw input chunk whose base
// is aligned to a sample only (input_stats.hpp, iq_moments.hpp, iq_balance.hpp, iq_swap.hpp, scrub.hpp).
//
// A lane reads 16 bytes at a time: SPV = 16 / bytes-per-sample samples.  The chunk is therefore cut into
//   * `head` samples up to the first 16-byte boundary (at most SPV - 1, at most n),
//   * nvec 16-byte pieces, which a grid-stride loop of at most kChunkMaxGrid workgroups of kChunkNT threads walks,
//   * the rest (at most SPV - 1 samples),
// and head and rest are handled one sample per thread by the first threads of the grid.
// Bounds (tests/test_chunk_span.py checks them on the host function, on which every pass relies): head + nvec * SPV <= n;
// the pieces cover bytes [head * bps, (head + nvec * SPV) * bps) from a 16-byte boundary; the scalar samples are
// [0, head) and [head + nvec * SPV, n), at most 2 * (SPV - 1) <= kChunkNT of them, so the first workgroup holds them all.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace irdm {

constexpr int kChunkNT = 256;                           // threads of a workgroup
constexpr int kChunkMaxGrid = 2048;                     // workgroups of a launch
constexpr int kChunkSlots = 4;                          // launches in flight per context (pass_ring.hpp)
constexpr size_t kChunkMaxLaunch = (size_t)1 << 31;     // samples of a launch: an index and a lane's 32-bit counts fit

struct ChunkSpan {
    long long n, head, nvec;
};

// the span of n samples of bps bytes (2, 4 or 8) at p, and the workgroups of nt threads (at most max_grid) of its launch
static inline ChunkSpan chunk_span(int bps, const void *p, size_t n, int nt, int max_grid, int *grid)
{
    const int spv = 16 / bps;
    const size_t mis = (size_t)(reinterpret_cast<uintptr_t>(p) & 15u);
    ChunkSpan sp;
    sp.n = (long long)n;
    sp.head = (long long)(((16 - mis) & 15u) / (size_t)bps);
    if (sp.head > sp.n) sp.head = sp.n;
    sp.nvec = (sp.n - sp.head) / spv;
    const long long want = (sp.nvec + nt - 1) / nt;
    *grid = (int)(want < 1 ? 1 : (want > max_grid ? max_grid : want));
    return sp;
}

// A thread's place in the span: its first piece and the step of the grid-stride loop over the nvec pieces, and, from
// scalar<SPV>(sp), the one sample of the scalar head or tail that is its own (-1: none).  (Asked for where the kernel
// handles that sample, in front of its loop or behind it: the index then is not kept in registers across the loop.)
struct ChunkLane {
    long long gid, stride;

    template <int SPV>
    __device__ __forceinline__ long long scalar(const ChunkSpan &sp) const
    {
        static_assert(kChunkNT >= 2 * (SPV - 1), "the first workgroup holds the scalar head and tail");
        const long long tail0 = sp.head + sp.nvec * SPV;
        if (gid < sp.head) return gid;
        return gid - sp.head < sp.n - tail0 ? tail0 + (gid - sp.head) : -1;
    }
};

__device__ __forceinline__ ChunkLane chunk_lane()
{
    return ChunkLane{ (long long)blockIdx.x * kChunkNT + threadIdx.x, (long long)gridDim.x * kChunkNT };
}

}  // namespace irdm
