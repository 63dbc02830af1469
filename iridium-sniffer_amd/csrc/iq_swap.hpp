// iq_swap.hpp -- option "swap_iq" / irdm_swap_iq_device (include/irdm_hip.h): the two components of every sample of a
// device buffer exchanged in place, for recordings whose I and Q arrive the other way round (a WAV with Q/I channels, a
// SigMF file of the other convention, a receiver whose mixer inverts the spectrum).
//
// One memory-bound pass: a pure byte permutation, no conversion (cu8 stays cu8, a NaN stays a NaN).  The component width is
// half a sample: 1 byte (ci8, cu8), 2 bytes (ci16, ci16-full, sc16q11), 4 bytes (cf32, ci32, ci32-24).
//   * a lane loads 16 bytes, permutes them and stores them to the address it loaded from: no lane reads what another
//     writes, so working in place has no hazard.  Width 1: the bytes of each 16-bit half of a dword exchanged; width 2: a
//     dword rotated by 16; width 4: the dwords of each pair renamed.
//   * the buffer need only be aligned to a sample: the span geometry of chunk_span.hpp.
// Bounds: it reads and writes the span's samples (chunk_span.hpp) and nothing else.
//
// Launched by host_chain.hpp (the host feeds of a context and a front end) and by irdm_swap_iq_device (feed.cpp).
#pragma once
#include "common.hpp"
#include "chunk_span.hpp"

namespace irdm {

template <int W>
__device__ __forceinline__ unsigned iq_swap_word(unsigned w)
{
    if (W == 1) return ((w & 0x00ff00ffu) << 8) | ((w >> 8) & 0x00ff00ffu);
    return (w << 16) | (w >> 16);
}

// the samples of 2 W bytes of span sp at `buf` (aligned to a sample)
template <int W>
__global__ __launch_bounds__(kChunkNT) void iq_swap_kernel(void *__restrict__ buf, const ChunkSpan sp)
{
    constexpr int BPS = 2 * W, SPV = 16 / BPS;
    const ChunkLane cl = chunk_lane();
    unsigned char *const bytes = static_cast<unsigned char *>(buf);
    uint4 *const pieces = reinterpret_cast<uint4 *>(bytes + sp.head * BPS);
    for (long long i = cl.gid; i < sp.nvec; i += cl.stride) {
        uint4 v = pieces[i];
        if (W == 4) {
            v = make_uint4(v.y, v.x, v.w, v.z);
        } else {
            v.x = iq_swap_word<W>(v.x);
            v.y = iq_swap_word<W>(v.y);
            v.z = iq_swap_word<W>(v.z);
            v.w = iq_swap_word<W>(v.w);
        }
        pieces[i] = v;
    }
    const long long si = cl.scalar<SPV>(sp);
    if (si < 0) return;
    if (W == 1) {
        unsigned short *q = reinterpret_cast<unsigned short *>(bytes + si * BPS);
        const unsigned w = *q;
        *q = (unsigned short)(((w & 0xffu) << 8) | (w >> 8));
    } else if (W == 2) {
        unsigned *q = reinterpret_cast<unsigned *>(bytes + si * BPS);
        *q = iq_swap_word<2>(*q);
    } else {
        unsigned *q = reinterpret_cast<unsigned *>(bytes + si * BPS);
        const unsigned a = q[0], b = q[1];
        q[0] = b;
        q[1] = a;
    }
}

// n samples of format fmt at d_buf, exchanged in place on `stream`.  0, or -1 for an unknown format, a pointer that is not
// aligned to a sample, or a launch that failed; n == 0 launches nothing.
static inline int launch_iq_swap(int fmt, void *d_buf, size_t n, hipStream_t stream)
{
    if (!fmt_valid(fmt) || (reinterpret_cast<uintptr_t>(d_buf) % (size_t)fmt_bytes(fmt)) != 0) return -1;
    if (n == 0) return 0;
    const int bps = fmt_bytes(fmt);
    int grid = 0;
    const ChunkSpan sp = chunk_span(bps, d_buf, n, kChunkNT, kChunkMaxGrid, &grid);
    switch (bps) {
    case 2: hipLaunchKernelGGL((iq_swap_kernel<1>), dim3(grid), dim3(kChunkNT), 0, stream, d_buf, sp); break;
    case 4: hipLaunchKernelGGL((iq_swap_kernel<2>), dim3(grid), dim3(kChunkNT), 0, stream, d_buf, sp); break;
    default: hipLaunchKernelGGL((iq_swap_kernel<4>), dim3(grid), dim3(kChunkNT), 0, stream, d_buf, sp); break;
    }
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace irdm
