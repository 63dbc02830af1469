// iq_balance.hpp -- irdm_iq_balance / irdm_frontend_iq_balance / irdm_iq_balance_device (include/irdm_hip.h): the
// correction of a receiver's I/Q imbalance.  n samples of any device format at `src` become cf32 at `dst`:
//     i' = i,   q' = alpha * i + beta * q,   alpha = -tan(phi), beta = 1 / (g cos(phi))
// for a Q arm with gain g and phase error phi against the I arm (what option "iq_moments" measures).  i and q are
// converted as load_iq<FMT> converts them (iq_piece.hpp); i' keeps i's bits; q' is two rounded binary32 products and one
// rounded sum, __fadd_rn(__fmul_rn(alpha, i), __fmul_rn(beta, q)) -- never a fused operation, whatever the compiler's
// contraction setting -- so plain float32 numpy (tests/balance_model.py) gives the same bits, NaN, Inf, -0.0 and subnormal
// results included.  (With alpha = +-0, beta = 1 every sample keeps its value; a Q of -0.0 may come out as +0.0.)
//
// One pass that reads b_in and writes 8 bytes per sample:
//   * a lane loads 16 bytes of src (8 / 4 / 2 samples), which become 64 / 32 / 16 bytes of dst, written in 16-byte stores
//     where the destination of the first piece lies on a 16-byte boundary, in 8-byte stores otherwise.  For the 2- and
//     4-byte formats the wavefront turns its 64 pieces through LDS first, so that each of its store instructions writes
//     1 KiB of consecutive bytes (straight from the lanes the ci8 pass took 226 us per 64 Mi samples where a copy of the
//     same bytes takes 124);
//   * the span geometry of chunk_span.hpp on src, at most kChunkMaxLaunch samples per launch.
// In place (dst == src) for the 8-byte formats: a lane has read its piece before it writes it and reads no other lane's.
// Bounds: it reads the samples of src's span (chunk_span.hpp) and writes the same sample indices of dst: the vector part
// dst samples [head, head + nvec * spv), the scalar part [0, head) and [head + nvec * spv, n).
//
// Included by the translation units that launch it (feed.cpp: irdm_feed_host of a context and irdm_iq_balance_device;
// frontend.cpp: the capture in front of K0 / K0r).
#pragma once
#include <math.h>
#include "common.hpp"
#include "chunk_span.hpp"
#include "iq_piece.hpp"

#if !defined(__HIP__)
// (a host compiler: the CPU emulation of the tests.  One rounding each, as the device intrinsics)
static inline float __fmul_rn(float a, float b) { volatile float p = a * b; return p; }
static inline float __fadd_rn(float a, float b) { volatile float s = a + b; return s; }
#endif

namespace irdm {

constexpr double kIbMaxGainDb = 6.0, kIbMaxPhaseDeg = 30.0;
// what those limits allow: |alpha| <= tan 30, 10^-0.3 <= beta <= 10^0.3 / cos 30 (the floats just outside)
constexpr float kIbMaxAlpha = 0.5773504f, kIbMinBeta = 0.5011872f, kIbMaxBeta = 2.303931f;

// alpha, beta for a Q arm that is gain_db above the I arm and phase_deg off quadrature: binary64, rounded once to float.
// -1 outside |gain_db| <= 6, |phase_deg| <= 30 (a NaN included).
static inline int iq_balance_coeffs(double gain_db, double phase_deg, float *alpha, float *beta)
{
    if (!(fabs(gain_db) <= kIbMaxGainDb) || !(fabs(phase_deg) <= kIbMaxPhaseDeg)) return -1;
    const double g = pow(10.0, gain_db / 20.0), phi = phase_deg * (M_PI / 180.0);
    if (alpha) *alpha = (float)(-tan(phi));
    if (beta) *beta = (float)(1.0 / (g * cos(phi)));
    return 0;
}
static inline bool iq_balance_coeffs_ok(float alpha, float beta)
{
    return fabsf(alpha) <= kIbMaxAlpha && beta >= kIbMinBeta && beta <= kIbMaxBeta;     // (a NaN fails)
}

__device__ __forceinline__ unsigned ib_q(unsigned i_bits, unsigned q_bits, float alpha, float beta)
{
    return __float_as_uint(__fadd_rn(__fmul_rn(alpha, __uint_as_float(i_bits)), __fmul_rn(beta, __uint_as_float(q_bits))));
}

// The samples of FMT of span sp at `src` (aligned to a sample) to cf32 at `dst` (aligned to 8 bytes).  dst16: dst + head
// samples lies on a 16-byte boundary.  (No __restrict__: dst may be src.)
template <int FMT>
__global__ __launch_bounds__(kChunkNT) void iq_balance_kernel(void *dst, const void *src, const ChunkSpan sp, float alpha, float beta,
                                                              int dst16)
{
    constexpr int BPS = kFmtBytes<FMT>, SPV = 16 / BPS;
    const ChunkLane cl = chunk_lane();
    const long long gid = cl.gid, stride = cl.stride, head = sp.head, nvec = sp.nvec;
    const unsigned char *const bytes = static_cast<const unsigned char *>(src);
    const uint4 *const pieces = reinterpret_cast<const uint4 *>(bytes + head * BPS);
    unsigned *const out = static_cast<unsigned *>(dst);
    if constexpr (BPS < 8) {
        // A lane's piece becomes QPL > 1 16-byte pieces of output, 16 QPL bytes apart from its neighbour's: stored straight from
        // the lane, every store instruction of the wavefront would touch 64 scattered quarters or halves of cache lines.  The
        // wavefront's 64 pieces are therefore turned through its own LDS block, and store j of lane k writes piece
        // 64 j + k of the wavefront's contiguous 1024 QPL bytes.  The trip count is the wavefront's, not the lane's: every
        // lane reaches both wavefront barriers.  (Slot s of lane k sits at k QPL + (s ^ k % QPL): the 8 lanes a b128 write
        // serves at once then cover all banks.)
        constexpr int QPL = SPV / 2;
        __shared__ uint4 sh[kChunkNT * QPL];
        const int lane = threadIdx.x & 63;
        uint4 *const mine = sh + (threadIdx.x >> 6) * 64 * QPL;
        for (long long b = gid - lane; dst16 && b < nvec; b += stride) {
            const long long i = b + lane;
            if (i < nvec) {
                unsigned o[2 * SPV];
                iq_piece_bits<FMT>(pieces[i], o);
#pragma unroll
                for (int k = 0; k < SPV; k++) o[2 * k + 1] = ib_q(o[2 * k], o[2 * k + 1], alpha, beta);
#pragma unroll
                for (int s = 0; s < QPL; s++)
                    mine[lane * QPL + (s ^ (lane & (QPL - 1)))] = make_uint4(o[4 * s], o[4 * s + 1], o[4 * s + 2], o[4 * s + 3]);
            }
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            __builtin_amdgcn_wave_barrier();
            uint4 *const q = reinterpret_cast<uint4 *>(out + 2 * (head + b * SPV));
            const long long left = nvec - b;
            const int live = (int)(left < 64 ? left : 64) * QPL;            // 16-byte pieces of this block that exist
#pragma unroll
            for (int j = 0; j < QPL; j++) {
                const int idx = j * 64 + lane, k = idx / QPL, s = idx % QPL;
                if (idx < live) q[idx] = mine[k * QPL + (s ^ (k & (QPL - 1)))];
            }
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            __builtin_amdgcn_wave_barrier();
        }
    }
    for (long long i = gid; (BPS == 8 || !dst16) && i < nvec; i += stride) {
        unsigned o[2 * SPV];
        iq_piece_bits<FMT>(pieces[i], o);
#pragma unroll
        for (int k = 0; k < SPV; k++) o[2 * k + 1] = ib_q(o[2 * k], o[2 * k + 1], alpha, beta);
        unsigned *q = out + 2 * (head + i * SPV);
        if (dst16) {
#pragma unroll
            for (int k = 0; k < SPV / 2; k++)
                reinterpret_cast<uint4 *>(q)[k] = make_uint4(o[4 * k], o[4 * k + 1], o[4 * k + 2], o[4 * k + 3]);
        } else {
#pragma unroll
            for (int k = 0; k < SPV; k++) reinterpret_cast<uint2 *>(q)[k] = uint2{ o[2 * k], o[2 * k + 1] };
        }
    }
    const long long si = cl.scalar<SPV>(sp);
    if (si < 0) return;
    unsigned o[2];
    iq_sample_bits<FMT>(bytes + si * BPS, o);
    reinterpret_cast<uint2 *>(out)[si] = uint2{ o[0], ib_q(o[0], o[1], alpha, beta) };
}

// n samples of format fmt at d_in to cf32 at d_out on `stream`, in launches of at most kChunkMaxLaunch samples.  0, or -1 for
// an unknown format, d_in not aligned to a sample or d_out not to 8 bytes, coefficients outside the limits, buffers that
// overlap (other than d_out == d_in with an 8-byte format) or a launch that failed; n == 0 launches nothing.
static inline int launch_iq_balance(int fmt, void *d_out, const void *d_in, size_t n, float alpha, float beta, hipStream_t stream)
{
    if (!fmt_valid(fmt) || !iq_balance_coeffs_ok(alpha, beta)) return -1;
    const uintptr_t a_in = reinterpret_cast<uintptr_t>(d_in), a_out = reinterpret_cast<uintptr_t>(d_out);
    const size_t bps = (size_t)fmt_bytes(fmt);
    if (a_in % bps != 0 || a_out % 8u != 0) return -1;
    if (n == 0) return 0;
    if (!(a_out == a_in && bps == 8) && a_in < a_out + n * 8 && a_out < a_in + n * bps) return -1;
    for (size_t off = 0; off < n; off += kChunkMaxLaunch) {
        const size_t piece = n - off < kChunkMaxLaunch ? n - off : kChunkMaxLaunch;
        const void *in = static_cast<const char *>(d_in) + off * bps;
        void *out = static_cast<char *>(d_out) + off * 8;
        int grid = 0;
        const ChunkSpan sp = chunk_span((int)bps, in, piece, kChunkNT, kChunkMaxGrid, &grid);
        const int dst16 = ((reinterpret_cast<uintptr_t>(out) + (uintptr_t)sp.head * 8u) & 15u) == 0 ? 1 : 0;
        fmt_dispatch(fmt, [&](auto f) {
            hipLaunchKernelGGL((iq_balance_kernel<decltype(f)::value>), dim3(grid), dim3(kChunkNT), 0, stream, out, in, sp, alpha, beta, dst16);
        });
        if (hipGetLastError() != hipSuccess) return -1;
    }
    return 0;
}

// irdm_iq_balance / irdm_frontend_iq_balance: the setting (configuration: it survives a reset; host_chain.hpp)
struct IqBalance {
    int on = 0, wire_fmt = 2;
    float alpha = 0.0f, beta = 1.0f;
};

}  // namespace irdm
