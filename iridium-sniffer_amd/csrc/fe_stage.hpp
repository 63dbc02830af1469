// fe_stage.hpp -- the load stage of the front end's three kernels, K0 (frontend.hip), K0r (resample.hip) and K0w
// (resample_wide.hip): a tile's `cnt` input samples from stream position n_start on are converted as load_iq converts them,
// rotated -- r[n] = cmul(x[n], T[(q n) mod 65536]), +0 + 0i outside the stream -- and written ONCE into LDS.  This is the
// only place a front-end kernel reads the capture.  The one thing a kernel supplies is `pad`: the pad samples its LDS layout
// has in front of staged sample g, which goes to slot g + pad(g).  (pad(g), not the slot itself: the sum is formed here, next
// to the index g + u NT it is formed from, which is where K0's compile-time row length folds into store offsets.)
//
// Bounds: a tile wholly inside the chunk is read without a test per sample -- the test in fe_stage covers the indices
// v0 .. v0 + cnt - 1 and the loops form no other; every other tile goes through fe_load, which returns zero for a position
// outside [tail | chunk].  The LDS writes are the slots of g = 0 .. cnt - 1: the kernel's *_lds_bytes function sizes them.
#pragma once
#include "common.hpp"
#include "types.hpp"
#include "kernels.hpp"

namespace irdm {

// a pair of fused multiply-adds with a common factor (v_pk_fma_f32)
#if defined(IRDM_HIP_EMULATED)
struct fe_v2 { float x, y; };
static inline fe_v2 fe_fma(float t, fe_v2 s, fe_v2 a) { return fe_v2{ fmaf(t, s.x, a.x), fmaf(t, s.y, a.y) }; }
#else
typedef float fe_v2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ fe_v2 fe_fma(float t, fe_v2 s, fe_v2 a) { return __builtin_elementwise_fma(fe_v2{ t, t }, s, a); }
#endif

// floor(a / b), b > 0 (the planners)
static inline long long fe_fdiv(long long a, long long b) { return a >= 0 ? a / b : -((-a + b - 1) / b); }

// K0r's and K0w's launchers: the kernel may be given up to 160 KB of dynamic LDS (once per instantiation and device: the
// most it is ever given)
template <auto Kernel>
static bool fe_raise_lds()
{
    static bool raised[64];
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return false;
    if (!raised[dev]) {
        if (hipFuncSetAttribute(reinterpret_cast<const void *>(Kernel), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024) !=
            hipSuccess)
            return false;
        raised[dev] = true;
    }
    return true;
}

// the rotation table's entry for stream position n: (q n) mod 65536
__device__ __forceinline__ unsigned fe_rot(const FrontendArgs &a, long long n)
{
    return (a.q16 * (unsigned)((unsigned long long)n & 0xffffull)) & 0xffffu;
}

// stream position n -> the rotated sample r[n]
__device__ __forceinline__ float2 fe_load(const FrontendArgs &a, long long n, const float2 *__restrict__ T)
{
    const long long v = n - a.pos0;
    if (n < 0 || v < 0 || v >= a.n_tail + a.n_in) return make_float2(0.0f, 0.0f);
    const float2 x = v < a.n_tail ? load_iq(a.fmt, a.tail, (size_t)v) : load_iq(a.fmt, a.in, (size_t)(v - a.n_tail));
    return cmul(x, T[fe_rot(a, n)]);
}

// The load stage of a tile that lies wholly inside the chunk (all but the first and last tiles of a launch): no bounds, one
// format, eight samples and their table entries requested before the first is used -- a lane's loads are otherwise
// issued and waited for one at a time, and with one or two wavefronts per SIMD nothing hides them (measured with K0 at
// D = 5: the kernel's span 4.0 ms per 64 Mi outputs with the general loop alone).  The same operations on the same operands.
template <int FMT, int NT, typename Pad>
__device__ __forceinline__ void fe_stage_inside(const FrontendArgs &a, long long v0, long long n_start, int cnt,
                                                const float2 *__restrict__ T, fe_v2 *s, int tid, Pad pad)
{
    constexpr int U = 8;
    int g = tid;
    for (; g + (U - 1) * NT < cnt; g += U * NT) {
        float2 x[U], t[U];
#pragma unroll
        for (int u = 0; u < U; u++) {
            const int gu = g + u * NT;
            x[u] = load_iq<FMT>(a.in, (size_t)(v0 + gu));
            t[u] = T[fe_rot(a, n_start + gu)];
        }
#pragma unroll
        for (int u = 0; u < U; u++) {
            const float2 r = cmul(x[u], t[u]);
            const int gu = g + u * NT;
            s[gu + pad(gu)] = fe_v2{ r.x, r.y };
        }
    }
    for (; g < cnt; g += NT) {
        const float2 x = load_iq<FMT>(a.in, (size_t)(v0 + g));
        const float2 r = cmul(x, T[fe_rot(a, n_start + g)]);
        s[g + pad(g)] = fe_v2{ r.x, r.y };
    }
}

// the load stage of a workgroup of NT lanes: staged sample g = input n_start + g, g = 0 .. cnt - 1, into s[g + pad(g)]
template <int NT, typename Pad>
__device__ __forceinline__ void fe_stage(const FrontendArgs &a, long long n_start, int cnt, const float2 *__restrict__ T, fe_v2 *s,
                                         int tid, Pad pad)
{
    const long long v0 = n_start - a.pos0 - a.n_tail;                   // the tile's first sample as an index into the chunk
    if (n_start >= 0 && v0 >= 0 && v0 + cnt <= a.n_in) {
        // (the order of the cases shapes the branch chain)
        switch (a.fmt) {
        case 2: fe_stage_inside<2, NT>(a, v0, n_start, cnt, T, s, tid, pad); break;
        case 1: fe_stage_inside<1, NT>(a, v0, n_start, cnt, T, s, tid, pad); break;
        case 3: fe_stage_inside<3, NT>(a, v0, n_start, cnt, T, s, tid, pad); break;
        case 4: fe_stage_inside<4, NT>(a, v0, n_start, cnt, T, s, tid, pad); break;
        case 6: fe_stage_inside<6, NT>(a, v0, n_start, cnt, T, s, tid, pad); break;
        case 8: fe_stage_inside<8, NT>(a, v0, n_start, cnt, T, s, tid, pad); break;
        case 9: fe_stage_inside<9, NT>(a, v0, n_start, cnt, T, s, tid, pad); break;
        default: fe_stage_inside<0, NT>(a, v0, n_start, cnt, T, s, tid, pad); break;
        }
    } else {
        for (int g = tid; g < cnt; g += NT) {
            const float2 r = fe_load(a, n_start + g, T);
            s[g + pad(g)] = fe_v2{ r.x, r.y };
        }
    }
}

}  // namespace irdm
