// resample_wide.hip -- K0w, the front end's rational mode at the ratios K0r's shape (resample.hip) does not fit: L up to
// 4096, M up to 65536.  The same function, behind the same irdm_frontend_* calls:
//
//   y[m] = sum_n P[m M + C - n L] * r[n]   (terms with 0 <= m M + C - n L < Np),   C = (Np - 1) / 2
//   r[n] = x[n] * T[(q n) mod 65536]       exactly K0's r[n]; +0 outside the stream
//
// and the same arithmetic contract (tests/resample_model.c): per output component ONE accumulator,
// starting at +0, and one fused multiply-add per term in ASCENDING INPUT ORDER n; the zero samples outside the stream take
// part; a tap index outside [0, Np) is no term (not a multiplication by zero).
//
// Shape.  K0r stages whole periods of M inputs and gives a wavefront one scalar tap row per phase block; at L in the
// hundreds a period no longer fits LDS and most lanes of that shape idle.  Here a tile is a run of B CONSECUTIVE outputs,
// wherever the periods fall, and a lane owns whole outputs: output mt + o of the tile that starts at mt belongs to thread
// o mod 256, so the 64 lanes of a wavefront work on 64 consecutive outputs.  Write m = L p + r.  Output m reads the
// inputs p M + nlo(r) + i, i = 0 .. S(r) - 1, nlo(r) = floor((r M + C - Np) / L) + 1, with the taps
// P[r M + C - (nlo(r) + i) L]: window start and taps depend on the phase alone, and every index that depends on p is
// formed once per tile in 64 bits.  The tile's inputs -- from the first input of its first output to the last of its last,
// at most floor(((B - 1) M + Np) / L) + 1 samples -- are converted and rotated ONCE into LDS, by K0's load stage (fe_stage.hpp).
// The prototype lies in memory as W[step i][phase r] (host-laid, resample_wide_plan): since gcd(L, M) = 1 consecutive
// outputs have consecutive phases, so in step i the lanes of a wavefront load consecutive floats (up to the wrap of
// m mod L, where the row starts again), and their LDS reads lie about M / L samples apart.  Where that stride, rounded, is
// even, a pad sample follows every `stride` staged samples so that the lane stride in LDS is odd.  The table is as large
// as the prototype (70 KB at 400/401, 0.7 MB at 4000/4001) and is read from L2.
//
// S(r) is S = ceil(Np / L) or S - 1.  The steps 0 .. S - 2 are terms of every output; step S - 1 is a term where the
// phase's tap index there is still >= 0 -- a per-lane predicate, not a multiplication by zero.  The tap loop runs in
// blocks of kRwU steps; the next block's taps (vector loads) and samples (LDS reads) are requested before the current
// block's multiply-adds, as K0r's loop does.
//
// Bounds: every global read of the capture is the load stage's (fe_stage.hpp: zero outside [tail | chunk], or a tile that
// its test finds wholly inside the chunk); every global write is guarded by o < nout, that is m < m1.  The requests that run
// ahead of the last step stay inside the slack of 2 kRwU rows behind W and of 2 kRwU + 2 samples behind the staged window
// (resample_wide_plan, resample_wide_lds_bytes) and are not used.
#include "common.hpp"
#include "types.hpp"
#include "kernels.hpp"
#include "fe_stage.hpp"

namespace irdm {

constexpr int kRwNT = 256;            // threads per workgroup (4 wavefronts)

// staged samples -> LDS samples, pad samples counted
static inline long long rw_slots(int pad_s, long long n) { return n + (pad_s ? n / pad_s : 0); }

size_t resample_wide_lds_bytes(const WideGeom &g)
{
    return (size_t)rw_slots(g.pad_s, (long long)g.cnt_max + 2 * kRwU + 2) * sizeof(float2);
}

bool resample_wide_plan(int L, int M, const float *taps, int ntaps, WideGeom *g, std::vector<int> *nlo, std::vector<float> *W)
{
    if (L < 2 || L > 4096 || M < 2 || M > 65536 || ntaps < 1 || !(ntaps & 1) || ntaps > kRwMaxTaps) return false;
    const long long Np = ntaps, C = (Np - 1) / 2;
    g->L = L;
    g->M = M;
    g->C = (int)C;
    g->S = (int)((Np + L - 1) / L);
    // the lane stride in the staged window, rounded: even -> one pad sample per stride
    const int stride = (2 * M + L) / (2 * L);
    g->pad_s = stride >= 2 && !(stride & 1) ? stride : 0;
    g->magic = g->pad_s ? (unsigned)(0x100000000ull / (unsigned)g->pad_s) + 1u : 0u;
    // outputs per tile: the most that leave a CU four workgroups (36 KB each); failing that 256 outputs at two or one
    g->B = 0;
    for (int B = 2048; B >= 256 && !g->B; B >>= 1) {
        g->cnt_max = (int)(((long long)(B - 1) * M + Np) / L + 1);
        if (resample_wide_lds_bytes(*g) <= 36 * 1024) {
            g->B = B;
            g->wg_per_cu = 4;
        }
    }
    if (!g->B) {
        const size_t b = resample_wide_lds_bytes(*g);       // (at 256 outputs)
        if (b > 160 * 1024) return false;
        g->B = 256;
        g->wg_per_cu = b <= 72 * 1024 ? 2 : 1;
    }
    nlo->resize(L);
    W->assign((size_t)(g->S + 2 * kRwU) * L, 0.0f);
    for (int r = 0; r < L; r++) {
        const long long lo = fe_fdiv((long long)r * M + C - Np, L) + 1;
        (*nlo)[r] = (int)lo;
        for (int i = 0; i < g->S; i++) {
            const long long k = (long long)r * M + C - (lo + i) * L;
            if (k >= Np || (k < 0 && i < g->S - 1)) return false;        // (the first S - 1 steps are terms of every phase)
            if (k >= 0) (*W)[(size_t)i * L + r] = taps[k];
        }
    }
    return true;
}

// the pad samples in front of staged sample gi; staged index -> LDS index
template <bool PAD>
__device__ __forceinline__ int rw_pad(const WideGeom &g, int gi)
{
    return PAD ? (int)(((unsigned long long)(unsigned)gi * g.magic) >> 32) : 0;
}
template <bool PAD>
__device__ __forceinline__ int rw_slot(const WideGeom &g, int gi)
{
    return gi + rw_pad<PAD>(g, gi);
}

template <bool PAD>
__global__ __launch_bounds__(kRwNT) void resample_wide_kernel(FrontendArgs a, WideGeom g, const int *__restrict__ nlo,
                                                              const float *__restrict__ W, const float2 *__restrict__ T,
                                                              unsigned long long *__restrict__ kclk)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char rw_lds[];
    fe_v2 *s = reinterpret_cast<fe_v2 *>(rw_lds);
    const int tid = threadIdx.x;
    const int L = g.L, M = g.M, S = g.S;
    kclk_enter(kclk);
    const long long mt = a.m0 + (long long)blockIdx.x * g.B;            // the tile's first output
    const int nout = a.m1 - mt < g.B ? (int)(a.m1 - mt) : g.B;          // ... and how many it has
    const long long pt = mt / L;
    const int rt = (int)(mt - pt * L);
    const int lo_t = nlo[rt];
    const long long n_start = pt * M + lo_t;                            // the tile's first input sample
    // ... to the last input of its last output, p M + floor((r M + C) / L)
    const int rl = rt + nout - 1, dl = rl / L;
    const int span = dl * M + ((rl - dl * L) * M + g.C) / L - lo_t + 1;
    const int cnt = span < g.cnt_max ? span : g.cnt_max;                // (span <= cnt_max: see the header comment)

    // ---- load stage: convert, rotate, into LDS ----
    fe_stage<kRwNT>(a, n_start, cnt, T, s, tid, [&](int gi) { return rw_pad<PAD>(g, gi); });
    __syncthreads();

    // ---- the taps: thread tid takes the outputs tid, tid + 256, ... of the tile ----
    constexpr int U = kRwU;
    const int F = S - 1;                                                // the steps [0, F) are terms of every output
#pragma unroll 1
    for (int o = tid; o < nout; o += kRwNT) {
        const int rr = rt + o, dp = rr / L, r = rr - dp * L;
        const int lo = nlo[r];
        const int w0 = dp * M + lo - lo_t;                              // the output's first input, as a staged index
        const bool last = r * M + g.C - (lo + F) * L >= 0;              // step F is a term: its tap index is inside the prototype
        const float *__restrict__ wp = W + r;
        fe_v2 acc = fe_v2{ 0.0f, 0.0f };
        float tc[U];
        fe_v2 xc[U];
        auto fetch = [&](float (&t)[U], fe_v2 (&x)[U], int at) {
#pragma unroll
            for (int k = 0; k < U; k++) t[k] = wp[(size_t)(at + k) * L];
#pragma unroll
            for (int k = 0; k < U; k++) x[k] = s[rw_slot<PAD>(g, w0 + at + k)];
        };
        fetch(tc, xc, 0);
        int i = 0;
#pragma unroll 1
        for (; i + U <= F; i += U) {
            float tn[U];
            fe_v2 xn[U];
            fetch(tn, xn, i + U);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int k = 0; k < U; k++) acc = fe_fma(tc[k], xc[k], acc);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int k = 0; k < U; k++) {
                tc[k] = tn[k];
                xc[k] = xn[k];
            }
        }
        // the rest of [0, F) and step F are in tc / xc already
#pragma unroll
        for (int k = 0; k < U; k++)
            if (i + k < F || (i + k == F && last)) acc = fe_fma(tc[k], xc[k], acc);
        a.out[mt - a.m0 + o] = make_float2(acc.x, acc.y);
    }
    kclk_leave(kclk);
}

template <bool PAD>
static int launch_resample_wide_p(const WideGeom &g, const FrontendArgs &a, const int *nlo, const float *W, const float2 *T,
                                  hipStream_t stream, unsigned long long *kclk, long long tiles)
{
    const size_t lds = resample_wide_lds_bytes(g);
    if (!fe_raise_lds<&resample_wide_kernel<PAD>>()) return -1;
    hipLaunchKernelGGL((resample_wide_kernel<PAD>), dim3((unsigned)tiles), dim3(kRwNT), lds, stream, a, g, nlo, W, T, kclk);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

int launch_resample_wide(const WideGeom &g, const FrontendArgs &a, const int *nlo, const float *W, const float2 *T,
                         hipStream_t stream, unsigned long long *kclk)
{
    if (!fmt_valid(a.fmt) || a.m1 < a.m0 || a.m0 < 0 || a.pos0 < 0 || g.L < 2 || g.M < 2 || g.B < 1 || g.S < 1) return -1;
    if (a.m1 == a.m0) return 0;
    if (resample_wide_lds_bytes(g) > 160 * 1024) return -1;
    const long long tiles = (a.m1 - a.m0 + g.B - 1) / g.B;
    if (tiles > 0x7fffffffll) return -1;
    return g.pad_s ? launch_resample_wide_p<true>(g, a, nlo, W, T, stream, kclk, tiles)
                   : launch_resample_wide_p<false>(g, a, nlo, W, T, stream, kclk, tiles);
}

}  // namespace irdm
