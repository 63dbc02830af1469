// resample.hip -- K0r, the front end's rational mode: frequency shift + real low-pass + resampling by L / M (polyphase), beside
// K0 (frontend.hip) and behind the same irdm_frontend_* calls.
//
//   y[m] = sum_n P[m M + C - n L] * r[n]   (terms with 0 <= m M + C - n L < Np),   C = (Np - 1) / 2
//   r[n] = x[n] * T[(q n) mod 65536]       exactly K0's r[n]; +0 outside the stream
//
// Arithmetic contract (restated in plain C in tests/resample_model.c): per output component ONE
// accumulator, starting at +0, and one fused multiply-add per term in ASCENDING INPUT ORDER n; the zero samples outside the
// stream take part; a tap index outside [0, Np) is no term (not a multiplication by zero).  For L = 1 this is K0 at D = M.
//
// Shape.  Output m = L p + r (period p, phase r) reads the inputs p M + nlo(r) .. p M + a(r), a(r) = floor((r M + C) / L),
// nlo(r) = floor((r M + C - Np) / L) + 1, with the taps P[r M + C - (n - p M) L]: they depend on the phase alone.  A tile is
// `nper` whole periods, so it starts at a multiple of L.  Its (nper - 1) M + a(L - 1) - nlo(0) + 1 input samples are
// converted and rotated ONCE into LDS, by K0's load stage (fe_stage.hpp).  A lane owns R consecutive outputs of ONE period -- a phase
// block -- and the 64 lanes of a wavefront own the same phase block of 64 consecutive periods: in step i every lane
// multiplies by the SAME taps, read as one aligned 8-dword scalar load per step from the block's table (host-laid,
// resample_plan), and lane l's window starts l M samples further on.  A sample read from LDS goes into up to R accumulator
// pairs (R v_pk_fma_f32).  A row of M staged samples is followed by one pad sample when M is even, so that the lane stride
// is odd and the 64 reads of an instruction fall into different banks; the step's offset in a lane's window, pad samples
// counted, is wave-uniform and comes from the block's table as well.  The steps at either end of a block's window, where
// only some of the R outputs take part, go by a per-step mask from the table (wave-uniform branches; a tap index outside
// the prototype is no term, so they cannot run as multiplications by zero).  The wavefronts of a workgroup take the units
// (64 periods x one phase block) in turn.  Finished outputs go to a second LDS region and from there to consecutive stores.
// R is the one of 5 .. 8 that leaves the workgroup's four wavefronts the least to do: the units -- groups of 64 periods
// times ceil(L / R) phase blocks -- go round the wavefronts, so the tap stage takes ceil(units / 4) rounds of R
// multiply-adds per step (L = 25 with one group: R = 7 makes 4 units, one round; R = 5 made 5 units, two rounds with
// three wavefronts idle in the second).
//
// Bounds: every global read of the capture is the load stage's (fe_stage.hpp: zero outside [tail | chunk], or a tile that
// its test finds wholly inside the chunk); every global write is guarded by m0 <= m < m1.  LDS: the host computes
// the same expressions (resample_plan, resample_lds_bytes); a lane beyond the tile's periods works on period 0's samples
// and stores nothing.
#include "common.hpp"
#include "types.hpp"
#include "kernels.hpp"
#include "fe_stage.hpp"

namespace irdm {

constexpr int kRsNT = 256;            // threads per workgroup (4 wavefronts)
constexpr int kRsU = 4;               // steps per block of the tap loop, at most

#if defined(IRDM_HIP_EMULATED)
static inline int rs_uniform(int v) { return v; }
#else
__device__ __forceinline__ int rs_uniform(int v) { return __builtin_amdgcn_readfirstlane(v); }
#endif

// descriptor of a phase block (kRsDesc ints): 0 S steps, 1 / 2 the steps [f0, f1) in which every phase of the block takes
// part, 3 r0, 4 rb phases, 5 / 6 / 7 offsets (dwords) into G of the block's tap rows (kRsRow floats per step), its LDS
// offsets (one int per step: the step's sample in a lane's window, pad samples counted) and its masks (one int per step: bit
// rr set where phase r0 + rr takes part).  Each of the three runs 2 kRsU steps past S (zero taps, the last offset, no
// phase) so that the tap loop requests ahead without a test.
bool resample_plan(int L, int M, const float *taps, int ntaps, ResampleGeom *g, std::vector<int> *desc, std::vector<float> *G)
{
    if (L < 2 || M < 2 || ntaps < 1 || !(ntaps & 1)) return false;
    const long long Np = ntaps, C = (Np - 1) / 2;
    auto a_of = [&](int r) { return (int)fe_fdiv((long long)r * M + C, L); };
    auto nlo_of = [&](int r) { return (int)fe_fdiv((long long)r * M + C - Np, L) + 1; };
    g->L = L;
    g->M = M;
    g->lo_min = nlo_of(0);
    g->pad = (M & 1) ? 0 : 1;
    g->magic = g->pad ? (unsigned)(0x100000000ull / (unsigned)M) + 1u : 0u;
    g->p_first = 0;
    const int span = a_of(L - 1) - g->lo_min + 1;
    // periods per tile: as many as fit 72 KB (two workgroups per CU) in whole wavefronts; failing that, what fits 144 KB
    auto bytes = [&](int nper) {
        const long long cnt = (long long)(nper - 1) * M + span;
        return (cnt + cnt / M + 2 + (long long)nper * L) * 8;
    };
    int nper = 0;
    for (int n = 256; n >= 64 && !nper; n -= 64)
        if (bytes(n) <= 72 * 1024) nper = n;
    if (!nper) {
        for (nper = 64; nper >= 1 && bytes(nper) > 144 * 1024; nper--) {}
        if (nper < 1) return false;
    }
    g->nper = nper;
    // outputs per lane: the fewest multiply-add rounds per wavefront; among equals the fewest padded phases, then the larger R
    int R = 0;
    long long best = 0;
    for (int r = kRsRow; r >= 5; r--) {
        const int nb = (L + r - 1) / r, units = ((nper + 63) / 64) * nb;
        const long long cost = (long long)((units + kRsNT / 64 - 1) / (kRsNT / 64)) * r * 1024 + (nb * r - L);
        if (!R || cost < best) {
            R = r;
            best = cost;
        }
    }
    g->R = R;
    g->nblk = (L + R - 1) / R;
    g->cnt = (nper - 1) * M + span;
    g->out_off = g->cnt + g->cnt / M + 2;
    desc->assign((size_t)g->nblk * kRsDesc, 0);
    G->clear();
    for (int b = 0; b < g->nblk; b++) {
        const int r0 = b * R, rb = std::min(R, L - r0);
        const int lo = nlo_of(r0), hi = a_of(r0 + rb - 1), S = hi - lo + 1;
        const int f0 = nlo_of(r0 + rb - 1) - lo, f1 = a_of(r0) - lo + 1;
        if (f0 > f1) return false;                   // (a phase's taps shorter than the block's spread: not with these designs)
        int *d = desc->data() + (size_t)b * kRsDesc;
        const int o = lo - g->lo_min, SP = S + 2 * kRsU;
        d[0] = S;
        d[1] = f0;
        d[2] = f1;
        d[3] = r0;
        d[4] = rb;
        d[5] = (int)G->size();
        d[6] = d[5] + SP * kRsRow;
        d[7] = d[6] + SP;
        G->resize((size_t)d[7] + SP, 0.0f);
        float *rows = G->data() + d[5];
        int *offs = reinterpret_cast<int *>(G->data() + d[6]), *mask = reinterpret_cast<int *>(G->data() + d[7]);
        for (int i = 0; i < SP; i++) {
            const int j = o + std::min(i, S - 1);
            offs[i] = j + (g->pad ? j / M : 0);
            mask[i] = 0;
            for (int rr = 0; rr < rb && i < S; rr++) {
                const long long k = (long long)(r0 + rr) * M + C - (long long)(lo + i) * L;
                if (k >= 0 && k < Np) {
                    rows[(size_t)i * kRsRow + rr] = taps[k];
                    mask[i] |= 1 << rr;
                }
            }
            // (the steps [f0, f1) run without the mask)
            if (i >= f0 && i < f1 && mask[i] != (1 << rb) - 1) return false;
        }
    }
    return resample_lds_bytes(*g) <= 160 * 1024;
}

size_t resample_lds_bytes(const ResampleGeom &g) { return (size_t)(g.out_off + g.nper * g.L) * sizeof(float2); }

// the pad samples in front of staged sample gi: gi / M (magic 0: none)
struct rs_pad {
    unsigned magic;
    __device__ __forceinline__ int operator()(int gi) const { return (int)(((unsigned long long)(unsigned)gi * magic) >> 32); }
};

template <int R>
__global__ __launch_bounds__(kRsNT) void resample_kernel(FrontendArgs a, ResampleGeom g, const int *__restrict__ desc,
                                                         const float *__restrict__ G, const float2 *__restrict__ T,
                                                         unsigned long long *__restrict__ kclk)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char rs_lds[];
    static_assert(R <= kRsRow, "a row of the tap table holds the block's phases");
    fe_v2 *s = reinterpret_cast<fe_v2 *>(rs_lds);
    fe_v2 *so = s + g.out_off;
    const int tid = threadIdx.x;
    const int L = g.L, M = g.M, pad = g.pad;
    kclk_enter(kclk);
    const long long pt = g.p_first + (long long)blockIdx.x * g.nper;     // the tile's first period
    const long long n_start = pt * M + g.lo_min;                        // ... and its first input sample

    // ---- load stage: convert, rotate, into LDS ----
    fe_stage<kRsNT>(a, n_start, g.cnt, T, s, tid, rs_pad{ g.magic });
    __syncthreads();

    // ---- the taps: a wavefront takes the units (64 periods x one phase block) wave, wave + 4, ... ----
    const int wave = rs_uniform(tid >> 6), lane = tid & 63;
    const int nunits = ((g.nper + 63) >> 6) * g.nblk;
#pragma unroll 1
    for (int u = wave; u < nunits; u += kRsNT / 64) {
        const int grp = u / g.nblk, b = u - grp * g.nblk;
        const int *__restrict__ d = desc + b * kRsDesc;
        const int S = d[0], f0 = d[1], f1 = d[2], r0 = d[3], rb = d[4];
        const float *__restrict__ gt = G + d[5];
        const int *__restrict__ offs = reinterpret_cast<const int *>(G + d[6]);
        const int *__restrict__ mask = reinterpret_cast<const int *>(G + d[7]);
        const int pl = grp * 64 + lane;
        const bool live = pl < g.nper;
        const fe_v2 *w = s + (live ? pl : 0) * (M + pad);
        fe_v2 acc[R];
#pragma unroll
        for (int r = 0; r < R; r++) acc[r] = fe_v2{ 0.0f, 0.0f };
        // the steps at either end, where only some of the block's phases take part: [0, f0) and [f1, S)
        auto edge = [&](int i0, int i1) {
#pragma unroll 1
            for (int i = i0; i < i1; i++) {
                const fe_v2 x = w[offs[i]];
                const float *t = gt + i * kRsRow;
                const int mk = mask[i];
#pragma unroll
                for (int r = 0; r < R; r++)
                    if (mk & (1 << r)) acc[r] = fe_fma(t[r], x, acc[r]);
            }
        };
        edge(0, f0);
        // steps f0 .. f1 - 1: all the block's phases, in blocks of U steps; the next block's taps (scalar loads) and
        // samples (LDS reads) are requested before the current block's multiply-adds (K0's tap loop), the LDS offsets one
        // block earlier still.  (The requests past f1 stay inside the tables' and the window's slack and are not used.)
        int i = f0;
        {
            constexpr int U = R > 5 ? kRsU / 2 : kRsU;      // (a scalar tap takes an aligned register pair: 2 U R of them)
            float tc[U * R];
            fe_v2 xc[U];
            int oc[U];
            auto fetch = [&](float (&t)[U * R], fe_v2 (&x)[U], const int (&o)[U], int at) {
                const float *gp = gt + at * kRsRow;
#pragma unroll
                for (int k = 0; k < U; k++)
#pragma unroll
                    for (int r = 0; r < R; r++) t[k * R + r] = gp[k * kRsRow + r];
#pragma unroll
                for (int k = 0; k < U; k++) x[k] = w[o[k]];
            };
#pragma unroll
            for (int k = 0; k < U; k++) oc[k] = offs[i + k];
            fetch(tc, xc, oc, i);
#pragma unroll
            for (int k = 0; k < U; k++) oc[k] = offs[i + U + k];
#pragma unroll 1
            for (; i + U <= f1; i += U) {
                float tn[U * R];
                fe_v2 xn[U];
                int on[U];
                fetch(tn, xn, oc, i + U);
#pragma unroll
                for (int k = 0; k < U; k++) on[k] = offs[i + 2 * U + k];
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int k = 0; k < U; k++)
#pragma unroll
                    for (int r = 0; r < R; r++) acc[r] = fe_fma(tc[k * R + r], xc[k], acc[r]);
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int k = 0; k < U * R; k++) tc[k] = tn[k];
#pragma unroll
                for (int k = 0; k < U; k++) {
                    xc[k] = xn[k];
                    oc[k] = on[k];
                }
            }
            // the rest of [f0, f1) is in tc / xc already
#pragma unroll
            for (int k = 0; k < U - 1; k++)
                if (i + k < f1) {
#pragma unroll
                    for (int r = 0; r < R; r++) acc[r] = fe_fma(tc[k * R + r], xc[k], acc[r]);
                }
            i = f1;
        }
        edge(f1, S);
        if (live) {
#pragma unroll
            for (int r = 0; r < R; r++)
                if (r < rb) so[pl * L + r0 + r] = acc[r];
        }
    }
    __syncthreads();

    // ---- consecutive stores ----
    const long long mt = pt * L;
    const int n_tile = g.nper * L;
    for (int o = tid; o < n_tile; o += kRsNT) {
        const long long m = mt + o;
        if (m >= a.m0 && m < a.m1) {
            const fe_v2 y = so[o];
            a.out[m - a.m0] = make_float2(y.x, y.y);
        }
    }
    kclk_leave(kclk);
}

template <int R>
static int launch_resample_r(const ResampleGeom &g, const FrontendArgs &a, const int *desc, const float *G, const float2 *T,
                             hipStream_t stream, unsigned long long *kclk, long long tiles)
{
    const size_t lds = resample_lds_bytes(g);
    if (!fe_raise_lds<&resample_kernel<R>>()) return -1;
    hipLaunchKernelGGL((resample_kernel<R>), dim3((unsigned)tiles), dim3(kRsNT), lds, stream, a, g, desc, G, T, kclk);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

int launch_resample(const ResampleGeom &g0, const FrontendArgs &a, const int *desc, const float *G, const float2 *T,
                    hipStream_t stream, unsigned long long *kclk)
{
    if (!fmt_valid(a.fmt) || a.m1 < a.m0 || a.m0 < 0 || a.pos0 < 0 || g0.L < 2 || g0.M < 2 || g0.nper < 1) return -1;
    if (a.m1 == a.m0) return 0;
    if (resample_lds_bytes(g0) > 160 * 1024) return -1;
    ResampleGeom g = g0;
    g.p_first = a.m0 / g.L;
    const long long periods = (a.m1 - 1) / g.L - g.p_first + 1;
    const long long tiles = (periods + g.nper - 1) / g.nper;
    if (tiles > 0x7fffffffll) return -1;
    switch (g.R) {
    case 5: return launch_resample_r<5>(g, a, desc, G, T, stream, kclk, tiles);
    case 6: return launch_resample_r<6>(g, a, desc, G, T, stream, kclk, tiles);
    case 7: return launch_resample_r<7>(g, a, desc, G, T, stream, kclk, tiles);
    case 8: return launch_resample_r<8>(g, a, desc, G, T, stream, kclk, tiles);
    default: return -1;
    }
}

}  // namespace irdm
