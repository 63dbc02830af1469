// resample_wide.cpp -- irdm_frontend_create_wide and irdm_frontend_create_resampler: the front end's rational mode on K0w
// (resample_wide.hip), for the ratios beyond K0r's L <= 125 and M <= 768 -- 2 <= L <= 4096, M <= 65536, 24/25 <= M / L <= 16,
// a prototype of at most 2^20 taps.  The object is irdm_frontend_create_rational's (frontend_obj.hpp, fe_new): the
// same checks, the same prototype from the same design_lpf call, so a ratio both kernels take has one set of taps and one
// output; everything behind creation is frontend.cpp's.  irdm_frontend_create_resampler picks the kernel: wherever
// irdm_frontend_create or irdm_frontend_create_rational make the object it hands over to them.
#include "frontend_obj.hpp"

namespace irdmh {

static int fe_launch_k0w(irdm_frontend *fe, const FrontendArgs &a, hipStream_t s)
{
    return launch_resample_wide(fe->wide, a, fe->d_desc, fe->d_G, fe->d_T, s, fe->d_kclk);
}

// K0w's limits on a ratio in lowest terms: 0 inside them, -1 with a message otherwise
static int wide_domain(int in_rate, int out_rate, long long L, long long M)
{
    if (L > 4096 || M > 65536) {
        fprintf(stderr, "irdm_hip: front end: %d -> %d samples/s is the ratio %lld/%lld; L <= 4096 and M <= 65536 are built\n",
                in_rate, out_rate, L, M);
        return -1;
    }
    if (L == M || 25 * M < 24 * L || M > 16 * L) {
        fprintf(stderr, "irdm_hip: front end: %d -> %d samples/s (ratio %lld/%lld): M / L must lie in 24/25 .. 16 and differ from 1\n",
                in_rate, out_rate, L, M);
        return -1;
    }
    if (L < 2) {
        fprintf(stderr, "irdm_hip: front end: %d -> %d samples/s is the integer ratio 1/%lld: that is irdm_frontend_create's\n",
                in_rate, out_rate, M);
        return -1;
    }
    return 0;
}

extern "C" int irdm_frontend_resampler_ratio(int in_rate, int out_rate, int *L_out, int *M_out, int *kernel)
{
    long long L = 0, M = 0;
    if (!fe_ratio(in_rate, out_rate, &L, &M)) return -1;
    if (L_out) *L_out = (int)L;
    if (M_out) *M_out = (int)M;
    int k = 2;
    if (L == 1 && M >= 2 && M <= 16) k = 0;
    else if (fe_rational_domain(L, M) == 0) k = 1;
    else if (wide_domain(in_rate, out_rate, L, M) != 0) return -1;
    if (kernel) *kernel = k;
    return 0;
}

// the prototype and K0w's plan for it; false with a message
static bool wide_plan(int in_rate, int out_rate, long long L, long long M, const std::vector<float> &taps, WideGeom *g,
                      std::vector<int> *nlo, std::vector<float> *W)
{
    if ((long long)taps.size() > kRwMaxTaps) {
        fprintf(stderr, "irdm_hip: front end: %d -> %d samples/s (ratio %lld/%lld) takes a prototype of %zu taps; at most %d are built\n",
                in_rate, out_rate, L, M, taps.size(), kRwMaxTaps);
        return false;
    }
    if (!resample_wide_plan((int)L, (int)M, taps.data(), (int)taps.size(), g, nlo, W)) {
        fprintf(stderr, "irdm_hip: front end: %zu taps at the ratio %lld/%lld do not fit the kernel\n", taps.size(), L, M);
        return false;
    }
    return true;
}

extern "C" irdm_frontend_t *irdm_frontend_create_wide(const irdm_frontend_rational_config_t *cfg)
{
    if (!cfg) return nullptr;
    long long L = 0, M = 0;
    if (!fe_ratio(cfg->in_rate, cfg->out_rate, &L, &M) || wide_domain(cfg->in_rate, cfg->out_rate, L, M) != 0) return nullptr;
    irdm_frontend *fe = fe_new(cfg, 0, L, M);
    if (!fe) return nullptr;
    fe->launch = fe_launch_k0w;
    std::vector<int> nlo;
    std::vector<float> W;
    if (!wide_plan(cfg->in_rate, cfg->out_rate, L, M, fe->taps, &fe->wide, &nlo, &W)) {
        delete fe;
        return nullptr;
    }
    return fe_finish(fe, &fe->d_desc, nlo, W);
}

extern "C" irdm_frontend_t *irdm_frontend_create_resampler(const irdm_frontend_rational_config_t *cfg)
{
    if (!cfg) return nullptr;
    int kernel = 0;
    if (irdm_frontend_resampler_ratio(cfg->in_rate, cfg->out_rate, nullptr, nullptr, &kernel) != 0) return nullptr;
    return kernel == 2 ? irdm_frontend_create_wide(cfg) : irdm_frontend_create_rational(cfg);
}

// K0w's launch geometry for a pair of rates, without a device
extern "C" int irdm_frontend_wide_geometry(int in_rate, int out_rate, int *ntaps, int *tile_outputs, int *lds_bytes, int *workgroups_per_cu)
{
    long long L = 0, M = 0;
    if (!fe_ratio(in_rate, out_rate, &L, &M) || wide_domain(in_rate, out_rate, L, M) != 0) return -1;
    const std::vector<float> taps = fe_resample_taps(in_rate, out_rate, L);
    WideGeom g{};
    std::vector<int> nlo;
    std::vector<float> W;
    if (!wide_plan(in_rate, out_rate, L, M, taps, &g, &nlo, &W)) return -1;
    if (ntaps) *ntaps = (int)taps.size();
    if (tile_outputs) *tile_outputs = g.B;
    if (lds_bytes) *lds_bytes = (int)resample_wide_lds_bytes(g);
    if (workgroups_per_cu) *workgroups_per_cu = g.wg_per_cu;
    return 0;
}

}  // namespace irdmh
