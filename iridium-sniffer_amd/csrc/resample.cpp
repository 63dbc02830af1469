// resample.cpp -- irdm_frontend_create_rational: the front end's rational mode (K0r, resample.hip), output rate = input rate
// * L / M.  It makes the same object irdm_frontend_create makes, on the same maker path (frontend_obj.hpp: fe_new, fe_finish);
// everything behind creation is frontend.cpp's.  An integer ratio 2 .. 16 is handed to irdm_frontend_create: K0, bit for bit.
//
// The prototype P is the pipeline's own low-pass design at the rate L * in_rate with gain L, cut-off 0.5 f_min and
// transition parameter 0.09 f_min, f_min = min(in_rate, out_rate).  design_lpf takes the rate as a float: L * in_rate is
// formed exactly (64-bit) and converted with one rounding to nearest.  For every ratio the limits admit from a capture rate
// that is a multiple of 2^k Hz with L * in_rate / 2^k below 2^24 the conversion is exact -- all the rates the README names
// (tests/test_resample_emul.py asserts them).
#include "frontend_obj.hpp"

namespace irdmh {

static int fe_launch_k0r(irdm_frontend *fe, const FrontendArgs &a, hipStream_t s)
{
    return launch_resample(fe->geom, a, fe->d_desc, fe->d_G, fe->d_T, s, fe->d_kclk);
}

// out_rate / in_rate in lowest terms, L / M; false (message) for a rate that is not positive
bool fe_ratio(int in_rate, int out_rate, long long *L, long long *M)
{
    if (in_rate <= 0 || out_rate <= 0) {
        fprintf(stderr, "irdm_hip: front end: sample rates %d -> %d\n", in_rate, out_rate);
        return false;
    }
    long long a = in_rate, b = out_rate;
    while (b) {
        const long long t = a % b;
        a = b;
        b = t;
    }
    *L = out_rate / a;
    *M = in_rate / a;
    return true;
}

// K0r's limits on a ratio in lowest terms: 0 inside them, 1 L or M too large, 2 M / L outside 24/25 .. 16 or equal to 1
int fe_rational_domain(long long L, long long M)
{
    if (L > 125 || M > 768) return 1;
    return L == M || 25 * M < 24 * L || M > 16 * L ? 2 : 0;
}

// the ratio in lowest terms and the limits on it, for the create call and for callers that must refuse before they start
// (the binary): 0 within the limits (an integer ratio 2 .. 16 included), -1 with a message otherwise.  Needs no device.
extern "C" int irdm_frontend_rational_ratio(int in_rate, int out_rate, int *L_out, int *M_out)
{
    long long L = 0, M = 0;
    if (!fe_ratio(in_rate, out_rate, &L, &M)) return -1;
    if (L_out) *L_out = (int)L;
    if (M_out) *M_out = (int)M;
    const int where = fe_rational_domain(L, M);
    if (where == 1) {
        fprintf(stderr, "irdm_hip: front end: %d -> %d samples/s is the ratio %lld/%lld; L <= 125 and M <= 768 are built\n",
                in_rate, out_rate, L, M);
        return -1;
    }
    if (where == 2) {
        fprintf(stderr, "irdm_hip: front end: %d -> %d samples/s (ratio %lld/%lld): M / L must lie in 24/25 .. 16 and differ from 1\n",
                in_rate, out_rate, L, M);
        return -1;
    }
    return 0;
}

extern "C" irdm_frontend_t *irdm_frontend_create_rational(const irdm_frontend_rational_config_t *cfg)
{
    if (!cfg) return nullptr;
    int Li = 0, Mi = 0;
    if (irdm_frontend_rational_ratio(cfg->in_rate, cfg->out_rate, &Li, &Mi) != 0) return nullptr;
    const long long L = Li, M = Mi;
    if (L == 1 && M >= 2 && M <= 16) {
        irdm_frontend_config_t ic;
        memset(&ic, 0, sizeof(ic));
        ic.device = cfg->device;
        ic.in_rate = cfg->in_rate;
        ic.in_format = cfg->in_format;
        ic.decim = (int)M;
        ic.shift_hz = cfg->shift_hz;
        return irdm_frontend_create(&ic);
    }
    irdm_frontend *fe = fe_new(cfg, 0, L, M);
    if (!fe) return nullptr;
    fe->launch = fe_launch_k0r;
    std::vector<int> desc;
    std::vector<float> G;
    if (!resample_plan(fe->L, fe->M, fe->taps.data(), fe->ntaps, &fe->geom, &desc, &G)) {
        fprintf(stderr, "irdm_hip: front end: %d taps at the ratio %lld/%lld do not fit the kernel\n", fe->ntaps, L, M);
        delete fe;
        return nullptr;
    }
    return fe_finish(fe, &fe->d_desc, desc, G);
}

}  // namespace irdmh
