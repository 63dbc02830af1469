// frontend_obj.hpp -- the front end's object, shared by its makers: irdm_frontend_create (frontend.cpp: K0, integer
// decimation), irdm_frontend_create_rational (resample.cpp: K0r, L / M) and irdm_frontend_create_wide (resample_wide.cpp:
// K0w, L / M at large L or M).  Everything behind creation -- the stream bookkeeping, the feeder, reset -- is frontend.cpp's
// and works on the ratio L / M (1 / D for K0); the object carries its kernel's launch function, so frontend.cpp refers to
// no kernel file by name beyond K0's.  The three makers share one path (fe_new, fe_finish below); each keeps its domain
// check, its plan, its tables and its launch function.
#pragma once
#include "pipeline.hpp"

struct irdm_frontend {
    irdm_frontend_config_t cfg;      // (rational mode: device, in_rate, in_format, shift_hz; decim 0)
    int D, fmt, bps, ntaps, c, out_rate;
    int L = 1, M = 0;                // output rate = input rate * L / M; K0: 1 / D
    long long q;
    std::vector<float> taps;
    float *d_hr = nullptr, *d_G = nullptr;
    float2 *d_T = nullptr;
    void *d_tail[2] = { nullptr, nullptr };
    // outputs [a.m0, a.m1) of [tail | chunk] on stream s: K0 (frontend.cpp), K0r (resample.cpp) or K0w (resample_wide.cpp)
    int (*launch)(irdm_frontend *fe, const irdm::FrontendArgs &a, hipStream_t s) = nullptr;
    // K0r: the launch geometry and the phase blocks' descriptors (d_G holds their tap rows)
    irdm::ResampleGeom geom{};
    int *d_desc = nullptr;
    // K0w: the launch geometry (d_desc holds the phases' first inputs, d_G the prototype laid out [step][phase])
    irdm::WideGeom wide{};
    // stream state (irdm_frontend_reset assigns a fresh one)
    struct State {
        int cur = 0;                // which of d_tail holds the carried tail
        long long n_tail = 0;
        uint64_t total = 0, n_out = 0;
        bool finished = false;
        // the feeder: outputs written but not fed yet lie at base[0 .. pend)
        float2 *base = nullptr;
        size_t room = 0, pend = 0;
        // saving the band: slot sv_next is filled next; a busy slot holds sv_bytes bytes not handed to the sink yet
        int sv_next = 0;
        bool sv_busy[2] = { false, false };
        size_t sv_bytes[2] = { 0, 0 };
        uint64_t sv_samples = 0;
        // input statistics: the totals of the capture and the passes in flight (input_stats.hpp)
        irdm::InputStatsStream is;
        // irdm_frontend_iq_moments: the sums of the capture and the passes in flight (iq_moments.hpp)
        irdm::IqMomentsStream iqm;
        // the corrections of irdm_frontend_feed_host: the scrub's totals and launches in flight (positions in the capture), the
        // DC tracker's position (host_chain.hpp)
        irdm::HostChainStream hc;
    } st;
    // Saving the band (irdm_frontend_save; off: sink == nullptr and nothing below exists).  fe_emit requantises what its
    // kernel wrote in pieces of at most slot_samples, each into one of two slots: device staging d[i] copied to the pinned
    // h[i] on the copy stream (ev_k[i]: the piece is in d[i]; ev[i]: it is in h[i]), or, with `direct`, written by the
    // kernel into h[i] itself.  A slot is handed to the sink, after its event, before it is filled again.
    struct Save {
        int format = 0, bytes_per_sample = 0;
        float gain = 1.0f, k = 0.0f;
        size_t slot_samples = 0;
        irdm_band_sink_t sink = nullptr;
        void *user = nullptr;
        bool direct = false;
        void *h[2] = { nullptr, nullptr }, *d[2] = { nullptr, nullptr };
        hipEvent_t ev[2] = { nullptr, nullptr }, ev_k[2] = { nullptr, nullptr };
        hipStream_t copy = nullptr;
        unsigned long long *d_stats = nullptr;      // launch_requant's three words
    } sv;
    // irdm_frontend_input_stats_enable: the pass over the capture's samples in front of the kernel (cache; is.on the switch)
    irdm::InputStatsPass is;
    // irdm_frontend_swap_iq, _scrub, _iq_balance and _dc_block (host_chain.hpp): what irdm_frontend_feed_host does to every
    // capture chunk on its way into the cf32 staging buffer (the switches and their settings: configuration; the scrub's
    // blocks, the DC tracker's rings and the wire staging buffer, grown as d_stage is: cache), and the mark of that call's own
    // device feed
    irdm::HostChain hc;
    // irdm_frontend_prime_host is running the capture's head through the kernel: fe_emit saves nothing of it
    bool priming = false;
    // irdm_frontend_iq_moments: the pass over the capture's samples in front of the kernel (cache; iqm.on the switch)
    irdm::IqMomentsPass iqm;
    hipStream_t stream = nullptr;
    hipEvent_t ev_in = nullptr, ev_caller = nullptr;
    unsigned long long *d_kclk = nullptr;
    float2 *d_scratch = nullptr;
    void *d_stage = nullptr;
    size_t stage_bytes = 0;
};

namespace irdmh {
void fe_free(irdm_frontend *fe);
// The maker path (frontend.cpp).  A maker checks its own domain, then:
//   fe_new     what the three kernels share of creation, for the ratio L / M in lowest terms (decim: K0's D, 1 / D; 0
//              otherwise): the checks of format, output rate, shift and device, the object and its prototype
//              (fe_resample_taps: the design of out_rate / in_rate = L / M).  nullptr with a message on stderr.
//   ...        the maker's launch function, its plan and its two tables
//   fe_finish  the two tables to the device (d_hr or d_desc, and d_G) and what every kernel needs beside them
//              (fe_alloc_common: the rotation table, the kernel clock record, the two tail buffers of tail_samples each,
//              8 bytes per sample, the stream in K1's priority class and the events; fe->cfg.device is current).  The
//              object, or nullptr with the message on stderr and the object freed.
std::vector<float> fe_resample_taps(int in_rate, int out_rate, long long L);
irdm_frontend *fe_new(const irdm_frontend_rational_config_t *cfg, int decim, long long L, long long M);
bool fe_alloc_common(irdm_frontend *fe, size_t tail_samples);
template <typename T>
irdm_frontend *fe_finish(irdm_frontend *fe, T **d_first, const std::vector<T> &first, const std::vector<float> &G)
{
    bool ok = (*d_first = dev_upload(first.data(), first.size())) != nullptr;
    ok = ok && (fe->d_G = dev_upload(G.data(), G.size())) != nullptr;
    ok = ok && fe_alloc_common(fe, (size_t)(fe->ntaps / fe->L + fe->M + 16));
    if (ok) return fe;
    fprintf(stderr, "irdm_hip: front end: device allocation failed\n");
    fe_free(fe);
    return nullptr;
}
// resample.cpp.  out_rate / in_rate in lowest terms, L / M (false, with a message: a rate that is not positive).  K0r's
// limits: 0 inside them, 1 L or M too large, 2 M / L outside its range.
bool fe_ratio(int in_rate, int out_rate, long long *L, long long *M);
int fe_rational_domain(long long L, long long M);
}  // namespace irdmh
