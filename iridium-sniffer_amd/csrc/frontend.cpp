// frontend.cpp -- irdm_frontend_*: the band-select front end's object (K0, frontend.hip): taps, tables, the carried tail,
// and the feeder that converts a wideband capture into the pipeline's ingest slot.
//
// Stream bookkeeping, for the ratio L / M (K0: 1 / D; K0r, resample.hip: any).  total = capture samples received, n_out =
// outputs produced.  Output m reads the inputs n with 0 <= m M + c - n L < ntaps, that is floor((m M - c - 1) / L) + 1 ..
// floor((m M + c) / L) (K0: m D - c .. m D + c), so after `total` samples the outputs below floor((total L - 1 - c) / M) + 1
// are complete, and the samples from floor((n_out M - c - 1) / L) + 1 on are still needed: they are kept, raw, in a device
// tail buffer (at most ntaps / L + 1 of them) and the kernel reads [tail | chunk] as one sequence.  The flush treats
// everything behind the last sample as zero and brings the count to ceil(total L / M).
#include "pipeline.hpp"
#include "frontend_obj.hpp"

namespace irdmh {

// saving off: the slots, the copy stream and the statistics words go (nothing of a stream is in flight, or is waited for)
static void fe_save_off(irdm_frontend *fe)
{
    irdm_frontend::Save &sv = fe->sv;
    if (sv.copy) (void)hipStreamSynchronize(sv.copy);
    for (int i = 0; i < 2; i++) {
        if (sv.h[i]) (void)hipHostFree(sv.h[i]);
        if (sv.d[i]) (void)hipFree(sv.d[i]);
        if (sv.ev[i]) (void)hipEventDestroy(sv.ev[i]);
        if (sv.ev_k[i]) (void)hipEventDestroy(sv.ev_k[i]);
    }
    if (sv.copy) (void)hipStreamDestroy(sv.copy);
    if (sv.d_stats) (void)hipFree(sv.d_stats);
    sv = irdm_frontend::Save{};
    for (int i = 0; i < 2; i++) fe->st.sv_busy[i] = false;
}

void fe_free(irdm_frontend *fe)
{
    if (!fe) return;
    (void)hipSetDevice(fe->cfg.device);
    if (fe->stream) (void)hipStreamSynchronize(fe->stream);
    fe_save_off(fe);
    fe->is.free();
    hc_free(fe->hc);
    fe->iqm.free();
    void *ptrs[] = { fe->d_hr, fe->d_G, fe->d_T, fe->d_tail[0], fe->d_tail[1], fe->d_kclk, fe->d_scratch, fe->d_stage, fe->d_desc };
    for (void *q : ptrs)
        if (q) (void)hipFree(q);
    if (fe->ev_in) (void)hipEventDestroy(fe->ev_in);
    if (fe->ev_caller) (void)hipEventDestroy(fe->ev_caller);
    if (fe->stream) (void)hipStreamDestroy(fe->stream);
    delete fe;
}

bool fe_alloc_common(irdm_frontend *fe, size_t tail_samples)
{
    // the rotation table (built in double)
    std::vector<float2> T(65536);
    for (int i = 0; i < 65536; i++) {
        const double a = -2.0 * M_PI * (double)i / 65536.0;
        T[i] = make_float2((float)cos(a), (float)sin(a));
    }
    int prio_lo = 0, prio_hi = 0;
    (void)hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi);
    const int prio_k1 = prio_hi < prio_lo - 1 ? prio_hi + 1 : prio_hi;          // K1's class (create.cpp)
    const size_t tail_bytes = tail_samples * 8;
    std::vector<unsigned long long> kinit(kKClkWords, 0ull);
    for (int i = 0; i < 64; i++) kinit[i] = ~0ull;
    bool ok = (fe->d_T = dev_upload(T.data(), T.size())) != nullptr;
    ok = ok && (fe->d_kclk = dev_upload(kinit.data(), kinit.size())) != nullptr;
    ok = ok && hipMalloc(&fe->d_tail[0], tail_bytes) == hipSuccess && hipMalloc(&fe->d_tail[1], tail_bytes) == hipSuccess;
    ok = ok && hipStreamCreateWithPriority(&fe->stream, hipStreamNonBlocking, prio_k1) == hipSuccess;
    ok = ok && hipEventCreateWithFlags(&fe->ev_in, hipEventDisableTiming) == hipSuccess;
    ok = ok && hipEventCreateWithFlags(&fe->ev_caller, hipEventDisableTiming) == hipSuccess;
    return ok;
}

static int fe_launch_k0(irdm_frontend *fe, const FrontendArgs &a, hipStream_t s)
{
    return launch_frontend(fe->D, a, fe->d_hr, fe->d_G, fe->d_T, s, fe->d_kclk);
}

// the prototype P of the ratio L / M = out_rate / in_rate (resample.cpp's header comment); L = 1: K0's taps at D = M
std::vector<float> fe_resample_taps(int in_rate, int out_rate, long long L)
{
    const float f_min = (float)std::min(in_rate, out_rate);
    return design_lpf((float)L, (float)(L * (long long)in_rate), 0.5f * f_min, 0.09f * f_min);
}

irdm_frontend *fe_new(const irdm_frontend_rational_config_t *cfg, int decim, long long L, long long M)
{
    if (!fmt_valid(cfg->in_format)) {
        fprintf(stderr, "irdm_hip: front end: unknown sample format %d\n", cfg->in_format);
        return nullptr;
    }
    int fft = 0;
    if (!rate_supported(cfg->out_rate, &fft)) {
        if (decim)
            fprintf(stderr, "irdm_hip: front end: output rate %d (%d / %d) is not one the pipeline takes (fft_size %d)\n",
                    cfg->out_rate, cfg->in_rate, decim, fft);
        else
            fprintf(stderr, "irdm_hip: front end: output rate %d (%d * %lld / %lld) is not one the pipeline takes (fft_size %d)\n",
                    cfg->out_rate, cfg->in_rate, L, M, fft);
        return nullptr;
    }
    const long long q = llround(cfg->shift_hz * 65536.0 / (double)cfg->in_rate);
    if (q < -32768 || q > 32768) {
        fprintf(stderr, "irdm_hip: front end: shift %.1f Hz is beyond half the capture rate %d\n", cfg->shift_hz, cfg->in_rate);
        return nullptr;
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) {
        fprintf(stderr, "irdm_hip: no HIP device -- there is no CPU fallback in this library\n");
        return nullptr;
    }
    if (hipSetDevice(cfg->device) != hipSuccess) return nullptr;
    irdm_frontend *fe = new (std::nothrow) irdm_frontend();
    if (!fe) return nullptr;
    memset(&fe->cfg, 0, sizeof(fe->cfg));
    fe->cfg.device = cfg->device;
    fe->cfg.in_rate = cfg->in_rate;
    fe->cfg.in_format = cfg->in_format;
    fe->cfg.decim = decim;
    fe->cfg.shift_hz = cfg->shift_hz;
    fe->D = decim;
    fe->L = (int)L;
    fe->M = (int)M;
    fe->fmt = cfg->in_format;
    fe->bps = fmt_bytes(fe->fmt);
    fe->out_rate = cfg->out_rate;
    fe->q = q;
    fe->taps = fe_resample_taps(cfg->in_rate, cfg->out_rate, L);
    fe->ntaps = (int)fe->taps.size();
    fe->c = (fe->ntaps - 1) / 2;
    return fe;
}

extern "C" irdm_frontend_t *irdm_frontend_create(const irdm_frontend_config_t *cfg)
{
    if (!cfg) return nullptr;
    if (cfg->decim < 2 || cfg->decim > 16) {
        fprintf(stderr, "irdm_hip: front end: decimation %d outside 2 .. 16\n", cfg->decim);
        return nullptr;
    }
    if (cfg->in_rate <= 0 || cfg->in_rate % cfg->decim != 0) {
        fprintf(stderr, "irdm_hip: front end: sample rate %d is not a multiple of the decimation %d\n", cfg->in_rate, cfg->decim);
        return nullptr;
    }
    const irdm_frontend_rational_config_t rc = { cfg->device, cfg->in_rate, cfg->in_format, cfg->in_rate / cfg->decim, cfg->shift_hz };
    irdm_frontend *fe = fe_new(&rc, cfg->decim, 1, cfg->decim);
    if (!fe) return nullptr;
    fe->launch = fe_launch_k0;
    const int R = 8, D = fe->D, nt = fe->ntaps;
    if (nt < (R - 1) * D + 1 || frontend_lds_bytes(D, nt) > 160 * 1024) {
        fprintf(stderr, "irdm_hip: front end: %d taps at decimation %d do not fit the kernel\n", nt, D);
        delete fe;
        return nullptr;
    }
    // reversed taps (ascending input order), the table of the full steps
    std::vector<float> hr(nt), G((size_t)(nt - (R - 1) * D) * R);
    for (int j = 0; j < nt; j++) hr[j] = fe->taps[nt - 1 - j];
    for (int i = (R - 1) * D; i < nt; i++)
        for (int r = 0; r < R; r++) G[(size_t)(i - (R - 1) * D) * R + r] = hr[i - r * D];
    return fe_finish(fe, &fe->d_hr, hr, G);
}

extern "C" void irdm_frontend_destroy(irdm_frontend_t *fe) { fe_free(fe); }
extern "C" int irdm_frontend_out_rate(const irdm_frontend_t *fe) { return fe ? fe->out_rate : -1; }
extern "C" double irdm_frontend_applied_shift_hz(const irdm_frontend_t *fe)
{
    return fe ? (double)fe->q * (double)fe->cfg.in_rate / 65536.0 : 0.0;
}
extern "C" int irdm_frontend_ratio(const irdm_frontend_t *fe, int *L, int *M)
{
    if (!fe) return -1;
    if (L) *L = fe->L;
    if (M) *M = fe->M;
    return 0;
}
extern "C" int irdm_frontend_ntaps(const irdm_frontend_t *fe) { return fe ? fe->ntaps : -1; }
extern "C" int irdm_frontend_taps(const irdm_frontend_t *fe, float *out, int max)
{
    if (!fe || !out || max < fe->ntaps) return -1;
    memcpy(out, fe->taps.data(), sizeof(float) * (size_t)fe->ntaps);
    return fe->ntaps;
}

// outputs complete once `total` samples are in (flush: with zeros behind them)
static uint64_t fe_outputs(const irdm_frontend *fe, uint64_t total, bool flush)
{
    const uint64_t L = (uint64_t)fe->L, M = (uint64_t)fe->M;
    if (flush) return (total * L + M - 1) / M;
    return total * L > (uint64_t)fe->c ? (total * L - 1 - (uint64_t)fe->c) / M + 1 : 0;
}

// ---- saving the band (irdm_frontend_save): the tap behind fe_emit's kernel ----

// slot i to the sink, once its bytes are in the pinned buffer
static int fe_save_deliver(irdm_frontend *fe, int i)
{
    if (!fe->st.sv_busy[i]) return 0;
    IRDM_HIP_CHECK(hipEventSynchronize(fe->sv.ev[i]));
    fe->st.sv_busy[i] = false;
    return fe->sv.sink(fe->sv.user, fe->sv.h[i], fe->st.sv_bytes[i]) == 0 ? 0 : -1;
}

// everything outstanding, in stream order (the slot to be filled next is the older one)
static int fe_save_drain(irdm_frontend *fe)
{
    if (!fe->sv.sink) return 0;
    if (fe_save_deliver(fe, fe->st.sv_next) != 0) return -1;
    return fe_save_deliver(fe, fe->st.sv_next ^ 1);
}

// out[0 .. n) has just been written on stream s: requantised (cf32: copied) in pieces of at most slot_samples, each into
// the slot whose turn it is.  s waits for no transfer: it runs the piece's kernel (cf32: a device copy) into staging and
// the copy stream takes it from there; with `direct` the kernel's own stores (cf32: the copy) go to the pinned slot.
static int fe_save_tap(irdm_frontend *fe, const float2 *out, size_t n, hipStream_t s)
{
    irdm_frontend::Save &sv = fe->sv;
    const int bits = sv.format == IRDM_FMT_CI8 ? 8 : (sv.format == IRDM_FMT_CI16 ? 16 : 0);
    for (size_t off = 0; off < n; off += sv.slot_samples) {
        const size_t piece = std::min(sv.slot_samples, n - off);
        const int i = fe->st.sv_next;
        if (fe_save_deliver(fe, i) != 0) return -1;
        const size_t bytes = piece * (size_t)sv.bytes_per_sample;
        void *dst = sv.direct ? sv.h[i] : sv.d[i];
        if (bits) {
            if (launch_requant(bits, out + off, (long long)piece, sv.k, dst, sv.d_stats, s) != 0) return -1;
        } else {
            IRDM_HIP_CHECK(hipMemcpyAsync(dst, out + off, bytes, sv.direct ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice, s));
        }
        if (sv.direct) {
            IRDM_HIP_CHECK(hipEventRecord(sv.ev[i], s));
        } else {
            IRDM_HIP_CHECK(hipEventRecord(sv.ev_k[i], s));
            IRDM_HIP_CHECK(hipStreamWaitEvent(sv.copy, sv.ev_k[i], 0));
            IRDM_HIP_CHECK(hipMemcpyAsync(sv.h[i], sv.d[i], bytes, hipMemcpyDeviceToHost, sv.copy));
            IRDM_HIP_CHECK(hipEventRecord(sv.ev[i], sv.copy));
        }
        fe->st.sv_busy[i] = true;
        fe->st.sv_bytes[i] = bytes;
        fe->st.sv_next = i ^ 1;
        fe->st.sv_samples += piece;
    }
    return 0;
}

// outputs [fe->st.n_out, m1) of [tail | d_in] into out
static int fe_emit(irdm_frontend *fe, const void *d_in, size_t n_in, uint64_t m1, float2 *out, hipStream_t s)
{
    if (m1 <= fe->st.n_out) return 0;
    FrontendArgs a;
    a.tail = fe->d_tail[fe->st.cur];
    a.in = d_in;
    a.n_tail = fe->st.n_tail;
    a.n_in = (long long)n_in;
    a.pos0 = (long long)fe->st.total - fe->st.n_tail;
    a.m0 = (long long)fe->st.n_out;
    a.m1 = (long long)m1;
    a.out = out;
    a.q16 = (unsigned)(fe->q & 0xffff);
    a.ntaps = fe->ntaps;
    a.fmt = fe->fmt;
    if (fe->launch(fe, a, s) != 0) return -1;
    if (launch_kclk_fold(fe->d_kclk, s) != 0) return -1;
    if (fe->sv.sink && !fe->priming && fe_save_tap(fe, out, (size_t)(m1 - fe->st.n_out), s) != 0) return -1;
    fe->st.n_out = m1;
    return 0;
}

// the chunk has been consumed: keep what later outputs need, advance the stream position
static int fe_commit(irdm_frontend *fe, const void *d_in, size_t n_in, hipStream_t s)
{
    const uint64_t total = fe->st.total + n_in;
    const long long edge = (long long)(fe->st.n_out * (uint64_t)fe->M) - fe->c - 1;
    const long long need = (edge >= 0 ? edge / fe->L : -((-edge + fe->L - 1) / fe->L)) + 1;     // first sample still needed
    const long long start = std::min<long long>(std::max<long long>(need, 0), (long long)total);
    const long long pos0 = (long long)fe->st.total - fe->st.n_tail;
    const int n_new = (int)((long long)total - start);
    if (n_new > fe->ntaps / fe->L + fe->M + 16) return -1;                                 // (cannot happen: see the header comment)
    if (launch_frontend_tail(fe->d_tail[fe->st.cur], fe->st.n_tail, d_in, (long long)n_in, start - pos0, n_new, fe->bps,
                             fe->d_tail[fe->st.cur ^ 1], s) != 0)
        return -1;
    fe->st.cur ^= 1;
    fe->st.n_tail = n_new;
    fe->st.total = total;
    return 0;
}

// ---- input statistics: the capture's samples in front of the kernel ----

// the pass over the chunk that has arrived on s, on the side stream
static int fe_stats_enqueue(irdm_frontend *fe, const void *d_in, size_t n_in, hipStream_t s)
{
    if (fe->iqm.on && n_in && iq_moments_enqueue(fe->iqm, fe->st.iqm, fe->fmt, d_in, n_in, s, fe->st.iqm.launches) != 0) return -1;
    if (!fe->is.on || !n_in) return 0;
    return input_stats_enqueue(fe->is, fe->st.is, fe->fmt, d_in, n_in, s, fe->st.is.launches);
}

// s goes on behind that pass: what s records or runs next may hand the chunk's memory back
static int fe_stats_join(irdm_frontend *fe, size_t n_in, hipStream_t s)
{
    if (fe->iqm.on && n_in && fe->iqm.lead(fe->st.iqm, s) != 0) return -1;
    return fe->is.on && n_in ? fe->is.lead(fe->st.is, s) : 0;
}

extern "C" int irdm_frontend_input_stats_enable(irdm_frontend_t *fe, int on)
{
    if (!fe) return -1;
    (void)hipSetDevice(fe->cfg.device);
    if (on && fe->is.alloc(kIsBlockBytes, true) != 0) return -1;
    fe->is.on = on ? 1 : 0;
    return 0;
}

extern "C" int irdm_frontend_input_stats(irdm_frontend_t *fe, irdm_input_stats_t *out)
{
    if (!fe || !out || !fe->is.stream) return -1;
    (void)hipSetDevice(fe->cfg.device);
    if (input_stats_settle(fe->is, fe->st.is, fe->fmt, ~0ull) != 0) return -1;
    input_stats_result(fe->st.is.run, fe->fmt, out);
    return 0;
}

extern "C" int irdm_frontend_iq_moments(irdm_frontend_t *fe, int on)
{
    if (!fe) return -1;
    (void)hipSetDevice(fe->cfg.device);
    if (on && fe->iqm.alloc(kImBlockBytes, true) != 0) return -1;
    fe->iqm.on = on ? 1 : 0;
    return 0;
}

extern "C" int irdm_frontend_iq_moments_stats(irdm_frontend_t *fe, irdm_iq_moments_t *out)
{
    if (!fe || !out || !fe->iqm.stream) return -1;
    (void)hipSetDevice(fe->cfg.device);
    if (iq_moments_settle(fe->iqm, fe->st.iqm, ~0ull) != 0) return -1;
    iq_moments_result(fe->st.iqm.run, out);
    return 0;
}

extern "C" int irdm_frontend_iq_balance(irdm_frontend_t *fe, int wire_format, double gain_db, double phase_deg)
{
    // a cf32 front end, and only before the capture's first chunk: the carried tail would hold uncorrected samples
    if (!fe || fe->fmt != IRDM_FMT_CF32 || fe->st.total != 0 || !fmt_valid(wire_format)) return -1;
    float alpha, beta;
    if (iq_balance_coeffs(gain_db, phase_deg, &alpha, &beta) != 0) return -1;
    fe->hc.bal = IqBalance{ 1, wire_format, alpha, beta };
    return 0;
}

extern "C" int irdm_frontend_dc_block(irdm_frontend_t *fe, int wire_format, int block_log2, float seed_i, float seed_q)
{
    // as irdm_frontend_iq_balance: a cf32 front end, and only before the capture's first chunk
    if (!fe || fe->fmt != IRDM_FMT_CF32 || fe->st.total != 0 || fe->st.hc.dc.pos != 0) return -1;
    (void)hipSetDevice(fe->cfg.device);
    if (block_log2 >= 0) IRDM_HIP_CHECK(hipStreamSynchronize(fe->stream));
    return dc_configure(fe->hc.dc, wire_format, block_log2, seed_i, seed_q, 0);
}

extern "C" int irdm_frontend_dc_stats(irdm_frontend_t *fe, irdm_dc_stats_t *out)
{
    if (!fe || !out || !fe->hc.dc.on) return -1;
    (void)hipSetDevice(fe->cfg.device);
    IRDM_HIP_CHECK(hipStreamSynchronize(fe->stream));
    return dc_result(fe->hc.dc, fe->st.hc.dc, out);
}

extern "C" int irdm_frontend_swap_iq(irdm_frontend_t *fe, int on)
{
    // no change between a stream's first chunk and irdm_frontend_reset: the carried tail would hold the other sense
    if (!fe || (fe->st.total != 0 && (on != 0) != (fe->hc.swap_iq != 0))) return -1;
    fe->hc.swap_iq = on ? 1 : 0;
    return 0;
}

extern "C" int irdm_frontend_scrub(irdm_frontend_t *fe, int on, int limit_log2)
{
    // no change between a stream's first chunk and irdm_frontend_reset: the figures would describe half a capture
    if (!fe || limit_log2 < 0 || limit_log2 > 127) return -1;
    if (fe->st.total != 0 && ((on != 0) != (fe->hc.scrub.on != 0) || limit_log2 != fe->hc.scrub.limit_log2)) return -1;
    (void)hipSetDevice(fe->cfg.device);
    if (on && fe->fmt == IRDM_FMT_CF32 && fe->hc.scrub.alloc(kSbBlockBytes, false) != 0) return -1;
    fe->hc.scrub.on = on ? 1 : 0;
    fe->hc.scrub.limit_log2 = limit_log2;
    return 0;
}

extern "C" int irdm_frontend_scrub_stats(irdm_frontend_t *fe, irdm_scrub_stats_t *out)
{
    if (!fe || !out || !fe->hc.scrub.on) return -1;
    (void)hipSetDevice(fe->cfg.device);
    if (scrub_settle(fe->hc.scrub, fe->st.hc.scrub) != 0) return -1;
    scrub_result(fe->st.hc.scrub.run, fe->hc.scrub.limit_log2, fe->fmt == IRDM_FMT_CF32 ? 1 : 0, out);
    return 0;
}

extern "C" long long irdm_frontend_run_device(irdm_frontend_t *fe, const void *d_in, size_t n_in, void *d_out, size_t out_cap,
                                              void *stream_v)
{
    if (!fe || fe->st.finished || (!d_in && n_in) || !d_out || hc_refuses(fe->hc, 1)) return -1;
    const uint64_t m1 = fe_outputs(fe, fe->st.total + n_in, false);
    const uint64_t n = m1 - fe->st.n_out;
    if (n > out_cap) return -1;
    (void)hipSetDevice(fe->cfg.device);
    hipStream_t s = stream_v ? static_cast<hipStream_t>(stream_v) : fe->stream;
    if (fe_stats_enqueue(fe, d_in, n_in, s) != 0) return -1;
    if (fe_emit(fe, d_in, n_in, m1, static_cast<float2 *>(d_out), s) != 0) return -1;
    if (fe_commit(fe, d_in, n_in, s) != 0) return -1;
    if (fe_stats_join(fe, n_in, s) != 0) return -1;
    IRDM_HIP_CHECK(hipEventRecord(fe->ev_in, s));
    if (!stream_v) IRDM_HIP_CHECK(hipStreamSynchronize(s));
    return (long long)n;
}

extern "C" long long irdm_frontend_finish_device(irdm_frontend_t *fe, void *d_out, size_t out_cap, void *stream_v)
{
    if (!fe || fe->st.finished || !d_out) return -1;
    const uint64_t m1 = fe_outputs(fe, fe->st.total, true);
    const uint64_t n = m1 - fe->st.n_out;
    if (n > out_cap) return -1;
    (void)hipSetDevice(fe->cfg.device);
    hipStream_t s = stream_v ? static_cast<hipStream_t>(stream_v) : fe->stream;
    if (fe_emit(fe, nullptr, 0, m1, static_cast<float2 *>(d_out), s) != 0) return -1;
    fe->st.finished = true;
    if (fe_save_drain(fe) != 0) return -1;
    if (!stream_v) IRDM_HIP_CHECK(hipStreamSynchronize(s));
    return (long long)n;
}

// ---- the feeder ----

// where the next outputs go: the pipeline's ingest slot for as many samples as lie between the stream position and the
// end of the ring (at most a chunk), or the scratch chunk (pipeline_depth 0)
static int fe_acquire(irdm_frontend *fe, irdm_pipeline *p)
{
    size_t room = p->max_chunk;
    if (p->depth) room = (size_t)std::min<uint64_t>(room, p->ring_len - p->st.begun_samples % p->ring_len);
    room = room / (size_t)p->feed_block * (size_t)p->feed_block;
    void *slot = room ? irdm_ingest_ptr(p, room) : nullptr;
    if (!slot) {
        if (!fe->d_scratch && hipMalloc(reinterpret_cast<void **>(&fe->d_scratch), p->max_chunk * sizeof(float2)) != hipSuccess) return -1;
        slot = fe->d_scratch;
        room = p->max_chunk;
    }
    fe->st.base = static_cast<float2 *>(slot);
    fe->st.room = room;
    return 0;
}

// outputs up to m1 of [tail | d_in] into the pipeline; every whole multiple of feed_block that accumulates is fed.
// last: the end of the stream -- what remains is fed as the ragged last chunk.
static int fe_pump(irdm_frontend *fe, irdm_pipeline *p, const void *d_in, size_t n_in, uint64_t m1, bool last)
{
    int bursts = 0;
    for (;;) {
        if (!fe->st.base && fe_acquire(fe, p) != 0) return -1;
        const size_t take = (size_t)std::min<uint64_t>(fe->st.room - fe->st.pend, m1 - fe->st.n_out);
        if (fe_emit(fe, d_in, n_in, fe->st.n_out + take, fe->st.base + fe->st.pend, fe->stream) != 0) return -1;
        fe->st.pend += take;
        const bool done = fe->st.n_out == m1;
        size_t feedable = fe->st.pend / (size_t)p->feed_block * (size_t)p->feed_block;
        if (last && done) feedable = fe->st.pend;
        if (feedable) {
            const int rc = irdm_feed_device(p, fe->st.base, feedable, fe->stream);
            if (rc < 0) return -1;
            bursts += rc;
            const float2 *rest = fe->st.base + feedable;
            const size_t n_rest = fe->st.pend - feedable;
            fe->st.base = nullptr;
            fe->st.pend = 0;
            if (n_rest) {
                if (fe_acquire(fe, p) != 0) return -1;
                // (in the ring the remainder already lies where the next slot begins, unless the ring wraps there)
                if (fe->st.base != rest)
                    IRDM_HIP_CHECK(hipMemcpyAsync(fe->st.base, rest, n_rest * sizeof(float2), hipMemcpyDeviceToDevice, fe->stream));
                fe->st.pend = n_rest;
            }
        }
        if (done) break;
    }
    return bursts;
}

static int fe_check(const irdm_frontend *fe, const irdm_pipeline *p)
{
    if (!fe || !p || fe->st.finished) return -1;
    if (p->dev_fmt != IRDM_FMT_CF32 || p->cfg.sample_rate != fe->out_rate || p->cfg.device != fe->cfg.device) {
        fprintf(stderr, "irdm_hip: front end: the pipeline must be a cf32 context at %d samples/s on device %d\n", fe->out_rate,
                fe->cfg.device);
        return -1;
    }
    return 0;
}

extern "C" int irdm_frontend_feed_device(irdm_frontend_t *fe, irdm_pipeline_t *p, const void *d_in, size_t n_in, void *stream_v)
{
    if (fe_check(fe, p) != 0 || (!d_in && n_in) || hc_refuses(fe->hc, 1)) return -1;
    pipeline_enter(p);
    if (stream_v && static_cast<hipStream_t>(stream_v) != fe->stream) {
        IRDM_HIP_CHECK(hipEventRecord(fe->ev_caller, static_cast<hipStream_t>(stream_v)));
        IRDM_HIP_CHECK(hipStreamWaitEvent(fe->stream, fe->ev_caller, 0));
    }
    if (fe_stats_enqueue(fe, d_in, n_in, fe->stream) != 0) return -1;
    const int bursts = fe_pump(fe, p, d_in, n_in, fe_outputs(fe, fe->st.total + n_in, false), false);
    if (bursts < 0) return -1;
    if (fe_commit(fe, d_in, n_in, fe->stream) != 0) return -1;
    if (fe_stats_join(fe, n_in, fe->stream) != 0) return -1;
    IRDM_HIP_CHECK(hipEventRecord(fe->ev_in, fe->stream));
    return bursts;
}

// n_in capture samples at h_in into the staging buffer on the front end's stream, the way irdm_frontend_feed_host takes a
// chunk: the corrections of host_chain.hpp applied in front of the statistics pass and K0 / K0r, the DC tone gone before the
// shift (count: with the scrub's figures, positions in the capture).  ev_caller is recorded behind the copy from h_in.
static int fe_land_host(irdm_frontend *fe, const void *h_in, size_t n_in, bool count)
{
    // (one staging buffer, and one for a wire format other than cf32, both grown on demand: the copy is ordered behind the
    // kernels that read the previous chunk, on the same stream)
    if (hc_grow(&fe->d_stage, &fe->stage_bytes, n_in * (size_t)fe->bps, fe->stream) != 0 || hc_reserve(fe->hc, n_in, fe->stream) != 0)
        return -1;
    void *const land = hc_landing(fe->hc, fe->d_stage);
    if (n_in)
        IRDM_HIP_CHECK(hipMemcpyAsync(land, h_in, n_in * (size_t)fmt_bytes(hc_wire_fmt(fe->hc, fe->fmt)), hipMemcpyHostToDevice, fe->stream));
    IRDM_HIP_CHECK(hipEventRecord(fe->ev_caller, fe->stream));
    return hc_apply(fe->hc, fe->st.hc, fe->fmt, fe->d_stage, land, n_in, fe->st.total, count, fe->stream);
}

extern "C" int irdm_frontend_feed_host(irdm_frontend_t *fe, irdm_pipeline_t *p, const void *h_in, size_t n_in)
{
    if (fe_check(fe, p) != 0 || (!h_in && n_in)) return -1;
    pipeline_enter(p);
    if (fe_land_host(fe, h_in, n_in, true) != 0) return -1;
    fe->hc.inner = true;
    const int bursts = irdm_frontend_feed_device(fe, p, fe->d_stage, n_in, nullptr);
    fe->hc.inner = false;
    IRDM_HIP_CHECK(hipEventSynchronize(fe->ev_caller));          // the host buffer has been read
    return bursts;
}

extern "C" int irdm_frontend_flush(irdm_frontend_t *fe, irdm_pipeline_t *p)
{
    if (fe_check(fe, p) != 0) return -1;
    pipeline_enter(p);
    int bursts = fe_pump(fe, p, nullptr, 0, fe_outputs(fe, fe->st.total, true), true);
    if (bursts < 0) return -1;
    fe->st.finished = true;
    if (fe_save_drain(fe) != 0) return -1;
    const int rc = irdm_flush(p);
    return rc < 0 ? -1 : bursts + rc;
}

// Back to irdm_frontend_create's state for another capture: no carried tail, stream position and output count (the NCO's
// phase index with them) zero, nothing held back by the feeder.  Taps, tables, the applied shift, the scratch chunk and the
// staging buffer stay.  (The tail buffers keep their bytes: with n_tail 0 the kernel reads none of them.)
extern "C" int irdm_frontend_reset(irdm_frontend_t *fe)
{
    if (!fe) return -1;
    (void)hipSetDevice(fe->cfg.device);
    IRDM_HIP_CHECK(hipStreamSynchronize(fe->stream));      // (launches in flight read the tail and the staging buffer)
    // saving: what the sink has not been given is dropped, the statistics start again; the sink and the slots stay
    if (fe->sv.copy) IRDM_HIP_CHECK(hipStreamSynchronize(fe->sv.copy));
    if (fe->sv.d_stats) IRDM_HIP_CHECK(hipMemset(fe->sv.d_stats, 0, 3 * sizeof(unsigned long long)));
    if (fe->is.stream) IRDM_HIP_CHECK(hipStreamSynchronize(fe->is.stream));       // (the passes in flight are dropped with the state)
    if (fe->iqm.stream) IRDM_HIP_CHECK(hipStreamSynchronize(fe->iqm.stream));
    fe->st = irdm_frontend::State{};
    return 0;
}

// The capture's first n_in samples through the kernel without a flush, in pieces of at most 4 Mi samples, until 512
// frames of the band are there (or the samples are used up); saving, the statistics passes and the scrub's figures off.
// The context is primed from the whole frames of that band (irdm_prime_device), and the front end is reset: the real run
// starts at input 0, and what it saves and reports is what the run without priming saves and reports.
extern "C" int irdm_frontend_prime_host(irdm_frontend_t *fe, irdm_pipeline_t *p, const void *h_in, size_t n_in)
{
    if (fe_check(fe, p) != 0 || !h_in || fe->st.total || fe->st.n_out || fe->st.n_tail || fe->st.pend) return -1;
    const size_t N = (size_t)p->P.n, H = (size_t)kHistory * N;
    // (no more of the capture than completes H outputs: fe_commit keeps a tail of a few taps, not a backlog)
    const uint64_t n_full = (((uint64_t)H - 1) * (uint64_t)fe->M + (uint64_t)fe->c + (uint64_t)fe->L) / (uint64_t)fe->L;
    n_in = (size_t)std::min<uint64_t>(n_in, n_full);
    const uint64_t m_all = fe_outputs(fe, n_in, false);
    if (prime_check(p, (size_t)m_all) < 0) return -1;
    pipeline_enter(p);
    float2 *d_band = dev_alloc<float2>((size_t)m_all);
    if (!d_band) return -1;
    const size_t piece_max = (size_t)4 << 20;
    int rc = 0;
    fe->priming = true;
    for (size_t off = 0; rc == 0 && off < n_in; off += piece_max) {
        const size_t piece = std::min(piece_max, n_in - off);
        const uint64_t m1 = fe_outputs(fe, fe->st.total + piece, false);
        rc = fe_land_host(fe, static_cast<const char *>(h_in) + off * (size_t)fmt_bytes(hc_wire_fmt(fe->hc, fe->fmt)), piece, false);
        if (rc == 0) rc = fe_emit(fe, fe->d_stage, piece, m1, d_band + fe->st.n_out, fe->stream);
        if (rc == 0) rc = fe_commit(fe, fe->d_stage, piece, fe->stream);
        if (rc == 0 && hipEventSynchronize(fe->ev_caller) != hipSuccess) rc = -1;
    }
    fe->priming = false;
    if (rc == 0) rc = irdm_prime_device(p, d_band, (size_t)fe->st.n_out, fe->stream);
    (void)hipStreamSynchronize(fe->stream);
    (void)hipFree(d_band);
    if (irdm_frontend_reset(fe) != 0) return -1;
    return rc;
}

// A capture taken up at input sample total_in: the state that fe_emit / fe_commit would have left behind total_in samples
// of zero codes -- the position, the count of outputs those samples complete, and as the carried tail the zeros from the
// first sample the next output still needs (fe_commit's count).  Nothing is launched.
extern "C" int irdm_frontend_seek(irdm_frontend_t *fe, uint64_t total_in)
{
    if (!fe || fe->st.total || fe->st.n_out || fe->st.n_tail || fe->st.finished || fe->st.pend) return -1;
    if (total_in >= IRDM_MAX_POSITION) {
        fprintf(stderr, "irdm_hip: front end: irdm_frontend_seek: stream position %llu is not below 2^53\n", (unsigned long long)total_in);
        return -1;
    }
    (void)hipSetDevice(fe->cfg.device);
    const uint64_t n_out = fe_outputs(fe, total_in, false);
    const long long edge = (long long)(n_out * (uint64_t)fe->M) - fe->c - 1;
    const long long need = (edge >= 0 ? edge / fe->L : -((-edge + fe->L - 1) / fe->L)) + 1;
    const long long start = std::min<long long>(std::max<long long>(need, 0), (long long)total_in);
    const long long n_tail = (long long)total_in - start;
    if (n_tail > fe->ntaps / fe->L + fe->M + 16) return -1;                                // (the tail buffers' size)
    // (waited for: the next call may run its kernel on a stream of the caller's)
    if (n_tail) {
        IRDM_HIP_CHECK(hipMemsetAsync(fe->d_tail[fe->st.cur], 0, (size_t)n_tail * (size_t)fe->bps, fe->stream));
        IRDM_HIP_CHECK(hipStreamSynchronize(fe->stream));
    }
    fe->st.total = total_in;
    fe->st.n_out = n_out;
    fe->st.n_tail = n_tail;
    return 0;
}

// ---- saving the band: the public calls ----

static int save_scale(int format) { return format == IRDM_FMT_CI8 ? 128 : (format == IRDM_FMT_CI16 ? 32768 : 0); }

static void save_stats_out(int format, const unsigned long long h[3], uint64_t n_samples, irdm_band_stats_t *out)
{
    const int S = save_scale(format);
    out->n_samples = S ? h[0] / 2 : n_samples;
    out->n_clipped = h[1];
    float peak = 0.0f;
    if (S) {
        const uint32_t b = (uint32_t)h[2];
        memcpy(&peak, &b, sizeof(peak));
        peak = peak / (float)S;
    }
    out->peak = peak;
}

extern "C" int irdm_frontend_save(irdm_frontend_t *fe, const irdm_frontend_save_config_t *cfg)
{
    if (!fe || fe->st.total || fe->st.n_out || fe->st.finished) return -1;
    (void)hipSetDevice(fe->cfg.device);
    IRDM_HIP_CHECK(hipStreamSynchronize(fe->stream));
    if (!cfg) {
        fe_save_off(fe);
        return 0;
    }
    const int S = save_scale(cfg->format);
    if ((!S && cfg->format != IRDM_FMT_CF32) || !cfg->sink || !(cfg->gain > 0.0f) || !std::isfinite(cfg->gain) ||
        (!S && cfg->gain != 1.0f) || (S && !std::isfinite(cfg->gain * (float)S))) {
        fprintf(stderr, "irdm_hip: front end: save: format ci8 / ci16 / cf32, a positive finite gain (1 for cf32) and a sink\n");
        return -1;
    }
    fe_save_off(fe);
    irdm_frontend::Save &sv = fe->sv;
    sv.format = cfg->format;
    sv.bytes_per_sample = S == 128 ? 2 : (S ? 4 : 8);
    sv.gain = cfg->gain;
    sv.k = S ? cfg->gain * (float)S : 0.0f;
    sv.slot_samples = cfg->slot_samples ? cfg->slot_samples : (size_t)4 << 20;
    sv.user = cfg->user;
    // (measurement aid, tools/saveband_rate.py: IRDM_SAVE_DIRECT=1 lets the kernel store into the pinned slot itself)
    const char *dm = getenv("IRDM_SAVE_DIRECT");
    sv.direct = dm && dm[0] == '1';
    const size_t slot_bytes = sv.slot_samples * (size_t)sv.bytes_per_sample;
    bool ok = true;
    for (int i = 0; i < 2 && ok; i++) {
        ok = hipHostMalloc(&sv.h[i], slot_bytes, hipHostMallocDefault) == hipSuccess;
        ok = ok && (sv.direct || hipMalloc(&sv.d[i], slot_bytes) == hipSuccess);
        ok = ok && hipEventCreateWithFlags(&sv.ev[i], hipEventDisableTiming) == hipSuccess;
        ok = ok && hipEventCreateWithFlags(&sv.ev_k[i], hipEventDisableTiming) == hipSuccess;
    }
    ok = ok && (sv.direct || hipStreamCreateWithFlags(&sv.copy, hipStreamNonBlocking) == hipSuccess);
    ok = ok && hipMalloc(reinterpret_cast<void **>(&sv.d_stats), 3 * sizeof(unsigned long long)) == hipSuccess;
    ok = ok && hipMemset(sv.d_stats, 0, 3 * sizeof(unsigned long long)) == hipSuccess;
    if (!ok) {
        fprintf(stderr, "irdm_hip: front end: save: allocating two slots of %zu bytes failed\n", slot_bytes);
        fe_save_off(fe);
        return -1;
    }
    sv.sink = cfg->sink;
    return 0;
}

extern "C" int irdm_frontend_save_stats(irdm_frontend_t *fe, irdm_band_stats_t *out)
{
    if (!fe || !out || !fe->sv.sink) return -1;
    (void)hipSetDevice(fe->cfg.device);
    IRDM_HIP_CHECK(hipStreamSynchronize(fe->stream));
    if (fe->sv.copy) IRDM_HIP_CHECK(hipStreamSynchronize(fe->sv.copy));
    unsigned long long h[3] = { 0, 0, 0 };
    IRDM_HIP_CHECK(hipMemcpy(h, fe->sv.d_stats, sizeof(h), hipMemcpyDeviceToHost));
    save_stats_out(fe->sv.format, h, fe->st.sv_samples, out);
    return 0;
}

extern "C" int irdm_requantize_device(const void *d_in, size_t n, int format, float gain, void *d_out, irdm_band_stats_t *stats,
                                      int device, void *stream_v)
{
    const int S = save_scale(format);
    if ((!S && format != IRDM_FMT_CF32) || !(gain > 0.0f) || !std::isfinite(gain) || (!S && gain != 1.0f) ||
        (S && !std::isfinite(gain * (float)S)) || (n && (!d_in || !d_out)))
        return -1;
    if (hipSetDevice(device) != hipSuccess) return -1;
    hipStream_t s = static_cast<hipStream_t>(stream_v);
    unsigned long long h[3] = { 0, 0, 0 };
    if (n && !S) {
        IRDM_HIP_CHECK(hipMemcpyAsync(d_out, d_in, n * sizeof(float2), hipMemcpyDeviceToDevice, s));
    } else if (n) {
        // (the statistics words of this call alone; read back, so the call waits for the stream whenever it has launched)
        unsigned long long *d_stats = nullptr;
        IRDM_HIP_CHECK(hipMalloc(reinterpret_cast<void **>(&d_stats), sizeof(h)));
        int rc = hipMemsetAsync(d_stats, 0, sizeof(h), s) == hipSuccess ? 0 : -1;
        if (rc == 0) rc = launch_requant(S == 128 ? 8 : 16, d_in, (long long)n, gain * (float)S, d_out, d_stats, s);
        if (rc == 0) rc = hipStreamSynchronize(s) == hipSuccess && hipMemcpy(h, d_stats, sizeof(h), hipMemcpyDeviceToHost) == hipSuccess ? 0 : -1;
        (void)hipFree(d_stats);
        if (rc != 0) return -1;
    }
    if (n && !S && !stream_v) IRDM_HIP_CHECK(hipStreamSynchronize(s));
    if (stats) save_stats_out(format, h, n, stats);
    return 0;
}

extern "C" int irdm_frontend_wait_input(irdm_frontend_t *fe)
{
    if (!fe) return -1;
    (void)hipSetDevice(fe->cfg.device);
    IRDM_HIP_CHECK(hipEventSynchronize(fe->ev_in));
    return 0;
}

extern "C" int irdm_frontend_kernel_clock(irdm_frontend_t *fe, double *sum_ms, uint64_t *launches, int reset)
{
    if (!fe) return -1;
    (void)hipSetDevice(fe->cfg.device);
    IRDM_HIP_CHECK(hipStreamSynchronize(fe->stream));
    unsigned long long h[3] = { 0, 0, 0 };
    IRDM_HIP_CHECK(hipMemcpy(h, fe->d_kclk + 128, sizeof(h), hipMemcpyDeviceToHost));
    if (sum_ms) *sum_ms = (double)h[0] * 1e-5;                   // 10 ns ticks
    if (launches) *launches = h[1];
    if (reset) {
        const unsigned long long z[3] = { 0, 0, 0 };
        IRDM_HIP_CHECK(hipMemcpy(fe->d_kclk + 128, z, sizeof(z), hipMemcpyHostToDevice));
    }
    return 0;
}

}  // namespace irdmh
