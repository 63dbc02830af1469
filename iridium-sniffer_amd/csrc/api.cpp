// api.cpp -- options and statistics of a context, the kernel clock, the RAW line printer (frame_output.c:160-199) and the
// --save-bursts file pair (qpsk_demod.c:339-389).
#include <stdarg.h>
#include "pipeline.hpp"

namespace irdmh {

extern "C" int irdm_set_option(irdm_pipeline_t *p, const char *key, int value)
{
    if (!p || !key) return -1;
    // (several keys allocate or launch: on the context's device, whichever device the calling thread was on)
    pipeline_enter(p);
    // ---- what a caller chooses (include/irdm_hip.h documents every key) ----
    if (!strcmp(key, "keep_frame_samples")) { p->keep_frame_samples = value; return 0; }
    if (!strcmp(key, "packed_records")) { p->packed_records = value; return 0; }
    if (!strcmp(key, "parsed_records")) { p->parsed_records = value; return 0; }
    if (!strcmp(key, "frame_records")) { p->frame_records = value; return 0; }
    if (!strcmp(key, "chunk_marks")) { p->chunk_marks = value ? 1 : 0; if (!value) p->st.q_marks.clear(); return 0; }
    if (!strcmp(key, "group_member")) { p->in_group = value != 0; return 0; }
    if (!strcmp(key, "spectrum_frames")) {
        // rows of `value` frames (0: off); not for a member of a group, and not between a stream's first feed and irdm_reset
        if (value < 0 || value > (1 << 20) || p->in_group || p->st.begin_no != 0) return -1;
        return spectrum_configure(p, value);
    }
    if (!strcmp(key, "input_stats")) {
        // 0 / 1; not for a member of a group (it is fed its chunk with the overlap in front: those samples would count twice),
        // and not while a chunk handed over with irdm_feed_begin waits for its irdm_feed_end
        if (p->in_group || p->st.begin_no != p->st.end_no) return -1;
        return input_stats_configure(p, value);
    }
    if (!strcmp(key, "symbol_clock")) {
        // 0 / 1; not for a member of a group (the summary is a context's, and a group merges no clock records), and not while
        // a chunk handed over with irdm_feed_begin waits for its irdm_feed_end
        if (p->in_group || p->st.begin_no != p->st.end_no) return -1;
        return symbol_clock_configure(p, value);
    }
    if (!strcmp(key, "fine_freq")) {
        // 0 / 1; not for a member of a group (the summary is a context's, and a group merges no such records), and not while
        // a chunk handed over with irdm_feed_begin waits for its irdm_feed_end
        if (p->in_group || p->st.begin_no != p->st.end_no) return -1;
        return fine_freq_configure(p, value);
    }
    if (!strcmp(key, "fine_time")) {
        // 0 / 1; as "fine_freq"
        if (p->in_group || p->st.begin_no != p->st.end_no) return -1;
        return fine_time_configure(p, value);
    }
    if (!strcmp(key, "iq_sense")) {
        // 0 / 1; not for a member of a group (the summary is a context's, and a group merges no votes), and not while a chunk
        // handed over with irdm_feed_begin waits for its irdm_feed_end
        if (p->in_group || p->st.begin_no != p->st.end_no) return -1;
        return iq_sense_configure(p, value);
    }
    if (!strcmp(key, "burst_resample")) {
        // 0 / 1; members of a group take it (no summary, no stream state); not while a chunk handed over with irdm_feed_begin
        // waits for its irdm_feed_end
        if (p->st.begin_no != p->st.end_no) return -1;
        return burst_resample_configure(p, value);
    }
    if (!strcmp(key, "swap_iq")) {
        // 0 / 1; not for a member of a group (it is fed on the device), and no change between a stream's first feed and
        // irdm_reset: the history ring would hold both senses
        if (p->in_group || (p->st.begin_no != 0 && (value != 0) != (p->hc.swap_iq != 0))) return -1;
        p->hc.swap_iq = value ? 1 : 0;
        return 0;
    }
    if (!strcmp(key, "scrub")) {
        // 0 / 1; not for a member of a group (it is fed on the device), and no change between a stream's first feed and
        // irdm_reset: the figures would describe half a stream
        if (p->in_group || (p->st.begin_no != 0 && (value != 0) != (p->hc.scrub.on != 0))) return -1;
        return scrub_configure(p, value);
    }
    if (!strcmp(key, "dc_block")) {
        // irdm_dc_block with a cf32 wire format, the block length of "dc_block_log2" and a zero seed (0: off)
        if (!value && !p->hc.dc.on) return 0;
        return dc_block_configure(p, IRDM_FMT_CF32, value ? p->hc.dc.log2 : -1, 0.0f, 0.0f);
    }
    if (!strcmp(key, "dc_block_log2")) {
        // 12 .. 24: the block length "dc_block" switches on with; as "dc_block", and not while it is on
        if (value < kDcMinLog2 || value > kDcMaxLog2 || p->in_group || p->hc.dc.on || p->st.begin_no != 0) return -1;
        p->hc.dc.DcRings::free();
        p->hc.dc.log2 = value;
        return 0;
    }
    if (!strcmp(key, "scrub_limit_log2")) {
        // 0 .. 127; as "scrub"
        if (value < 0 || value > 127 || p->in_group || (p->st.begin_no != 0 && value != p->hc.scrub.limit_log2)) return -1;
        p->hc.scrub.limit_log2 = value;
        return 0;
    }
    if (!strcmp(key, "iq_moments")) {
        // 0 / 1; as "input_stats"
        if (p->in_group || p->st.begin_no != p->st.end_no) return -1;
        return iq_moments_configure(p, value);
    }
    if (!strcmp(key, "decode_frames")) { p->decode_frames = value; return 0; }
    if (!strcmp(key, "decode_ida")) { p->decode_ida = value; return 0; }
    if (!strcmp(key, "detect_only")) { p->detect_only = value; return 0; }
    if (!strcmp(key, "fir_order") || !strcmp(key, "simd_order")) { p->fir_order = value ? 1 : 0; return 0; }
    if (!strcmp(key, "host_cfo")) { p->dev_cfo = p->dev_cfo_ok && value == 0; return 0; }      // 1: the fine-CFO libm step on the helper thread
    if (!strcmp(key, "scan_mode")) { p->scan_mode = value; return 0; }
    if (!strcmp(key, "kernel_clock")) { p->kernel_clock = value != 0; return 0; }
    if (!strcmp(key, "rot_prebuild")) {
        // 1: every centre bin's row in one background launch now (the default of a context with pipeline_depth >= 1);
        // 0: rows on demand only (the default otherwise); only before the first burst
        if (value) return p->rot_pre_runs ? 0 : rot_prebuild(p);
        return p->rot_pre_runs ? rot_arena_reset(p, (long long)std::min(p->P.n, 1024) * p->rot_runs) : 0;
    }
    // ---- diagnostic ----
    if (!strcmp(key, "band_timeline")) { p->band_tune.timeline = value != 0; return 0; }
    // ---- test hooks: paths a default run takes only on rare inputs ----
    if (!strcmp(key, "fir_generic")) { p->fir_generic = value != 0; return 0; }
    if (!strcmp(key, "post_generic")) { p->post_generic = value != 0; return 0; }
    if (!strcmp(key, "k1_lists")) { p->k1_lists = value; return 0; }
    if (!strcmp(key, "band_first")) { p->band_first = value < 0 ? 0 : value > kBandRounds ? kBandRounds : value; return 0; }
    if (!strcmp(key, "band_spec")) { p->band_spec_opt = value != 0; return 0; }
    if (!strcmp(key, "band_selfcheck")) { p->band_tune.selfcheck = value; return 0; }
    if (!strcmp(key, "rot_pool_rows")) {
        // (test hook) an empty on-demand rotator checkpoint arena with room for `value` whole rows (a prebuilt one is given
        // up); only before the first burst
        if (value < 1 || value > p->P.n) return -1;
        return rot_arena_reset(p, (long long)value * p->rot_runs);
    }
    if (!strcmp(key, "scratch_outputs")) {
        // (test hook) the decimated / low-passed scratch of every context with room for `value` outputs to begin with;
        // only while no batch is in flight
        if (value < 16) return -1;
        for (int i = 0; i < p->n_bc; i++)
            if (p->bc[i].st.n != 0) return -1;
        IRDM_HIP_CHECK(hipDeviceSynchronize());
        for (int i = 0; i < p->n_bc; i++) {
            BatchCtx &b = p->bc[i];
            float2 *d2 = dev_alloc<float2>((size_t)value), *l2 = dev_alloc<float2>(lpf_alloc((size_t)value));
            if (!d2 || !l2) return -1;
            (void)hipFree(b.d_dec);
            (void)hipFree(b.d_lpf);
            b.d_dec = d2;
            b.d_lpf = l2;
            if (b.d_res) {
                (void)hipFree(b.d_res);
                if (!(b.d_res = dev_alloc<float2>((size_t)value))) return -1;
            }
            b.dec_cap = (size_t)value;
            if (!b.owns_buffers) { p->d_dec = d2; p->d_lpf = l2; }
        }
        return 0;
    }
    return -1;
}

// ---- the frame line estimators (frame_line.hpp): the pinned records `hp` of every batch context, when an option is first set ----
template <typename Rec>
static int line_records_alloc(irdm_pipeline *p, Rec *BatchCtx::*hp)
{
    for (int i = 0; i < p->n_bc; i++) {
        BatchCtx &b = p->bc[i];
        if (!(b.*hp) &&
            hipHostMalloc(reinterpret_cast<void **>(&(b.*hp)), sizeof(Rec) * (size_t)p->burst_cap, hipHostMallocDefault) != hipSuccess)
            return -1;
    }
    return 0;
}

// ---- option "symbol_clock" (symbol_clock.hpp) ----
int symbol_clock_configure(irdm_pipeline *p, int on)
{
    if (on && line_records_alloc(p, &BatchCtx::hp_clock) != 0) return -1;
    p->symbol_clock = on ? 1 : 0;
    return 0;
}

extern "C" int irdm_poll_symbol_clock(irdm_pipeline_t *p, irdm_clock_est_t *out, int max)
{
    if (!p || !out || max < 0) return -1;
    return drain(p->st.clock.q, out, max);
}

extern "C" int irdm_symbol_clock(irdm_pipeline_t *p, irdm_symbol_clock_t *out)
{
    if (!p || !out || !p->bc[0].hp_clock) return -1;
    symbol_clock_result(p->st.clock, p->decim, out);
    return 0;
}

// ---- option "burst_resample" (burst_resample.hpp) ----
// L / M = decim 250000 / sample_rate in lowest terms
bool burst_resample_ratio(int sample_rate, int decim, long long *L, long long *M)
{
    if (sample_rate <= 0 || decim < 1) return false;
    long long a = (long long)decim * 250000, b = sample_rate;
    long long x = a, y = b;
    while (y) { const long long t = x % y; x = y; y = t; }
    *L = a / x;
    *M = b / x;
    return true;
}

// the ratio, its table on the device and the second scratch of every batch context, when the option is first set at a rate
// off the 250 kHz grid; at a rate on it, and with 0, nothing is allocated
int burst_resample_configure(irdm_pipeline *p, int on)
{
    if (!on) {
        p->burst_resample = 0;
        return 0;
    }
    long long L = 1, M = 1;
    if (!burst_resample_ratio(p->cfg.sample_rate, p->decim, &L, &M)) return -1;
    if (L > kBrMaxL) {
        fprintf(stderr, "irdm_hip: burst_resample: %d samples/s needs the ratio %lld/%lld, L = %lld is beyond %d\n",
                p->cfg.sample_rate, L, M, L, kBrMaxL);
        return -1;
    }
    if (L != M) {
        if (!burst_resample_ratio_ok(L, M)) return -1;
        for (int i = 0; i < p->n_bc; i++)
            if (p->bc[i].st.n != 0) return -1;
        if (!p->d_br_taps) {
            p->br_taps = design_resample_taps((int)L, (int)M, kBrTaps);
            if (!(p->d_br_taps = dev_upload(p->br_taps.data(), p->br_taps.size()))) return -1;
        }
        for (int i = 0; i < p->n_bc; i++) {
            BatchCtx &b = p->bc[i];
            if (!b.d_res && !(b.d_res = dev_alloc<float2>(b.dec_cap))) return -1;
        }
    }
    p->br_L = (int)L;
    p->br_M = (int)M;
    p->burst_resample = 1;
    return 0;
}

extern "C" int irdm_burst_resample_ratio(irdm_pipeline_t *p, int *L, int *M, int *taps_per_phase)
{
    if (!p || !p->burst_resample) return -1;
    const bool on_grid = p->br_L == p->br_M;
    if (L) *L = on_grid ? 1 : p->br_L;
    if (M) *M = on_grid ? 1 : p->br_M;
    if (taps_per_phase) *taps_per_phase = on_grid ? 0 : kBrTaps;
    return 0;
}

// the phase-major table [L][taps_per_phase] (irdm_burst_resample_ratio says how large): the floats copied, 0 at a rate on the
// grid, -1 where `cap` is too small -- as irdm_frontend_taps
extern "C" int irdm_burst_resample_taps(irdm_pipeline_t *p, float *out, int cap)
{
    if (!p || !p->burst_resample) return -1;
    if (p->br_L == p->br_M) return 0;
    const int n = (int)p->br_taps.size();
    if (!out || cap < n) return -1;
    memcpy(out, p->br_taps.data(), sizeof(float) * (size_t)n);
    return n;
}

// ---- option "fine_freq" (fine_freq.hpp) ----
int fine_freq_configure(irdm_pipeline *p, int on)
{
    if (on && line_records_alloc(p, &BatchCtx::hp_fine) != 0) return -1;
    p->fine_freq = on ? 1 : 0;
    return 0;
}

extern "C" int irdm_poll_fine_freq(irdm_pipeline_t *p, irdm_fine_freq_t *out, int max)
{
    if (!p || !out || max < 0) return -1;
    return drain(p->st.fine.q, out, max);
}

extern "C" int irdm_fine_freq(irdm_pipeline_t *p, irdm_fine_freq_summary_t *out)
{
    if (!p || !out || !p->bc[0].hp_fine) return -1;
    fine_freq_result(p->st.fine, out);
    return 0;
}

// ---- option "fine_time" (fine_time.hpp) ----
int fine_time_configure(irdm_pipeline *p, int on)
{
    if (on && line_records_alloc(p, &BatchCtx::hp_ftime) != 0) return -1;
    p->fine_time = on ? 1 : 0;
    return 0;
}

extern "C" int irdm_poll_fine_time(irdm_pipeline_t *p, irdm_fine_time_t *out, int max)
{
    if (!p || !out || max < 0) return -1;
    return drain(p->st.ftime.q, out, max);
}

extern "C" int irdm_fine_time(irdm_pipeline_t *p, irdm_fine_time_summary_t *out)
{
    if (!p || !out || !p->bc[0].hp_ftime) return -1;
    fine_time_result(p->st.ftime, out);
    return 0;
}

// ---- option "iq_sense" (iq_sense.hpp): the pinned records of every batch context, when the option is first set ----
int iq_sense_configure(irdm_pipeline *p, int on)
{
    for (int i = 0; on && i < p->n_bc; i++) {
        BatchCtx &b = p->bc[i];
        if (!b.hp_sense &&
            hipHostMalloc(reinterpret_cast<void **>(&b.hp_sense), sizeof(SenseRec) * (size_t)p->burst_cap, hipHostMallocDefault) != hipSuccess)
            return -1;
    }
    p->iq_sense = on ? 1 : 0;
    return 0;
}

extern "C" int irdm_poll_iq_votes(irdm_pipeline_t *p, irdm_iq_vote_t *out, int max)
{
    if (!p || !out || max < 0) return -1;
    return drain(p->st.iq.q, out, max);
}

extern "C" int irdm_iq_sense(irdm_pipeline_t *p, irdm_iq_sense_t *out)
{
    if (!p || !out || !p->bc[0].hp_sense) return -1;
    iq_sense_result(p->st.iq, out);
    return 0;
}

extern "C" int64_t irdm_get_stat(const irdm_pipeline_t *p, const char *key)
{
    if (!p || !key) return -1;
    if (!strcmp(key, "resets")) return (int64_t)p->stat_resets;
    if (!strcmp(key, "scan_fast_chunks")) return (int64_t)p->stat_fast_chunks;
    if (!strcmp(key, "scan_fallbacks")) return (int64_t)p->stat_fallbacks;
    if (!strncmp(key, "host_us_", 8) && key[8] >= '0' && key[8] <= '9') return (int64_t)p->host_us[key[8] - '0'];
    if (!strcmp(key, "band_chunks")) return (int64_t)p->stat_band_chunks;
    if (!strcmp(key, "band_extra")) return (int64_t)p->stat_band_extra;
    if (!strcmp(key, "scan_chained")) return (int64_t)p->stat_chained;
    if (!strcmp(key, "scan_chain_undone")) return (int64_t)p->stat_chain_undone;
    if (!strcmp(key, "k1_lists")) return (int64_t)p->stat_k1_lists;
    if (!strcmp(key, "band_rounds")) return (int64_t)p->stat_band_rounds;
    if (!strcmp(key, "band_retries")) return (int64_t)p->stat_band_retries;
    if (!strcmp(key, "band_aborts")) return (int64_t)p->stat_band_aborts;
    if (!strncmp(key, "tl_dur_", 7)) { const int i = atoi(key + 7); return i >= 0 && i < 32 ? (int64_t)p->stat_tl_dur[i] : -1; }
    if (!strncmp(key, "tl_gap_", 7)) { const int i = atoi(key + 7); return i >= 0 && i < 32 ? (int64_t)p->stat_tl_gap[i] : -1; }
    if (!strncmp(key, "tl_n_", 5)) { const int i = atoi(key + 5); return i >= 0 && i < 32 ? (int64_t)p->stat_tl_n[i] : -1; }
    if (!strncmp(key, "plan_tp_", 8)) {
        const int i = atoi(key + 8);
        return i >= 0 && i < 16 ? (int64_t)p->stat_plan_tp[i] : -1;
    }
    if (!strcmp(key, "rot_rows")) return (int64_t)p->rot_rows_used;
    if (!strcmp(key, "rot_prebuilt_runs")) return (int64_t)p->rot_pre_runs;
    if (!strcmp(key, "rot_rows_cap")) return (int64_t)(p->rot_blocks_cap / p->rot_runs);      // (in whole rows)
    if (!strcmp(key, "rot_blocks")) return (int64_t)p->rot_blocks_used;
    if (!strcmp(key, "rot_blocks_cap")) return (int64_t)p->rot_blocks_cap;
    if (!strcmp(key, "rot_grows")) return (int64_t)p->stat_rot_grows;
    if (!strcmp(key, "rot_builds")) return (int64_t)p->stat_rot_builds;
    if (!strcmp(key, "rot_runs")) return (int64_t)p->stat_rot_rows;
    if (!strcmp(key, "rot_ckpts")) return (int64_t)p->stat_rot_ckpts;
    if (!strcmp(key, "band_steps")) return (int64_t)p->stat_band_steps;
    if (!strcmp(key, "scratch_outputs")) return (int64_t)p->bc[0].dec_cap;
    if (!strcmp(key, "scratch_grows")) return (int64_t)p->stat_scratch_grows;
    if (!strcmp(key, "tiles_grows")) return (int64_t)p->stat_tiles_grows;
    if (!strcmp(key, "ring_waits")) return (int64_t)p->stat_ring_waits;
    if (!strcmp(key, "spec_passes")) return (int64_t)p->stat_spec_passes;
    if (!strcmp(key, "spec_scans")) return (int64_t)p->stat_spec_scans;
    if (!strcmp(key, "sum_restarts")) return (int64_t)p->stat_sum_restarts;
    if (!strcmp(key, "scratch_peak")) return (int64_t)p->stat_scratch_peak;
    if (!strcmp(key, "band_last_flags")) return (int64_t)p->last_band_flags;
    if (!strcmp(key, "scan_dense_frames")) return (int64_t)p->stat_dense_frames;
    if (!strcmp(key, "burst_resample_launches")) return (int64_t)p->stat_br_launches;
    if (!strcmp(key, "fine_freq_launches")) return (int64_t)p->stat_ff_launches;
    if (!strcmp(key, "fine_time_launches")) return (int64_t)p->stat_ft_launches;
    return -1;
}

// Kernel clock (option "kernel_clock" 1): the device's own record of a kernel's launches -- first wavefront in to last
// wavefront out, s_memrealtime -- summed since the last reset.  which: 0 the register-resident decimator, 1 K1.
extern "C" int irdm_kernel_clock(irdm_pipeline_t *p, int which, double *sum_ms, uint64_t *launches, double *last_ms, int reset)
{
    if (!p || !p->d_kclk || which < 0 || which > 1) return -1;
    pipeline_enter(p);
    if (hipDeviceSynchronize() != hipSuccess) return -1;
    std::vector<unsigned long long> h((size_t)(6 + kMaxBc - 3) * kKClkWords);
    if (hipMemcpy(h.data(), p->d_kclk, sizeof(unsigned long long) * h.size(), hipMemcpyDeviceToHost) != hipSuccess) return -1;
    unsigned long long ticks = 0, n = 0, last = 0;
    // (records 0..2 and 6..: the decimator per batch context; 3..5: K1 per feed slot)
    std::vector<int> recs;
    if (which == 1) recs = { 3, 4, 5 };
    else
        for (int c = 0; c < kMaxBc; c++) recs.push_back(c < 3 ? c : 3 + c);
    for (int r : recs) {
        ticks += h[(size_t)r * kKClkWords + 128];
        n += h[(size_t)r * kKClkWords + 129];
        if (h[(size_t)r * kKClkWords + 130] > last) last = h[(size_t)r * kKClkWords + 130];
    }
    if (sum_ms) *sum_ms = (double)ticks * 1e-5;          // 10 ns ticks
    if (launches) *launches = n;
    if (last_ms) *last_ms = (double)last * 1e-5;
    if (reset) {
        for (int r : recs) {
            unsigned long long z[3] = { 0, 0, 0 };
            if (hipMemcpy(p->d_kclk + (size_t)r * kKClkWords + 128, z, sizeof(z), hipMemcpyHostToDevice) != hipSuccess) return -1;
        }
    }
    return 0;
}

extern "C" int irdm_last_timings(const irdm_pipeline_t *p, float *ms_out, int n)
{
    if (!p || !ms_out) return -1;
    for (int i = 0; i < n && i < 6; i++) ms_out[i] = p->st.last_ms[i];
    return n < 6 ? n : 6;
}

// ===========================================================================
// 3. RAW line (frame_output.c:144-199)
// ===========================================================================
extern "C" int irdm_format_raw(const irdm_demod_t *f, const char *file_info, uint64_t *t0_io, char *buf,
                               size_t cap)
{
    if (!f || !t0_io || !buf) return -1;
    char auto_info[64];
    if (*t0_io == 0) *t0_io = (f->timestamp / 1000000000ULL) * 1000000000ULL;
    const uint64_t t0 = *t0_io;
    if (!file_info || !file_info[0]) {
        snprintf(auto_info, sizeof(auto_info), "i-%llu-t1", (unsigned long long)(t0 / 1000000000ULL));
        file_info = auto_info;
    }
    const double ts_ms = (double)(f->timestamp - t0) / 1000000.0;
    const int freq_hz = (int)(f->center_frequency + 0.5);
    const int payload = f->n_payload_symbols < 0 ? 0 : f->n_payload_symbols;
    int pos = snprintf(buf, cap, "RAW: %s %012.4f %010d N:%05.2f%+06.2f I:%011llu %3d%% %.5f %3d ", file_info,
                       ts_ms, freq_hz, f->magnitude, f->noise, (unsigned long long)f->id, f->confidence,
                       f->level, payload);
    if (pos < 0 || (size_t)pos + (size_t)f->n_bits + 2 > cap) return -1;
    for (int i = 0; i < f->n_bits; i++) buf[pos++] = (char)('0' + f->bits[i]);
    buf[pos++] = '\n';
    buf[pos] = 0;
    return pos;
}

// the same line from a compact record (option packed_records): bits 8 per byte, MSB first
extern "C" int irdm_format_raw_packed(const irdm_demod_packed_t *f, const char *file_info, uint64_t *t0_io, char *buf,
                                      size_t cap)
{
    if (!f || !t0_io || !buf) return -1;
    char auto_info[64];
    if (*t0_io == 0) *t0_io = (f->timestamp / 1000000000ULL) * 1000000000ULL;
    const uint64_t t0 = *t0_io;
    if (!file_info || !file_info[0]) {
        snprintf(auto_info, sizeof(auto_info), "i-%llu-t1", (unsigned long long)(t0 / 1000000000ULL));
        file_info = auto_info;
    }
    const double ts_ms = (double)(f->timestamp - t0) / 1000000.0;
    const int freq_hz = (int)(f->center_frequency + 0.5);
    const int payload = f->n_payload_symbols < 0 ? 0 : f->n_payload_symbols;
    int pos = snprintf(buf, cap, "RAW: %s %012.4f %010d N:%05.2f%+06.2f I:%011llu %3d%% %.5f %3d ", file_info,
                       ts_ms, freq_hz, f->magnitude, f->noise, (unsigned long long)f->id, f->confidence,
                       f->level, payload);
    const int nb = f->n_bits < 0 ? 0 : (f->n_bits > IRDM_MAX_BITS ? IRDM_MAX_BITS : f->n_bits);
    if (pos < 0 || (size_t)pos + (size_t)nb + 2 > cap) return -1;
    for (int i = 0; i < nb; i++) buf[pos++] = (char)('0' + ((f->bits[i >> 3] >> (7 - (i & 7))) & 1));
    buf[pos++] = '\n';
    buf[pos] = 0;
    return pos;
}

extern "C" long long irdm_format_raw_packed_batch(const irdm_demod_packed_t *f, int n, const char *file_info, uint64_t *t0_io,
                                                  char *buf, size_t cap)
{
    if (!f || n < 0 || !t0_io || !buf) return -1;
    size_t pos = 0;
    for (int i = 0; i < n; i++) {
        const int len = irdm_format_raw_packed(&f[i], file_info, t0_io, buf + pos, cap - pos);
        if (len < 0) return -1;
        pos += (size_t)len;
    }
    return (long long)pos;
}

// ===========================================================================
// 3b. IDA line (frame_output.c:203-361, --parsed)
// ===========================================================================
extern "C" void irdm_ida_unpack(const irdm_ida_packed_t *ida, const irdm_demod_packed_t *f, irdm_ida_t *out)
{
    if (!ida || !f || !out) return;
    // the IdaOut the decode_ida path would have, then its finish_ida with the frame fields that path reads
    IdaOut d;
    memset(&d, 0, sizeof(d));
    d.ok = ida->ok;
    d.ft = ida->ft; d.lcw_ft = ida->lcw_ft; d.lcw_code = ida->lcw_code; d.ec_lcw = ida->ec_lcw;
    d.lcw3_val = ida->lcw3_val;
    d.da_ctr = ida->da_ctr; d.da_len = ida->da_len; d.cont = ida->cont; d.crc_ok = ida->crc_ok;
    d.stored_crc = ida->stored_crc; d.computed_crc = ida->computed_crc;
    d.fixederrs = ida->fixederrs; d.payload_len = ida->payload_len; d.bch_len = ida->bch_len;
    memcpy(d.payload, ida->payload, sizeof(d.payload));
    for (int i = 0; i < 256; i++) d.bch_stream[i] = (uint8_t)((ida->bch_stream[i >> 3] >> (7 - (i & 7))) & 1);
    irdm_demod_t fr;
    memset(&fr, 0, offsetof(irdm_demod_t, bits));
    fr.id = f->id;
    fr.direction = f->direction;
    fr.timestamp = f->timestamp;
    fr.center_frequency = f->center_frequency;
    fr.magnitude = f->magnitude;
    fr.noise = f->noise;
    fr.level = f->level;
    fr.confidence = f->confidence;
    fr.n_payload_symbols = f->n_payload_symbols;
    *out = finish_ida(d, fr);
}

extern "C" void irdm_frame_unpack(const irdm_frame_packed_t *fr, const irdm_demod_packed_t *f, irdm_decoded_t *out)
{
    if (!fr || !f || !out) return;
    // the DecodedOut the decode_frames path would have, then its finish_decoded with the frame fields that path reads
    DecodedOut d;
    memset(&d, 0, sizeof(d));
    d.type = fr->type;
    d.sat_id = fr->sat_id;
    d.beam_id = fr->beam_id;
    for (int k = 0; k < 3; k++) d.pos_xyz[k] = fr->pos_xyz[k];
    d.n_pages = fr->n_pages;
    for (int k = 0; k < 12; k++) { d.page_tmsi[k] = fr->page_tmsi[k]; d.page_msc[k] = fr->page_msc[k]; }
    d.timeslot = fr->timeslot;
    d.sv_blocking = fr->sv_blocking;
    d.bc_type = fr->bc_type;
    d.iri_time = fr->iri_time;
    d.bch_len = fr->bch_len;
    *out = finish_decoded(d, f->id, f->timestamp, f->center_frequency);
}

namespace {

// an snprintf-style appender that fails once the line does not fit
struct LineBuf {
    char *buf;
    size_t cap, pos = 0;
    bool bad = false;
    void printf(const char *fmt, ...) __attribute__((format(printf, 2, 3)))
    {
        if (bad) return;
        va_list ap;
        va_start(ap, fmt);
        const int n = vsnprintf(buf + pos, cap - pos, fmt, ap);
        va_end(ap);
        if (n < 0 || (size_t)n >= cap - pos) bad = true;
        else pos += (size_t)n;
    }
    void put(char c)
    {
        if (bad || pos + 1 >= cap) { bad = true; return; }
        buf[pos++] = c;
        buf[pos] = 0;
    }
};

}  // namespace

extern "C" int irdm_format_ida(const irdm_ida_t *b, uint64_t *t0_io, char *buf, size_t cap)
{
    if (!b || !t0_io || !buf || cap == 0) return -1;
    if (*t0_io == 0) *t0_io = (b->timestamp / 1000000000ULL) * 1000000000ULL;
    const uint64_t t0 = *t0_io;
    LineBuf o{ buf, cap };
    buf[0] = 0;
    char parsed_info[64];
    snprintf(parsed_info, sizeof(parsed_info), "p-%llu", (unsigned long long)(t0 / 1000000000ULL));
    const double ts_ms = (double)(b->timestamp - t0) / 1000000.0;
    const int freq_hz = (int)(b->frequency + 0.5);
    const double leveldb = (b->level > 0) ? 20.0 * log10(b->level) : -99.99;
    const double noise = b->noise, snr = b->magnitude;
    const char *dir = b->direction == 2 ? "UL" : "DL";                  // DIR_UPLINK
    const int syms = b->n_symbols < 0 ? 0 : b->n_symbols;
    o.printf("IDA: %s %014.4f %010d %3d%% %06.2f|%07.2f|%05.2f %3d %s ", parsed_info, ts_ms, freq_hz, b->confidence,
             leveldb, noise, snr, syms, dir);
    o.printf("%.*s", (int)sizeof(b->lcw_header), b->lcw_header);
    const uint8_t *bs = b->bch_stream;
    const int bch_len = b->bch_len;
    if (bch_len >= 20) {
        o.printf("%c%c%c", '0' + bs[0], '0' + bs[1], '0' + bs[2]);
        o.printf(" cont=%c", '0' + bs[3]);
        o.printf(" %c", '0' + bs[4]);
        o.printf(" ctr=%c%c%c", '0' + bs[5], '0' + bs[6], '0' + bs[7]);
        o.printf(" %c%c%c", '0' + bs[8], '0' + bs[9], '0' + bs[10]);
        o.printf(" len=%02d", b->da_len);
        o.printf(" 0:%c%c%c%c", '0' + bs[16], '0' + bs[17], '0' + bs[18], '0' + bs[19]);
        o.printf(" [");
        // the payload's tail behind da_len all zero: da_len bytes, else all 20 with '!' at da_len (:261-289)
        bool all_zero = true;
        if (b->da_len > 0)
            for (int i = b->da_len + 1; i < 20; i++)
                if (b->payload[i] != 0) { all_zero = false; break; }
        const int nbytes = b->da_len > 0 && all_zero ? b->da_len : 20;
        for (int i = 0; i < nbytes; i++) {
            if (i > 0) o.put(nbytes == 20 && i == b->da_len && b->da_len > 0 && b->da_len < 20 ? '!' : '.');
            o.printf("%02x", b->payload[i]);
        }
        o.printf("]");
        for (int i = nbytes * 3; i < 60; i++) o.put(' ');               // hex + ']' padded to 60 columns
        if (b->da_len > 0) {
            o.printf(" %04x/%04x", b->stored_crc, b->computed_crc);
            o.printf(b->crc_ok ? " CRC:OK" : " CRC:no");
        } else {
            o.printf("  ---   ");
        }
        const int shown = bch_len < 256 ? bch_len : 256;
        if (bch_len > 9 * 20 + 16) {
            o.put(' ');
            for (int i = 9 * 20 + 16; i < shown; i++) o.put((char)('0' + bs[i]));
        } else {
            o.printf(" 0000");
        }
        if (b->da_len > 0 && bch_len >= 9 * 20) {
            o.printf(" SBD: ");
            for (int i = 0; i < 20; i++) {
                int byte = 0;
                for (int k = 0; k < 8; k++) byte = (byte << 1) | bs[1 * 20 + i * 8 + k];
                o.put(byte >= 32 && byte < 127 ? (char)byte : '.');
            }
        }
    }
    o.put('\n');
    return o.bad ? -1 : (int)o.pos;
}

extern "C" long long irdm_format_parsed_packed_batch(const irdm_demod_packed_t *f, const irdm_ida_packed_t *idas, int n,
                                                     const char *file_info, uint64_t *t0_io, char *buf, size_t cap)
{
    if (!f || !idas || n < 0 || !t0_io || !buf) return -1;
    size_t pos = 0;
    for (int i = 0; i < n; i++) {
        int len;
        if (idas[i].ok) {
            irdm_ida_t b;
            irdm_ida_unpack(&idas[i], &f[i], &b);
            len = irdm_format_ida(&b, t0_io, buf + pos, cap - pos);
        } else {
            len = irdm_format_raw_packed(&f[i], file_info, t0_io, buf + pos, cap - pos);
        }
        if (len < 0) return -1;
        pos += (size_t)len;
    }
    return (long long)pos;
}

// ===========================================================================
// 4. --save-bursts (qpsk_demod.c:339-389)
// ===========================================================================
extern "C" int irdm_save_burst(const irdm_frame_info_t *info, const float *samples, const char *dir)
{
    if (!info || !samples || !dir || info->drop_reason != 0 || info->num_samples <= 0) return -1;
    struct stat st;
    memset(&st, 0, sizeof(st));
    if (stat(dir, &st) == -1) {
        if (mkdir(dir, 0755) == -1 && errno != EEXIST) {
            fprintf(stderr, "Warning: failed to create burst save directory: %s\n", strerror(errno));
            return -1;
        }
    }
    const char *dir_str = info->demod_direction == 1 ? "DL" : info->demod_direction == 2 ? "UL" : "UN";
    char base[512];
    snprintf(base, sizeof(base), "%s/%020lu_%011.0f_%lu_%s", dir, (unsigned long)info->timestamp,
             info->center_frequency, (unsigned long)info->id, dir_str);
    char path[520];
    snprintf(path, sizeof(path), "%s.cf32", base);
    FILE *f = fopen(path, "wb");
    if (!f) {
        fprintf(stderr, "Warning: failed to save burst IQ: %s\n", strerror(errno));
        return -1;
    }
    fwrite(samples, 2 * sizeof(float), (size_t)info->num_samples, f);
    fclose(f);
    snprintf(path, sizeof(path), "%s.meta", base);
    f = fopen(path, "w");
    if (!f) return -1;
    fprintf(f, "burst_id: %lu\n", (unsigned long)info->id);
    fprintf(f, "timestamp_ns: %lu\n", (unsigned long)info->timestamp);
    fprintf(f, "center_freq_hz: %.0f\n", info->center_frequency);
    fprintf(f, "sample_rate_hz: %.0f\n", info->sample_rate);
    fprintf(f, "samples_per_symbol: %.2f\n", info->samples_per_symbol);
    fprintf(f, "direction: %s\n", dir_str);
    fprintf(f, "magnitude_db: %.2f\n", info->magnitude);
    fprintf(f, "noise_dbfs_hz: %.2f\n", info->noise);
    fprintf(f, "num_samples: %zu\n", (size_t)info->num_samples);
    fprintf(f, "uw_start_offset: %.2f\n", info->uw_start);
    fclose(f);
    return 0;
}

// many lines into one buffer: one write()/fwrite() per poll batch instead of the reference's fflush per line
// (frame_output.c:196-198), which is the sink bottleneck at >= 1e5 lines/s; the bytes are identical
extern "C" long long irdm_format_raw_batch(const irdm_demod_t *f, int n, const char *file_info, uint64_t *t0_io,
                                           char *buf, size_t cap)
{
    if (!f || n < 0 || !t0_io || !buf) return -1;
    size_t pos = 0;
    for (int i = 0; i < n; i++) {
        const int len = irdm_format_raw(&f[i], file_info, t0_io, buf + pos, cap - pos);
        if (len < 0) return -1;          // cap too small (IRDM_RAW_LINE_MAX bytes per frame always suffice)
        pos += (size_t)len;
    }
    return (long long)pos;
}

extern "C" const char *irdm_version(void) { return "irdm_hip 0.1 (gfx950)"; }

}  // namespace irdmh
