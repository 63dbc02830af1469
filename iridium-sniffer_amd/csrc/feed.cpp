// feed.cpp -- the feeding calls (irdm_feed_begin / _end / _device / _host, irdm_flush, irdm_advance), irdm_reset, the polls, and the
// buffer helpers for hosts without HIP headers.
#include <mutex>
#include "pipeline.hpp"

namespace irdmh {

// ---- option "spectrum_frames": mean and peak-hold spectra of K1's plane (detect.hip, KS) ----

// Buffers for rows of R frames, made when the option is first set (and again should a later R need larger ones): the two
// carry sets, the workspace of a chunk's cells, the device rows of one chunk and the pinned buffers they are copied to.
int spectrum_configure(irdm_pipeline *p, int R)
{
    if (R == 0) {
        p->spectrum_R = 0;
        return 0;
    }
    pipeline_enter(p);
    const size_t n = (size_t)p->P.n, max_frames = p->max_chunk / n;
    const size_t cells = (size_t)spectrum_cells_max((int)max_frames, R), rows = max_frames / (size_t)R + 1;
    if (!p->d_spec_carry) {
        if (!(p->d_spec_carry = dev_alloc<float>(6 * n))) return -1;
        IRDM_HIP_CHECK(hipMemset(p->d_spec_carry, 0, sizeof(float) * 6 * n));
        for (auto &e : p->ev_spec) IRDM_HIP_CHECK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    }
    if (cells > p->spec_ws_cells || rows > p->spec_out_rows) {
        IRDM_HIP_CHECK(hipStreamSynchronize(p->fstream));     // (nothing of a stream is in flight: the option is refused then)
        if (p->d_spec_ws) (void)hipFree(p->d_spec_ws);
        if (p->d_spec_out) (void)hipFree(p->d_spec_out);
        for (auto &h : p->hp_spec)
            if (h) (void)hipHostFree(h);
        p->d_spec_ws = p->d_spec_out = nullptr;
        for (auto &h : p->hp_spec) h = nullptr;
        p->spec_ws_cells = std::max(cells, p->spec_ws_cells);
        p->spec_out_rows = std::max(rows, p->spec_out_rows);
        p->d_spec_ws = dev_alloc<float>(2 * p->spec_ws_cells * n);
        p->d_spec_out = dev_alloc<float>(2 * p->spec_out_rows * n);
        bool ok = p->d_spec_ws && p->d_spec_out;
        for (auto &h : p->hp_spec)
            ok = ok && hipHostMalloc(reinterpret_cast<void **>(&h), sizeof(float) * 2 * p->spec_out_rows * n, hipHostMallocDefault) == hipSuccess;
        if (!ok) {
            p->spec_ws_cells = p->spec_out_rows = 0;
            p->spectrum_R = 0;
            return -1;
        }
    }
    p->spectrum_R = R;
    return 0;
}

// Batches whose copy has completed move from their pinned buffer to the row queue, oldest first.  wait_slot >= 0: the
// batch that holds that pinned buffer (and every older one) is waited for -- it was enqueued kSpecSlots feeds ago;
// wait_slot == kSpecSlots: all of them.
static int spectrum_harvest(irdm_pipeline *p, int wait_slot)
{
    StreamState &s = p->st;
    const size_t n = (size_t)p->P.n;
    while (!s.spec_pending.empty()) {
        const SpecBatch b = s.spec_pending.front();
        bool must = wait_slot == kSpecSlots;
        for (const SpecBatch &o : s.spec_pending) must = must || o.slot == wait_slot;
        if (must) IRDM_HIP_CHECK(hipEventSynchronize(p->ev_spec[b.slot]));
        else if (hipEventQuery(p->ev_spec[b.slot]) != hipSuccess) break;
        for (int i = 0; i < b.rows; i++) {
            SpecRow r;
            r.hdr.row = b.row0 + (uint64_t)i;
            r.hdr.first_frame = b.frame0 + (uint64_t)i * (uint64_t)p->spectrum_R;
            r.hdr.timestamp_ns = s.start_time_ns + s.prime_shift_ns + (uint64_t)((double)(r.hdr.first_frame * n) / (double)p->cfg.sample_rate * 1e9);
            r.hdr.n_frames = (uint32_t)b.n_frames;
            r.hdr.n_bins = (uint32_t)n;
            const float *src = p->hp_spec[b.slot] + (size_t)i * 2 * n;
            r.data.assign(src, src + 2 * n);
            s.spec_q.push_back(std::move(r));
        }
        s.spec_pending.pop_front();
    }
    return 0;
}

// `rows` rows of n_frames frames in d_spec_out, behind the launch that writes them on K1's stream: on their way to a pinned buffer
static int spectrum_send(irdm_pipeline *p, int rows, int n_frames)
{
    StreamState &s = p->st;
    const int slot = (int)(s.spec_batches % kSpecSlots);
    IRDM_HIP_CHECK(hipMemcpyAsync(p->hp_spec[slot], p->d_spec_out, sizeof(float) * 2 * (size_t)rows * (size_t)p->P.n, hipMemcpyDeviceToHost, p->fstream));
    IRDM_HIP_CHECK(hipEventRecord(p->ev_spec[slot], p->fstream));
    s.spec_pending.push_back(SpecBatch{ slot, rows, n_frames, s.spec_row, s.spec_row_frame });
    s.spec_batches++;
    s.spec_row += (uint64_t)rows;
    s.spec_row_frame += (uint64_t)rows * (uint64_t)n_frames;
    return 0;
}

// The reduction of a chunk's plane, behind its K1 on K1's stream: `mag` is written again by the K1 of a later feed on that
// same stream, so stream order alone keeps the plane until it has been read.
static int spectrum_enqueue(irdm_pipeline *p, const float *mag, int n_frames, uint64_t c0)
{
    StreamState &s = p->st;
    const int R = p->spectrum_R;
    if (!s.spec_started) {
        s.spec_started = true;
        s.spec_row_frame = (c0 - s.primed_samples) / (uint64_t)p->P.n;    // (a primed stream: frames of the recording)
    }
    if (spectrum_harvest(p, (int)(s.spec_batches % kSpecSlots)) != 0) return -1;
    if (launch_spectrum(mag, p->P.n, n_frames, R, s.spec_fill, p->spec_carry(s.spec_sel), p->spec_carry(s.spec_sel ^ 1), p->d_spec_ws,
                        p->spec_ws_cells, p->d_spec_out, p->spec_out_rows, p->fstream) != 0)
        return -1;
    const int rows = (s.spec_fill + n_frames) / R;
    s.spec_sel ^= 1;
    s.spec_fill = (s.spec_fill + n_frames) % R;
    return rows > 0 ? spectrum_send(p, rows, R) : 0;
}

// irdm_flush: the open row leaves with the frames it has, and every row enqueued so far arrives
static int spectrum_flush(irdm_pipeline *p)
{
    StreamState &s = p->st;
    if (s.spec_fill > 0) {
        if (spectrum_harvest(p, (int)(s.spec_batches % kSpecSlots)) != 0) return -1;
        if (launch_spectrum_close(p->P.n, s.spec_fill, p->spec_carry(s.spec_sel), p->d_spec_out, p->fstream) != 0) return -1;
        const int fill = s.spec_fill;
        s.spec_fill = 0;
        if (spectrum_send(p, 1, fill) != 0) return -1;
    }
    return spectrum_harvest(p, kSpecSlots);
}

// ---- option "input_stats": one reduction pass over the raw samples of every chunk (input_stats.hpp) ----

int input_stats_configure(irdm_pipeline *p, int on)
{
    if (on && p->in_stats.alloc(kIsBlockBytes, true) != 0) return -1;
    p->in_stats.on = on ? 1 : 0;
    return 0;
}

// ---- the chunk passes alone, on a buffer the caller owns (irdm_*_device) ----

// The stream such a call works on: the caller's, or one of its own, which finish() waits for and destroys.
struct CallerStream {
    hipStream_t s = nullptr, own = nullptr;
    CallerStream(int device, void *stream_v)
    {
        if (hipSetDevice(device) != hipSuccess) {
            fprintf(stderr, "irdm_hip: hipSetDevice(%d) failed\n", device);
            return;
        }
        s = static_cast<hipStream_t>(stream_v);
        if (!s && hipStreamCreateWithFlags(&own, hipStreamNonBlocking) == hipSuccess) s = own;
    }
    bool ok() const { return s != nullptr; }
    int finish(int rc)
    {
        if (own) {
            if (hipStreamSynchronize(own) != hipSuccess) rc = -1;
            (void)hipStreamDestroy(own);
            own = nullptr;
        }
        return rc;
    }
    ~CallerStream() { (void)finish(0); }
    CallerStream(const CallerStream &) = delete;
    CallerStream &operator=(const CallerStream &) = delete;
};

// A pass whose figures the call returns: n samples of bps bytes at d_in in launches of at most max_launch samples on s,
// all into one device block of block_bytes.  launch(in, piece, d_block) enqueues one and returns how many bytes of the
// block to read back (< 0: failed); they are waited for and handed to fold(host copy, off, piece).
template <typename Launch, typename Fold>
static int one_block_pass(const void *d_in, size_t n, size_t bps, size_t max_launch, size_t block_bytes, hipStream_t s,
                          Launch &&launch, Fold &&fold)
{
    void *d_block = nullptr;
    if (hipMalloc(&d_block, block_bytes) != hipSuccess) return -1;
    std::vector<unsigned char> h(block_bytes);
    int rc = 0;
    for (size_t off = 0; rc == 0 && off < n; off += max_launch) {
        const size_t piece = std::min(max_launch, n - off);
        const long long bytes = launch(static_cast<const char *>(d_in) + off * bps, piece, d_block);
        if (bytes < 0 || hipMemcpyAsync(h.data(), d_block, (size_t)bytes, hipMemcpyDeviceToHost, s) != hipSuccess ||
            hipStreamSynchronize(s) != hipSuccess)
            rc = -1;
        else
            fold(static_cast<const void *>(h.data()), off, piece);
    }
    (void)hipFree(d_block);
    return rc;
}

extern "C" int irdm_input_stats(irdm_pipeline_t *p, irdm_input_stats_t *out)
{
    if (!p || !out || !p->in_stats.stream) return -1;
    pipeline_enter(p);
    if (input_stats_settle(p->in_stats, p->st.in_stats, p->dev_fmt, ~0ull) != 0) return -1;
    input_stats_result(p->st.in_stats.run, p->dev_fmt, out);
    return 0;
}

extern "C" int irdm_input_stats_device(const void *d_in, size_t n, int format, irdm_input_stats_t *out, int device, void *stream_v)
{
    if (!out || (!d_in && n) || !fmt_valid(format) || (reinterpret_cast<uintptr_t>(d_in) % (size_t)fmt_bytes(format)) != 0) return -1;
    CallerStream cs(device, stream_v);
    if (!cs.ok()) return -1;
    InputStatsRun run;
    int grid = 0;
    const int rc = cs.finish(one_block_pass(
        d_in, n, (size_t)fmt_bytes(format), kIsMaxLaunch, kIsBlockBytes, cs.s,
        [&](const void *in, size_t piece, void *d_block) {
            grid = launch_input_stats(format, in, piece, d_block, cs.s);
            return grid < 0 ? -1ll : (long long)kIsBlockBytes;
        },
        [&](const void *h_block, size_t, size_t piece) { input_stats_fold(run, format, h_block, grid, piece); }));
    if (rc == 0) input_stats_result(run, format, out);
    return rc;
}

extern "C" int irdm_spectrum_bins(const irdm_pipeline_t *p) { return p ? p->P.n : -1; }

extern "C" int irdm_poll_spectrum(irdm_pipeline_t *p, irdm_spectrum_row_t *hdr, float *mean, float *peak, int max)
{
    if (!p || !hdr || !mean || !peak || max < 0) return -1;
    if (!p->st.spec_pending.empty()) {
        pipeline_enter(p);
        if (spectrum_harvest(p, -1) != 0) return -1;
    }
    const size_t n = (size_t)p->P.n;
    int k = 0;
    for (; k < max && !p->st.spec_q.empty(); k++) {
        const SpecRow &r = p->st.spec_q.front();
        hdr[k] = r.hdr;
        memcpy(mean + (size_t)k * n, r.data.data(), sizeof(float) * n);
        memcpy(peak + (size_t)k * n, r.data.data() + n, sizeof(float) * n);
        p->st.spec_q.pop_front();
    }
    return k;
}

extern "C" int irdm_flush(irdm_pipeline_t *p)
{
    if (!p) return -1;
    if (p->spectrum_R && p->st.begin_no == p->st.end_no) {
        pipeline_enter(p);
        if (spectrum_flush(p) != 0) return -1;
    }
    if (!p->depth) return 0;
    if (p->st.begin_no != p->st.end_no) return -1;        // a chunk handed over with irdm_feed_begin is still pending
    pipeline_enter(p);
    if (settle(p) != 0) return -1;
    int emitted = 0;
    // records leave in chunk order: the batches in flight, oldest first, then the pending bursts of the last scan
    for (;;) {
        BatchCtx *oldest = nullptr;
        for (int i = 0; i < p->n_bc; i++)
            if (p->bc[i].st.n > 0 && (!oldest || p->bc[i].st.chunk_no < oldest->st.chunk_no)) oldest = &p->bc[i];
        if (!oldest) break;
        const int e = deferred_finish(p, *oldest);
        if (e < 0) return -1;
        emitted += e;
    }
    if (p->st.has_pending) {
        BatchCtx &b = p->bc[p->st.pend_no % p->n_bc];
        if (deferred_enqueue(p) != 0) return -1;
        const int e = deferred_finish(p, b);
        if (e < 0) return -1;
        emitted += e;
    }
    return emitted;
}

// irdm_flush without the waiting: the detector scan in flight is settled and its bursts' per-burst chain ENQUEUED; records
// of batches that have finished come out, nothing else is waited for (a context that is still busy with an older batch is
// waited for only if the new chain needs that very context).  What a rank of a time-sharded stream calls at the end of a
// super-step: its chain then runs beside the next super-step's scatter, K1 and scan (sharding.TimeShard).  Returns the
// number of bursts whose records were emitted, -1 on error.
extern "C" int irdm_advance(irdm_pipeline_t *p)
{
    if (!p) return -1;
    if (!p->depth) return 0;
    if (p->st.begin_no != p->st.end_no) return -1;
    pipeline_enter(p);
    if (settle(p) != 0) return -1;
    int emitted = 0;
    auto oldest_of = [&]() -> BatchCtx * {
        BatchCtx *o = nullptr;
        for (int i = 0; i < p->n_bc; i++)
            if (p->bc[i].st.n > 0 && (!o || p->bc[i].st.chunk_no < o->st.chunk_no)) o = &p->bc[i];
        return o;
    };
    for (BatchCtx *o; (o = oldest_of()) != nullptr && (p->detect_only || hipStreamQuery(o->stream) == hipSuccess);) {
        const int e = deferred_finish(p, *o);
        if (e < 0) return -1;
        emitted += e;
    }
    if (p->st.has_pending) {
        BatchCtx &b = p->bc[p->st.pend_no % p->n_bc];
        while (b.st.n > 0) {            // (records leave in chunk order: everything older than the batch in the way goes first)
            const int e = deferred_finish(p, *oldest_of());
            if (e < 0) return -1;
            emitted += e;
        }
        if (deferred_enqueue(p) != 0) return -1;
    }
    return emitted;
}

// The context back to what irdm_create returned, for another stream at the same rate, format and options (DESIGN.md
// section 4 sorts every field of irdm_pipeline into configuration, cache and stream state; the third kind is StreamState,
// BatchCtx::State and FeedSlot::State of pipeline.hpp, and this function assigns fresh ones).  The old stream is abandoned
// where it stands: the scan and the chains in flight are waited for -- stream by stream, the device as a whole is not --
// and what they produced is dropped with the queues.  The history ring keeps its contents: no reader takes a slot of an
// absolute index the NEW stream has not written (burst_src.hpp: a sample at or past avail_end comes from index
// a - ref_ring, zero below ref_ring; K1 reads the chunk it is handed, in place or not).
extern "C" int irdm_reset(irdm_pipeline_t *p, double center_frequency, uint64_t start_time_ns)
{
    if (!p || p->in_group) return -1;
    if (p->st.begin_no != p->st.end_no) return -1;  // a chunk handed over with irdm_feed_begin still waits for its irdm_feed_end
    if (p->st.gate_open_pending) {
        fprintf(stderr, "irdm_hip: irdm_reset while a scan waits for a history import (irdm_expect_history)\n");
        return -1;
    }
    pipeline_enter(p);
    // 1. whatever the old stream still has on the device: K1 and ring copies, the scan (and a speculation pass beside it),
    //    the per-burst chains with their host step
    IRDM_HIP_CHECK(hipStreamSynchronize(p->fstream));
    if (p->stream != p->fstream) IRDM_HIP_CHECK(hipStreamSynchronize(p->stream));
    if (p->stream_spec) IRDM_HIP_CHECK(hipStreamSynchronize(p->stream_spec));
    if (p->in_stats.stream) IRDM_HIP_CHECK(hipStreamSynchronize(p->in_stats.stream));   // (its totals go with the stream state)
    if (p->iqm.stream) IRDM_HIP_CHECK(hipStreamSynchronize(p->iqm.stream));             // (likewise)
    for (int i = 0; i < p->n_bc; i++) {
        BatchCtx &b = p->bc[i];
        IRDM_HIP_CHECK(hipStreamSynchronize(b.stream));
        p->rot_done_gen[i] = p->rot_gen[i];         // (its rotator checkpoint builds are complete: the rows are kept)
        b.st = BatchCtx::State{};                   // only now: the helper thread reads st.n while the chain is in flight
        b.hp_flag[1] = 0;
    }
    // 2. device side, on the detector's stream: the detector state, the running sums and the 512-frame history as
    //    irdm_create leaves them; the band scan's commit / void markers and the speculation workspace's carried state.
    //    (K1's candidate lists are rebuilt by every irdm_feed_begin and marked per feed slot below; every other scan
    //    buffer is written before it is read.)  The first scan of the new stream is enqueued behind this on the same
    //    stream; K1 reads the sums only once the host has seen a scan prime the detector.
    const DetParams &P = p->P;
    IRDM_HIP_CHECK(hipMemsetAsync(p->d_hist, 0, sizeof(float) * (size_t)kHistory * P.n, p->stream));
    ZeroRegions z;
    bool ok = z.add(p->d_state, sizeof(DetState)) && z.add(p->d_sum, sizeof(float) * (size_t)P.n);
    if (p->band_ok) ok = ok && z.add(p->band.bar, 256);
    if (p->d_band_spec)
        ok = ok && z.add(p->band_spec.ctl, sizeof(BandCtl)) && z.add(p->band_spec.bar, 256) &&
             z.add(p->band_spec.rec_count, 4 * 64) && z.add(p->band_spec.flags, 256) && z.add(p->d_state_spec, sizeof(DetState));
    if (!ok || launch_zero_regions(z, p->stream) != 0) return -1;
    // (option "spectrum_frames": both carry sets, on the stream the next reduction runs on)
    if (p->d_spec_carry) IRDM_HIP_CHECK(hipMemsetAsync(p->d_spec_carry, 0, sizeof(float) * 6 * (size_t)P.n, p->fstream));
    // 3. host side: a fresh stream state (the types say which fields that is), the pinned words the scans export to
    p->st = StreamState{};
    for (auto &f : p->fs) f.st = FeedSlot::State{};
    for (int s = 0; s < 2; s++) memset(p->h_pin_set[s], 0, sizeof(int) * 128);
    p->cfg.center_frequency = center_frequency;
    p->st.start_time_ns = start_time_ns;
    if (p->st.start_time_ns == 0) {
        struct timespec ts;
        clock_gettime(CLOCK_REALTIME, &ts);
        p->st.start_time_ns = ts.tv_sec * 1000000000ULL + ts.tv_nsec;
    }
    p->stat_resets++;
    return 0;
}

// A feed in two halves.  irdm_feed_begin: everything that does not depend on the detector state -- K1 of the chunk and
// (pipeline_depth >= 1) its copy into the history ring.  irdm_feed_end: the detector scan and the per-burst work.  A
// time-sharded rank calls them around the arrival of the previous rank's state (sharding.py); irdm_feed_device is the
// two back to back.
extern "C" int irdm_feed_begin(irdm_pipeline_t *p, const void *d_iq, size_t n_samples, void *stream_v)
{
    if (!p || (!d_iq && n_samples) || hc_refuses(p->hc, 0)) return -1;
    if (p->st.begin_no - p->st.end_no > (p->depth ? kLookAhead : 0u)) return -1;    // two chunks of look-ahead, pipeline_depth >= 1 only
    if (p->st.stream_closed) {
        fprintf(stderr, "irdm_hip: stream already ended by a chunk that was not a multiple of feed_block\n");
        return -1;
    }
    if (n_samples > p->max_chunk) {
        fprintf(stderr, "irdm_hip: chunk of %zu samples exceeds max_chunk_samples %zu\n", n_samples, p->max_chunk);
        return -1;
    }
    if (n_samples % p->feed_block != 0) p->st.stream_closed = true;     // last, ragged chunk of the stream
    pipeline_enter(p);
    // order after the caller's stream (the producer of d_iq)
    hipStream_t caller = static_cast<hipStream_t>(stream_v);
    // stream == NULL: the chunk is already complete in memory, nothing to order against.  (Not the legacy null stream,
    // which would wait for every other stream including the detector scan in flight; and no event on a foreign stream
    // when it is not needed: streams share hardware queues, and an event recorded on a stream that shares one with the
    // detector's sits behind the scan -- measured: K1 of the next chunk then started only after the scan had ended.)
    if (caller) {
        IRDM_HIP_CHECK(hipEventRecord(p->ev[8], caller));
        if (caller != p->fstream) IRDM_HIP_CHECK(hipStreamWaitEvent(p->fstream, p->ev[8], 0));
    }
    const DetParams &P = p->P;
    const uint64_t c0 = p->st.begun_samples, c1 = c0 + n_samples;
    const int n_frames = (int)(n_samples / (size_t)P.n);
    // option "input_stats": the chunk's pass, on its side stream behind the chunk's arrival (settled by this chunk's
    // irdm_feed_end, before the caller may overwrite d_iq)
    if (p->in_stats.on && !p->priming &&
        input_stats_enqueue(p->in_stats, p->st.in_stats, p->dev_fmt, d_iq, n_samples, caller, p->st.begin_no) != 0)
        return -1;
    // option "iq_moments": likewise, on a side stream of its own
    if (p->iqm.on && !p->priming && iq_moments_enqueue(p->iqm, p->st.iqm, p->dev_fmt, d_iq, n_samples, caller, p->st.begin_no) != 0) return -1;

    // K1 of this chunk.  pipeline_depth 1: on its own stream and into the other magnitude buffer, while the detector
    // scan of the previous chunk may still be running
    FeedSlot &f = p->fs[p->st.begin_no % kFeedSlots];
    float *const mags[kFeedSlots] = { p->d_mag, p->d_mag2, p->d_mag3 };
    float *mag = p->depth ? mags[p->st.begin_no % kFeedSlots] : p->d_mag;
    // written in place (irdm_ingest_ptr)?  Then the ring already holds the chunk.
    const uint64_t pos = c0 % p->ring_len;
    const bool in_ring = p->depth && n_samples > 0 && pos + n_samples <= p->ring_len &&
                         d_iq == static_cast<const char *>(p->d_ring) + pos * p->bps;
    IRDM_HIP_CHECK(hipEventRecord(f.ev_start, p->fstream));
    // K1, with the band scan's candidate lists where the scan will want them: the reference levels are the running
    // sums as they are NOW (the previous chunk's scan may still be at work on them -- any levels do, the scan checks the
    // lists against the ones they were built with, scan_band.hip band_sum_kernel); not before the detector is primed
    // (no sums yet: every bin would be listed)
    const int ls = p->depth ? (int)(p->st.begin_no % kFeedSlots) : 0;       // (pipeline_depth 0: one chunk at a time, one set)
    f.st.lists = false;
    if (p->k1_lists && p->st.host_primed && scan_pick(p) == 2 && p->k1_pre[ls] && n_frames > 0) {
        if (launch_prefilter_threshold(p->d_sum, P.threshold, p->k1_pre[ls], P.n, p->fstream) != 0) return -1;
        const int rc = launch_fft_mag_lists(P.log_n, p->dev_fmt, d_iq, p->d_window, p->d_tw, mag, n_frames, p->k1_pre[ls],
                                            p->k1_counts[ls], p->k1_entries[ls], band_list_cap(P.n), p->fstream,
                                            p->kclk_rec(3 + ls % 3), p->fir_order);
        if (rc < 0) return -1;
        f.st.lists = rc == 0;
    }
    if (!f.st.lists && launch_fft_mag(P.log_n, p->dev_fmt, d_iq, p->d_window, p->d_tw, mag, n_frames, p->fstream,
                                   p->kclk_rec(3 + ls % 3), p->fir_order) != 0)
        return -1;
    IRDM_HIP_CHECK(hipEventRecord(f.ev_k1, p->fstream));
    if (n_frames > 0 && launch_kclk_fold(p->kclk_rec(3 + ls % 3), p->fstream) != 0) return -1;   // (behind the event the scan waits for)
    // this chunk into the history ring, behind K1 on its stream (the ring keeps the chunks the per-burst chains in
    // flight still read: the copy never overwrites them)
    if (p->depth && !in_ring && (ring_guard(p, c0, c1, p->fstream) != 0 || ring_update(p, d_iq, c0, c1, p->fstream) != 0)) return -1;
    IRDM_HIP_CHECK(hipEventRecord(f.ev_copy, p->fstream));
    // option "spectrum_frames": the plane's reduction, behind everything a feed waits for
    if (p->spectrum_R && !p->priming && n_frames > 0 && spectrum_enqueue(p, mag, n_frames, c0) != 0) return -1;
    f.st.iq = d_iq;
    f.st.c0 = c0;
    f.st.c1 = c1;
    f.st.mag = mag;
    f.st.frames = n_frames;
    f.st.in_ring = in_ring;
    p->st.begun_samples = c1;
    p->st.begin_no++;
    return 0;
}

extern "C" int irdm_feed_end(irdm_pipeline_t *p)
{
    if (!p || p->st.begin_no == p->st.end_no) return -1;
    pipeline_enter(p);
    FeedSlot &f = p->fs[p->st.end_no % kFeedSlots];
    const void *d_iq = f.st.iq;
    const uint64_t c0 = f.st.c0, c1 = f.st.c1;
    float *mag = f.st.mag;
    const int n_frames = f.st.frames;
    float ms = 0;

    int emitted = 0;
    if (!p->depth) {
        int n_gone = 0;
        p->st.fl_feed = &f;
        if (scan_launch(p, mag, n_frames, c1) != 0 || scan_finish(p, &n_gone) != 0) return -1;
        p->st.last_bursts.clear();
        p->st.last_chunk = d_iq;
        p->st.last_chunk_start = c0;
        p->st.last_chunk_end = c1;
        const SampleSource src = make_source(p, d_iq, c0, c1);
        // record the stage events once so an empty chunk has valid timings
        for (int i = 0; i < 4; i++) IRDM_HIP_CHECK(hipEventRecord(p->bc[0].ev[i], p->bc[0].stream));
        if (process_bursts(p, p->bc[0], src, p->h_gone.data(), n_gone) != 0) return -1;
        if (ring_update(p, d_iq, c0, c1, p->stream) != 0) return -1;
        IRDM_HIP_CHECK(hipEventRecord(p->ev[7], p->stream));
        IRDM_HIP_CHECK(hipStreamSynchronize(p->stream));
        emitted = n_gone;
    } else {
        auto now_us = [] {
            struct timespec ts;
            clock_gettime(CLOCK_MONOTONIC, &ts);
            return ts.tv_sec * 1e6 + ts.tv_nsec * 1e-3;
        };
        double t0 = now_us(), t1;
#define IRDM_HOST_PHASE(i) do { t1 = now_us(); p->host_us[i] += t1 - t0; t0 = t1; } while (0)
        IRDM_HOST_PHASE(0);
        p->st.last_bursts.clear();
        // 0. if the oldest chain has already finished, its records are built NOW, while the previous chunk's detector
        //    scan is still running (0.3 ms of host work that would otherwise follow the wait for the scan)
        BatchCtx &oldest = p->bc[p->st.chunk_no % p->n_bc];
        bool finished_early = false;
        if (oldest.st.n > 0 && !p->detect_only && p->st.fl_active && hipStreamQuery(oldest.stream) == hipSuccess) {
            emitted = deferred_finish(p, oldest);
            if (emitted < 0) return -1;
            finished_early = true;
        }
        IRDM_HOST_PHASE(4);
        // 1. this chunk's band scan goes behind the previous chunk's (scan_chain_try), then the previous chunk's is
        //    settled and its bursts collected
        // (already chained at the end of the previous feed -- scan_chain_early, below -- unless that could not be done)
        if (!(p->st.chain_pending && p->st.chain_no == p->st.chunk_no) && scan_chain_try(p, f, p->st.chunk_no) != 0) return -1;
        if (settle(p) != 0) return -1;
        if (p->st.chain_pending && !p->st.settle_clean) {
            // the scan in front did not commit on its own: the chained launch has declined itself (nothing written)
            IRDM_HIP_CHECK(hipStreamSynchronize(p->stream));
            p->st.chain_pending = false;
            p->stat_chain_undone++;
        }
        IRDM_HOST_PHASE(1);
        // 2. this chunk's detector (needs K1's output) goes first: the next chunk's scan can only start when this one
        //    has ended, so every microsecond before its launch is added to the period
        IRDM_HIP_CHECK(hipStreamWaitEvent(p->stream, f.ev_k1, 0));
        p->st.fl_feed = &f;
        if (scan_launch(p, mag, n_frames, c1) != 0) return -1;
        IRDM_HOST_PHASE(3);
        // 3. the per-burst stages of the chunk just settled: enqueued on the idle batch context, nothing waits.  (The
        //    context of the chunk before that is still at work: its tail overlaps this one's FIR.)
        if (deferred_enqueue(p) != 0) return -1;
        IRDM_HOST_PHASE(2);
        // 3b. the next chunk, if its feed has begun (look-ahead): its round 0 as a speculation pass beside this chunk's scan
        if (p->st.begin_no > p->st.end_no + 1 && p->st.fl_mode == 2 && p->st.fl_band_ran &&
            spec_enqueue(p, p->fs[(p->st.end_no + 1) % kFeedSlots], p->st.chunk_no + 1) != 0)
            return -1;
        // 3c. ... and its scan, chained behind this chunk's, NOW: what follows -- the wait for the oldest chain, the records,
        //     the caller's polls and its next irdm_feed_begin -- took 0.4-0.8 ms, during which the scan's stream ran dry
        //     after every scan: the period was (that host time + a scan) / 2, not a scan.
        //     The same launch the next irdm_feed_end would make first thing -- it finds it done.
        if (p->st.begin_no > p->st.end_no + 1 && !p->st.chain_pending &&
            scan_chain_try(p, p->fs[(p->st.end_no + 1) % kFeedSlots], p->st.chunk_no + 1) != 0)
            return -1;
        // 4. results of the older batch: its context is the one the NEXT chunk's bursts will use
        if (!finished_early) {
            emitted = deferred_finish(p, oldest);
            if (emitted < 0) return -1;
        }
        IRDM_HOST_PHASE(4);
        // 5. the caller may overwrite d_iq once we return: K1 and the ring copy are done with it.  (A chunk written in
        //    place stays where it is; K1 is waited for only so that its time can be read.)
        IRDM_HIP_CHECK(hipEventSynchronize(f.st.in_ring ? f.ev_k1 : f.ev_copy));
        IRDM_HOST_PHASE(5);
#undef IRDM_HOST_PHASE
    }
    if (!p->st.in_stats.pending.empty() &&
        input_stats_settle(p->in_stats, p->st.in_stats, p->dev_fmt, p->st.end_no) != 0)
        return -1;
    if (!p->st.iqm.pending.empty() && iq_moments_settle(p->iqm, p->st.iqm, p->st.end_no) != 0) return -1;
    p->st.chunk_no++;
    p->st.end_no++;
    p->st.total_samples = c1;

    // [0] K1, [5] the whole call on the detector side; [1] is set by scan_finish, [2..4] by bursts_finish
    p->st.last_ms[0] = hipEventElapsedTime(&ms, f.ev_start, f.ev_k1) == hipSuccess ? ms : -1.0f;
    p->st.last_ms[5] = !p->depth && hipEventElapsedTime(&ms, f.ev_start, p->ev[7]) == hipSuccess ? ms : -1.0f;
    return emitted;
}

extern "C" int irdm_feed_device(irdm_pipeline_t *p, const void *d_iq, size_t n_samples, void *stream_v)
{
    if (irdm_feed_begin(p, d_iq, n_samples, stream_v) != 0) return -1;
    return irdm_feed_end(p);
}

// Where the producer of the next chunk (an H2D copy, a conversion kernel) may write it so that it needs no copy into
// the history ring: the ring slot of the absolute sample index the next irdm_feed_begin starts at.  NULL when the
// context keeps no ring copy (pipeline_depth 0) or the chunk would straddle the end of the ring (it cannot when every
// chunk but the last has max_chunk_samples: the ring is a whole number of them).  The slot is the producer's until it
// hands it over with irdm_feed_begin(p, ptr, n, stream); it is overwritten ring_len samples later.
extern "C" void *irdm_ingest_ptr(irdm_pipeline_t *p, size_t n_samples)
{
    if (!p || !p->depth || n_samples == 0 || n_samples > p->max_chunk) return nullptr;
    const uint64_t pos = p->st.begun_samples % p->ring_len;
    if (pos + n_samples > p->ring_len) return nullptr;
    return static_cast<char *>(p->d_ring) + pos * p->bps;
}

extern "C" void *irdm_ring_ptr(irdm_pipeline_t *p, uint64_t *len_samples)
{
    if (!p) return nullptr;
    if (len_samples) *len_samples = p->ring_len;
    return p->d_ring;
}

// Pinned host memory for irdm_feed_host callers that have no HIP headers (the C99 host): H2D copies from pinned
// memory are asynchronous DMA at PCIe rate; from pageable memory they are staged and block the host.
extern "C" void *irdm_host_alloc(size_t bytes)
{
    void *q = nullptr;
    if (hipHostMalloc(&q, bytes, hipHostMallocDefault) != hipSuccess) return nullptr;
    return q;
}

extern "C" void irdm_host_free(void *q)
{
    if (q) (void)hipHostFree(q);
}

extern "C" void *irdm_device_alloc(int device, size_t bytes)
{
    void *q = nullptr;
    if (hipSetDevice(device) != hipSuccess || hipMalloc(&q, bytes) != hipSuccess) return nullptr;
    return q;
}

extern "C" void irdm_device_free(void *q)
{
    if (q) (void)hipFree(q);
}

extern "C" int irdm_device_upload(void *dptr, const void *host, size_t bytes)
{
    if (!dptr || (!host && bytes)) return -1;
    IRDM_HIP_CHECK(hipMemcpy(dptr, host, bytes, hipMemcpyHostToDevice));
    return 0;
}

extern "C" int irdm_device_download(void *host, const void *dptr, size_t bytes)
{
    if ((!dptr || !host) && bytes) return -1;
    IRDM_HIP_CHECK(hipMemcpy(host, dptr, bytes, hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int irdm_device_copy(void *dst, const void *src, size_t bytes)
{
    if ((!dst || !src) && bytes) return -1;
    IRDM_HIP_CHECK(hipMemcpy(dst, src, bytes, hipMemcpyDeviceToDevice));
    return 0;
}

// The own place of the next chunk of irdm_feed_host, n_samples long.  Throughput mode: its slot of the history ring, where it
// is fed in place (no staging buffer, no device-to-device copy behind K1); else d_stage -- irdm_feed_device returns only
// after K1 and the history-ring copy of its chunk are done, so one staging buffer is enough.  nullptr: no memory.
static void *feed_host_place(irdm_pipeline *p, size_t n_samples)
{
    if (void *slot = irdm_ingest_ptr(p, n_samples)) return slot;
    if (!p->d_stage && hipMalloc(&p->d_stage, p->max_chunk * p->bps) != hipSuccess) return nullptr;
    return p->d_stage;
}

// a chunk of irdm_feed_host whose bytes have been put at hc_landing(d_iq) on fstream: corrected into d_iq, its own place,
// behind the copy and in front of everything that reads it (host_chain.hpp; the prefix of irdm_prime_* like any chunk, without
// figures), and fed from there
static int feed_host_arrived(irdm_pipeline *p, void *d_iq, size_t n_samples)
{
    if (hc_apply(p->hc, p->st.hc, p->dev_fmt, d_iq, hc_landing(p->hc, d_iq), n_samples, p->st.begun_samples - p->st.primed_samples,
                 !p->priming, p->fstream) != 0)
        return -1;
    p->hc.inner = true;
    const int rc = irdm_feed_device(p, d_iq, n_samples, p->fstream);
    p->hc.inner = false;
    return rc;
}

extern "C" int irdm_feed_host(irdm_pipeline_t *p, const void *h_iq, size_t n_samples)
{
    if (!p || (!h_iq && n_samples)) return -1;
    if (n_samples > p->max_chunk) return -1;
    pipeline_enter(p);
    void *place = feed_host_place(p, n_samples);
    if (!place) return -1;
    // Raw bytes in the wire format (the ci16 narrowing of main.c:245-246 happens in the kernels' load stage).
    // The copy goes on K1's stream, never the null stream: with pipeline_depth 1 the previous chunk's detector scan is
    // still running and must not be waited for.
    IRDM_HIP_CHECK(hipMemcpyAsync(hc_landing(p->hc, place), h_iq, n_samples * (size_t)fmt_bytes(hc_wire_fmt(p->hc, p->dev_fmt)),
                                  hipMemcpyHostToDevice, p->fstream));
    return feed_host_arrived(p, place, n_samples);
}

// ---- irdm_prime_host / irdm_prime_device: the detector's 512-frame history filled from the recording's own head ----

// May the context be primed from n_samples leading samples?  The whole frames that would be used (1 .. 512), or -1: not a
// fresh stream (something has been fed, imported or primed since irdm_create / irdm_reset), a member of a group, fewer
// samples than one frame, or a feed_block that 512 frames are not a whole number of.
int prime_check(const irdm_pipeline *p, size_t n_samples)
{
    if (!p || p->in_group) return -1;
    const StreamState &s = p->st;
    if (s.begin_no || s.begun_samples || s.total_samples || s.chunk_no || s.host_primed || s.primed_samples || s.stream_closed ||
        s.gate_armed || s.gate_open_pending)
        return -1;
    const size_t N = (size_t)p->P.n, H = (size_t)kHistory * N;
    if (H % (size_t)p->feed_block != 0 || n_samples < N) return -1;
    return (int)std::min<size_t>((size_t)kHistory, n_samples / N);
}

// The prefix P -- frame k of it is frame k mod F of the F whole frames at d_head (device memory, the format irdm_feed_host
// takes; whatever produced them lies in front on fstream) -- fed as the head of the stream: every piece of at most
// max_chunk is put together by device copies where a chunk of irdm_feed_host lands, and goes the way such a chunk goes
// (swap_iq, irdm_iq_balance, scrub, K1, the ring, the scan) with the side passes off; the time origin moves back by the
// prefix.  -1: a feed failed and the stream stands where it stopped (irdm_reset starts over).
int prime_from_device(irdm_pipeline *p, const void *d_head, int F)
{
    const size_t N = (size_t)p->P.n, H = (size_t)kHistory * N, period = (size_t)F * N;
    const size_t wb = (size_t)fmt_bytes(hc_wire_fmt(p->hc, p->dev_fmt));
    const size_t step = p->max_chunk / (size_t)p->feed_block * (size_t)p->feed_block;
    // (the origin first: the records of bursts that end inside the prefix are built during these feeds)
    const uint64_t shift = (uint64_t)H * 1000000000ull / (uint64_t)p->cfg.sample_rate;
    p->st.start_time_ns -= shift;
    p->st.prime_shift_ns = shift;
    p->st.primed_samples = H;
    p->st.primed_frames = F;
    int rc = 0;
    p->priming = true;
    for (size_t s0 = 0; rc >= 0 && s0 < H; s0 += step) {
        const size_t len = std::min(step, H - s0);
        void *place = feed_host_place(p, len);
        if (!place) rc = -1;
        char *land = static_cast<char *>(hc_landing(p->hc, place));
        for (size_t pos = s0; rc >= 0 && pos < s0 + len;) {
            const size_t o = pos % period, run = std::min(period - o, s0 + len - pos);
            if (hipMemcpyAsync(land + (pos - s0) * wb, static_cast<const char *>(d_head) + o * wb, run * wb, hipMemcpyDeviceToDevice,
                               p->fstream) != hipSuccess)
                rc = -1;
            pos += run;
        }
        if (rc >= 0) rc = feed_host_arrived(p, place, len);
    }
    p->priming = false;
    if (rc < 0) return -1;
    // (the copies read d_head on fstream: behind them the caller's buffer is its own again)
    IRDM_HIP_CHECK(hipStreamSynchronize(p->fstream));
    return 0;
}

extern "C" int irdm_prime_host(irdm_pipeline_t *p, const void *h_iq, size_t n_samples)
{
    const int F = prime_check(p, n_samples);
    if (F < 0 || !h_iq) return -1;
    pipeline_enter(p);
    const size_t bytes = (size_t)F * (size_t)p->P.n * (size_t)fmt_bytes(hc_wire_fmt(p->hc, p->dev_fmt));
    void *d_head = nullptr;
    if (hipMalloc(&d_head, bytes) != hipSuccess) return -1;
    int rc = hipMemcpyAsync(d_head, h_iq, bytes, hipMemcpyHostToDevice, p->fstream) == hipSuccess ? 0 : -1;
    if (rc == 0) rc = prime_from_device(p, d_head, F);
    if (rc != 0) (void)hipStreamSynchronize(p->fstream);
    (void)hipFree(d_head);
    return rc;
}

extern "C" int irdm_prime_device(irdm_pipeline_t *p, const void *d_iq, size_t n_samples, void *stream_v)
{
    const int F = prime_check(p, n_samples);
    if (F < 0 || !d_iq) return -1;
    pipeline_enter(p);
    hipStream_t caller = static_cast<hipStream_t>(stream_v);
    if (caller && caller != p->fstream) {
        IRDM_HIP_CHECK(hipEventRecord(p->ev[8], caller));
        IRDM_HIP_CHECK(hipStreamWaitEvent(p->fstream, p->ev[8], 0));
    }
    return prime_from_device(p, d_iq, F);
}

extern "C" uint64_t irdm_primed_samples(const irdm_pipeline_t *p) { return p ? p->st.primed_samples : 0; }
extern "C" int irdm_primed_frames(const irdm_pipeline_t *p) { return p ? p->st.primed_frames : 0; }

// irdm_swap_iq_device: the exchange alone, on a buffer the caller owns (iq_swap.hpp)
extern "C" int irdm_swap_iq_device(void *d_iq, size_t n_samples, int format, int device, void *stream_v)
{
    if ((!d_iq && n_samples) || !fmt_valid(format) || (reinterpret_cast<uintptr_t>(d_iq) % (size_t)fmt_bytes(format)) != 0) return -1;
    if (n_samples == 0) return 0;
    CallerStream cs(device, stream_v);
    return cs.ok() ? cs.finish(launch_iq_swap(format, d_iq, n_samples, cs.s)) : -1;
}

// ---- option "iq_moments" (iq_moments.hpp) and irdm_iq_balance (iq_balance.hpp) ----
int iq_moments_configure(irdm_pipeline *p, int on)
{
    if (on && p->iqm.alloc(kImBlockBytes, true) != 0) return -1;
    p->iqm.on = on ? 1 : 0;
    return 0;
}

extern "C" int irdm_iq_moments(irdm_pipeline_t *p, irdm_iq_moments_t *out)
{
    if (!p || !out || !p->iqm.stream) return -1;
    pipeline_enter(p);
    if (iq_moments_settle(p->iqm, p->st.iqm, ~0ull) != 0) return -1;
    iq_moments_result(p->st.iqm.run, out);
    return 0;
}

extern "C" int irdm_iq_moments_device(const void *d_in, size_t n, int format, irdm_iq_moments_t *out, int device, void *stream_v)
{
    if ((!d_in && n) || !fmt_valid(format) || (reinterpret_cast<uintptr_t>(d_in) % (size_t)fmt_bytes(format)) != 0) return -1;
    if (!out && !stream_v) return -1;
    IqmRun run;
    if (n == 0) {
        if (out) iq_moments_result(run, out);
        return 0;
    }
    CallerStream cs(device, stream_v);
    if (!cs.ok()) return -1;
    if (!out) {
        // the launches alone, on the caller's stream without waiting (for timing the kernel): the rows go to a block that
        // is never read, one per device for the life of the process
        static std::mutex mu;
        static void *d_unread[64] = {};
        if (device < 0 || device >= 64) return -1;
        {
            std::lock_guard<std::mutex> lock(mu);
            if (!d_unread[device] && hipMalloc(&d_unread[device], kImBlockBytes) != hipSuccess) return -1;
        }
        const size_t bps0 = (size_t)fmt_bytes(format);
        for (size_t off = 0; off < n; off += kChunkMaxLaunch)
            if (launch_iq_moments(format, static_cast<const char *>(d_in) + off * bps0, std::min(kChunkMaxLaunch, n - off), d_unread[device],
                                  cs.s) < 0)
                return -1;
        return 0;
    }
    int grid = 0;
    const int rc = cs.finish(one_block_pass(
        d_in, n, (size_t)fmt_bytes(format), kChunkMaxLaunch, kImBlockBytes, cs.s,
        [&](const void *in, size_t piece, void *d_block) {
            grid = launch_iq_moments(format, in, piece, d_block, cs.s);
            return grid < 0 ? -1ll : (long long)(sizeof(IqmRow) * (size_t)grid);
        },
        [&](const void *h_rows, size_t, size_t piece) { iq_moments_fold(run, h_rows, grid, piece); }));
    if (rc == 0) iq_moments_result(run, out);
    return rc;
}

extern "C" int irdm_iq_balance_coeffs(double gain_db, double phase_deg, float *alpha, float *beta)
{
    return iq_balance_coeffs(gain_db, phase_deg, alpha, beta);
}

extern "C" int irdm_iq_balance_device(void *d_out, const void *d_in, size_t n, int format, float alpha, float beta, int device,
                                      void *stream_v)
{
    if (((!d_in || !d_out) && n) || !fmt_valid(format)) return -1;
    if (n == 0) return launch_iq_balance(format, d_out, d_in, 0, alpha, beta, nullptr);     // (the checks alone)
    CallerStream cs(device, stream_v);
    return cs.ok() ? cs.finish(launch_iq_balance(format, d_out, d_in, n, alpha, beta, cs.s)) : -1;
}

extern "C" int irdm_iq_balance(irdm_pipeline_t *p, int wire_format, double gain_db, double phase_deg)
{
    // a cf32 context, not a member of a group (it is fed on the device), and only before the stream's first feed: the ring
    // would hold corrected and uncorrected samples
    if (!p || p->dev_fmt != IRDM_FMT_CF32 || p->in_group || p->st.begin_no != 0 || !fmt_valid(wire_format)) return -1;
    float alpha, beta;
    if (iq_balance_coeffs(gain_db, phase_deg, &alpha, &beta) != 0) return -1;
    pipeline_enter(p);
    p->hc.bal = IqBalance{ 1, wire_format, alpha, beta };
    // (a whole chunk of the wire format now: a feed never allocates; without the memory the correction is off)
    if (hc_reserve(p->hc, p->max_chunk, p->fstream) == 0) return 0;
    p->hc.bal.on = 0;
    return -1;
}

// ---- irdm_dc_block (dc_block.hpp) ----
int dc_block_configure(irdm_pipeline *p, int wire_format, int block_log2, float seed_i, float seed_q)
{
    // as irdm_iq_balance: a cf32 context, not a member of a group, and only before the stream's first feed
    if (!p || p->dev_fmt != IRDM_FMT_CF32 || p->in_group || p->st.begin_no != 0) return -1;
    pipeline_enter(p);
    if (block_log2 >= 0) IRDM_HIP_CHECK(hipStreamSynchronize(p->fstream));
    if (dc_configure(p->hc.dc, wire_format, block_log2, seed_i, seed_q, p->max_chunk) != 0) return -1;
    // (on or off, the wire format in effect may have changed: as irdm_iq_balance)
    if (hc_reserve(p->hc, p->max_chunk, p->fstream) == 0) return 0;
    p->hc.dc.on = 0;
    return -1;
}

extern "C" int irdm_dc_block(irdm_pipeline_t *p, int wire_format, int block_log2, float seed_i, float seed_q)
{
    return dc_block_configure(p, wire_format, block_log2, seed_i, seed_q);
}

extern "C" int irdm_dc_stats(irdm_pipeline_t *p, irdm_dc_stats_t *out)
{
    if (!p || !out || !p->hc.dc.on) return -1;
    pipeline_enter(p);
    IRDM_HIP_CHECK(hipStreamSynchronize(p->fstream));
    return dc_result(p->hc.dc, p->st.hc.dc, out);
}

extern "C" int irdm_dc_mean_host(int format, const void *h_iq, size_t n, float out[2]) { return dc_mean_host(format, h_iq, n, out); }

// irdm_dc_block_device: the pass alone, on buffers the caller owns, in rounds of at most kDcDevicePiece samples with rings of
// the call's own; the open block's sums enter copy 0 of its slot and leave through the record
extern "C" int irdm_dc_block_device(int format, void *d_out, const void *d_in, size_t n, int block_log2, uint64_t first_sample,
                                    irdm_dc_state_t *state_io, void *stream_v)
{
    if (!fmt_valid(format) || block_log2 < kDcMinLog2 || block_log2 > kDcMaxLog2 || !state_io || ((!d_in || !d_out) && n)) return -1;
    if (!(fabsf(state_io->mean_i) <= 64.0f) || !(fabsf(state_io->mean_q) <= 64.0f)) return -1;
    const uintptr_t a_in = reinterpret_cast<uintptr_t>(d_in), a_out = reinterpret_cast<uintptr_t>(d_out);
    const size_t bps = (size_t)fmt_bytes(format);
    if (a_in % bps != 0 || a_out % 8u != 0) return -1;
    if (n == 0) return 0;
    if (!(a_out == a_in && bps == 8) && a_in < a_out + n * 8 && a_out < a_in + n * bps) return -1;
    int device = 0;
    if (hipGetDevice(&device) != hipSuccess) return -1;
    CallerStream cs(device, stream_v);
    if (!cs.ok()) return -1;
    const uint64_t B = 1ull << block_log2;
    DcRings r;
    int rc = r.alloc(std::min(n, kDcDevicePiece), block_log2);
    uint64_t pos = first_sample, opened = pos >> block_log2;
    if (rc == 0 && pos % B != 0) {
        // the block under way: its slot cleared, the sums so far into copy 0
        const long long sums[2] = { (long long)state_io->sum_i, (long long)state_io->sum_q };
        rc = dc_clear_slots(r, opened, opened + 1, cs.s);
        if (rc == 0 && hipMemcpyAsync(r.d_acc + (opened & (r.slots - 1)) * kDcSlotWords, sums, sizeof(sums), hipMemcpyHostToDevice, cs.s) != hipSuccess)
            rc = -1;
        if (rc == 0 && hipStreamSynchronize(cs.s) != hipSuccess) rc = -1;     // (sums: this frame's)
        opened++;
    }
    uint64_t k0 = pos >> block_log2;
    float m0[2] = { state_io->mean_i, state_io->mean_q };
    DcRec rec{};
    for (size_t off = 0; rc == 0 && off < n; off += kDcDevicePiece) {
        const size_t piece = std::min(kDcDevicePiece, n - off);
        rc = dc_enqueue(r, block_log2, format, static_cast<char *>(d_out) + off * 8, static_cast<const char *>(d_in) + off * bps, piece, pos,
                        opened, k0, m0[0], m0[1], true, true, cs.s);
        if (rc == 0 && (hipMemcpyAsync(&rec, r.d_rec, sizeof(rec), hipMemcpyDeviceToHost, cs.s) != hipSuccess ||
                        hipStreamSynchronize(cs.s) != hipSuccess))
            rc = -1;
        if (rc != 0) break;
        pos += piece;
        if (rec.blocks) {
            // the next round's first block is corrected by the mean of the last block this one closed
            k0 = pos >> block_log2;
            m0[0] = rec.last[0];
            m0[1] = rec.last[1];
        }
    }
    rc = cs.finish(rc);
    r.free();
    if (rc != 0) return -1;
    state_io->mean_i = m0[0];
    state_io->mean_q = m0[1];
    state_io->sum_i = pos % B ? rec.open[0] : 0;
    state_io->sum_q = pos % B ? rec.open[1] : 0;
    return 0;
}

// irdm_dc_block_time_device (measurement surface, tools/dc_block_rate.py): the three launches over one resident buffer, each
// kind `reps` times between two events of its own.  The sums are added `reps` times into the same slots and the means are
// those of that sum: the figures mean nothing, the spans are those of the kernels.
extern "C" int irdm_dc_block_time_device(int format, void *d_out, const void *d_in, size_t n, int block_log2, int reps, float us[3])
{
    if (!fmt_valid(format) || block_log2 < kDcMinLog2 || block_log2 > kDcMaxLog2 || !d_in || !d_out || !us || reps < 1 || n == 0 ||
        n > kDcSpan)
        return -1;
    const size_t bps = (size_t)fmt_bytes(format);
    if (reinterpret_cast<uintptr_t>(d_in) % bps != 0 || reinterpret_cast<uintptr_t>(d_out) % 8u != 0) return -1;
    int device = 0;
    if (hipGetDevice(&device) != hipSuccess) return -1;
    CallerStream cs(device, nullptr);
    if (!cs.ok()) return -1;
    DcRings r;
    hipEvent_t ev[6] = {};
    int rc = r.alloc(n, block_log2);
    for (auto &e : ev) rc = rc == 0 && hipEventCreate(&e) == hipSuccess ? 0 : -1;
    if (rc == 0) {
        int grid = 0;
        const ChunkSpan sp = chunk_span((int)bps, d_in, n, kChunkNT, kChunkMaxGrid, &grid);
        const DcGeom g{ 0ull, block_log2, r.slots - 1 };
        const DcPrev pv{ 0ull, 0.0f, 0.0f };
        const unsigned long long k_end = (unsigned long long)n >> block_log2;
        const int dst16 = ((reinterpret_cast<uintptr_t>(d_out) + (uintptr_t)sp.head * 8u) & 15u) == 0 ? 1 : 0;
        rc = dc_clear_slots(r, 0, ((n - 1) >> block_log2) + 1, cs.s);
        // (one warm-up launch of each in front of the events)
        for (int i = -1; rc == 0 && i < reps; i++) {
            if (i == 0) (void)hipEventRecord(ev[0], cs.s);
            fmt_dispatch(format, [&](auto f) {
                hipLaunchKernelGGL((dc_sums_kernel<decltype(f)::value>), dim3(grid), dim3(kChunkNT), 0, cs.s, d_in, sp, g, r.d_acc);
            });
        }
        (void)hipEventRecord(ev[1], cs.s);
        for (int i = -1; rc == 0 && i < reps; i++) {
            if (i == 0) (void)hipEventRecord(ev[2], cs.s);
            hipLaunchKernelGGL((dc_close_kernel<kDcCopies>), dim3(1), dim3(64), 0, cs.s, r.d_acc, r.d_means, r.d_rec, g, 0ull, k_end, 1,
                               k_end < ((n - 1) >> block_log2) + 1 ? 1 : 0);
        }
        (void)hipEventRecord(ev[3], cs.s);
        for (int i = -1; rc == 0 && i < reps; i++) {
            if (i == 0) (void)hipEventRecord(ev[4], cs.s);
            fmt_dispatch(format, [&](auto f) {
                hipLaunchKernelGGL((dc_sub_kernel<decltype(f)::value>), dim3(grid), dim3(kChunkNT), 0, cs.s, d_out, d_in, sp, g, r.d_means, pv, dst16);
            });
        }
        (void)hipEventRecord(ev[5], cs.s);
        if (hipGetLastError() != hipSuccess || hipStreamSynchronize(cs.s) != hipSuccess) rc = -1;
        for (int k = 0; rc == 0 && k < 3; k++) {
            float ms = 0.0f;
            if (hipEventElapsedTime(&ms, ev[2 * k], ev[2 * k + 1]) != hipSuccess) rc = -1;
            us[k] = ms * 1e3f / (float)reps;
        }
    }
    rc = cs.finish(rc);
    for (auto &e : ev)
        if (e) (void)hipEventDestroy(e);
    r.free();
    return rc;
}

// ---- option "scrub" (scrub.hpp): the blocks of the passes, when the option is first set on a cf32 context ----
int scrub_configure(irdm_pipeline *p, int on)
{
    if (on && p->dev_fmt == IRDM_FMT_CF32 && p->hc.scrub.alloc(kSbBlockBytes, false) != 0) return -1;
    p->hc.scrub.on = on ? 1 : 0;
    return 0;
}

extern "C" int irdm_scrub_stats(irdm_pipeline_t *p, irdm_scrub_stats_t *out)
{
    if (!p || !out || !p->hc.scrub.on) return -1;
    pipeline_enter(p);
    IRDM_HIP_CHECK(hipStreamSynchronize(p->fstream));
    if (scrub_settle(p->hc.scrub, p->st.hc.scrub) != 0) return -1;
    scrub_result(p->st.hc.scrub.run, p->hc.scrub.limit_log2, p->dev_fmt == IRDM_FMT_CF32 ? 1 : 0, out);
    return 0;
}

// irdm_scrub_device: the pass alone, on a buffer the caller owns (scrub.hpp)
extern "C" int irdm_scrub_device(void *d_iq, size_t n_samples, int format, int limit_log2, irdm_scrub_stats_t *stats, int device,
                                 void *stream_v)
{
    if ((!d_iq && n_samples) || !fmt_valid(format) || (reinterpret_cast<uintptr_t>(d_iq) % (size_t)fmt_bytes(format)) != 0 ||
        limit_log2 < 0 || limit_log2 > 127)
        return -1;
    ScrubRun run;
    if (format != IRDM_FMT_CF32 || n_samples == 0) {
        if (stats) scrub_result(run, limit_log2, format == IRDM_FMT_CF32 ? 1 : 0, stats);
        return 0;
    }
    CallerStream cs(device, stream_v);
    if (!cs.ok()) return -1;
    if (!stats) return cs.finish(scrub_plain(d_iq, n_samples, limit_log2, cs.s));
    // (with stats: one block for the call, read back after every launch of at most 2^31 samples)
    const int rc = cs.finish(one_block_pass(
        d_iq, n_samples, 8, kChunkMaxLaunch, kSbBlockBytes, cs.s,
        [&](const void *in, size_t piece, void *d_block) {
            if (hipMemsetAsync(d_block, 0, kSbBlockBytes, cs.s) != hipSuccess) return -1ll;
            return launch_scrub(const_cast<void *>(in), piece, limit_log2, static_cast<ScrubAcc *>(d_block), cs.s) != 0 ? -1ll : (long long)kSbBlockBytes;
        },
        [&](const void *h_acc, size_t off, size_t piece) { scrub_fold(run, static_cast<const ScrubAcc *>(h_acc), off, piece); }));
    if (rc == 0) scrub_result(run, limit_log2, 1, stats);
    return rc;
}

extern "C" int irdm_poll_chunk_marks(irdm_pipeline_t *p, irdm_chunk_mark_t *out, int max)
{
    if (!p || !out || max < 0) return -1;
    return drain(p->st.q_marks, out, max);
}

// chunks (in the order fed, counted from 0) below this number have all their records in the queues: nothing of theirs is
// in a scan in flight, a pending burst list or a batch context
extern "C" uint64_t irdm_chunks_complete(const irdm_pipeline_t *p)
{
    if (!p) return 0;
    uint64_t w = p->st.chunk_no;
    if (p->st.fl_active) w = std::min<uint64_t>(w, p->st.fl_no);
    if (p->st.has_pending) w = std::min<uint64_t>(w, p->st.pend_no);
    for (int i = 0; i < p->n_bc; i++)
        if (p->bc[i].st.n > 0) w = std::min<uint64_t>(w, p->bc[i].st.chunk_no);
    return w;
}

extern "C" int irdm_poll_demods_packed(irdm_pipeline_t *p, irdm_demod_packed_t *out, int max)
{
    if (!p || !out || max < 0) return -1;
    return drain(p->st.q.packed, out, max);
}

extern "C" int irdm_poll_ida_packed(irdm_pipeline_t *p, irdm_ida_packed_t *out, int max)
{
    if (!p || !out || max < 0) return -1;
    return drain(p->st.q.ida_packed, out, max);
}

extern "C" int irdm_poll_frame_packed(irdm_pipeline_t *p, irdm_frame_packed_t *out, int max)
{
    if (!p || !out || max < 0) return -1;
    return drain(p->st.q.frame_packed, out, max);
}

extern "C" int irdm_poll_bursts(irdm_pipeline_t *p, irdm_burst_t *out, int max)
{
    if (!p || !out || max < 0) return -1;
    return drain(p->st.q.bursts, out, max);
}

extern "C" int irdm_poll_frames(irdm_pipeline_t *p, irdm_frame_info_t *out, float *samples_out, int max)
{
    if (!p || !out || max < 0) return -1;
    int n = 0;
    while (n < max && !p->st.q.frames.empty()) {
        out[n] = p->st.q.frames.front();
        p->st.q.frames.pop_front();
        if (!p->st.q.frame_samples.empty()) {
            if (samples_out) {
                const std::vector<float> &s = p->st.q.frame_samples.front();
                memcpy(samples_out + (size_t)n * 2 * IRDM_MAX_FRAME_SAMPLES, s.data(), s.size() * sizeof(float));
            }
            p->st.q.frame_samples.pop_front();
        }
        n++;
    }
    return n;
}

extern "C" int irdm_poll_demods(irdm_pipeline_t *p, irdm_demod_t *out, int max)
{
    if (!p || !out || max < 0) return -1;
    return drain(p->st.q.demods, out, max);
}

extern "C" int irdm_last_magnitudes(irdm_pipeline_t *p, float *out, size_t max_frames)
{
    if (!p || !out) return -1;
    if (quiesce(p) != 0) return -1;
    const size_t nf = std::min<size_t>(max_frames, (size_t)p->st.last_frames);
    if (!nf) return 0;
    IRDM_HIP_CHECK(hipMemcpy(out, p->st.d_mag_last, nf * p->P.n * sizeof(float), hipMemcpyDeviceToHost));
    return (int)nf;
}

extern "C" int irdm_detector_stats(irdm_pipeline_t *p, irdm_detector_stats_t *out)
{
    if (!p || !out || quiesce(p) != 0) return -1;
    const DetParams &P = p->P;
    std::vector<float> sum((size_t)P.n);
    IRDM_HIP_CHECK(hipMemcpy(sum.data(), p->d_sum, sizeof(float) * (size_t)P.n, hipMemcpyDeviceToHost));
    DetState head;
    IRDM_HIP_CHECK(hipMemcpy(&head, p->d_state, offsetof(DetState, act), hipMemcpyDeviceToHost));
    const int n_act = head.n_act < 0 ? 0 : (head.n_act > kMaxActive ? kMaxActive : head.n_act);
    std::vector<ActiveBurst> act((size_t)n_act);
    if (n_act)
        IRDM_HIP_CHECK(hipMemcpy(act.data(), reinterpret_cast<const char *>(p->d_state) + offsetof(DetState, act),
                                 sizeof(ActiveBurst) * (size_t)n_act, hipMemcpyDeviceToHost));
    out->active_bursts = n_act;
    out->primed = head.primed;
    // burst_detect.c:363-380
    double s = 0;
    for (int i = 0; i < P.n; i++) s += sum[i];
    const float avg = (float)(s / ((double)P.n * kHistory));
    const float bin_width = (float)p->cfg.sample_rate / P.n;
    out->noise_floor_dbfs_hz = (avg > 0 && bin_width > 0) ? 10.0f * log10f(avg / bin_width) : -120.0f;
    // burst_detect.c:572-576: the running maximum of the magnitude a burst is created with
    float peak = p->st.peak_signal_db;
    for (const ActiveBurst &a : act) {
        const float m = 10.0f * log10f(a.peak_rel * kHistory * 1.72f);
        if (m > peak) peak = m;
    }
    out->peak_signal_db = peak;
    return 0;
}

extern "C" int irdm_baseline_sum(irdm_pipeline_t *p, float *out)
{
    if (!p || !out || quiesce(p) != 0) return -1;
    IRDM_HIP_CHECK(hipMemcpy(out, p->d_sum, p->P.n * sizeof(float), hipMemcpyDeviceToHost));
    return p->P.n;
}

extern "C" int irdm_burst_samples(irdm_pipeline_t *p, int burst_in_chunk, float *out, size_t max_samples)
{
    if (!p || !out || burst_in_chunk < 0 || burst_in_chunk >= (int)p->st.last_bursts.size() || (!p->depth && !p->st.last_chunk))
        return -1;
    const irdm_burst_t &r = p->st.last_bursts[burst_in_chunk];
    const size_t n = std::min<size_t>(std::min<size_t>(max_samples, r.num_samples), p->l_cap);
    // NOTE: valid only until the next feed (the chunk pointer and ring are read again)
    SampleSource src = p->depth ? make_source(p, nullptr, 0, r.avail_end)
                                : make_source(p, p->st.last_chunk, p->st.last_chunk_start, p->st.last_chunk_end);
    // the ring already holds the chunk tail; reading through the chunk pointer is equivalent
    if (launch_gather_burst(src, r.start, r.avail_end, (int)n, p->d_probe, p->stream) != 0) return -1;
    IRDM_HIP_CHECK(hipMemcpyAsync(out, p->d_probe, n * sizeof(float2), hipMemcpyDeviceToHost, p->stream));
    IRDM_HIP_CHECK(hipStreamSynchronize(p->stream));
    return (int)n;
}

}  // namespace irdmh
