// state.cpp -- detector-state export / import and history seeding (time-chunk sharding), and the stage-level batch
// entry points (irdm_downmix_burst, irdm_qpsk_demod_batch, irdm_frame_decode_batch, irdm_ida_decode_batch,
// irdm_frame_packed_batch, irdm_ida_packed_batch).
#include "pipeline.hpp"

namespace irdmh {

// ---- detector-state hand-off for time-chunk sharding ----
struct StateHeader {
    uint64_t magic, n, hist, total_samples, tagged, start_time_ns;
    int32_t host_primed, host_hist_idx;
};

// Stream positions stay below 2^53 (include/irdm_hip.h): from there (double)start, which every timestamp is made of, is no
// longer exact.  The entries that SET a position refuse one at or above it.  (A feed that crosses it mid-stream is not checked:
// at 22.6 MHz that is 12 years of samples.)
static bool position_refused(const char *entry, uint64_t pos)
{
    if (pos < IRDM_MAX_POSITION) return false;
    fprintf(stderr, "irdm_hip: %s: stream position %llu is not below 2^53\n", entry, (unsigned long long)pos);
    return true;
}

// the positions a state blob's head carries: the header's sample count, the detector's next frame, the active bursts
static bool blob_refused(const char *entry, const StateHeader &h, const DetState &d)
{
    uint64_t top = std::max(h.total_samples, d.index);
    for (int i = 0; i < std::min(std::max(d.n_act, 0), kMaxActive); i++) top = std::max(top, std::max(d.act[i].start, d.act[i].last_active));
    return position_refused(entry, top);
}

extern "C" size_t irdm_state_bytes(const irdm_pipeline_t *p)
{
    if (!p) return 0;
    return sizeof(StateHeader) + sizeof(DetState) + sizeof(float) * (size_t)p->P.n * (1 + kHistory);
}

extern "C" long long irdm_export_state(irdm_pipeline_t *p, void *buf, size_t cap)
{
    if (!p || !buf || cap < irdm_state_bytes(p) || quiesce(p) != 0) return -1;
    pipeline_enter(p);
    char *o = static_cast<char *>(buf);
    StateHeader h = { 0x4952444d53544154ull, (uint64_t)p->P.n, (uint64_t)kHistory, p->st.total_samples, p->st.tagged,
                      p->st.start_time_ns, p->st.host_primed, p->st.host_hist_idx };
    memcpy(o, &h, sizeof(h));
    o += sizeof(h);
    IRDM_HIP_CHECK(hipMemcpy(o, p->d_state, sizeof(DetState), hipMemcpyDeviceToHost));
    o += sizeof(DetState);
    IRDM_HIP_CHECK(hipMemcpy(o, p->d_sum, sizeof(float) * p->P.n, hipMemcpyDeviceToHost));
    o += sizeof(float) * p->P.n;
    IRDM_HIP_CHECK(hipMemcpy(o, p->d_hist, sizeof(float) * (size_t)kHistory * p->P.n, hipMemcpyDeviceToHost));
    return (long long)irdm_state_bytes(p);
}

// A detector state may only be replaced while no scan that ran on the OLD state is ahead of the caller: with two chunks begun
// ahead, or with the next chunk's scan already chained behind the one in flight (scan_chain_early), that scan has read -- or
// committed against -- the state the import is about to overwrite, and irdm_feed_end would book its results as the
// imported stream's.  The time-sharded callers begin one chunk ahead at most and import before its irdm_feed_end.
static inline bool import_allowed(const irdm_pipeline *p) { return !p->st.chain_pending && p->st.begin_no <= p->st.end_no + 1; }

extern "C" int irdm_import_state(irdm_pipeline_t *p, const void *buf, size_t n)
{
    if (!p || !buf || n < irdm_state_bytes(p) || !import_allowed(p) || quiesce(p) != 0) return -1;
    pipeline_enter(p);
    const char *i = static_cast<const char *>(buf);
    StateHeader h;
    memcpy(&h, i, sizeof(h));
    if (h.magic != 0x4952444d53544154ull || h.n != (uint64_t)p->P.n || h.hist != (uint64_t)kHistory) return -1;
    i += sizeof(h);
    {
        std::vector<DetState> d(1);
        memcpy(d.data(), i, sizeof(DetState));
        if (blob_refused("irdm_import_state", h, d[0])) return -1;
    }
    IRDM_HIP_CHECK(hipMemcpy(p->d_state, i, sizeof(DetState), hipMemcpyHostToDevice));
    i += sizeof(DetState);
    IRDM_HIP_CHECK(hipMemcpy(p->d_sum, i, sizeof(float) * p->P.n, hipMemcpyHostToDevice));
    i += sizeof(float) * p->P.n;
    IRDM_HIP_CHECK(hipMemcpy(p->d_hist, i, sizeof(float) * (size_t)kHistory * p->P.n, hipMemcpyHostToDevice));
    // (a feed already begun has fixed its own position)
    if (p->st.begin_no == p->st.end_no) p->st.total_samples = p->st.begun_samples = h.total_samples;
    p->st.tagged = h.tagged;
    p->st.start_time_ns = h.start_time_ns;
    p->st.host_primed = h.host_primed;
    p->st.host_hist_idx = h.host_hist_idx;
    return 0;
}

// The same blob in DEVICE memory (e.g. a torch tensor that RCCL sends to the next rank): no host bounce of the 16-32 MiB
// history, and no device-wide synchronisation -- only the detector has to have settled; K1 / the ring copy of the next
// chunk and the per-burst chains in flight do not touch the detector state.
extern "C" long long irdm_export_state_device(irdm_pipeline_t *p, void *d_buf, size_t cap)
{
    if (!p || !d_buf || cap < irdm_state_bytes(p)) return -1;
    pipeline_enter(p);
    if (settle(p) != 0) return -1;
    char *o = static_cast<char *>(d_buf);
    const StateHeader h = { 0x4952444d53544154ull, (uint64_t)p->P.n, (uint64_t)kHistory, p->st.total_samples, p->st.tagged,
                            p->st.start_time_ns, p->st.host_primed, p->st.host_hist_idx };
    IRDM_HIP_CHECK(hipMemcpyAsync(o, &h, sizeof(h), hipMemcpyHostToDevice, p->stream));
    o += sizeof(h);
    IRDM_HIP_CHECK(hipMemcpyAsync(o, p->d_state, sizeof(DetState), hipMemcpyDeviceToDevice, p->stream));
    o += sizeof(DetState);
    IRDM_HIP_CHECK(hipMemcpyAsync(o, p->d_sum, sizeof(float) * p->P.n, hipMemcpyDeviceToDevice, p->stream));
    o += sizeof(float) * p->P.n;
    IRDM_HIP_CHECK(hipMemcpyAsync(o, p->d_hist, sizeof(float) * (size_t)kHistory * p->P.n, hipMemcpyDeviceToDevice, p->stream));
    IRDM_HIP_CHECK(hipStreamSynchronize(p->stream));
    return (long long)irdm_state_bytes(p);
}

extern "C" int irdm_import_state_device(irdm_pipeline_t *p, const void *d_buf, size_t n)
{
    if (!p || !d_buf || n < irdm_state_bytes(p) || !import_allowed(p)) return -1;
    pipeline_enter(p);
    if (settle(p) != 0) return -1;
    const char *i = static_cast<const char *>(d_buf);
    StateHeader h;
    IRDM_HIP_CHECK(hipMemcpyAsync(&h, i, sizeof(h), hipMemcpyDeviceToHost, p->stream));
    IRDM_HIP_CHECK(hipStreamSynchronize(p->stream));
    if (h.magic != 0x4952444d53544154ull || h.n != (uint64_t)p->P.n || h.hist != (uint64_t)kHistory) return -1;
    // (the header's position only: the detector state stays on the device)
    if (position_refused("irdm_import_state_device", h.total_samples)) return -1;
    i += sizeof(h);
    IRDM_HIP_CHECK(hipMemcpyAsync(p->d_state, i, sizeof(DetState), hipMemcpyDeviceToDevice, p->stream));
    i += sizeof(DetState);
    IRDM_HIP_CHECK(hipMemcpyAsync(p->d_sum, i, sizeof(float) * p->P.n, hipMemcpyDeviceToDevice, p->stream));
    i += sizeof(float) * p->P.n;
    IRDM_HIP_CHECK(hipMemcpyAsync(p->d_hist, i, sizeof(float) * (size_t)kHistory * p->P.n, hipMemcpyDeviceToDevice, p->stream));
    IRDM_HIP_CHECK(hipStreamSynchronize(p->stream));
    // (a feed already begun has fixed its own position)
    if (p->st.begin_no == p->st.end_no) p->st.total_samples = p->st.begun_samples = h.total_samples;
    p->st.tagged = h.tagged;
    p->st.start_time_ns = h.start_time_ns;
    p->st.host_primed = h.host_primed;
    p->st.host_hist_idx = h.host_hist_idx;
    return 0;
}

// ---- the same hand-off in two parts, so that the 16-32 MiB history can FOLLOW the detector's head ----
// head = header + DetState + sums (65 KB at 12 MHz): everything round 0 of the band scan reads.  The history (512 x N
// floats) is first read by round 1's sums pass: a rank takes the head, enqueues its scan and imports the history when it
// arrives; the scan waits for it on the device (launch_band_scan's gate).
extern "C" size_t irdm_state_head_bytes(const irdm_pipeline_t *p)
{
    if (!p) return 0;
    return sizeof(StateHeader) + sizeof(DetState) + sizeof(float) * (size_t)p->P.n;
}

extern "C" int irdm_import_state_head_device(irdm_pipeline_t *p, const void *d_buf, size_t n)
{
    if (!p || !d_buf || n < irdm_state_head_bytes(p) || !import_allowed(p)) return -1;
    pipeline_enter(p);
    if (settle(p) != 0) return -1;
    const char *i = static_cast<const char *>(d_buf);
    StateHeader h;
    IRDM_HIP_CHECK(hipMemcpyAsync(&h, i, sizeof(h), hipMemcpyDeviceToHost, p->stream));
    IRDM_HIP_CHECK(hipStreamSynchronize(p->stream));
    if (h.magic != 0x4952444d53544154ull || h.n != (uint64_t)p->P.n || h.hist != (uint64_t)kHistory) return -1;
    // (the header's position only: the detector state stays on the device)
    if (position_refused("irdm_import_state_head_device", h.total_samples)) return -1;
    i += sizeof(h);
    IRDM_HIP_CHECK(hipMemcpyAsync(p->d_state, i, sizeof(DetState), hipMemcpyDeviceToDevice, p->stream));
    i += sizeof(DetState);
    IRDM_HIP_CHECK(hipMemcpyAsync(p->d_sum, i, sizeof(float) * p->P.n, hipMemcpyDeviceToDevice, p->stream));
    IRDM_HIP_CHECK(hipStreamSynchronize(p->stream));
    if (p->st.begin_no == p->st.end_no) p->st.total_samples = p->st.begun_samples = h.total_samples;
    p->st.tagged = h.tagged;
    p->st.start_time_ns = h.start_time_ns;
    p->st.host_primed = h.host_primed;
    p->st.host_hist_idx = h.host_hist_idx;
    return 0;
}

// Call between irdm_import_state_head_device and irdm_feed_end.  d_hist_buf: device memory (irdm_state_bytes() -
// irdm_state_head_bytes() bytes) the history WILL be in.  1 = the scan that irdm_feed_end enqueues waits on the device --
// behind its round 0 -- until irdm_import_state_history_device(p, d_hist_buf, n) says the history has arrived there, and
// copies it into the context itself; the caller MUST make that call before anything settles the scan
// (irdm_export_state_device, irdm_flush, the next irdm_feed_end).  0 = this scan cannot wait (pipeline_depth 0, a
// detector that is not primed, a scan other than the band scan): import the history before irdm_feed_end.
extern "C" int irdm_expect_history(irdm_pipeline_t *p, const void *d_hist_buf)
{
    if (!p || !d_hist_buf || !p->hp_gate_dev || !p->depth || !p->st.host_primed || scan_pick(p) != 2 || p->st.begin_no == p->st.end_no)
        return 0;
    // (test hook band_first 1: the launch ends with round 0's verdict, before the pass the gate sits in front of -- the
    // continuation would run on a history that was never copied in)
    if (p->band_first == 1) return 0;
    p->gate_seq++;
    p->st.gate_src = d_hist_buf;
    p->st.gate_armed = true;
    return 1;
}

// d_hist_buf: the history part of the blob (behind irdm_state_head_bytes()), device memory, complete and visible to the
// device when this is called
extern "C" int irdm_import_state_history_device(irdm_pipeline_t *p, const void *d_hist_buf, size_t n)
{
    const size_t bytes = p ? sizeof(float) * (size_t)kHistory * p->P.n : 0;
    if (!p || !d_hist_buf || n < bytes) return -1;
    pipeline_enter(p);
    if (p->st.gate_open_pending) {
        // a scan is waiting for it: the word it polls is written by the HOST (no GPU work of ours that could queue up
        // behind the waiting kernel); the scan's stream copies the history in and goes on
        if (d_hist_buf != p->st.gate_src) return -1;
        __atomic_store_n(&p->hp_gate[0], p->gate_seq, __ATOMIC_RELEASE);
        return 0;
    }
    p->st.gate_armed = false;               // (announced, but the scan was never enqueued: the ordinary import)
    if (settle(p) != 0) return -1;
    IRDM_HIP_CHECK(hipMemcpyAsync(p->d_hist, d_hist_buf, bytes, hipMemcpyDeviceToDevice, p->stream));
    IRDM_HIP_CHECK(hipStreamSynchronize(p->stream));
    return 0;
}

// the preceding samples from DEVICE memory (a chunk overlap received from the previous rank)
extern "C" int irdm_seed_history_device(irdm_pipeline_t *p, const void *d_iq, size_t n_samples, uint64_t abs_start)
{
    if (!p || (!d_iq && n_samples) || n_samples > abs_start || p->st.begin_no != p->st.end_no) return -1;
    if (position_refused("irdm_seed_history_device", abs_start)) return -1;
    pipeline_enter(p);
    if (n_samples > p->ring_len) {
        d_iq = static_cast<const char *>(d_iq) + (n_samples - p->ring_len) * p->bps;
        n_samples = p->ring_len;
    }
    // behind whatever the ring stream still has to do -- and behind the decimators in flight that still read the slots
    // (irdm_advance leaves the previous chunk's chain running); the per-burst chains wait for ev_ring before they read the ring
    if (ring_guard(p, abs_start - n_samples, abs_start, p->fstream) != 0) return -1;
    if (ring_update(p, d_iq, abs_start - n_samples, abs_start, p->fstream) != 0) return -1;
    IRDM_HIP_CHECK(hipEventRecord(p->ev_ring, p->fstream));
    IRDM_HIP_CHECK(hipStreamSynchronize(p->fstream));
    p->st.total_samples = p->st.begun_samples = abs_start;
    return 0;
}

extern "C" int irdm_seed_history(irdm_pipeline_t *p, const void *h_iq, size_t n_samples, uint64_t abs_start)
{
    if (!p || (!h_iq && n_samples) || n_samples > abs_start || p->st.begin_no != p->st.end_no) return -1;
    if (position_refused("irdm_seed_history", abs_start)) return -1;
    if (quiesce(p) != 0) return -1;
    if (n_samples > p->ring_len) {       // only the most recent ring_len samples can matter
        h_iq = static_cast<const char *>(h_iq) + (n_samples - p->ring_len) * p->bps;
        n_samples = p->ring_len;
    }
    const char *src = static_cast<const char *>(h_iq);
    uint64_t a0 = abs_start - n_samples;
    size_t done = 0;
    while (done < n_samples) {
        const uint64_t pos = (a0 + done) % p->ring_len;
        const size_t run = std::min<size_t>(n_samples - done, p->ring_len - pos);
        IRDM_HIP_CHECK(hipMemcpy(static_cast<char *>(p->d_ring) + pos * p->bps, src + done * p->bps, run * p->bps,
                                 hipMemcpyHostToDevice));
        done += run;
    }
    p->st.total_samples = p->st.begun_samples = abs_start;
    return 0;
}

extern "C" int irdm_downmix_burst(irdm_pipeline_t *p, const irdm_burst_t *info, const float *samples,
                                  size_t num_samples, irdm_frame_info_t *frame, float *frame_samples)
{
    if (!p || !info || !samples || !frame || p->dev_fmt != 2) return -1;
    if (num_samples > p->l_cap) return -1;
    if (quiesce(p) != 0) return -1;
    IRDM_HIP_CHECK(hipMemcpy(p->d_probe, samples, num_samples * sizeof(float2), hipMemcpyHostToDevice));
    // the burst window is presented as a "chunk" that starts at info->start
    SampleSource src = make_source(p, p->d_probe, info->start, info->start + num_samples);
    GoneBurst g;
    memset(&g, 0, sizeof(g));
    g.id = info->id;
    g.start = info->start;
    g.stop = info->start + num_samples - (uint64_t)p->P.pre_len;     // num_samples = stop + pre_len - start
    g.last_active = info->last_active;
    g.center_bin = info->center_bin;
    g.peak_rel = info->peak_rel;
    g.base_sum = info->base_sum;
    // keep the result queues of the stream untouched: they stand aside while the call runs on empty ones
    RecordQueues stream_q;
    std::swap(stream_q, p->st.q);
    const int keep = p->keep_frame_samples, dec = p->decode_frames, dec_ida = p->decode_ida, det = p->detect_only;
    p->decode_frames = 0;
    p->decode_ida = 0;
    p->detect_only = 0;          // a stage-B call on a detect-only context still runs stage B
    const int marks = p->chunk_marks, clock = p->symbol_clock, sense = p->iq_sense, fine = p->fine_freq, ftime = p->fine_time;
    p->chunk_marks = 0;          // (the records go to private queues: no chunk mark for them)
    p->symbol_clock = 0;         // (and the probe's frame is none of the stream's)
    p->iq_sense = 0;
    p->fine_freq = 0;
    p->fine_time = 0;
    const uint64_t tagged = p->st.tagged;
    std::vector<irdm_burst_t> last; last.swap(p->st.last_bursts);
    p->keep_frame_samples = 1;
    p->whole_window = 1;         // avail_end = info->start + num_samples, not what a feed block would have delivered
    const int rc = process_bursts(p, p->bc[0], src, &g, 1);
    p->whole_window = 0;
    int ret = -1;
    if (rc == 0 && !p->st.q.frames.empty()) {
        *frame = p->st.q.frames.front();
        frame->magnitude = info->magnitude;
        frame->noise = info->noise;
        if (frame->drop_reason == 0 && frame_samples && !p->st.q.frame_samples.empty())
            memcpy(frame_samples, p->st.q.frame_samples.front().data(), p->st.q.frame_samples.front().size() * sizeof(float));
        ret = frame->drop_reason == 0 ? 1 : 0;
    }
    std::swap(stream_q, p->st.q);
    p->keep_frame_samples = keep;
    p->chunk_marks = marks;
    p->symbol_clock = clock;
    p->iq_sense = sense;
    p->fine_freq = fine;
    p->fine_time = ftime;
    p->detect_only = det;
    p->decode_frames = dec;
    p->decode_ida = dec_ida;
    p->st.tagged = tagged;
    p->st.last_bursts.swap(last);
    return ret;
}

// stage C alone on n caller-supplied frames, burst_cap of them per launch.  packed_out == nullptr: the DemodOut records come
// back by a copy (out).  packed_out != nullptr: the packed record path -- demod_par_kernel writes the DemodPacked and work
// records into the first batch buffer's pinned memory (demod_export), out is filled from d_demod only where keep_bits is set
static int demod_batch(irdm_pipeline_t *p, const float *samples, const int *num_samples, const int *direction, int n,
                       int keep_bits, irdm_demod_packed_t *packed_out, irdm_demod_t *out)
{
    BatchCtx &b = p->bc[0];
    for (int base = 0; base < n; base += p->burst_cap) {
        const int nb = std::min(p->burst_cap, n - base);
        p->h_work.assign(nb, BurstWork());
        for (int i = 0; i < nb; i++) {
            if (num_samples[base + i] < 0 || num_samples[base + i] > kMaxFrameSamples) return -1;
            p->h_work[i].num_samples = num_samples[base + i];
            p->h_work[i].direction = direction[base + i];
            p->h_work[i].drop_reason = 0;
        }
        IRDM_HIP_CHECK(hipMemcpyAsync(p->d_work, p->h_work.data(), sizeof(BurstWork) * nb, hipMemcpyHostToDevice, p->stream));
        IRDM_HIP_CHECK(hipMemcpyAsync(p->d_frames, samples + (size_t)base * 2 * kMaxFrameSamples,
                                      sizeof(float2) * (size_t)nb * kMaxFrameSamples, hipMemcpyHostToDevice, p->stream));
        if (packed_out) {
            // (no record of an earlier launch passes for this one's)
            memset(b.hp_packed, 0xff, sizeof(DemodPacked) * (size_t)nb);
            memset(b.hp_work, 0xff, sizeof(BurstWork) * (size_t)nb);
        }
        if (launch_demod(p->d_work, nb, p->d_frames, p->cfg.use_gardner, p->sps, p->d_demod_ws, p->d_demod,
                         p->stream, packed_out ? b.hp_packed : nullptr, packed_out ? b.hp_work_dev : nullptr, keep_bits) != 0)
            return -1;
        if (out) {
            p->h_demod.resize(nb);
            IRDM_HIP_CHECK(hipMemcpyAsync(p->h_demod.data(), p->d_demod, sizeof(DemodOut) * nb, hipMemcpyDeviceToHost, p->stream));
        }
        IRDM_HIP_CHECK(hipStreamSynchronize(p->stream));
        for (int i = 0; packed_out && i < nb; i++) {
            // the record as the chain queues it (chain.cpp: packed_records), the bit words as the kernel left them
            const DemodPacked &d = b.hp_packed[i];
            irdm_demod_packed_t &o = packed_out[base + i];
            memset(&o, 0, sizeof(o));
            if (b.hp_work[i].num_samples != num_samples[base + i] || b.hp_work[i].direction != direction[base + i]) return -1;
            memcpy(o.bits, d.bits, sizeof(o.bits));
            o.ok = d.ok;
            if (!d.ok) continue;
            o.direction = d.direction;
            o.confidence = d.confidence;
            o.level = d.level;
            o.n_symbols = d.n_symbols;
            o.n_payload_symbols = d.n_symbols - 12;
            o.n_bits = 2 * d.n_symbols;
            o.total_phase = d.total_phase;
        }
        for (int i = 0; out && i < nb; i++) {
            const DemodOut &d = p->h_demod[i];
            irdm_demod_t &o = out[base + i];
            memset(&o, 0, sizeof(o));
            o.ok = d.ok;
            if (!d.ok) continue;
            o.direction = d.direction;
            o.confidence = d.confidence;
            o.level = d.level;
            o.n_symbols = d.n_symbols;
            o.n_payload_symbols = d.n_symbols - 12;
            o.n_bits = 2 * d.n_symbols;
            o.total_phase = d.total_phase;
            // (the frame's own bits only, as the chain queues a record: the kernel writes 2 * n_symbols of them, behind
            // those the row of d_demod still holds an earlier frame's)
            const size_t nbits = (size_t)std::min(std::max(2 * d.n_symbols, 0), kMaxBits);
            memcpy(o.bits, d.bits, nbits * sizeof(o.bits[0]));
            memcpy(o.llr, d.llr, nbits * sizeof(o.llr[0]));
        }
    }
    return 0;
}

extern "C" int irdm_qpsk_demod_batch(irdm_pipeline_t *p, const float *samples, const int *num_samples,
                                     const int *direction, int n, irdm_demod_t *out)
{
    if (!p || !samples || !num_samples || !direction || !out || n < 0) return -1;
    pipeline_enter(p);
    return demod_batch(p, samples, num_samples, direction, n, 0, nullptr, out);
}

extern "C" int irdm_qpsk_demod_packed_batch(irdm_pipeline_t *p, const float *samples, const int *num_samples,
                                            const int *direction, int n, int keep_bits, irdm_demod_packed_t *packed_out,
                                            irdm_demod_t *full_out)
{
    if (!p || !samples || !num_samples || !direction || !packed_out || n < 0) return -1;
    if (keep_bits != 0 && keep_bits != 1) return -1;
    if (keep_bits ? !full_out : full_out != nullptr) return -1;
    pipeline_enter(p);
    return demod_batch(p, samples, num_samples, direction, n, keep_bits, packed_out, full_out);
}

// what the public records of symbol_clock and fine_freq share with the kernel's
template <typename PublicRec>
static inline void line_public(PublicRec &o, const LineRec &r)
{
    o.quality = r.quality;
    o.flags = r.flags;
    o.n = r.n;
}

// A frame line estimator's kernel alone (frame_line.hpp), on the buffers of irdm_qpsk_demod_batch: frames in, one record per
// frame out, in launches of burst_cap.  launch(nb, hp) starts the kernel on the first nb rows of d_work / d_frames, whose
// records are KernelRec; fill(o, r) makes the public record of one (its id is set here).  simplex: BurstWork::simplex of
// every frame, or nullptr for 0.
template <typename KernelRec, typename PublicRec, typename Launch, typename Fill>
static int line_batch(irdm_pipeline_t *p, const float *samples, const int *num_samples, const int *simplex, int n, PublicRec *out,
                      Launch launch, Fill fill)
{
    if (!p || !samples || !num_samples || !out || n < 0) return -1;
    for (int i = 0; i < n; i++)
        if (num_samples[i] < 0 || num_samples[i] > kMaxFrameSamples) return -1;
    pipeline_enter(p);
    KernelRec *hp = nullptr;
    IRDM_HIP_CHECK(hipHostMalloc(reinterpret_cast<void **>(&hp), sizeof(KernelRec) * (size_t)std::max(1, std::min(n, p->burst_cap)),
                                 hipHostMallocDefault));
    int rc = 0;
    for (int base = 0; base < n && rc == 0; base += p->burst_cap) {
        const int nb = std::min(p->burst_cap, n - base);
        p->h_work.assign(nb, BurstWork());
        for (int i = 0; i < nb; i++) {
            p->h_work[i].num_samples = num_samples[base + i];
            p->h_work[i].simplex = simplex && simplex[base + i] ? 1 : 0;
        }
        rc = hipMemcpyAsync(p->d_work, p->h_work.data(), sizeof(BurstWork) * nb, hipMemcpyHostToDevice, p->stream) == hipSuccess &&
                     hipMemcpyAsync(p->d_frames, samples + (size_t)base * 2 * kMaxFrameSamples,
                                    sizeof(float2) * (size_t)nb * kMaxFrameSamples, hipMemcpyHostToDevice, p->stream) == hipSuccess &&
                     launch(nb, hp) == 0 && hipStreamSynchronize(p->stream) == hipSuccess
                 ? 0 : -1;
        for (int i = 0; rc == 0 && i < nb; i++) {
            PublicRec &o = out[base + i];
            fill(o, hp[i]);
            o.id = (uint64_t)(base + i);
        }
    }
    (void)hipHostFree(hp);
    return rc;
}

extern "C" int irdm_symbol_clock_batch(irdm_pipeline_t *p, const float *samples, const int *num_samples, int n, irdm_clock_est_t *out)
{
    return line_batch<LineRec>(p, samples, num_samples, nullptr, n, out,
                               [p](int nb, LineRec *hp) { return launch_symbol_clock(p->d_work, nb, p->d_frames, p->sps, hp, p->stream); },
                               [](irdm_clock_est_t &o, const LineRec &r) { line_public(o, r); o.eps = r.value; });
}

extern "C" int irdm_fine_freq_batch(irdm_pipeline_t *p, const float *samples, const int *num_samples, int n, irdm_fine_freq_t *out)
{
    return line_batch<LineRec>(p, samples, num_samples, nullptr, n, out,
                               [p](int nb, LineRec *hp) { return launch_fine_freq(p->d_work, nb, p->d_frames, (double)p->out_rate, hp, p->stream); },
                               [](irdm_fine_freq_t &o, const LineRec &r) { line_public(o, r); o.df_hz = r.value; o.freq_hz = (double)r.value; });
}

extern "C" int irdm_fine_time_batch(irdm_pipeline_t *p, const float *samples, const int *num_samples, const int *simplex, int n,
                                    irdm_fine_time_t *out)
{
    return line_batch<TimeRec>(p, samples, num_samples, simplex, n, out,
                               [p](int nb, TimeRec *hp) { return launch_fine_time(p->d_work, nb, p->d_frames, p->sps, hp, p->stream); },
                               [p](irdm_fine_time_t &o, const TimeRec &r) { fine_time_public(r, p->sps, &o); });
}

extern "C" int irdm_poll_decoded(irdm_pipeline_t *p, irdm_decoded_t *out, int max)
{
    if (!p || !out || max < 0) return -1;
    return drain(p->st.q.decoded, out, max);
}

extern "C" int irdm_frame_decode_batch(irdm_pipeline_t *p, const irdm_demod_t *in, int n, int use_llr, irdm_decoded_t *out)
{
    if (!p || !in || !out || n < 0) return -1;
    pipeline_enter(p);
    std::vector<int> nbits;
    for (int base = 0; base < n; base += p->burst_cap) {
        const int nb = std::min(p->burst_cap, n - base);
        p->h_demod.assign(nb, DemodOut());
        nbits.assign(nb, 0);
        for (int i = 0; i < nb; i++) {
            const irdm_demod_t &f = in[base + i];
            if (f.n_bits < 0 || f.n_bits > kMaxBits) return -1;
            DemodOut &d = p->h_demod[i];
            d.ok = 1;
            d.n_symbols = f.n_bits / 2;
            memcpy(d.bits, f.bits, sizeof(d.bits));
            memcpy(d.llr, f.llr, sizeof(d.llr));
            nbits[i] = f.n_bits;
        }
        IRDM_HIP_CHECK(hipMemcpyAsync(p->d_demod, p->h_demod.data(), sizeof(DemodOut) * nb, hipMemcpyHostToDevice, p->stream));
        IRDM_HIP_CHECK(hipMemcpyAsync(p->d_nbits, nbits.data(), sizeof(int) * nb, hipMemcpyHostToDevice, p->stream));
        if (launch_frame_decode(p->d_demod, nb, p->d_syn_ra, p->d_syn_hdr, use_llr ? 1 : 0, p->d_nbits, p->d_decoded,
                                p->stream) != 0)
            return -1;
        p->h_decoded.resize(nb);
        IRDM_HIP_CHECK(hipMemcpyAsync(p->h_decoded.data(), p->d_decoded, sizeof(DecodedOut) * nb, hipMemcpyDeviceToHost, p->stream));
        IRDM_HIP_CHECK(hipStreamSynchronize(p->stream));
        for (int i = 0; i < nb; i++)
            out[base + i] = finish_decoded(p->h_decoded[i], in[base + i].id, in[base + i].timestamp,
                                           in[base + i].center_frequency);
    }
    return 0;
}

extern "C" int irdm_poll_ida(irdm_pipeline_t *p, irdm_ida_t *out, int max)
{
    if (!p || !out || max < 0) return -1;
    return drain(p->st.q.ida, out, max);
}

extern "C" int irdm_ida_decode_batch(irdm_pipeline_t *p, const irdm_demod_t *in, int n, int use_llr, irdm_ida_t *out)
{
    if (!p || !in || !out || n < 0) return -1;
    pipeline_enter(p);
    std::vector<int> nbits, dirs;
    for (int base = 0; base < n; base += p->burst_cap) {
        const int nb = std::min(p->burst_cap, n - base);
        p->h_demod.assign(nb, DemodOut());
        nbits.assign(nb, 0);
        dirs.assign(nb, 0);
        for (int i = 0; i < nb; i++) {
            const irdm_demod_t &f = in[base + i];
            if (f.n_bits < 0 || f.n_bits > kMaxBits) return -1;
            DemodOut &d = p->h_demod[i];
            d.ok = 1;
            d.n_symbols = f.n_bits / 2;
            memcpy(d.bits, f.bits, sizeof(d.bits));
            memcpy(d.llr, f.llr, sizeof(d.llr));
            nbits[i] = f.n_bits;
            dirs[i] = f.direction;
        }
        IRDM_HIP_CHECK(hipMemcpyAsync(p->d_demod, p->h_demod.data(), sizeof(DemodOut) * nb, hipMemcpyHostToDevice, p->stream));
        IRDM_HIP_CHECK(hipMemcpyAsync(p->d_nbits, nbits.data(), sizeof(int) * nb, hipMemcpyHostToDevice, p->stream));
        IRDM_HIP_CHECK(hipMemcpyAsync(p->d_dirs, dirs.data(), sizeof(int) * nb, hipMemcpyHostToDevice, p->stream));
        if (launch_ida_decode(p->d_demod, nb, p->d_syn_da, p->d_syn_l1, p->d_syn_l2, p->d_syn_l3, use_llr ? 1 : 0,
                              p->d_nbits, p->d_dirs, p->d_ida, p->stream) != 0)
            return -1;
        p->h_ida.resize(nb);
        IRDM_HIP_CHECK(hipMemcpyAsync(p->h_ida.data(), p->d_ida, sizeof(IdaOut) * nb, hipMemcpyDeviceToHost, p->stream));
        IRDM_HIP_CHECK(hipStreamSynchronize(p->stream));
        for (int i = 0; i < nb; i++) out[base + i] = finish_ida(p->h_ida[i], in[base + i]);
    }
    return 0;
}

// the packed record path's kernels alone: frame_packed_kernel / ida_packed_kernel read n_bits as 2 * n_symbols, the
// direction and the LLRs from the record (the chain's keep_bits DemodOut), and write their records into pinned host memory
template <typename Rec, typename Launch>
static int packed_batch(irdm_pipeline_t *p, const irdm_demod_t *in, int n, Rec *out, Launch launch)
{
    if (!p || !in || !out || n < 0) return -1;
    for (int i = 0; i < n; i++)
        if (in[i].n_bits < 0 || in[i].n_bits > kMaxBits || (in[i].n_bits & 1)) return -1;
    pipeline_enter(p);
    Rec *hp = nullptr;
    IRDM_HIP_CHECK(hipHostMalloc(reinterpret_cast<void **>(&hp), sizeof(Rec) * (size_t)std::max(1, std::min(n, p->burst_cap)),
                                 hipHostMallocDefault));
    int rc = 0;
    for (int base = 0; base < n && rc == 0; base += p->burst_cap) {
        const int nb = std::min(p->burst_cap, n - base);
        p->h_demod.assign(nb, DemodOut());
        for (int i = 0; i < nb; i++) {
            const irdm_demod_t &f = in[base + i];
            DemodOut &d = p->h_demod[i];
            d.ok = 1;
            d.direction = f.direction;
            d.n_symbols = f.n_bits / 2;
            memcpy(d.bits, f.bits, sizeof(d.bits));
            memcpy(d.llr, f.llr, sizeof(d.llr));
        }
        rc = hipMemcpyAsync(p->d_demod, p->h_demod.data(), sizeof(DemodOut) * nb, hipMemcpyHostToDevice, p->stream) == hipSuccess &&
                     launch(p, nb, hp) == 0 && hipStreamSynchronize(p->stream) == hipSuccess
                 ? 0 : -1;
        if (rc == 0) memcpy(out + base, hp, sizeof(Rec) * nb);
    }
    (void)hipHostFree(hp);
    return rc;
}

extern "C" int irdm_frame_packed_batch(irdm_pipeline_t *p, const irdm_demod_t *in, int n, irdm_frame_packed_t *out)
{
    static_assert(sizeof(irdm_frame_packed_t) == sizeof(FramePacked), "the public record is the kernel's");
    return packed_batch(p, in, n, reinterpret_cast<FramePacked *>(out), [](irdm_pipeline_t *q, int nb, FramePacked *hp) {
        return launch_frame_packed(q->d_demod, nb, q->d_syn_ra, q->d_syn_hdr, hp, q->stream);
    });
}

extern "C" int irdm_ida_packed_batch(irdm_pipeline_t *p, const irdm_demod_t *in, int n, irdm_ida_packed_t *out)
{
    static_assert(sizeof(irdm_ida_packed_t) == sizeof(IdaPacked), "the public record is the kernel's");
    return packed_batch(p, in, n, reinterpret_cast<IdaPacked *>(out), [](irdm_pipeline_t *q, int nb, IdaPacked *hp) {
        return launch_ida_packed(q->d_demod, nb, q->d_syn_da, q->d_syn_l1, q->d_syn_l2, q->d_syn_l3, hp, q->stream);
    });
}

// the I/Q sense kernel alone (bitlayer.hip, iq_sense.hpp): bits, LLRs, n_bits (rounded down to whole dibits) and direction
// of every record are read, as the chain's DemodOut carries them
extern "C" int irdm_iq_sense_batch(irdm_pipeline_t *p, const irdm_demod_t *in, int n, irdm_iq_vote_t *out)
{
    if (!p || !in || !out || n < 0) return -1;
    for (int i = 0; i < n; i++)
        if (in[i].n_bits < 0 || in[i].n_bits > kMaxBits) return -1;
    pipeline_enter(p);
    SenseRec *hp = nullptr;
    IRDM_HIP_CHECK(hipHostMalloc(reinterpret_cast<void **>(&hp), sizeof(SenseRec) * (size_t)std::max(1, std::min(n, p->burst_cap)),
                                 hipHostMallocDefault));
    int rc = 0;
    for (int base = 0; base < n && rc == 0; base += p->burst_cap) {
        const int nb = std::min(p->burst_cap, n - base);
        p->h_demod.assign(nb, DemodOut());
        for (int i = 0; i < nb; i++) {
            const irdm_demod_t &f = in[base + i];
            DemodOut &d = p->h_demod[i];
            d.ok = 1;
            d.direction = f.direction;
            d.n_symbols = f.n_bits / 2;
            memcpy(d.bits, f.bits, sizeof(d.bits));
            memcpy(d.llr, f.llr, sizeof(d.llr));
        }
        rc = hipMemcpyAsync(p->d_demod, p->h_demod.data(), sizeof(DemodOut) * nb, hipMemcpyHostToDevice, p->stream) == hipSuccess &&
                     launch_iq_sense(p->d_demod, nb, p->d_syn_da, p->d_syn_l1, p->d_syn_l2, p->d_syn_l3, hp, p->stream) == 0 &&
                     hipStreamSynchronize(p->stream) == hipSuccess
                 ? 0 : -1;
        for (int i = 0; rc == 0 && i < nb; i++) out[base + i] = iq_vote_of((uint64_t)(base + i), hp[i]);
    }
    (void)hipHostFree(hp);
    return rc;
}

// the table irdm_burst_resample_batch resamples at L / M with: what a context at that ratio holds
extern "C" int irdm_burst_resample_design(int L, int M, float *out, int cap)
{
    if (!burst_resample_ratio_ok(L, M) || !out || cap < L * kBrTaps) return -1;
    const std::vector<float> taps = design_resample_taps(L, M, kBrTaps);
    memcpy(out, taps.data(), sizeof(float) * taps.size());
    return (int)taps.size();
}

// burst_resample_kernel alone (burst_resample.hpp) on n caller-supplied rows: no context, its own table by the same design
extern "C" int irdm_burst_resample_batch(int device, const float *rows, const int *lens, int n, int stride, int L, int M,
                                         float *out, int out_stride, int *res_lens)
{
    if (!rows || !lens || !out || !res_lens || n < 0 || stride < 0 || out_stride < 0) return -1;
    if (!burst_resample_ratio_ok(L, M)) {
        fprintf(stderr, "irdm_hip: burst_resample: the ratio %d/%d is outside 7/8 .. 8/7 or L = %d is beyond %d\n", L, M, L, kBrMaxL);
        return -1;
    }
    if (n == 0) return 0;
    std::vector<BurstWork> work((size_t)n);
    size_t need = 0;
    int max_len = 0;
    for (int i = 0; i < n; i++) {
        const int len = lens[i], rl = len >= 0 ? burst_resample_len(len, L, M) : 0;
        if (len < 0 || len > stride || rl > out_stride) return -1;
        BurstWork &w = work[(size_t)i];
        memset(&w, 0, sizeof(w));
        w.dec_len = len;
        w.dec_off = (int32_t)need;
        need += ((size_t)std::max(len, rl) + 15) & ~(size_t)15;
        if (need > (size_t)0x7fffffff) return -1;
        max_len = std::max(max_len, len);
        res_lens[i] = rl;
    }
    IRDM_HIP_CHECK(hipSetDevice(device));
    const std::vector<float> taps = design_resample_taps(L, M, kBrTaps);
    float *d_taps = dev_upload(taps.data(), taps.size());
    BurstWork *d_work = dev_upload(work.data(), work.size());
    float2 *d_in = dev_alloc<float2>(std::max<size_t>(need, 16)), *d_out = dev_alloc<float2>(std::max<size_t>(need, 16));
    int rc = d_taps && d_work && d_in && d_out ? 0 : -1;
    for (int i = 0; rc == 0 && i < n; i++)
        if (lens[i] > 0 && hipMemcpy(d_in + work[(size_t)i].dec_off, rows + (size_t)i * 2 * stride, sizeof(float2) * (size_t)lens[i],
                                     hipMemcpyHostToDevice) != hipSuccess)
            rc = -1;
    if (rc == 0) rc = launch_burst_resample(d_work, n, max_len, d_in, d_out, d_taps, L, M, nullptr);
    if (rc == 0 && hipDeviceSynchronize() != hipSuccess) rc = -1;
    for (int i = 0; rc == 0 && i < n; i++)
        if (res_lens[i] > 0 && hipMemcpy(out + (size_t)i * 2 * out_stride, d_out + work[(size_t)i].dec_off,
                                         sizeof(float2) * (size_t)res_lens[i], hipMemcpyDeviceToHost) != hipSuccess)
            rc = -1;
    for (void *q : { (void *)d_taps, (void *)d_work, (void *)d_in, (void *)d_out })
        if (q) (void)hipFree(q);
    return rc;
}

}  // namespace irdmh
