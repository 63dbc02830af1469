// pipeline.hpp -- INTERNAL header of the host side above the C-ABI (include/irdm_hip.h): the context's state and the functions
// its source files share.  One context = one stream of IQ on one GPU, driven by one host thread (the reference's convention for
// gpu_burst_fft_t / burst_downmix_t contexts, burst_downmix.c:107-112).
//
//   plug.cpp        gpu_burst_fft_*: the reference's accelerator plug point (opencl/burst_fft.h:35-47)
//   create.cpp      irdm_create / irdm_destroy, the small getters
//   chain.cpp       the per-burst chain of a chunk (K4 .. K7): rotator checkpoint arena, enqueue, records
//   scan_host.cpp   the detector scan of a chunk from the host's side: launch, chaining, speculation pass, settle, fallbacks
//   feed.cpp        irdm_feed_* / irdm_flush / irdm_advance / irdm_reset, the polls, buffers for hosts without HIP headers
//   state.cpp       detector-state export / import (time-chunk sharding), the stage-level batch calls
//   api.cpp         options, statistics, kernel clock, RAW line formatting, --save-bursts
//   frame_line.hpp  the per-frame line estimators' core and stream summary; symbol_clock.hpp, fine_freq.hpp and fine_time.hpp are the three
//                   kernels on it (launched by chain.cpp and state.cpp)
//
// Every field of a context is configuration, cache or stream state.  The third kind lives in types of
// its own -- StreamState (irdm_pipeline::st), BatchCtx::State, FeedSlot::State, with the record queues of record_queues.hpp
// inside -- so that `p->st.` marks it where it is used and irdm_reset clears it by assigning fresh values.  A new field
// goes into the struct of its kind; one that belongs to the stream needs no line in irdm_create or irdm_reset.
#pragma once
#include <math.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>
#include <errno.h>
#include <sys/stat.h>
#include <algorithm>
#include <deque>
#include <new>
#include <vector>
#include <thread>
#include <mutex>
#include <condition_variable>
#include "../../include/irdm_hip.h"
#include "common.hpp"
#include "host_design.hpp"
#include "kernels.hpp"
#include "libm_port.hpp"
#include "band_core.hpp"
#include "types.hpp"
#include "record_queues.hpp"
#include "input_stats.hpp"
#include "symbol_clock.hpp"
#include "fine_freq.hpp"
#include "fine_time.hpp"
#include "iq_moments.hpp"
#include "host_chain.hpp"
#include "iq_sense.hpp"
#include "burst_resample.hpp"

using namespace irdm;

namespace irdmh {

template <typename T>
inline T *dev_alloc(size_t count)
{
    void *p = nullptr;
    if (hipMalloc(&p, count * sizeof(T)) != hipSuccess) return nullptr;
    return static_cast<T *>(p);
}

template <typename T>
inline T *dev_upload(const T *src, size_t count)
{
    T *p = dev_alloc<T>(count);
    if (!p) return nullptr;
    if (hipMemcpy(p, src, count * sizeof(T), hipMemcpyHostToDevice) != hipSuccess) {
        (void)hipFree(p);
        return nullptr;
    }
    return p;
}

inline int ilog2(int n)
{
    int l = 0;
    while ((1 << l) < n) l++;
    return (1 << l) == n ? l : -1;
}

}  // namespace irdmh


// ===========================================================================
// 2. batched pipeline
// ===========================================================================
struct irdm_pipeline;

// Batch contexts a pipeline may hold (pipeline_depth + 1 of them are used).  A chunk's per-burst chain is a string of
// dependent launches, several of them a handful of wavefronts long (the phase recurrence, the Gardner / PLL loop): 2.5-3 ms
// from first to last in run, whatever the chip could do beside it.  With three contexts the pipeline's period was that
// latency divided by three -- the feeding thread spent 0.6 ms of every 1.05 ms step waiting for the oldest chain
// (profiles/r5_spec_ab.json, host_us "wait_older_chain") -- and nothing done to the scan or the decimator moved it.
constexpr int kMaxBc = 6;
// the low-passed scratch of a batch context holds `cap` float2 outputs and, behind them, `cap` floats: the start filter's
// outputs (post_tiles_kernel -> post_cfo_kernel)
static inline size_t lpf_alloc(size_t cap) { return cap + cap / 2 + 8; }
static inline float *box_of(float2 *lpf, size_t cap) { return reinterpret_cast<float *>(lpf + cap); }
// Feed slots: chunks that may be between irdm_feed_begin and the settling of their scan -- the one being scanned, the one
// whose scan is chained behind it, and TWO begun ahead (round 5: one more than before, so that K1 of chunk k + 2 is on the GPU
// a period early and runs in the stretches where the chains in flight are in their lane-per-burst kernels instead of in
// front of the decimator of every period, kernel trace in profiles/r5_kernel_trace_gantt.txt).  A slot owns a magnitude
// buffer, K1's candidate lists with the levels they were built against, and the events of its K1 and ring copy.
constexpr int kFeedSlots = 3;
constexpr unsigned kLookAhead = 1;
// option "spectrum_frames": pinned buffers the finished rows of a chunk land in, taken in turn -- the one a feed takes was
// filled three feeds earlier
constexpr int kSpecSlots = 3;

// Rows of one launch of the spectrum reduction on their way to the host: `rows` rows of n_frames frames each, the first
// one row number `row0`, starting at absolute frame `frame0`, in pinned buffer `slot` once its event has completed
struct SpecBatch {
    int slot, rows, n_frames;
    uint64_t row0, frame0;
};
struct SpecRow {
    irdm_spectrum_row_t hdr;
    std::vector<float> data;        // mean[n], peak[n]
};

// One batch of finished bursts on its way through the per-burst stages K4..K7.  pipeline_depth 0 uses one context on the
// detector's stream; pipeline_depth >= 1 alternates between two, each on a stream of its own, so that the FIR of one
// chunk's bursts overlaps the latency-bound tail (sync correlation, demodulator, result copies) of the previous one's.
struct BatchCtx {
    irdm_pipeline *owner;
    hipStream_t stream;
    hipEvent_t ev[4];            // FIR begin / FIR end / post end / demod end
    hipEvent_t ev_cfo;           // work records are in the mapped buffer: the helper thread may do the host step
    hipEvent_t ev_rot;           // behind this context's latest build of rotator checkpoints (rot_rows_prepare)
    BurstWork *d_work;
    FirTile *d_tiles;
    size_t tiles_cap;
    float2 *d_dec, *d_lpf, *d_rrc_ws, *d_frames, *d_demod_ws;
    size_t dec_cap;              // outputs (float2) d_dec and d_lpf hold each: a batch's rows lie end to end by actual length
    float2 *d_res = nullptr;     // burst_resample: the rows at 250 kHz, dec_cap outputs at the offsets of d_dec (this context's own,
                                 // allocated when the option is first set at a rate off the grid)
    DemodOut *d_demod;
    DecodedOut *d_decoded;
    IdaOut *d_ida;
    BurstWork *hp_work, *hp_work_dev;   // host / device view of the same mapped pinned buffer
    FirTile *hp_tiles;
    DemodOut *hp_demod;
    DemodPacked *hp_packed;                 // packed_records: the demodulator's result without LLRs, bits 8 per byte (pinned; written by demod_par_kernel)
    IdaPacked *hp_ida;                      // parsed_records: ida_decode() of each of them (pinned; written by ida_packed_kernel)
    FramePacked *hp_frame;                  // frame_records: frame_decode() of each of them (pinned; written by frame_packed_kernel)
    LineRec *hp_fine;                       // fine_freq: one record per burst (pinned; written by fine_freq_kernel; allocated with the option)
    TimeRec *hp_ftime;                      // fine_time: one record per burst (pinned; written by fine_time_kernel; allocated with the option)
    LineRec *hp_clock;                      // symbol_clock: one record per burst (pinned; written by symbol_clock_kernel; allocated with the option)
    SenseRec *hp_sense;                     // iq_sense: one record per burst (pinned; written by iq_sense_kernel; allocated with the option)
    uint32_t *hp_flag, *hp_flag_dev;    // [0] sequence number the helper publishes, [1] time-out flag of the waiting kernel
    int4 *hp_rot_new, *hp_rot_new_dev, *d_rot_new;   // (bin, row, from, to) of the checkpoint runs this batch has to build: mapped pinned / device
    uint32_t cfo_seq;
    bool packed;                 // this batch came back as DemodPacked records
    bool parsed;                 // ... and IdaPacked records
    bool framed;                 // ... and FramePacked records
    bool fined;                  // this batch ran the carrier frequency kernel: hp_fine holds its records
    bool timed;                  // this batch ran the symbol timing kernel: hp_ftime holds its records
    bool clocked;                // this batch ran the symbol clock kernel: hp_clock holds its records
    bool sensed;                 // this batch ran the I/Q sense kernel: hp_sense holds its records
    bool cfo_on_device;          // this batch's libm step ran on the device: h_cfreq is filled from the returned records
    std::vector<double> h_cfreq;
    // stream state (irdm_reset assigns a fresh one): the batch in flight
    struct State {
        int n = 0;                   // bursts in flight (0: idle)
        uint64_t chunk_no = 0;       // the chunk they come from
        uint64_t ring_lo = 0, ring_hi = 0;   // absolute sample range this batch's decimator may read from the history ring (incl.
                                     // the stale slots one reference ring length back); it reads nothing behind ev[1]
        std::vector<irdm_burst_t> recs;
    } st;
    bool owns_buffers;           // context 1 allocates its own device scratch; context 0 aliases the pipeline's
    float ms[3];                 // fir, post, demod of the last finished batch
};

// A chunk between irdm_feed_begin and the settling of its scan (kFeedSlots above).
struct FeedSlot {
    // stream state (irdm_reset assigns a fresh one): the chunk the slot holds
    struct State {
        const void *iq = nullptr;
        uint64_t c0 = 0, c1 = 0;
        float *mag = nullptr;
        int frames = 0;
        bool in_ring = false;       // the caller wrote the chunk where irdm_ingest_ptr() said: no copy into the ring
        bool lists = false;         // K1 wrote the band scan's candidate lists of the chunk (k1_pre / k1_counts / k1_entries)
    } st;
    hipEvent_t ev_start, ev_k1, ev_copy;
};

// Everything on the host side of a context that belongs to the STREAM it carries (a field is
// configuration, cache or stream state).  irdm_create leaves it as `StreamState{}` (but start_time_ns), irdm_reset assigns
// `StreamState{}`: a field whose fresh value is not zero says so here, and a field added here needs no line anywhere else.
// The per-element stream state of the batch contexts and feed slots: BatchCtx::State, FeedSlot::State.
struct StreamState {
    uint64_t total_samples = 0, tagged = 0, start_time_ns = 0;
    uint64_t begun_samples = 0;     // absolute index the next irdm_feed_begin starts at
    uint64_t begin_no = 0, end_no = 0;  // feeds begun / ended; slot = number % kFeedSlots
    uint64_t chunk_no = 0;          // chunks fed so far
    int host_primed = 0, host_hist_idx = 0;
    float peak_signal_db = 0;       // burst_detector_peak_signal over the finished bursts (starts at 0 like the reference's calloc)
    bool stream_closed = false;
    // detector scan in flight (scan_launch .. scan_finish)
    bool fl_active = false;
    bool fl_band_ran = false;       // the band scan's control block on the device belongs to the scan in flight
    int fl_mode = 0;                // 0 dense, 1 sparse (leader/updaters), 2 band
    int fl_done = 0;                // frames the dense scan primed before the in-flight scan proper
    int fl_frames = 0, fl_band_first = 0;
    const float *fl_mag = nullptr, *d_mag_last = nullptr;
    uint64_t fl_c1 = 0, fl_c0 = 0, fl_no = 0;
    const FeedSlot *fl_feed = nullptr;      // feed slot of the scan in flight
    int out_sel = 0;                // which set of export targets (h_pin_set ...) the scan that scan_finish settles next writes
    // the chained launch (scan_chain_try), taken over by scan_launch
    bool chain_pending = false;     // feed_end has enqueued this chunk's scan behind the previous one
    int chain_sel = 0, chain_band_first = 0;
    uint64_t chain_no = 0;          // the chunk the chained launch in flight scans
    bool settle_clean = true;       // the scan settled last committed on its own (no continuation, retry or fallback)
    // the speculation pass
    uint64_t spec_for_no = ~0ull;   // the chunk the speculation workspace holds a pass for (~0: none)
    int spec_frames = 0;            // ... and its frames
    // pipeline_depth >= 1: bursts of the last scanned chunk, processed during the next feed / irdm_flush
    bool has_pending = false;
    std::vector<GoneBurst> pend_gone;
    uint64_t pend_c1 = 0, pend_no = 0;
    // time-chunk sharding (hp_gate below)
    bool gate_armed = false;        // the next band scan enqueued from frame 0 waits for gate_seq before its first history read
    bool gate_open_pending = false; // a scan in flight waits for the history to arrive in gate_src
    const void *gate_src = nullptr; // the caller's receive buffer (device memory) the scan copies the history from
    // last chunk (probes)
    int last_frames = 0;
    const void *last_chunk = nullptr;
    uint64_t last_chunk_start = 0, last_chunk_end = 0;
    std::vector<irdm_burst_t> last_bursts;
    float last_ms[6] = {};
    // result queues; option "chunk_marks": one mark per batch of records pushed to them -- which chunk (in the order fed)
    // they belong to and how many records went to each queue -- for a caller that merges the records of several contexts
    // in stream order (group.cpp)
    RecordQueues q;
    std::deque<irdm_chunk_mark_t> q_marks;
    // option "spectrum_frames": the row still open -- its number, the absolute frame it starts at, the frames it holds and
    // which of the two carry sets on the device holds its sums (the reset zeroes both) --, the batches of finished rows
    // in flight and the rows that have arrived, until they are polled
    bool spec_started = false;
    uint64_t spec_row = 0, spec_row_frame = 0;
    int spec_fill = 0, spec_sel = 0;
    uint64_t spec_batches = 0;      // batches enqueued; pinned buffer = number % kSpecSlots
    std::deque<SpecBatch> spec_pending;
    std::deque<SpecRow> spec_q;
    // option "input_stats": the totals of the stream's raw samples and the passes in flight (input_stats.hpp)
    InputStatsStream in_stats;
    // option "symbol_clock": the per-frame records until they are polled and the summary's histogram (symbol_clock.hpp)
    SymbolClockStream clock{ kScHist };
    // option "fine_freq": the per-frame records until they are polled and the summary's histogram (fine_freq.hpp)
    FineFreqStream fine{ kFfHist };
    // option "fine_time": likewise (fine_time.hpp)
    FineTimeStream ftime{ kFtHist };
    // option "iq_sense": the per-frame votes until they are polled and the counts of the summary (iq_sense.hpp)
    IqSenseStream iq;
    // option "iq_moments": the sums of the stream and the passes whose rows are still on their way (iq_moments.hpp)
    IqMomentsStream iqm;
    // the corrections of irdm_feed_host: the scrub's totals and launches in flight, the DC tracker's position (host_chain.hpp)
    HostChainStream hc;
    // irdm_prime_host / _device (feed.cpp): the samples of the prefix fed in front of the recording (0: not primed), the
    // whole frames of the recording's head it was tiled from, and what the prefix moved start_time_ns back by -- the side
    // passes count positions and times from the recording's first sample, that is from primed_samples and
    // start_time_ns + prime_shift_ns
    uint64_t primed_samples = 0, prime_shift_ns = 0;
    int primed_frames = 0;
};

struct irdm_pipeline {
    irdm_config_t cfg;
    StreamState st;
    DetParams P;
    int dev_fmt;                // device sample format == cfg.format: 0 ci8, 1 ci16 (narrowed in the load stage,
                                // main.c:245-246), 2 cf32, 3 ci16 full precision, 4 SC16Q11, 6 cu8, 8 ci32,
                                // 9 24-bit in int32 (common.hpp load_iq)
    size_t bps;                 // bytes per device sample
    int feed_block, decim, out_rate;
    bool dev_cfo;            // the fine-CFO libm step runs on the device (the port reproduces this host's cexpf)
    bool dev_cfo_ok;         // irdm_create's self-check: libm_port.hpp reproduces THIS host's cexpf (option host_cfo cannot override a failed check)
    float sps;
    uint64_t ref_ring, ring_len;
    size_t l_cap;
    int n_ckpt, dec_stride, burst_cap, gone_cap;
    size_t max_chunk;
    int search_depth, pre_start;
    int in_ntaps, noise_ntaps, start_ntaps, rrc_ntaps, dl_len, ul_len;

    hipStream_t stream;      // detector (K1, prefilter, K2)
    hipStream_t bstream;     // per-burst stages + history ring (== stream unless pipeline_depth 1)
    hipStream_t stream2;
    int bstream_prio;        // priority of the per-burst streams
    hipStream_t sstream;     // detector scan kernels; pipeline_depth 1: a stream with CUs of its own (CU mask), so that the
                             // sequential leader wavefront is not slowed down by the per-burst kernels running beside it
    hipEvent_t ev_scan_in, ev_scan_out;
    // band_spec (scan_band.hip): round 0 of chunk k + 1 as a speculation pass on a second workspace and stream, beside chunk
    // k's scan; the scan of chunk k + 1 then opens with round 1
    int band_spec_opt = 1;                  // option band_spec
    void *d_band_spec = nullptr;
    BandWork band_spec = {};
    DetState *d_state_spec = nullptr;       // the carried bursts a speculation pass starts from (the previous pass's survivors)
    hipStream_t stream_spec = nullptr;
    hipEvent_t ev_sums1 = nullptr;          // behind the first sums pass of the latest band-scan launch (its sum_new: the pass's sums)
    hipEvent_t ev_spec_done = nullptr;      // behind the latest speculation pass
    uint64_t stat_spec_passes = 0, stat_spec_scans = 0, stat_sum_restarts = 0;
    int fir_order = 1;       // option fir_order / simd_order: 1 simd_avx2.c's operation order, 0 simd_generic.c's (--no-simd); per pipeline
    int fir_generic = 0;     // test hook fir_generic: 1 = always the any-M decimator (what 2 / 4 MHz streams take)
    int post_generic = 0;    // test hook post_generic: 1 = the runtime-tap-count instances of post_tiles / post_cfo / post2
    irdm::BandTune band_tune;   // options band_selfcheck / band_timeline / band_sum_restart
    hipEvent_t ev[10];   // 0 start,1 fft,2 scan,3 pre-fir,4 fir,5 post,6 demod,7 end,8 caller sync

    float *d_window, *d_hist, *d_sum, *d_mag;
    float2 *d_tw, *d_tw4096, *d_tw2048, *d_dl_fft, *d_ul_fft, *d_rot_incr, *d_rot_table;
    DetState *d_state;
    GoneBurst *d_gone;
    PeakCand *d_cand_a, *d_cand_b;
    void *d_ring, *d_stage;
    float *d_in_taps, *d_noise_taps, *d_start_taps, *d_rrc_taps, *d_cfo_window;
    int *d_fir_off;
    BurstWork *d_work;
    FirTile *d_tiles;
    size_t tiles_cap;
    float2 *d_dec, *d_lpf, *d_rrc_ws, *d_frames, *d_demod_ws, *d_probe;
    DemodOut *d_demod;
    DecodedOut *d_decoded;      // post-demod bit layer (bitlayer.hip)
    int2 *d_syn_ra, *d_syn_hdr; // BCH syndrome -> (error count, locator) tables (frame_decode.c:95-135)
    int *d_nbits;
    int decode_frames, decode_ida, detect_only;
    IdaOut *d_ida;
    int2 *d_syn_da, *d_syn_l1, *d_syn_l2, *d_syn_l3;
    int *d_dirs;
    std::vector<IdaOut> h_ida;
    std::vector<DecodedOut> h_decoded;
    // sparse scan (scan_fast.hip): prefilter lists, status word, pre-chunk snapshot for the dense fallback
    unsigned *d_counts, *d_goff;
    ListEntry *d_entries, *d_compact;
    float *d_pre, *d_sum_bak, *d_hist_bak;
    DetState *d_state_bak;
    int *d_status;
    unsigned long long *d_mc_ops;   // multi-CU sparse scan: operation words leader -> updaters, completion counters back
    unsigned *d_mc_done;
    int mc_ops_cap, mc_updaters, mc_auto;
    int scan_cus;               // CUs the scan stream may use (its CU mask, or the whole device)
    int n_cu = 0;               // compute units of cfg.device (the resident decimator's grid, fir_reg.hip)
    int scan_mode;              // 0 auto (sparse multi-CU where the device has the CUs, dense fallback), 1 dense only,
                                // 2 sparse on one CU, 3 sparse multi-CU
    uint64_t stat_fast_chunks, stat_fallbacks, stat_dense_frames;
    // band-parallel speculative scan (scan_band.hip): the default where band_scan_supported()
    void *d_band;               // one allocation, carved into `band`
    BandWork band;
    float *d_smin;              // smallest sum every bin went through in the last band scan (stale-list retry)
    bool band_ok;
    uint64_t stat_plan_tp[16] = {};
    uint64_t stat_tl_dur[32] = {}, stat_tl_gap[32] = {}, stat_tl_n[32] = {};
    uint64_t stat_band_chunks, stat_band_rounds, stat_band_retries, stat_band_aborts, stat_band_extra, stat_chain_undone, stat_chained;
    uint32_t last_band_flags;

    std::vector<GoneBurst> h_gone;
    int depth;
    int k1_first;            // per-burst chains start behind K1 (1) / K1 + ring copy (2) of the chunk just fed
    hipStream_t fstream;     // K1 (== stream unless pipeline_depth 1)
    float *d_mag2;           // pipeline_depth 1: second magnitude buffer
    std::vector<BurstWork> h_work;
    // the per-burst chains (bursts_enqueue / bursts_finish) and the helper thread that does their host step
    BatchCtx bc[kMaxBc];
    int n_bc;
    std::thread cfo_thread;
    std::mutex cfo_mu;
    std::condition_variable cfo_cv;
    std::deque<BatchCtx *> cfo_jobs;
    bool cfo_quit;
    int hp_gone_cap;
    // Two sets of the scan's export targets: a band scan launched BEHIND the one still in flight (scan_chain) exports into
    // the other set.  st.out_sel is the set of the scan that scan_finish settles next: h_pin() .. ev_end() are its targets.
    int *h_pin_set[2];          // pinned host words: [0..63] scan status, [64..65] n_gone/overflow, [66..67] hist_idx/primed.
                                // (a D2H copy into pageable memory blocks the host until the stream drains -- that would
                                // serialise pipeline_depth 1's deferred work behind the detector scan)
    GoneBurst *hp_gone_set[2];  // pinned copy of the finished-burst records of a scan
    hipEvent_t ev_sk_set[2][2]; // bracket the scan kernel itself on sstream (last_timings[1], bench.py's roofline)
    hipEvent_t ev_end_set[2];
    int *h_pin() const { return h_pin_set[st.out_sel]; }
    GoneBurst *hp_gone() const { return hp_gone_set[st.out_sel]; }
    hipEvent_t ev_sk(int i) const { return ev_sk_set[st.out_sel][i]; }
    hipEvent_t ev_end() const { return ev_end_set[st.out_sel]; }
    hipEvent_t ev_ring;         // pipeline_depth >= 1: the history-ring copy of the last fed chunk
    // chunks between irdm_feed_begin and irdm_feed_end: at most one at pipeline_depth 0, two (one chunk of look-ahead:
    // K1 of chunk N+1 is on the GPU before the host waits for the scan of chunk N-1) otherwise
    FeedSlot fs[kFeedSlots];
    // candidate lists written by K1 (fft_mag_r16_kernel<.., LISTS>), one set per feed slot: the reference levels the
    // lists were built against, the per-frame counts and entries
    float *k1_pre[kFeedSlots];
    unsigned *k1_counts[kFeedSlots];
    ListEntry *k1_entries[kFeedSlots];
    int k1_lists;               // option: 1 = let K1 build the lists where it can
    int band_first;             // band-scan rounds enqueued up front: 0 = as many as the previous chunk needed (at least
                                // 2, kBandFirst to begin with), n = always n (test hook)
    int band_auto;
    uint64_t stat_k1_lists;
    float *d_mag3;
    double host_us[10];         // pipeline_depth >= 1, accumulated host time: K1+ring enqueue, settle, chain enqueue, scan enqueue, wait for the older chain, final sync
    std::vector<DemodOut> h_demod;
    std::vector<float> h_frames;

    int packed_records;         // option: queue irdm_demod_packed_t records only
    int parsed_records;         // option: packed_records, and one irdm_ida_packed_t per irdm_demod_packed_t
    int frame_records;          // option: packed_records, and one irdm_frame_packed_t per irdm_demod_packed_t
    int chunk_marks;            // option: StreamState::q_marks
    int keep_frame_samples;
    int whole_window = 0;       // irdm_downmix_burst is running: the source IS the burst window, every sample of it delivered
    // rotator checkpoint rows on demand (rot_rows_prepare)
    int *d_rot_slot = nullptr;              // [n][rot_runs] centre bin, run -> block of d_rot_table, -1: none yet (written by the kernel that builds the run)
    int rot_runs = 0;                       // runs of kRotRun checkpoints per bin
    int rot_rows_used = 0;                  // bins that have a row
    int rot_blocks_used = 0, rot_blocks_cap = 0;
    std::vector<int> rot_len_h, rot_want, rot_touched;   // per bin: checkpoints built (or being built) / wanted by the batch at hand
    std::vector<int> rot_build_ctx;         // per bin: the batch context whose chain built (or is building) its latest run, -1: none
    std::vector<uint32_t> rot_build_gen;    // ... and which of that context's builds it was
    uint32_t rot_gen[kMaxBc] = {}, rot_done_gen[kMaxBc] = {};   // per context: builds enqueued / known to be complete (its stream was waited for)
    std::vector<float2 *> rot_retired;      // outgrown pools
    uint64_t stat_rot_builds = 0, stat_rot_rows = 0, stat_rot_ckpts = 0, stat_rot_grows = 0, stat_band_steps = 0;
    // rot_prebuild (default where pipeline_depth >= 1): every centre bin's row, as far as an ordinary burst needs it, built by
    // ONE background launch behind create instead of by the chains that first meet the bin (a stream's first chunks bring
    // hundreds of new bins each: 2.4-3.9 ms of checkpoint recurrence in front of a chain, 11.5 ms at 12 MHz dense)
    hipStream_t stream_rot_pre = nullptr;
    hipEvent_t ev_rot_pre = nullptr;
    int4 *d_rot_pre_news = nullptr;
    bool rot_pre_pending = false;           // chains wait for ev_rot_pre until the host has seen it complete
    int rot_pre_runs = 0;                   // runs of kRotRun checkpoints every bin's row was prebuilt with (0: none)
    size_t scratch_init = 0;                 // outputs the decimated / low-passed scratch of a context holds to begin with
    std::vector<float2 *> scratch_retired;   // outgrown scratch (freed when the context is closed, like the rotator pools)
    std::vector<void *> tiles_retired, tiles_host_retired;   // outgrown strip lists (device / pinned host): likewise
    uint64_t stat_scratch_grows = 0, stat_scratch_peak = 0, stat_tiles_grows = 0, stat_ring_waits = 0;
    // time-chunk sharding: the previous chunk's 512-frame history may arrive AFTER this chunk's scan has been enqueued
    // (irdm_expect_history / irdm_import_state_history_device): [0] sequence number the import publishes, [1] time-out
    // flag of the waiting kernel, in mapped pinned memory; the import's copies run on gstream
    uint32_t *hp_gate = nullptr, *hp_gate_dev = nullptr;
    uint32_t gate_seq = 0;
    // kernel clock (option "kernel_clock", common.hpp): records 0..2 the decimator of bc[0..2], 3..5 K1 of feed slot 0..2
    unsigned long long *d_kclk = nullptr;
    int kernel_clock = 0;
    unsigned long long *kclk_rec(int i) const { return kernel_clock && d_kclk ? d_kclk + (size_t)i * kKClkWords : nullptr; }
    // (the decimator of batch context c: records 0..2, and 6.. for the contexts beyond the third)
    unsigned long long *kclk_fir(int c) const { return kclk_rec(c < 3 ? c : 3 + c); }
    // option "spectrum_frames" (feed.cpp): R frames per row, 0 = off (configuration); the carry sets, the workspace, the
    // device rows of one chunk and the pinned buffers they are copied to (cache: allocated when the option is first set)
    int spectrum_R = 0;
    float *d_spec_carry = nullptr;          // [2 sets][3 planes][n]
    float *d_spec_ws = nullptr, *d_spec_out = nullptr;
    size_t spec_ws_cells = 0, spec_out_rows = 0;
    float *hp_spec[kSpecSlots] = {};
    hipEvent_t ev_spec[kSpecSlots] = {};
    SpectrumCarry spec_carry(int sel) const
    {
        float *b = d_spec_carry + (size_t)sel * 3 * (size_t)P.n;
        return SpectrumCarry{ b, b + P.n, b + 2 * (size_t)P.n };
    }
    // option "input_stats" (feed.cpp, input_stats.hpp): the side stream and the blocks of the passes (cache: allocated when
    // the option is first set); in_stats.on is the switch (configuration)
    InputStatsPass in_stats;
    // option "symbol_clock" (chain.cpp, symbol_clock.hpp): the switch (configuration); the batch contexts' hp_clock are the
    // cache, allocated when the option is first set
    int symbol_clock = 0;
    // option "fine_freq" (chain.cpp, fine_freq.hpp): likewise, with the batch contexts' hp_fine
    int fine_freq = 0;
    // option "fine_time" (chain.cpp, fine_time.hpp): likewise, with the batch contexts' hp_ftime
    int fine_time = 0;
    // option "iq_sense" (chain.cpp, iq_sense.hpp): the switch (configuration); the batch contexts' hp_sense are the cache,
    // allocated when the option is first set
    int iq_sense = 0;
    // option "burst_resample" (chain.cpp, burst_resample.hpp): the switch, the ratio decim 250000 / sample_rate in lowest
    // terms and its phase-major table (configuration: kept across irdm_reset; br_L == br_M == 1 at a rate on the grid, where
    // there is no table and nothing is launched); the batch contexts' d_res are the cache
    int burst_resample = 0;
    int br_L = 1, br_M = 1;
    std::vector<float> br_taps;
    float *d_br_taps = nullptr;
    uint64_t stat_br_launches = 0;
    uint64_t stat_ff_launches = 0;      // fine_freq_kernel launches by the chains
    uint64_t stat_ft_launches = 0;      // fine_time_kernel launches by the chains
    bool br_active() const { return burst_resample && br_L != br_M && d_br_taps; }
    // options "swap_iq", "scrub" / "scrub_limit_log2", irdm_iq_balance and irdm_dc_block (feed.cpp, host_chain.hpp): what
    // irdm_feed_host does to every chunk on the device before anything reads it -- the switches and their settings
    // (configuration), the scrub's blocks, the DC tracker's rings and the wire staging buffer (cache: allocated when a
    // setting first needs them), and the mark of irdm_feed_host's own call of irdm_feed_device
    HostChain hc;
    // irdm_prime_*'s own feeds of the prefix are under way: every side pass is off for them (feed.cpp)
    bool priming = false;
    // option "iq_moments" (feed.cpp, iq_moments.hpp): the pass over every chunk on its side stream (iqm.on: configuration;
    // the stream and the blocks: cache, allocated when the option is first set)
    IqMomentsPass iqm;
    // irdm_reset (feed.cpp)
    bool in_group = false;      // option group_member: a member of an irdm_group (group.cpp), irdm_reset is refused
    uint64_t stat_resets = 0;   // irdm_reset calls that went through
};

// The rotator checkpoints (rotator.h:36-46 restated: the phase of the float recurrence every 16 samples -- a whole row for
// a centre bin would be l_cap / 16 of them, 0.55 MB at 10 MHz) are kept for the centre bins bursts have actually appeared
// on and as far as those bursts have needed them: an arena of blocks of kRotRun checkpoints, a bin's row = its list of
// blocks (d_rot_slot[bin][run]), built by one lane per bin on the chain that needs them (the recurrence is sequential:
// 9 ns a sample) and continued when a longer burst comes.  The whole table -- a row for every FFT bin, 4.5 GB at 10 MHz
// and 10.9 GB at 12 MHz, built at create in rounds 1-3 -- is the arena's upper bound: it grows by doubling; an arena that
// has been outgrown stays allocated until the context is closed (chains in flight still read it).

// Every C-ABI entry that enqueues work for a pipeline: the calling thread is put on the pipeline's device.  (Every switch a
// launch helper reads -- the arithmetic order, the test hooks -- is a field of the pipeline and travels as an argument: two
// contexts of one process may differ in all of them.)
static inline void pipeline_enter(const irdm_pipeline *p) { (void)hipSetDevice(p->cfg.device); }

namespace irdmh {
bool rate_supported(int fs, int *fft_size);      // create.cpp: a sample rate irdm_create takes

// create.cpp
void pipeline_free(irdm_pipeline *p);
bool chain_stream_create(irdm_pipeline *, hipStream_t *out, int prio);

// chain.cpp
SampleSource make_source(const irdm_pipeline *p, const void *chunk, uint64_t c0, uint64_t c1);
int ring_guard(irdm_pipeline *p, uint64_t a0, uint64_t a1, hipStream_t st);
int ring_update(irdm_pipeline *p, const void *d_iq, uint64_t c0, uint64_t c1, hipStream_t st);
irdm_decoded_t finish_decoded(const DecodedOut &d, uint64_t id, uint64_t timestamp, double frequency);
int lcw_field(const char *b, int from, int to);
void format_lcw_header(int ft, int lcw_ft, int lcw_code, uint32_t lcw3_val, char *out, size_t outsz);
irdm_ida_t finish_ida(const IdaOut &d, const irdm_demod_t &f);
void cfreq_from_records(BatchCtx &b);
void fine_cfo_host(BatchCtx &b);
void cfo_helper_main(irdm_pipeline *p);
int rot_arena_reset(irdm_pipeline *p, long long blocks);
int rot_prebuild(irdm_pipeline *p);
int rot_rows_prepare(irdm_pipeline *p, BatchCtx &b, int nb, hipStream_t st);
int bursts_enqueue(irdm_pipeline *p, BatchCtx &b, const SampleSource &src, const GoneBurst *gone_list, int nb);
int bursts_finish(irdm_pipeline *p, BatchCtx &b);
int bursts_finish_records(irdm_pipeline *p, BatchCtx &b);
int process_bursts(irdm_pipeline *p, BatchCtx &b, const SampleSource &src, const GoneBurst *gone_list, int n_gone);

// feed.cpp
int spectrum_configure(irdm_pipeline *p, int R);
int input_stats_configure(irdm_pipeline *p, int on);
int symbol_clock_configure(irdm_pipeline *p, int on);
int fine_freq_configure(irdm_pipeline *p, int on);
int fine_time_configure(irdm_pipeline *p, int on);
int iq_sense_configure(irdm_pipeline *p, int on);
int burst_resample_configure(irdm_pipeline *p, int on);      // api.cpp
bool burst_resample_ratio(int sample_rate, int decim, long long *L, long long *M);
int scrub_configure(irdm_pipeline *p, int on);
int iq_moments_configure(irdm_pipeline *p, int on);
int dc_block_configure(irdm_pipeline *p, int wire_format, int block_log2, float seed_i, float seed_q);
int prime_check(const irdm_pipeline *p, size_t n_samples);
int prime_from_device(irdm_pipeline *p, const void *d_head, int F);

// scan_host.cpp
int scan_hop_in(irdm_pipeline *p);
int scan_hop_out(irdm_pipeline *p);
int scan_dense(irdm_pipeline *p, const float *mag, int n_frames, bool timed);
int scan_pick(const irdm_pipeline *p);
int scan_snapshot(irdm_pipeline *p);
int scan_restore(irdm_pipeline *p);
int scan_band_enqueue_at(irdm_pipeline *p, const float *mag, int n_frames, int done, int retry, bool more_rounds,
                                uint64_t c0, const FeedSlot *feed, int sel, int first, int chained, bool use_spec = false);
int scan_band_enqueue(irdm_pipeline *p, const float *mag, int n_frames, int done, int retry, bool more_rounds = false);
int scan_legacy_enqueue(irdm_pipeline *p, const float *mag, int n_frames, int done, bool sparse);
int scan_export(irdm_pipeline *p);
int scan_chain_try(irdm_pipeline *p, FeedSlot &f, uint64_t no);
int spec_enqueue(irdm_pipeline *p, FeedSlot &nx, uint64_t no);
int scan_launch(irdm_pipeline *p, const float *mag, int n_frames, uint64_t c1);
int scan_finish(irdm_pipeline *p, int *n_gone_out);
int settle(irdm_pipeline *p);
int quiesce(irdm_pipeline *p);
int deferred_enqueue(irdm_pipeline *p);
int deferred_finish(irdm_pipeline *p, BatchCtx &b);

}  // namespace irdmh
