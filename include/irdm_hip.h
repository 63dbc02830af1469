/*
 * irdm_hip.h -- C-ABI of the MI355X (gfx950) Iridium hot path.
 *
 * Plain C, no HIP or torch types: a C99 host (the reference's main.c /
 * burst_detect.c) links this library and nothing else.  Every entry point
 * names the reference interface it replaces (file:line into the reference).
 *
 * Layers
 *   1. gpu_burst_fft_*      -- the reference's one accelerator plug point
 *                              (opencl/burst_fft.h:35-47), same names and
 *                              conventions, so burst_detect.c's USE_GPU branch
 *                              (burst_detect.c:304-319, :655-674) links unchanged.
 *   2. irdm_*               -- batched superset: detect -> downmix -> demod for
 *                              whole chunks of the IQ stream, device-resident or
 *                              host buffers.  Same conventions as layer 1: opaque
 *                              context, NULL / -1 on error, caller-owned buffers,
 *                              one thread per context.
 *   3. irdm_format_raw      -- frame_output.c:160-199 RAW line, host C.
 */
#ifndef IRDM_HIP_H
#define IRDM_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------ */
/* 1. Reference plug point (opencl/burst_fft.h)                        */
/* ------------------------------------------------------------------ */

typedef struct gpu_burst_fft gpu_burst_fft_t;

/* opencl/burst_fft.h:35-36.  fft_size: power of two (2048..16384 use the
 * LDS-resident kernel).  window: fft_size floats, already /0.42
 * (burst_detect.c:247-250), copied.  NULL on failure => the caller falls back
 * to its CPU path (burst_detect.c:316-318). */
gpu_burst_fft_t *gpu_burst_fft_create(int fft_size, int batch_size, const float *window);

/* opencl/burst_fft.h:39.  NULL-safe. */
void gpu_burst_fft_destroy(gpu_burst_fft_t *g);

/* opencl/burst_fft.h:46-47.  input: batch_count*fft_size interleaved (re,im)
 * host floats; output: batch_count*fft_size host floats, |X|^2 DC-shifted.
 * 0 ok, -1 error (batch_count <= 0 or > batch_size, opencl/burst_fft.c:325-326)
 * => the caller discards the batch (burst_detect.c:659-665). */
int gpu_burst_fft_process(gpu_burst_fft_t *g, const float *input, float *output,
                          int batch_count);

/* Same computation on device-resident buffers (no H2D/D2H); stream is a
 * hipStream_t passed as void* (NULL = default stream).  Asynchronous. */
int gpu_burst_fft_process_device(gpu_burst_fft_t *g, const void *d_input, void *d_output,
                                 int batch_count, void *stream);

/* ------------------------------------------------------------------ */
/* 2. Batched pipeline                                                  */
/* ------------------------------------------------------------------ */

#define IRDM_FMT_CI8  0   /* options.c FMT_CI8  */
#define IRDM_FMT_CI16 1   /* options.c FMT_CI16: raw int16 pairs; narrowed to (int8)(v >> 8) (main.c:245-246) in the
                             kernels' load stage, on the device */
#define IRDM_FMT_CF32 2   /* options.c FMT_CF32 */
/* Full-precision interleaved int16 I/Q, 4 bytes per sample, converted in the kernels' load stage exactly as the
 * reference's live paths convert the same hardware's samples:
 *   IRDM_FMT_CI16_FULL  (float)v * (1.0f / 32768.0f)   SoapySDR CS16 (soapysdr.c:213-216)
 *   IRDM_FMT_SC16Q11    (float)v * (1.0f / 2048.0f)    bladeRF SC16Q11 (bladerf.c:93-96)
 * Contract: a context in either format produces exactly -- bit for bit, not within a tolerance -- the records (bursts,
 * frames, demods with their LLRs, packed, parsed and frame records) of an IRDM_FMT_CF32 context fed the same samples
 * converted to float and multiplied by the scale: int16 -> float is exact, and the power-of-two scale keeps every
 * product exact and far from the subnormal range. */
#define IRDM_FMT_CI16_FULL 3
#define IRDM_FMT_SC16Q11   4
/* rtl_sdr's files: unsigned 8-bit I/Q in offset binary, 2 bytes per sample, interleaved I, Q.
 *   IRDM_FMT_CU8        ((float)u - 127.5f) / 128.0f = (2u - 255) / 256, every step exact
 * 127.5 is the converter's mid-scale: with 128 every recording would carry a constant half-LSB DC term, which behind a band
 * selected off centre is a tone inside the band.  The same contract as formats 3 and 4: a cu8 context produces, bit for
 * bit, every record queue of an IRDM_FMT_CF32 context fed the converted samples.  The reference has no such input, so
 * the reference-shaped burst_detector_feed of irdm_compat.h does not take it.
 * The code is 6: irdm_create and both front ends refuse every format outside {0, 1, 2, 3, 4, 6}, and 5 and 7 in
 * particular stay refused ("unknown sample format N") -- callers and tests rely on those two as the unknown formats
 * next to the known ones. */
#define IRDM_FMT_CU8       6
/* 32-bit integer I/Q: interleaved little-endian int32 I, Q, 8 bytes per sample.
 *   IRDM_FMT_CI32       (float)v * 2^-31   SigMF ci32_le, 32-bit PCM WAV
 *   IRDM_FMT_CI32_24    (float)v * 2^-23   24-bit samples held in int32 (SDRangel's .sdriq at sample size 24)
 * (float)v rounds to nearest, ties to even -- v_cvt_f32_i32 on the device, numpy's astype(float32) on the host -- and the
 * power-of-two product is exact: INT32_MAX converts to exactly 1.0f in format 8.  The contract of formats 3, 4 and 6: a
 * context in either format produces, bit for bit, every record queue of an IRDM_FMT_CF32 context fed
 * v.astype(np.float32) * np.float32(scale).  The reference-shaped burst_detector_feed of irdm_compat.h does not take them.
 * irdm_create and both front ends refuse every format outside {0, 1, 2, 3, 4, 6, 8, 9}: 5, 7 and everything from 10 up. */
#define IRDM_FMT_CI32      8
#define IRDM_FMT_CI32_24   9

typedef struct {
    double center_frequency;   /* -c, burst_config_t.center_frequency (burst_detect.h:52) */
    int sample_rate;           /* -r, burst_config_t.sample_rate */
    float threshold_db;        /* -d; <= 0 -> 16 dB (iridium.h:37) */
    int format;                /* IRDM_FMT_* */
    int feed_block;            /* samples per reference feed call; 0 -> 32768 (main.c:225).
                                  Results equal the reference fed in blocks of this size. */
    int use_gardner;           /* main.c:143 default 1; 0 = --no-gardner */
    uint64_t start_time_ns;    /* replaces the wall clock read at burst_detect.c:849-853; 0 -> now */
    int device;                /* HIP device ordinal */
    size_t max_chunk_samples;  /* largest chunk passed to irdm_feed_*; 0 -> 64 Mi */
    int max_bursts_per_chunk;  /* sizing hint for the burst-record buffers, 0 -> 4096; a chunk with more finished bursts
                                  is redone with larger buffers (costs one dense scan), never dropped */
    int pipeline_depth;        /* 0: irdm_feed_* returns with the chunk's results pollable.
                                  1 .. 5: throughput mode.  irdm_feed_*(k) returns once chunk k is ingested (FFT done,
                                     samples in the history ring) and its detector scan is launched; the scan stays in
                                     flight while the caller produces chunk k+1.  The bursts of chunk k enter their
                                     per-burst chain (decimator .. demodulator, on a stream of its own) during
                                     irdm_feed_*(k+1); pipeline_depth + 1 chains are in flight and their records
                                     become pollable when their context is needed again, i.e. during
                                     irdm_feed_*(k+1+pipeline_depth), or at irdm_flush -- identical records, same order.
                                     A chain is 2.5-3 ms of dependent launches: the pipeline's period is at least that
                                     latency / (pipeline_depth + 1).  Every context holds ~0.5 GB of per-burst scratch and
                                     the history ring one more chunk.  Values above 5 are treated as 5. */
} irdm_config_t;

/* burst_info_t (burst_detect.h:29-37) + what emit_gone_bursts adds (burst_detect.c:703-742) */
typedef struct {
    uint64_t id;
    uint64_t start;
    uint64_t stop;
    uint64_t last_active;
    int32_t center_bin;
    float magnitude;           /* dB */
    float noise;               /* dBFS/Hz */
    float peak_rel;            /* raw relative magnitude of the creating peak */
    float base_sum;            /* baseline_sum[center_bin] at creation */
    uint64_t num_samples;      /* burst_data_t.num_samples */
    uint64_t avail_end;        /* sample_count at extraction time */
} irdm_burst_t;

#define IRDM_MAX_FRAME_SAMPLES 4440     /* IR_MAX_FRAME_LENGTH_SIMPLEX * 10 sps */
#define IRDM_MAX_BITS 896

/* downmix_frame_t (burst_downmix.h:32-51) without the sample pointer, plus stage probes */
typedef struct {
    uint64_t id;
    uint64_t timestamp;
    double center_frequency;
    float sample_rate;
    float samples_per_symbol;
    int32_t direction;         /* ir_direction_t */
    float magnitude;
    float noise;
    float uw_start;
    int32_t num_samples;
    int32_t dec_len;
    int32_t start;
    float center_offset;
    int32_t uw_start_idx;
    float corr_re, corr_im;
    int32_t drop_reason;       /* 0 = frame produced; 1..5 = the reference's five early returns
                                  (burst_downmix.c:645, :677, :702, :744, :773) */
    int32_t demod_ok;          /* qpsk_demod()'s return value for this frame (0 when no frame was produced) */
    int32_t demod_direction;   /* in->direction as qpsk_demod leaves it (qpsk_demod.c:444, :454-463): DIR_UNDEF (0)
                                  when the unique word was rejected, else the verified direction */
} irdm_frame_info_t;

/* demod_frame_t (qpsk_demod.h:24-38), bits/llr inline */
typedef struct {
    uint64_t id;
    uint64_t timestamp;
    double center_frequency;
    int32_t direction;
    float magnitude;
    float noise;
    int32_t confidence;
    float level;
    int32_t n_symbols;
    int32_t n_payload_symbols;
    int32_t n_bits;
    int32_t ok;
    float total_phase;
    uint8_t bits[IRDM_MAX_BITS];
    float llr[IRDM_MAX_BITS];
} irdm_demod_t;

/* The same frame without the soft outputs, hard bits 8 per byte (MSB first: bit i of the frame is
 * (bits[i / 8] >> (7 - i % 8)) & 1): everything frame_output_print reads (frame_output.c:168-197) in 176 bytes.  With
 * option "packed_records" 1 a context queues ONLY these (and the burst records): irdm_poll_demods / irdm_poll_frames
 * then return nothing, and 136 bytes per burst cross PCIe instead of 4.5 KB. */
typedef struct {
    uint64_t id;
    uint64_t timestamp;
    double center_frequency;
    int32_t direction;
    float magnitude;
    float noise;
    int32_t confidence;
    float level;
    int32_t n_symbols;
    int32_t n_payload_symbols;
    int32_t n_bits;
    int32_t ok;
    float total_phase;
    uint8_t bits[IRDM_MAX_BITS / 8];
} irdm_demod_packed_t;

/* decoded_frame_t (frame_decode.h:26-60), flattened: the post-demod bit layer's result for one demodulated frame */
typedef struct {
    int32_t type;              /* frame_type_t: 0 FRAME_UNKNOWN, 1 FRAME_IRA, 2 FRAME_IBC */
    int32_t sat_id, beam_id;
    int32_t pos_xyz[3];        /* ira_data_t */
    int32_t alt;
    int32_t n_pages;
    double lat, lon;
    uint32_t page_tmsi[12];
    int32_t page_msc[12];
    int32_t timeslot, sv_blocking, bc_type;    /* ibc_data_t */
    uint32_t iri_time;
    int32_t bch_len;           /* decoded data bits assembled (probe; not in the reference's struct) */
    int32_t pad;
    uint64_t id;               /* the frame's burst id */
    uint64_t timestamp;        /* decoded_frame_t.timestamp */
    double frequency;          /* decoded_frame_t.frequency = the refined centre frequency */
} irdm_decoded_t;

/* ida_burst_t (ida_decode.h:31-56), flattened: one IDA burst after LCW + BCH decoding, before multi-burst reassembly */
typedef struct {
    int32_t ok;                /* ida_decode()'s return value */
    int32_t ft, lcw_ft, lcw_code, ec_lcw;      /* lcw_t */
    uint32_t lcw3_val;
    int32_t da_ctr, da_len, cont, crc_ok;
    uint32_t stored_crc, computed_crc;
    int32_t fixederrs, payload_len, bch_len;
    int32_t direction;         /* ir_direction_t of the frame */
    uint8_t payload[32];
    uint8_t bch_stream[256];
    char lcw_header[128];      /* "LCW(...)" padded to 110 characters + one space (format_lcw_header) */
    uint64_t id;               /* the frame's burst id */
    uint64_t timestamp;
    double frequency;
    float magnitude, noise, level;
    int32_t confidence, n_symbols;             /* n_symbols = the frame's payload symbols (ida_decode.c:648) */
    int32_t pad;
} irdm_ida_t;

/* ida_decode()'s result for one frame of the packed record path in 88 bytes (option "parsed_records" 1): the fields
 * irdm_ida_t takes from the decoder; the frame's own (direction, timestamp, levels, ...) are in the irdm_demod_packed_t
 * it belongs to.  bch_stream holds the first 256 bits of the decoded stream 8 per byte, MSB first (bit i is
 * (bch_stream[i / 8] >> (7 - i % 8)) & 1); bch_len counts all of them, as ida_burst_t.bch_len does.
 * irdm_ida_unpack turns the pair into the irdm_ida_t the "decode_ida" path returns. */
typedef struct {
    int32_t ok;                /* ida_decode()'s return value; every other field is 0 when it is 0 */
    uint32_t lcw3_val;
    uint8_t ft, lcw_ft, lcw_code, ec_lcw;
    uint8_t da_ctr, da_len, cont, crc_ok;
    uint16_t stored_crc, computed_crc;
    uint8_t fixederrs, payload_len;
    uint16_t bch_len;
    uint8_t payload[32];
    uint8_t bch_stream[32];
} irdm_ida_packed_t;

/* frame_decode()'s result for one frame of the packed record path in 80 bytes (option "frame_records" 1): the fields
 * irdm_decoded_t takes from the decoder, in narrow types (pos_xyz are 12-bit signed, page_msc 5 bits).  type is 0 for
 * every frame frame_decode() does not take, and every other field is 0 then.  irdm_frame_unpack turns the record and the
 * irdm_demod_packed_t it belongs to into the irdm_decoded_t the "decode_frames" path returns. */
typedef struct {
    uint8_t type;              /* 0 FRAME_UNKNOWN, 1 FRAME_IRA, 2 FRAME_IBC */
    uint8_t sat_id, beam_id, n_pages;
    int16_t pos_xyz[3];
    uint16_t bch_len;
    uint8_t timeslot, sv_blocking, bc_type, pad;
    uint32_t iri_time;
    uint32_t page_tmsi[12];
    uint8_t page_msc[12];
} irdm_frame_packed_t;

/* option "chunk_marks" 1: one mark per batch of records a context pushes to its queues -- the chunk they belong to (chunks
 * counted from 0 in the order fed) and how many records each queue received, in queue order.  A chunk without bursts
 * leaves no mark; a chunk with more bursts than a batch holds leaves several, one after the other. */
typedef struct {
    uint64_t chunk;
    uint32_t n_bursts, n_frames, n_demods, n_packed, n_decoded, n_ida;
} irdm_chunk_mark_t;

/* option "spectrum_frames": one row of the waterfall (irdm_poll_spectrum) */
typedef struct {
    uint64_t row;              /* rows of a stream counted from 0 */
    uint64_t first_frame;      /* absolute frame the row starts at: frame f holds samples f * n_bins .. f * n_bins + n_bins - 1 */
    uint64_t timestamp_ns;     /* of that frame's first sample: irdm_start_time_ns + sample offset at the context's rate */
    uint32_t n_frames;         /* frames in the row: R, or fewer in the row irdm_flush closed */
    uint32_t n_bins;           /* irdm_spectrum_bins */
} irdm_spectrum_row_t;

/* option "input_stats": what the raw samples of the input say about the recording (irdm_input_stats).  x is the converted
 * value, exactly as the pipeline's load stage gives it; a component "at a rail" holds the file code the converter clips to:
 *   ci8 -128 / 127;  cu8 0 / 255;  ci16 and ci16-full -32768 / 32767;  sc16q11 v <= -2048 / v >= 2047;  cf32 x <= -1 / x >= 1;
 *   ci32 INT32_MIN / INT32_MAX;  24-bit in int32 v <= -2^23 / v >= 2^23 - 1.
 * Plain ci16: rails and code_min / code_max are taken on the 16-bit code v, sum / sum_sq / abs_max on the narrowed value
 * (v >> 8) / 128 the pipeline sees -- a 12-bit recording read as ci16 reports an RMS of a fraction of an LSB, which is true.
 * Integer formats: x = c * 2^-k with an integer c; the sums of c and c^2 are kept as integers and sum / sum_sq formed from
 * the totals with one rounding, so these fields and every count do not depend on how the stream was cut into chunks.
 * (The int32 formats: c = v, k = 31 / 23; c^2 reaches 2^62, its sums are carried in two words on the device; abs_max is
 * the converted value of the extreme code, rounded as the load stage rounds it.)
 * cf32: sum / sum_sq are double sums of the exact x and x^2 over the finite components, reproducible for a given cut. */
typedef struct {
    uint64_t n_samples;
    uint64_t n_rail_lo[2], n_rail_hi[2];  /* [0] = I, [1] = Q: components at the format's negative / positive rail */
    uint64_t n_nonfinite[2];              /* cf32: NaN or Inf; left out of everything below */
    int32_t  code_min[2], code_max[2];    /* integer formats: extreme file codes seen; 0 for cf32 */
    double   sum[2], sum_sq[2];           /* of the converted value x, as load_iq gives it */
    float    abs_max[2];                  /* max |x| over finite components */
} irdm_input_stats_t;

/* option "symbol_clock": the symbol clock error of one downmixed frame, estimated on the device from the samples the
 * demodulator is handed (irdm_poll_symbol_clock, irdm_symbol_clock_batch).  |x|^2 of a frame carries a spectral line at the
 * symbol rate, 1 / (sps (1 + eps)) cycles per sample at the context's nominal sps = 10: the line is looked for on the grid
 * eps = -0.08 + 0.001 k, k = 0 .. 160, and refined by a three-point parabola.  eps is the README's clock error
 * fs / decim / 250000 - 1 as the samples show it, whatever rate was declared. */
#define IRDM_CLOCK_INVALID       1u   /* no estimate (eps = quality = 0): the frame was dropped in front of the demodulator, is
                                       * shorter than 64 samples, all zero, or holds a sample that is not finite */
#define IRDM_CLOCK_OUT_OF_RANGE  2u   /* the maximum is at an edge of the grid, or one of 30 guard points of the same step beyond
                                       * an edge (to +-11 %) exceeds it: eps is that edge */
#define IRDM_CLOCK_NOT_OK        4u   /* (set by the context, never by the stage call) the demodulator rejected the frame's
                                       * unique word: no demodulator record goes with this one */
typedef struct {
    uint64_t id;               /* the burst's id; irdm_symbol_clock_batch: the frame's index */
    float    eps;              /* clock error, a fraction (0.0025 = +0.25 %) */
    float    quality;          /* the maximum over the mean of the grid: 12 and more on a clean frame, 2 .. 7 without a line */
    uint32_t flags;            /* IRDM_CLOCK_* */
    uint32_t n;                /* samples of the frame */
} irdm_clock_est_t;

/* irdm_symbol_clock: the stream so far.  Frames count as used when their unique word passed and their record is neither
 * invalid nor out of range; median and quartiles are centres of the 0.01 % bins of a histogram over +-8 %, so they do not
 * depend on how the stream was cut into chunks or feeds (0 while frames_used is 0). */
typedef struct {
    uint64_t frames_used, frames_not_ok, frames_out_of_range;
    double   median, q25, q75;       /* fractions */
    double   implied_rate_hz;        /* 250000 * decim * (1 + median): the rate the samples look like */
    uint64_t frames_invalid;         /* unique word passed, record invalid */
} irdm_symbol_clock_t;

/* option "fine_freq": the carrier frequency of one downmixed frame, estimated on the device from the samples the
 * demodulator is handed (irdm_poll_fine_freq, irdm_fine_freq_batch).  The fourth power of a QPSK frame carries a spectral
 * line at four times its residual carrier offset: the line is looked for on the grid -1000 + 20 k Hz, k = 0 .. 100, then on
 * 11 points 4 Hz apart around the maximum, and refined by a three-point parabola; df is a quarter of its place.  The result
 * is the frequency at the middle of the frame, to about 1 Hz at the signal levels the detector decodes at all (README:
 * "Carrier frequency to 1 Hz").  Beyond +-300 Hz of the downmixer's value the estimator is blind: the line is then past the
 * guard points and the grid shows the frame's modulation. */
#define IRDM_FINE_FREQ_INVALID       1u   /* no estimate (df = quality = 0): the frame was dropped in front of the demodulator,
                                           * is shorter than 64 samples, all zero, or holds a sample that is not finite */
#define IRDM_FINE_FREQ_OUT_OF_RANGE  2u   /* the coarse maximum is at an edge of the grid, or one of 10 guard points of the same
                                           * step beyond an edge (to +-1200 Hz) exceeds it: df is that edge, +-250 Hz */
#define IRDM_FINE_FREQ_NOT_OK        4u   /* (set by the context, never by the stage call) the demodulator rejected the frame's
                                           * unique word: no demodulator record goes with this one */
typedef struct {
    uint64_t id;               /* the burst's id; irdm_fine_freq_batch: the frame's index */
    double   freq_hz;          /* the downmixer's centre frequency of the frame + df_hz; irdm_fine_freq_batch: df_hz */
    float    df_hz;            /* what the frame's samples add to the downmixer's value */
    float    quality;          /* the coarse maximum over the mean of the coarse grid: 9 .. 14 on a clean frame, 3 .. 4 on noise */
    uint32_t flags;            /* IRDM_FINE_FREQ_* */
    uint32_t n;                /* samples of the frame */
} irdm_fine_freq_t;

/* irdm_fine_freq: the stream so far.  A frame counts as applied when its unique word passed and its record is neither invalid
 * nor out of range: its demodulator record then carries freq_hz as center_frequency.  median and quartiles are those of
 * (refined - PLL), the PLL's being the value the record carries with the option off; they are centres of the 1 Hz bins of a
 * histogram over +-500 Hz, so they do not depend on how the stream was cut into chunks or feeds (0 while frames_applied is 0). */
typedef struct {
    uint64_t frames_seen;                 /* frames that reached the demodulator: the sum of the four below */
    uint64_t frames_applied, frames_not_ok, frames_out_of_range, frames_invalid;
    double   median, q25, q75;            /* Hz */
} irdm_fine_freq_summary_t;

/* option "fine_time": the arrival time of one downmixed frame's first symbol, refined on the device from the samples the
 * demodulator is handed (irdm_poll_fine_time, irdm_fine_time_batch).  |x|^2 of a frame carries a spectral line at the symbol
 * rate, and the phase of that line is the symbol timing.  Over the window W = min(n, 131 sps) samples (simplex: 80 sps) at the
 * context's nominal sps = 10, with p' = |x|^2 less its mean over the window and S(f) = sum p'[k] exp(-2 pi i f k):
 *   tau = -arg S(1 / sps) / 2 pi * sps, in [-sps / 2, sps / 2): the distance in samples from the frame's sample 0 to the
 *   nearest symbol centre.
 * The device leaves S(1 / sps) and the floor in doubles, bit for bit the same on every build; arg is taken on the host.
 * Without the option a demodulator record's timestamp is the reference's: the burst's time plus the first sample at which the
 * smoothed magnitude crosses 0.28 of its maximum, about 0.73 ms in front of the frame and wandering by 6 to 60 us with the
 * noise.  With it the timestamp is the time of the frame's sample 0 -- the centre of the unique word's first symbol on a
 * downlink frame, 32 symbols behind the start of the correlator's match on an uplink one, as the reference cuts it --
 * to about 0.3 us at the levels the detector decodes at all (README: "Arrival time to 0.1 us"):
 *   timestamp + llrint((uw_start_idx + delta) 1e9 / 250000), delta = tau, or corr where the record carries a flag. */
#define IRDM_FINE_TIME_INVALID    1u   /* no estimate (tau = quality = s_re = s_im = floor = 0): the frame was dropped in front of
                                        * the demodulator, is shorter than 64 samples, all zero, or holds a sample that is not
                                        * finite */
#define IRDM_FINE_TIME_AMBIGUOUS  2u   /* (set by the context, never by the stage call) |tau - corr| is above sps / 4: the line
                                        * and the correlator name different places; the time is the correlator's */
#define IRDM_FINE_TIME_NOT_OK     4u   /* (set by the context, never by the stage call) the demodulator rejected the frame's
                                        * unique word: no demodulator record goes with this one */
typedef struct {
    uint64_t id;               /* the burst's id; irdm_fine_time_batch: the frame's index */
    uint64_t time_ns;          /* the time of the frame's sample 0 as its demodulator record carries it; irdm_fine_time_batch: 0 */
    double   tau;              /* samples; the double the time was computed from */
    double   s_re, s_im;       /* S(1 / sps): the kernel's sums */
    double   floor;            /* the mean of |S|^2 at 1 / sps (1 + 0.02 j), j = +-2 .. +-9 */
    float    corr;             /* the correlator's parabola correction (irdm_frame_info_t.uw_start), samples; irdm_fine_time_batch: 0 */
    float    quality;          /* |S(1 / sps)|^2 / floor.  Reported, and flags nothing: 3 .. 30 on frames whose unique word
                                * passed, up to 7 on pure noise */
    uint32_t flags;            /* IRDM_FINE_TIME_* */
    uint32_t n;                /* samples of the frame */
} irdm_fine_time_t;

/* irdm_fine_time: the stream so far.  A frame counts as applied when its unique word passed and its record is neither invalid
 * nor ambiguous: its demodulator record then carries the line's time; an ambiguous or invalid one carries the correlator's.
 * median and quartiles are those of tau - corr over the applied frames, in samples; they are centres of the 0.01-sample bins of
 * a histogram over +-2.5 samples, so they do not depend on how the stream was cut into chunks or feeds (0 while
 * frames_applied is 0). */
typedef struct {
    uint64_t frames_seen;                 /* frames that reached the demodulator: the sum of the four below */
    uint64_t frames_applied, frames_not_ok, frames_ambiguous, frames_invalid;
    double   median, q25, q75;            /* samples */
} irdm_fine_time_summary_t;

/* option "iq_sense": which way round I and Q of one demodulated frame were (irdm_poll_iq_votes, irdm_iq_sense_batch).
 * A recording with its two components exchanged (a Q/I WAV, the other SigMF convention, an inverting mixer) demodulates
 * with ok = 1 and full confidence -- preamble and unique words use the DQPSK states 0 and 2 alone, which conjugation maps
 * onto themselves -- but every frequency is mirrored about the centre and the two bits of every dibit are exchanged, so no
 * payload decodes.  Three predicates that chance does not satisfy are evaluated on the frame's bits as they are
 * ("recorded") and with b'[2i] = b[2i+1], b'[2i+1] = b[2i] over the whole frame, LLRs following ("exchanged"):
 *   IRA (bit 0)  a DL or UL access code, n_bits >= 24 + 96, each of the three header blocks of the 3-way de-interleave has
 *                a zero BCH(31,21) remainder (polynomial 1207) and its 32nd bit is their parity, nothing corrected;
 *   IBC (bit 1)  the access code, n_bits >= 24 + 6 + 64, a zero BCH(7,3) remainder (polynomial 29) of the 6 header bits,
 *                and the first two blocks of the 2-way de-interleave clean in the same way;
 *   IDA (bit 2)  the device's IDA decode (Chase decoding on the LLRs, as irdm_ida_decode_batch with use_llr) succeeds
 *                with da_len > 0 and a CRC that holds.
 * A frame votes recorded when recorded != 0 && exchanged == 0, exchanged when the reverse holds, counts as "both" when
 * both are non-zero and is silent otherwise. */
#define IRDM_IQ_IRA 1u
#define IRDM_IQ_IBC 2u
#define IRDM_IQ_IDA 4u
typedef struct {
    uint64_t id;               /* the burst's id; irdm_iq_sense_batch: the frame's index */
    uint8_t  recorded;         /* IRDM_IQ_* that hold on the bits as they are */
    uint8_t  exchanged;        /* ... with the two bits of every dibit exchanged */
    uint16_t pad;
    uint32_t n_bits;           /* the bits looked at: the frame's, rounded down to whole dibits */
} irdm_iq_vote_t;

#define IRDM_IQ_TOO_FEW      0     /* fewer than 5 deciding frames (the threshold of the symbol clock check) */
#define IRDM_IQ_AS_RECORDED  1     /* at least 9 in 10 of the deciding frames vote recorded */
#define IRDM_IQ_EXCHANGED    2     /* at least 9 in 10 vote exchanged: the recording is I/Q-swapped */
#define IRDM_IQ_MIXED        3
/* irdm_iq_sense: the stream so far.  kind index 0 IRA, 1 IBC, 2 IDA: a deciding frame is counted under every kind its
 * deciding sense holds (a frame that is IRA and IDA at once under both).  verdict over d = votes_recorded +
 * votes_exchanged: TOO_FEW when d < 5, AS_RECORDED when 10 votes_recorded >= 9 d, EXCHANGED when 10 votes_exchanged >= 9 d,
 * MIXED otherwise. */
typedef struct {
    uint64_t frames;                        /* frames seen (unique word passed) */
    uint64_t votes_recorded, votes_exchanged, votes_both;
    uint64_t kind_recorded[3], kind_exchanged[3], kind_both[3];
    int32_t  verdict;                       /* IRDM_IQ_TOO_FEW .. IRDM_IQ_MIXED */
    int32_t  pad;
} irdm_iq_sense_t;

/* option "scrub": what the pass that zeroes non-finite and out-of-range cf32 samples has done (irdm_scrub_stats,
 * irdm_frontend_scrub_stats, irdm_scrub_device).  With L = ldexpf(1, limit_log2) a component c is good iff fabsf(c) <= L
 * (a NaN fails the comparison); a sample with a component that is not good becomes +0.0f, +0.0f, all 64 bits zero; every
 * other sample keeps its bits (-0.0, subnormals and a component equal to +-L among them).  A stream position is the
 * sample's index in the stream, counted from 0 at create / reset as irdm_sample_count counts; in front of a front end it
 * is the index in the capture.  No figure depends on how the stream is cut into chunks. */
#define IRDM_SCRUB_DEFAULT_LOG2 40
typedef struct {
    uint64_t n_samples;              /* samples the pass has covered since create / reset */
    uint64_t n_zeroed;               /* samples zeroed */
    uint64_t n_nonfinite;            /* components whose exponent field is all ones */
    uint64_t n_over;                 /* finite components with |c| > L */
    uint64_t first, last;            /* stream positions of the first and the last zeroed sample; valid when n_zeroed > 0 */
    int32_t  limit_log2;
    int32_t  active;                 /* 0 when the format is not cf32: nothing was launched, every figure above is 0 */
} irdm_scrub_stats_t;

/* option "iq_moments": the second moments of the stream's I and Q and the receiver's I/Q imbalance derived from them
 * (irdm_iq_moments, irdm_frontend_iq_moments_stats, irdm_iq_moments_device).  The samples are taken as the pipeline's load
 * stage converts them; every term is formed in binary64, where i, q and their products are exact, so the sums depend on
 * the order of addition alone.  A cf32 sample with a component that is not finite is left out (n_samples - n_used of them).
 * Derived on the host in binary64 with N = n_used and the central moments C_ab = sum_ab / N - (sum_a / N)(sum_b / N):
 *   valid      1 iff N >= 2, C_II > 0, C_QQ > 0 and |C_IQ| < sqrt(C_II C_QQ); otherwise the three figures below are 0
 *   gain_db    10 log10(C_QQ / C_II): the Q arm's gain over the I arm's (g = sqrt(C_QQ / C_II))
 *   phase_deg  asin(C_IQ / sqrt(C_II C_QQ)) in degrees: by how much the two arms miss quadrature
 *   image_db   20 log10(|1 - g e^{j phi}| / |1 + g e^{-j phi}|), not below -120: the level of the image at -f of a signal
 *              at +f.  The estimator's own floor on 2 M samples of a clean scene is -70 to -82 dB.
 * A DC offset in either arm does not disturb the figures (the moments are central). */
typedef struct {
    uint64_t n_samples, n_used;              /* seen; with both components finite */
    double   sum_i, sum_q, sum_ii, sum_qq, sum_iq;
    double   gain_db, phase_deg, image_db;
    int      valid, reserved;
} irdm_iq_moments_t;

typedef struct irdm_pipeline irdm_pipeline_t;

/* burst_detector_create + burst_downmix_create (burst_detect.c:174, burst_downmix.c:223):
 * derives every constant the reference derives, designs the filters on the host with the
 * host libm, uploads them.  NULL on failure (no device, bad config, allocation). */
irdm_pipeline_t *irdm_create(const irdm_config_t *cfg);
void irdm_destroy(irdm_pipeline_t *p);

/* burst_detector_feed / _feed_cf32 (burst_detect.h:74-79) for a whole chunk.
 * n_samples must be a multiple of feed_block except for the last chunk of the stream.
 * _device: d_iq is a device pointer to raw samples in the configured format (cf32 pairs, int16 pairs or int8
 * pairs), stream = the hipStream_t that produced them, or NULL when the data is already complete (no ordering is
 * established then; NULL does not mean the legacy default stream).  The buffer may be reused when the call returns.
 * pipeline_depth 0: returns after the chunk is fully processed (results pollable); pipeline_depth 1: see above.
 * _host: the same for a host buffer; the H2D copy is asynchronous DMA when the buffer is pinned
 * (irdm_host_alloc, hipHostMalloc, hipHostRegister) and overlaps the previous chunk's detector scan.
 * Returns the number of bursts whose records became pollable, or -1 on error. */
int irdm_feed_device(irdm_pipeline_t *p, const void *d_iq, size_t n_samples, void *stream);
/* irdm_feed_device in two halves: _begin = what does not depend on the detector state (K1 of the chunk, its copy into
 * the history ring), _end = detector scan + per-burst work.  A time-sharded rank calls _begin, receives the previous
 * rank's state (irdm_import_state_device), then calls _end.
 * pipeline_depth >= 1: one chunk of look-ahead -- irdm_feed_begin(k+1) may be called before irdm_feed_end(k) (the calls
 * alternate after that; a third pending begin returns -1), which puts K1 of the next chunk on the GPU before the host
 * waits for the detector scan of chunk k-1, and lets the library enqueue the speculation pass and the scan of chunk k+1 with
 * chunk k's.  (A second chunk begun ahead was measured in rounds 5 and 6 -- 70.6 against 74.1-74.4 Gsamples/s -- and removed.)
 * The buffer handed to _begin may be reused when the matching _end has returned.  A detector state may only be imported
 * (irdm_import_state*) while no chunk but the one begun last is pending. */
int irdm_feed_begin(irdm_pipeline_t *p, const void *d_iq, size_t n_samples, void *stream);
int irdm_feed_end(irdm_pipeline_t *p);
/* pipeline_depth >= 1: where the producer of the next chunk (an H2D copy, a conversion kernel) may write it so that the
 * context does not have to copy it into its history ring (8 B/sample read + written for cf32): the ring slot of the
 * stream position the next irdm_feed_begin starts at.  Pass the pointer to irdm_feed_begin / irdm_feed_device as
 * d_iq; nothing waits for the chunk to be "released" then.  NULL at pipeline_depth 0 or if the chunk would straddle the
 * end of the ring -- it never does when every chunk but the last has max_chunk_samples.  The slot belongs to the
 * producer until it is fed; it is reused one ring length (irdm_ring_ptr) later. */
void *irdm_ingest_ptr(irdm_pipeline_t *p, size_t n_samples);
/* the history ring (device memory, configured sample format) and its length in samples: sample i of the stream lives
 * at index i % length */
void *irdm_ring_ptr(irdm_pipeline_t *p, uint64_t *len_samples);
int irdm_feed_host(irdm_pipeline_t *p, const void *h_iq, size_t n_samples);
/* pipeline_depth >= 1: finish the detector scan in flight and every per-burst chain, oldest first; all records of the
 * chunks fed so far are pollable afterwards.  Returns bursts processed or -1 (also when a chunk handed over with
 * irdm_feed_begin still waits for its irdm_feed_end). */
int irdm_flush(irdm_pipeline_t *p);
/* irdm_flush without the waiting (pipeline_depth >= 1): settles the detector scan in flight, enqueues the per-burst work of
 * its bursts and returns; records of batches that have already finished become pollable.  For callers that interleave
 * other work -- a time-sharded rank's next super-step -- with the chain.  Returns the number of bursts whose records were
 * emitted, -1 on error.  (No reference counterpart: burst_downmix / qpsk_demod run on their own threads there,
 * main.c:667-694.) */
int irdm_advance(irdm_pipeline_t *p);
/* Another stream through the same context (no reference counterpart: burst_detector_destroy + _create cost microseconds
 * there; here irdm_create builds hundreds of MB of device state).  Ends whatever stream the context carried and leaves it
 * indistinguishable, in every result it will produce, from a context just returned by irdm_create with the same
 * irdm_config_t -- but this centre frequency and start time (0 -> now, as in irdm_create) -- and the same options set:
 * burst ids, sample indices, the detector's 512-frame priming, timestamps, irdm_tagged_bursts, irdm_sample_count,
 * irdm_detector_stats and irdm_export_state all start over.  May be called after irdm_flush, or mid-stream: the scan and
 * the per-burst chains in flight are then waited for and abandoned, and EVERY record queue is emptied, polled or not.
 * What depends only on rate, format and options is kept and nothing is allocated: filters and tables, the rotator
 * checkpoint rows, scratch that has grown, streams and events.  The "stat" counters of irdm_get_stat and the
 * irdm_kernel_clock sums are diagnostics of the context, not of a stream: they run on ("resets" counts these calls).
 * Waits for the context's own streams, not for the device.  0 ok; -1 and nothing changed when a chunk handed over with
 * irdm_feed_begin still waits for its irdm_feed_end, when a scan waits for a history import (irdm_expect_history), or for
 * a member of a group (a group is not reset: destroy and create it). */
int irdm_reset(irdm_pipeline_t *p, double center_frequency, uint64_t start_time_ns);
/* Priming from the recording's own head (no reference counterpart: burst_detect.c can start no burst before its 512-frame
 * history is full, so a recording's first 512 FFT frames -- 0.37 to 0.70 s -- are searched by nobody; a program that has
 * the whole file can do better).  Given the n_samples leading samples of a recording -- in the format irdm_feed_host
 * takes: the configured one, or irdm_iq_balance's wire format --, with N = irdm_fft_size and H = 512 N:
 *   F = min(512, n_samples / N) whole frames are used (F == 0: -1);
 *   the prefix P is H samples long, frame k of it is frame k mod F of the given samples (a recording shorter than H is
 *   primed from itself, tiled: the tiling is device copies, F frames are uploaded once);
 *   P is fed as the head of the stream through the ordinary path, in pieces of at most max_chunk_samples: K1, the detector
 *   scan and the history ring as usual, options swap_iq and scrub and irdm_iq_balance applied as on any chunk of
 *   irdm_feed_host -- and every side pass off: nothing of P enters irdm_input_stats, irdm_iq_moments, irdm_scrub_stats or
 *   the rows of option spectrum_frames;
 *   the time origin moves to T0' = T0 - floor(H 10^9 / sample_rate) ns, which irdm_start_time_ns returns from then on.
 * The caller then feeds the recording from its sample 0 as usual: file sample i is stream position H + i.
 * Records (bursts, frames, demods, packed, parsed and frame records, symbol_clock and iq_sense votes): exactly those of a
 * plain context with the same options, created with start time T0' and fed P followed by the recording; sample indices
 * in them count from the start of P.  Bursts of P itself are found and queued like any others (they repeat the
 * recording's).  Not promised: equality with the unprimed run on later bursts -- the baseline is a running float sum with a
 * different past.
 * Side passes: the results of a plain context fed the recording alone with start time T0 -- counts and sums without P,
 * positions relative to the recording (irdm_scrub_stats first / last; a spectrum row's first_frame and timestamp_ns).
 * irdm_sample_count, chunk marks and irdm_chunks_complete count the priming feeds like any other feed.
 * Valid only on a fresh stream -- after irdm_create or irdm_reset, before the first feed, import or seed -- and not for a
 * member of a group; feed_block must divide H (the default does).  Otherwise -1 and nothing changed.  -1 from a failed feed
 * leaves the stream where it stopped: irdm_reset starts over.  irdm_reset ends the priming with the stream;
 * irdm_export_state / irdm_import_state work as on any stream at a position >= H.
 * _device: the same from a device buffer (stream: its producer, as in irdm_feed_device); the buffer may be reused when the
 * call returns.  Unlike irdm_feed_device it goes the way of irdm_feed_host's chunks, swap_iq / scrub / irdm_iq_balance
 * included: the prefix is assembled in the context's own buffers, the caller's is only read. */
int irdm_prime_host(irdm_pipeline_t *p, const void *h_iq, size_t n_samples);
int irdm_prime_device(irdm_pipeline_t *p, const void *d_iq, size_t n_samples, void *stream);
uint64_t irdm_primed_samples(const irdm_pipeline_t *p);  /* H, or 0 when the stream is not primed */
int irdm_primed_frames(const irdm_pipeline_t *p);        /* F, or 0 */
/* Pinned (page-locked) host memory for feed buffers, for hosts without HIP headers.  NULL on failure. */
void *irdm_host_alloc(size_t bytes);
void irdm_host_free(void *ptr);

/*
 * Device buffers for hosts without HIP headers (the C99 binary, tests): an IQ chunk that lives in HBM before it is
 * fed with irdm_feed_device (the case the headline metric is quoted on).  irdm_device_upload is synchronous.
 */
void *irdm_device_alloc(int device, size_t bytes);
void irdm_device_free(void *dptr);
int irdm_device_upload(void *dptr, const void *host, size_t bytes);
/* synchronous copy back to host memory (tests, tools) */
int irdm_device_download(void *host, const void *dptr, size_t bytes);
/* synchronous device-to-device copy on the current device (e.g. a resident chunk into its irdm_ingest_ptr slot) */
int irdm_device_copy(void *dst, const void *src, size_t bytes);

/* Results of all chunks fed so far, in burst-emission order; each call drains up to max
 * entries.  bursts: one per emitted burst (burst_callback_t payload minus samples).
 * frames: one per emitted burst (drop_reason says whether a frame was produced).
 * demods: one per frame that passed the unique-word check (frame_output_print input). */
int irdm_poll_bursts(irdm_pipeline_t *p, irdm_burst_t *out, int max);
int irdm_poll_frames(irdm_pipeline_t *p, irdm_frame_info_t *out, float *samples_out /* max*2*4440 or NULL */, int max);
int irdm_poll_demods(irdm_pipeline_t *p, irdm_demod_t *out, int max);
int irdm_poll_demods_packed(irdm_pipeline_t *p, irdm_demod_packed_t *out, int max);   /* option "packed_records" 1 */
/* option "parsed_records" 1: exactly one record per irdm_poll_demods_packed record, in the same order */
int irdm_poll_ida_packed(irdm_pipeline_t *p, irdm_ida_packed_t *out, int max);
/* option "frame_records" 1: exactly one record per irdm_poll_demods_packed record, in the same order */
int irdm_poll_frame_packed(irdm_pipeline_t *p, irdm_frame_packed_t *out, int max);

/* "tagged N bursts total" (burst_detect.c:350-351) and stat_sample_count (main.c:199) */
uint64_t irdm_tagged_bursts(const irdm_pipeline_t *p);
uint64_t irdm_sample_count(const irdm_pipeline_t *p);
size_t irdm_max_chunk_samples(const irdm_pipeline_t *p);      /* the configured value with its default resolved */
size_t irdm_bytes_per_sample(const irdm_pipeline_t *p);       /* of the configured input format */
size_t irdm_format_bytes(int format);                         /* bytes per sample of an IRDM_FMT_*; 0: no such format */
/* samples in front of a stream position that a context taking over there must be given (irdm_seed_history*): the
 * reference's ring (stale-slot reads reach one ring length back, burst_detect.c:292-296, :401-422) + the longest burst window */
size_t irdm_required_overlap(const irdm_pipeline_t *p);
/* host wait until K1 and the history-ring copy of every chunk handed over so far have read their input buffers */
int irdm_wait_ingest(irdm_pipeline_t *p);
int irdm_fft_size(const irdm_pipeline_t *p);
int irdm_set_stream_origin(irdm_pipeline_t *p, double center_frequency, uint64_t start_time_ns);  /* for the stage-level calls */
uint64_t irdm_start_time_ns(const irdm_pipeline_t *p);   /* burst_data_t.start_time_ns (burst_detect.c:849-853) */

/* Stage probes (parity tests): magnitudes of the last chunk (frames x fft_size floats,
 * device -> host copy), current baseline sum. */
/* What the reference's stats thread asks the detector (main.c:455-456): burst_detector_active_count / _noise_floor /
 * _peak_signal (burst_detect.c:355-395).  Settles the scan in flight and reads the detector state back (a few tens of
 * KB): call it from the feeding thread, at most once per feed.  peak_signal_db covers the bursts finished or still
 * active; bursts a squelch dumped (burst_detect.c:594-631) were seen by the reference's running maximum only. */
typedef struct {
    int32_t active_bursts;
    int32_t primed;
    float noise_floor_dbfs_hz;
    float peak_signal_db;
} irdm_detector_stats_t;
int irdm_detector_stats(irdm_pipeline_t *p, irdm_detector_stats_t *out);

int irdm_last_magnitudes(irdm_pipeline_t *p, float *out, size_t max_frames);
/* Band survey (option "spectrum_frames" = R, 1 <= R <= 2^20; 0 = off, the default): the windowed, fft-shifted |X|^2 plane the
 * detector's FFT kernel writes for every frame of every chunk, reduced on the device to a waterfall.  Row r covers the R
 * consecutive frames r R .. r R + R - 1 of the stream, whatever chunks they came in; per bin (bin 0 is -fs/2, values are
 * linear |X|^2, as in the plane)
 *   mean = (sum of the row's frames) / n_frames, in fp32        peak = the largest of them.
 * Summation order: the row's frames are taken in groups of min(R, 64), counted from the row's first frame; a group's frames
 * are added one after the other in frame order, starting from 0, and the groups' sums one after the other in group order,
 * starting from 0 (a last group of fewer frames likewise); then the one division.  The order depends on a frame's place in
 * its row alone: a stream yields the same bytes however it is cut into chunks, at every pipeline_depth.  For R = 1 mean and
 * peak are the plane itself.
 * irdm_feed_begin enqueues the reduction behind the chunk's FFT kernel; the trailing samples of a ragged last chunk that do
 * not fill a frame belong to no row.  irdm_flush closes the open row -- n_frames < R, the mean over those frames -- and
 * waits for every row; should the stream go on after that, the next row starts at the next frame.
 * irdm_poll_spectrum returns up to max finished rows in stream order -- rows whose kernels and copies have completed, after
 * irdm_flush all of them --: hdr[i], mean[i * n_bins ..], peak[i * n_bins ..] (max * n_bins floats each).  Unpolled rows
 * queue on the host without bound, like the records.  irdm_reset drops them and starts at row 0 again; it allocates
 * nothing.  The open row's sums live on the device and are NOT part of irdm_export_state: a context that takes a stream
 * over from another starts a row of its own.  Returns rows written, or -1. */
int irdm_spectrum_bins(const irdm_pipeline_t *p);      /* bins per row = irdm_fft_size */
int irdm_poll_spectrum(irdm_pipeline_t *p, irdm_spectrum_row_t *hdr, float *mean, float *peak, int max);
int irdm_baseline_sum(irdm_pipeline_t *p, float *out);
/* burst_data_t.samples of the i-th burst emitted by the LAST chunk (re-gathered) */
int irdm_burst_samples(irdm_pipeline_t *p, int burst_in_chunk, float *out, size_t max_samples);

/* Stage B alone for one burst: burst_downmix_process() (burst_downmix.h:70).  `info` carries the
 * burst_info_t fields (id, start, center_bin, magnitude, noise are used), `samples` the burst_data_t IQ
 * (host, num_samples complex floats), used verbatim whatever info->start: the window need not lie where the detector's
 * feed blocks would have delivered it.  Fills *frame (drop_reason 0 = frame produced, 1..5 = the reference's
 * early returns) and, when a frame was produced, frame_samples (2 * IRDM_MAX_FRAME_SAMPLES floats).
 * cf32 contexts only.  Returns 1 (frame), 0 (dropped) or -1 (error). */
int irdm_downmix_burst(irdm_pipeline_t *p, const irdm_burst_t *info, const float *samples, size_t num_samples,
                       irdm_frame_info_t *frame, float *frame_samples);

/* Stage C alone, batched: qpsk_demod() (qpsk_demod.h:42) for n downmixed frames.
 * samples: n rows of 2*IRDM_MAX_FRAME_SAMPLES floats (re,im interleaved, row-padded);
 * num_samples[i] <= IRDM_MAX_FRAME_SAMPLES; direction[i] = the downmixer's ir_direction_t.
 * out[i].ok = the reference's return value (1 = unique word accepted); metadata fields other
 * than direction, confidence, level, the symbol counts, bits, llr and total_phase are left zero.  Returns 0 or -1. */
int irdm_qpsk_demod_batch(irdm_pipeline_t *p, const float *samples, const int *num_samples,
                          const int *direction, int n, irdm_demod_t *out);
/* The same frames on the packed record path (options "packed_records" / "parsed_records"): the kernel writes the compact
 * records straight into the context's pinned memory, and these are what the call returns in packed_out[i] -- ok, and for an
 * accepted frame direction, confidence, level, the symbol counts and total_phase; bits[] as the kernel left it for every
 * frame, accepted or not; the other fields zero.  keep_bits = 1 (as "parsed_records" runs it): the kernel also writes the
 * full records' bits and LLRs, returned in full_out[i] as irdm_qpsk_demod_batch returns them.  keep_bits = 0: full_out must
 * be NULL.  Returns 0 or -1. */
int irdm_qpsk_demod_packed_batch(irdm_pipeline_t *p, const float *samples, const int *num_samples,
                                 const int *direction, int n, int keep_bits, irdm_demod_packed_t *packed_out,
                                 irdm_demod_t *full_out);

/* Post-demod bit layer alone, batched: frame_decode() (frame_decode.h:63) for n demodulated frames -- access code,
 * de-interleave, BCH(31,21)/(7,3) syndromes, Chase decoding on the LLRs (use_llr = 0: hard decisions only, as
 * frame->llr == NULL), IRA / IBC fields.  in[i].bits / llr / n_bits / id / timestamp / center_frequency are read.
 * out[i].type is 0 when frame_decode() returns 0.  Returns 0 or -1.
 * With the option "decode_frames" = 1 the pipeline runs the same kernel behind the demodulator and
 * irdm_poll_decoded returns one record per irdm_poll_demods record, in the same order. */
int irdm_frame_decode_batch(irdm_pipeline_t *p, const irdm_demod_t *in, int n, int use_llr, irdm_decoded_t *out);
int irdm_poll_decoded(irdm_pipeline_t *p, irdm_decoded_t *out, int max);
/* ida_decode() (ida_decode.h) the same way: LCW extraction, payload descramble, BCH(31,20) + Chase, CRC-CCITT.
 * in[i].direction is the demodulator's direction.  Option "decode_ida" = 1 runs it in the pipeline;
 * irdm_poll_ida returns one record per irdm_poll_demods record (ok = 0 when ida_decode() returns 0).
 * Multi-burst reassembly (ida_reassemble) stays on the host and consumes these records. */
int irdm_ida_decode_batch(irdm_pipeline_t *p, const irdm_demod_t *in, int n, int use_llr, irdm_ida_t *out);
/* The packed record path's kernels alone, batched: frame_decode() / ida_decode() of n frames into the records options
 * "frame_records" / "parsed_records" poll, written by the kernels into pinned host memory.  As behind the demodulator they
 * always use the LLRs and read in[i].direction; in[i].n_bits must be even (the kernels take 2 * n_symbols bits).
 * Returns 0, or -1 (an odd or out-of-range n_bits among them included). */
int irdm_frame_packed_batch(irdm_pipeline_t *p, const irdm_demod_t *in, int n, irdm_frame_packed_t *out);
int irdm_ida_packed_batch(irdm_pipeline_t *p, const irdm_demod_t *in, int n, irdm_ida_packed_t *out);
int irdm_poll_ida(irdm_pipeline_t *p, irdm_ida_t *out, int max);

/* ---- time-chunk sharding of ONE stream across GPUs ----
 * The detector is sequential across frames (noise-floor ring, active bursts, ids); exact
 * sharding hands its state from the rank that scanned chunk k to the rank that scans chunk k+1.
 * irdm_state_bytes: size of the blob (DetState + baseline sum + 512-frame history).
 * irdm_export_state / irdm_import_state: blob to / from a HOST buffer (the caller moves it
 * between ranks, e.g. RCCL send/recv of the same bytes).  Returns bytes written / 0, or -1.
 * irdm_seed_history: tells a fresh context that its stream position is abs_start and gives it
 * the n_samples of IQ (host buffer, configured format) that precede that position, so burst
 * windows reaching back across the chunk boundary read real samples (the chunk overlap).
 * STREAM POSITIONS STAY BELOW IRDM_MAX_POSITION = 2^53 samples.  Every index is 64-bit, but a frame's timestamp is made of
 * (double)start / sample_rate, as in the reference, and from 2^53 on (double)start is no longer the sample it names.
 * The entries that SET a position -- irdm_seed_history*, irdm_import_state* -- return -1, with one line on stderr, for a
 * position at or above it and leave the context as it was.  irdm_import_state checks the blob's sample count, the
 * detector's frame index and every active burst; the device forms check the header's sample count only (the detector
 * state stays on the device).  A stream that is FED across 2^53 is not checked: that is 12 years at 22.6 MHz. */
#define IRDM_MAX_POSITION (1ull << 53)
size_t irdm_state_bytes(const irdm_pipeline_t *p);
long long irdm_export_state(irdm_pipeline_t *p, void *buf, size_t cap);
int irdm_import_state(irdm_pipeline_t *p, const void *buf, size_t n);
int irdm_seed_history(irdm_pipeline_t *p, const void *h_iq, size_t n_samples, uint64_t abs_start);
/* the same three with DEVICE buffers (a blob RCCL moves GPU to GPU; a chunk overlap received from the previous rank):
 * no host bounce, and only the detector is waited for -- K1 of the next chunk and per-burst work in flight go on */
long long irdm_export_state_device(irdm_pipeline_t *p, void *d_buf, size_t cap);
int irdm_import_state_device(irdm_pipeline_t *p, const void *d_buf, size_t n);
/* The same hand-off in two parts, so that the history (512 x N floats: 16-32 MiB) can FOLLOW the part a scan needs first:
 * head = the first irdm_state_head_bytes() bytes of the blob (header, detector state, baseline sums), history = the rest.
 * Round 0 of the band scan reads no history; a rank imports the head, asks irdm_expect_history(p, buf) -- 1: the scan
 * that the next irdm_feed_end enqueues waits ON THE DEVICE (a one-lane kernel polling a word the host writes) until
 * irdm_import_state_history_device(p, buf, n) says the history has arrived in buf, copies it in and goes on; the caller
 * must make that call before it settles the scan (irdm_export_state_device, irdm_flush, the next irdm_feed_end); 0: this
 * scan cannot wait (pipeline_depth 0, an unprimed detector, a sequential scan mode): import the history first -- calls
 * irdm_feed_end, receives the history while K1 and round 0 run, and imports it.  0 ok, -1 error. */
size_t irdm_state_head_bytes(const irdm_pipeline_t *p);
int irdm_import_state_head_device(irdm_pipeline_t *p, const void *d_buf, size_t n);
int irdm_expect_history(irdm_pipeline_t *p, const void *d_hist_buf);   /* d_hist_buf: where the history will arrive (device memory) */
int irdm_import_state_history_device(irdm_pipeline_t *p, const void *d_hist_buf, size_t n);
int irdm_seed_history_device(irdm_pipeline_t *p, const void *d_iq, size_t n_samples, uint64_t abs_start);

/* ---- a group: ONE stream across several GPUs of ONE process (replaces main.c:667-694's thread layout
 * for N > 1) ----
 * irdm_group_create builds one context per device (cfg->device is ignored; devices == NULL: 0 .. n_gpus-1; pipeline_depth
 * at least 1), two RCCL communicator sets over them (ncclCommInitAll: one for IQ samples, one for the detector state, so
 * that a 16-32 MiB state hop never queues behind a 0.5 GB slice) and per member two landing buffers of
 * [overlap | cfg->max_chunk_samples] samples.  The stream is cut into chunks of max_chunk_samples; chunk k goes to member
 * k mod N.  librccl is loaded when the first group is created (dlopen: a process that never makes a group never loads it;
 * IRDM_RCCL_LIB names another file); a group of one member needs no RCCL at all unless "group_loopback" is set.
 *
 * irdm_group_stage_host / _device: the samples of the next feed start moving -- from host memory (pinned for speed: each
 *   member's slice over its own PCIe link) or from device memory of member 0 (an RCCL scatter: grouped ncclSend / ncclRecv
 *   from member 0 to every other member) -- into the landing buffers the current feed does not use, together with each
 *   chunk's overlap (the samples in front of it that burst windows and the reference's stale ring reads reach back to:
 *   the tail of the previous member's landing buffer, GPU to GPU).  Returns at once; n_samples <= n_gpus *
 *   max_chunk_samples, chunks of max_chunk_samples except the last of the stream.  Calling it before the previous
 *   irdm_group_feed puts the scatter under that feed's compute (two super-steps may be staged at most: the one being fed
 *   and the one behind it).  The buffer must be complete when the call is made and stay unchanged until the
 *   irdm_group_feed_* that consumes it has returned.
 * irdm_group_feed_host / _device: stages (unless exactly this buffer was staged) and runs the super-step: K1 of every
 *   chunk at once, then the detector's chain member by member -- ncclRecv of the previous member's state head, import, scan
 *   (round 0 while the 512-frame history is still arriving), export, ncclSend to the next member -- and every chunk's
 *   per-burst chain enqueued behind its scan (irdm_advance): the chains overlap the other members' scans and the next
 *   super-step.  Returns the number of chunks fed, -1 on error.
 * irdm_group_flush: everything in flight completes.
 * irdm_group_poll_*: the members' records merged in STREAM order (chunk by chunk, as one context would have queued them);
 *   a chunk's records come out once every earlier chunk is complete.
 * irdm_group_set_option: an option of every member ("group_loopback" 1: a group of one member runs the whole protocol --
 *   overlap seed, state export, ncclSend / ncclRecv to itself, import -- for tests on one GPU).
 * irdm_group_get_stat: "hops", "hop_bytes", "scatter_bytes", "overlap_bytes", "overlap_samples", "chunks", "late_history"
 *   (scans that took their history behind round 0), "tagged" (the stream's burst count: it travels with the detector
 *   state), any other key: the sum of irdm_get_stat over the members.
 * One thread drives a group.  Feeding or polling a member directly (irdm_group_member) is not allowed; options, statistics
 * and kernel clocks of a member are. */
typedef struct irdm_group irdm_group_t;
int irdm_device_count(void);                           /* GPUs this process sees (0: none, or no HIP runtime) */
/* EXPERIMENTAL for n_gpus > 1 (a warning says so once): run on emulated devices and as ranks sharing one GPU only.
 * While the RCCL communicators are made (in irdm_group_create for n_gpus > 1, and when "group_loopback" is first set on a
 * group of one) the process's file descriptor 1 is pointed at its stderr and restored afterwards: librccl prints a version
 * banner on stdout, the stream a host prints its RAW lines to.  A host with other threads writing to stdout in that window
 * sees their output on stderr; IRDM_GROUP_KEEP_STDOUT=1 in the environment leaves the descriptor alone (banner included). */
irdm_group_t *irdm_group_create(const irdm_config_t *cfg, int n_gpus, const int *devices);
void irdm_group_destroy(irdm_group_t *g);
int irdm_group_size(const irdm_group_t *g);
irdm_pipeline_t *irdm_group_member(irdm_group_t *g, int i);
int irdm_group_set_option(irdm_group_t *g, const char *key, int value);
int64_t irdm_group_get_stat(const irdm_group_t *g, const char *key);
int irdm_group_stage_host(irdm_group_t *g, const void *h_iq, size_t n_samples);
int irdm_group_stage_device(irdm_group_t *g, const void *d_iq, size_t n_samples);
int irdm_group_feed_host(irdm_group_t *g, const void *h_iq, size_t n_samples);
int irdm_group_feed_device(irdm_group_t *g, const void *d_iq, size_t n_samples);
int irdm_group_flush(irdm_group_t *g);
int irdm_group_poll_bursts(irdm_group_t *g, irdm_burst_t *out, int max);
int irdm_group_poll_frames(irdm_group_t *g, irdm_frame_info_t *out, float *samples_out /* max*2*4440 or NULL */, int max);
int irdm_group_poll_demods(irdm_group_t *g, irdm_demod_t *out, int max);
int irdm_group_poll_demods_packed(irdm_group_t *g, irdm_demod_packed_t *out, int max);
int irdm_group_poll_decoded(irdm_group_t *g, irdm_decoded_t *out, int max);
int irdm_group_poll_ida(irdm_group_t *g, irdm_ida_t *out, int max);
int irdm_group_poll_ida_packed(irdm_group_t *g, irdm_ida_packed_t *out, int max);   /* option "parsed_records" 1 */
int irdm_group_poll_frame_packed(irdm_group_t *g, irdm_frame_packed_t *out, int max);   /* option "frame_records" 1 */
/* what the group rests on in a single context: the marks (option "chunk_marks") and the number of chunks whose records
 * are all in the queues */
int irdm_poll_chunk_marks(irdm_pipeline_t *p, irdm_chunk_mark_t *out, int max);
uint64_t irdm_chunks_complete(const irdm_pipeline_t *p);

/* Options (irdm_set_option; every one a field of THIS context -- two contexts of a process may differ in all of them; set them
 * before the first feed unless noted; irdm_reset keeps them all).  Twenty-four keys:
 *
 *   what a caller chooses
 *   "keep_frame_samples"  0/1, default 0: irdm_poll_frames returns metadata only
 *   "packed_records"      0/1, default 0: 1 = only burst records and compact frame records (irdm_poll_demods_packed: what
 *                         frame_output_print reads, hard bits 8 per byte, no LLRs), written to pinned memory by the chain's
 *                         last kernel
 *   "parsed_records"      0/1, default 0: 1 = "packed_records", and ida_decode() (LCW, BCH(31,20) with Chase on the LLRs,
 *                         CRC) of every frame on the device, behind the demodulator, on its bits and LLRs where it leaves
 *                         them: irdm_poll_ida_packed returns one irdm_ida_packed_t per compact frame record, written to
 *                         pinned memory by that kernel.  With "decode_frames", "decode_ida" or "keep_frame_samples" the
 *                         chain is on the full-record path and neither kind of compact record is queued.
 *   "frame_records"       0/1, default 0: 1 = "packed_records", and frame_decode() (access code, IBC / IRA blocks, BCH(31,21)
 *                         with Chase on the LLRs) of every frame on the device, behind the demodulator, on its bits and
 *                         LLRs where it leaves them: irdm_poll_frame_packed returns one irdm_frame_packed_t per compact
 *                         frame record, written to pinned memory by that kernel.  May be combined with "parsed_records"
 *                         (both kernels run on the same frames).  "decode_frames", "decode_ida" and "keep_frame_samples"
 *                         win as for "parsed_records".
 *   "chunk_marks"         0/1, default 0: see irdm_chunk_mark_t (what a group merges its members' records with)
 *   "spectrum_frames"     R, default 0 = off; 1 .. 2^20: mean and peak-hold spectra over rows of R frames, see irdm_poll_spectrum.
 *                         The workspace (two planes per min(R, 64) frames of max_chunk_samples), the rows of one
 *                         chunk and three pinned buffers of that size are allocated when the option is first set to a non-zero
 *                         value, never before.  -1 for a value out of range, for a member of a group (and so through
 *                         irdm_group_set_option), and between a stream's first irdm_feed_begin and irdm_reset
 *   "input_stats"         0/1, default 0: one reduction pass over the raw samples of every chunk fed from then on, see
 *                         irdm_input_stats.  A side stream, four small device blocks and their pinned copies are allocated
 *                         when the option is first set to 1, never before.  -1 for a member of a group (and so through
 *                         irdm_group_set_option) and while a chunk handed over with irdm_feed_begin waits for its
 *                         irdm_feed_end
 *   "symbol_clock"        0/1, default 0: 1 = one more kernel in the per-burst chain of every chunk fed from then on, behind
 *                         the downmixer and beside the demodulator: the symbol clock error of every frame, see
 *                         irdm_poll_symbol_clock / irdm_symbol_clock.  It reads the frames only: no other record changes.
 *                         One pinned buffer of 16 bytes per burst and batch context is allocated when the option is first
 *                         set to 1, never before; with 0 nothing is launched.  -1 for a member of a group (and so through
 *                         irdm_group_set_option) and while a chunk handed over with irdm_feed_begin waits for its
 *                         irdm_feed_end
 *   "fine_freq"           0/1, default 0: 1 = one more kernel in the per-burst chain of every chunk fed from then on, behind
 *                         the downmixer and beside the demodulator: the carrier frequency of every frame from its own
 *                         samples, see irdm_poll_fine_freq / irdm_fine_freq.  center_frequency of every demodulator record
 *                         (irdm_demod_t, irdm_demod_packed_t, and the irdm_decoded_t / irdm_ida_t derived from them) whose
 *                         estimate is neither invalid nor out of range is then the refined frequency; a flagged frame keeps
 *                         the PLL's value bit for bit, and no other field of any record changes (irdm_frame_info_t keeps the
 *                         downmixer's frequency).  One pinned buffer of 16 bytes per burst and batch context is allocated
 *                         when the option is first set to 1, never before; with 0 nothing is launched (stat
 *                         "fine_freq_launches").  -1 for a member of a group (and so through irdm_group_set_option) and
 *                         while a chunk handed over with irdm_feed_begin waits for its irdm_feed_end
 *   "fine_time"           0/1, default 0: 1 = one more kernel in the per-burst chain of every chunk fed from then on, behind
 *                         the downmixer and beside the demodulator: the symbol timing of every frame from its own samples,
 *                         see irdm_poll_fine_time / irdm_fine_time.  timestamp of every demodulator record (irdm_demod_t,
 *                         irdm_demod_packed_t, and the irdm_decoded_t / irdm_ida_t derived from them) is then the time of
 *                         the frame's sample 0, from the line where the estimate is neither invalid nor ambiguous and from
 *                         the correlator otherwise; no other field of any record changes (irdm_frame_info_t keeps the
 *                         downmixer's timestamp).  One pinned buffer of 32 bytes per burst and batch context is allocated
 *                         when the option is first set to 1, never before; with 0 nothing is launched (stat
 *                         "fine_time_launches").  -1 for a member of a group (and so through irdm_group_set_option) and
 *                         while a chunk handed over with irdm_feed_begin waits for its irdm_feed_end
 *   "iq_sense"            0/1, default 0: 1 = one more kernel in the per-burst chain of every chunk fed from then on, behind
 *                         the demodulator: whether each frame's bits make sense as they are or with I and Q exchanged, see
 *                         irdm_poll_iq_votes / irdm_iq_sense.  It reads the demodulator's bits and LLRs only: no other
 *                         record changes (on the packed record path the demodulator then leaves them on the device, as
 *                         for parsed_records).  One pinned buffer of 8 bytes per burst and batch context is allocated
 *                         when the option is first set to 1, never before; with 0 nothing is launched.  -1 for a member
 *                         of a group and while a chunk handed over with irdm_feed_begin waits for its irdm_feed_end
 *   "burst_resample"      0/1, default 0: 1 = at a sample rate that is no multiple of 250 kHz, one more stage in the per-burst
 *                         chain of every chunk fed from then on, between the decimator and the 25-tap low-pass: every
 *                         burst's decimated row (at sample_rate / decim, decim = round(sample_rate / 250000)) is resampled to
 *                         exactly 250 000 samples/s by a rational polyphase filter at L / M = decim 250000 / sample_rate
 *                         in lowest terms, see irdm_burst_resample_ratio.  The default, 0, is the reference's arithmetic:
 *                         the row is taken for 250 kHz whatever its rate, and frames at a rate off the grid lose their tail.
 *                         The table (L x 20 floats) and one more row scratch per batch context are allocated when the option
 *                         is first set to 1 at such a rate, never before; at a rate on the grid, and with 0, nothing is
 *                         allocated and nothing launched, and every record is the one of the option off.  -1 where L
 *                         exceeds 4096 (a line on stderr names it), while a chunk handed over with irdm_feed_begin waits
 *                         for its irdm_feed_end, and while a batch of bursts is in flight (irdm_flush first).  A member of a group takes it (irdm_group_set_option sets every member's)
 *   "swap_iq"             0/1, default 0: 1 = irdm_feed_host exchanges the two components of every sample of every chunk
 *                         on the device (irdm_swap_iq_device's kernel on the feed's stream, between the host-to-device
 *                         copy and the feed; the ring slot of irdm_ingest_ptr and the staging buffer alike), so the
 *                         detector, the history ring, the per-burst chains, input_stats and spectrum_frames all see the
 *                         exchanged stream.  The device feeds take const buffers the caller owns: with the option on
 *                         irdm_feed_device / irdm_feed_begin return -1 with a line on stderr -- exchange the buffer with
 *                         irdm_swap_iq_device first.  -1 for a member of a group, and for a change of the value between
 *                         a stream's first feed and irdm_reset (the ring would hold both senses)
 *   "scrub"               0/1, default 0: 1 = irdm_feed_host zeroes every cf32 sample of every chunk that has a non-finite
 *                         component or one beyond +-2^scrub_limit_log2 (irdm_scrub_device's kernel on the feed's stream,
 *                         behind the host-to-device copy and behind swap_iq's exchange, in front of the feed; the ring slot
 *                         of irdm_ingest_ptr and the staging buffer alike), so the detector, the history ring, the
 *                         per-burst chains, input_stats and spectrum_frames never see such a sample; irdm_scrub_stats says
 *                         what was zeroed and where.  One such sample otherwise puts a NaN or an Inf into the detector's
 *                         baseline sums, which never recover: no burst is found behind it.  A context of another format
 *                         takes the option and launches nothing (its samples are always finite).  Four 8 KiB blocks on
 *                         the device and in pinned memory are allocated when the option is first set to 1 on a cf32
 *                         context, never before; with 0 nothing is launched.  With the option on irdm_feed_device /
 *                         irdm_feed_begin return -1 with a line on stderr (the caller's buffer is not ours to change) --
 *                         scrub the buffer with irdm_scrub_device first.  -1 for a member of a group, and for a change of
 *                         the value between a stream's first feed and irdm_reset
 *   "scrub_limit_log2"    0 .. 127, default 40: the limit's base-2 logarithm.  The limit keeps every square, and the sums
 *                         the detector makes of them, finite (2^14 samples of 2^40 in one FFT frame square to 2^108); it
 *                         does not judge what a glitch is -- un-normalised int16-, int24- and int32-scaled floats pass.  A
 *                         caller who wants finite glitches gone picks a lower limit.  -1 outside 0 .. 127, for a member of
 *                         a group, and for a change between a stream's first feed and irdm_reset
 *   "dc_block"            0/1, default 0: 1 = irdm_dc_block(p, IRDM_FMT_CF32, dc_block_log2, 0, 0) -- irdm_feed_host tracks the DC
 *                         offset of every chunk over aligned blocks and subtracts the mean of the block in front; 0 =
 *                         off.  See irdm_dc_block for the rule, the order among the passes and the refusals
 *   "dc_block_log2"       12 .. 24, default 20: the block length's base-2 logarithm "dc_block" switches on with.  -1 outside
 *                         12 .. 24, for a member of a group, while the pass is on and after a stream's first feed
 *   "iq_moments"          0/1, default 0: 1 = every chunk's samples are reduced on the GPU to the sums of irdm_iq_moments_t
 *                         (one pass on a side stream behind the chunk's arrival, beside K1, where "input_stats" runs its
 *                         own; device feeds included); irdm_iq_moments returns them with the imbalance derived from them.
 *                         It measures the stream as processed: behind swap_iq, irdm_iq_balance and scrub.  A side stream,
 *                         four 128 KiB blocks on the device and in pinned memory are allocated when the option is first
 *                         set, never before; with 0 nothing is launched.  irdm_reset starts the sums over.  -1 for a
 *                         member of a group and while a chunk handed over with irdm_feed_begin waits for its irdm_feed_end
 *   "decode_frames" / "decode_ida"  0/1, default 0: the post-demod bit layer, see irdm_poll_decoded / irdm_poll_ida
 *   "detect_only"         0/1, default 0: 1 = stage A alone (burst_detector_feed's role): burst records only
 *   "fir_order" (alias "simd_order")   default 1 = the arithmetic of the reference's AVX2 kernels, simd_avx2.c -- what
 *                         simd_init() (simd_generic.c:33-57) selects on x86: fir_ccf_dec :62-108, fir_ccf :28-55, fir_fff
 *                         :115-138, fftshift_mag :177-221, mag_squared :304-323; 0 = simd_generic.c, what --no-simd and every
 *                         non-x86 build run.  (The other six dispatched kernels are the same operations in both files.)
 *   "host_cfo"            0/1, default 0: 1 = the fine-CFO libm step (cexpf) on a host helper thread instead of the device's
 *                         restatement of glibc's sincosf (forced when irdm_create finds that restatement differs from THIS
 *                         host's libm)
 *   "scan_mode"           0 = band-parallel speculative scan where the FFT size supports it, the sequential scans as its
 *                         exact fallback (default); 1 = dense sequential scan only; 2 / 3 = the sparse leader scan on one CU /
 *                         with updater workgroups, dense fallback; 4 = band scan with the dense scan as its only fallback
 *   "rot_prebuild"        0/1, default 1 where pipeline_depth >= 1: every centre bin's rotator-checkpoint row, as far as a burst
 *                         of ordinary length needs it, built by one background launch behind create (n bins x runs x 16 KB:
 *                         0.07 / 1.3 / 3.2 GB at 2 / 10 / 12 MHz) instead of by the chains that first meet the bin; only
 *                         before the first burst
 *   "kernel_clock"        0/1, default 0: see irdm_kernel_clock
 *   "group_member"        0/1, default 0: set by irdm_group_create on its members; irdm_reset refuses such a context
 *
 *   diagnostic
 *   "band_timeline"       0/1: the band scan's passes stamp a device timeline (stats "tl_dur_i" / "tl_gap_i" / "tl_n_i")
 *
 *   test hooks (paths a default run at the standard rates takes rarely or never)
 *   "fir_generic"         1 = the any-M decimator (what 2 / 4 MHz streams take) at every rate
 *   "post_generic"        1 = the runtime-tap-count instances of the per-burst filters
 *   "k1_lists"            default 1: the FFT kernel writes the band scan's candidate lists; 0 = a prefilter pass does (what a
 *                         stale-list retry and an unprimed detector take)
 *   "band_first"          default 0 = as many band-scan rounds up front as the previous chunk needed; n = always n
 *   "band_spec"           default 1: round 0 of a chained scan is a speculation pass beside the previous scan; 0 = classical
 *   "band_selfcheck"      bit mask, see BandParams::selfcheck (csrc/band_core.hpp): both boundary tests compared, records
 *                         spoilt, the walk without look-ahead, the plan pass without its LDS, the guess spoilt in one frame
 *   "rot_pool_rows"       n = an empty on-demand checkpoint arena of n whole rows (a prebuilt one is given up)
 *   "scratch_outputs"     n = the decimated / low-passed scratch of every batch context with room for n outputs to begin with
 *
 * Stats (irdm_get_stat): "scan_fast_chunks", "scan_fallbacks", "scan_dense_frames", "band_chunks", "band_rounds",
 * "band_retries", "band_aborts", "band_extra", "band_last_flags", "k1_lists", "resets", "scan_chained", "scan_chain_undone", "spec_passes",
 * "spec_scans", "sum_restarts", "host_us_0".."host_us_9", "rot_rows", "rot_prebuilt_runs",
 * "rot_rows_cap", "rot_blocks", "rot_blocks_cap", "rot_builds", "rot_runs", "rot_ckpts", "rot_grows" (rotator checkpoints:
 * centre bins with a row / runs per bin prebuilt / the arena in whole rows / blocks of 2048 checkpoints in use / allocated /
 * build launches on chains / runs built / checkpoints built / times the arena doubled), "band_steps" (update steps the scans'
 * last rounds walked), "burst_resample_launches" (launches of burst_resample_kernel by the chains), "fine_freq_launches" (of fine_freq_kernel), "fine_time_launches" (of fine_time_kernel),"scratch_outputs", "scratch_grows", "scratch_peak" (decimated samples a batch context holds / times it
 * doubled / most a batch needed). */
int irdm_set_option(irdm_pipeline_t *p, const char *key, int value);
int64_t irdm_get_stat(const irdm_pipeline_t *p, const char *key);

/* per-stage device time of the last chunk in milliseconds (hipEvent):
 * [0] fft+mag  [1] detector scan  [2] rotate+FIR decimate  [3] downmix post  [4] demod  [5] total */
int irdm_last_timings(const irdm_pipeline_t *p, float *ms_out, int n);
/* Option "kernel_clock" 1: the chip-filling kernels stamp the 100 MHz device clock when their first wavefront starts and
 * when their last one ends (s_memrealtime, per launch); this returns the spans summed over the launches since the last
 * reset -- the kernel's own duration on the device, free of the dispatch wait a host-side event bracket includes (what
 * bench.py's roofline divides the algorithmic bytes by).  which: 0 = the register-resident decimator
 * (fir_decimate_kernel_f / _r), 1 = K1 (fft_mag_p32_kernel / fft_mag_r16_kernel).  Waits for the device.  0 ok, -1 error. */
int irdm_kernel_clock(irdm_pipeline_t *p, int which, double *sum_ms, uint64_t *launches, double *last_ms, int reset);

/* ------------------------------------------------------------------ */
/* 3. RAW line (frame_output.c:160-199)                                 */
/* ------------------------------------------------------------------ */
/* t0_io: 0 on first call -> set as ensure_initialized does (frame_output.c:144-158).
 * file_info NULL/"" -> "i-<t0 s>-t1".  Returns the line length incl. '\n', or -1. */
int irdm_format_raw(const irdm_demod_t *f, const char *file_info, uint64_t *t0_io,
                    char *buf, size_t cap);
/* The same for n frames, lines concatenated in buf (NUL-terminated): one write per batch instead of the
 * reference's fflush per line (frame_output.c:196-198).  cap >= n * IRDM_RAW_LINE_MAX always suffices.
 * Returns the total length or -1. */
#define IRDM_RAW_LINE_MAX 1280          /* 256 B of prefix (file_info <= 128 chars) + IRDM_MAX_BITS + newline, rounded up */
long long irdm_format_raw_batch(const irdm_demod_t *f, int n, const char *file_info, uint64_t *t0_io,
                                char *buf, size_t cap);
/* the same lines from compact records (option "packed_records") */
int irdm_format_raw_packed(const irdm_demod_packed_t *f, const char *file_info, uint64_t *t0_io, char *buf, size_t cap);
long long irdm_format_raw_packed_batch(const irdm_demod_packed_t *f, int n, const char *file_info, uint64_t *t0_io,
                                       char *buf, size_t cap);

/* 3b. IDA line (frame_output.c:203-361, --parsed)                      */
/* ------------------------------------------------------------------ */
/* The irdm_ida_t the "decode_ida" path makes of the same frame (lcw_header included) from a compact pair. */
void irdm_ida_unpack(const irdm_ida_packed_t *ida, const irdm_demod_packed_t *f, irdm_ida_t *out);
/* frame_output_print_ida's line for a decoded burst (b->ok != 0): "IDA: p-<t0 s> ..." whatever the file info.  t0_io is
 * shared with irdm_format_raw*, as the reference's one ensure_initialized is.  bits past the 256 bch_stream keeps are not
 * printed (the reference reads past the array there).  Returns the line length incl. '\n', or -1. */
int irdm_format_ida(const irdm_ida_t *b, uint64_t *t0_io, char *buf, size_t cap);
/* --parsed: per frame the IDA line where idas[i].ok, the RAW line otherwise (main.c:322-331), concatenated.
 * cap >= n * IRDM_RAW_LINE_MAX always suffices.  Returns the total length or -1. */
long long irdm_format_parsed_packed_batch(const irdm_demod_packed_t *f, const irdm_ida_packed_t *idas, int n,
                                          const char *file_info, uint64_t *t0_io, char *buf, size_t cap);

/* The irdm_decoded_t the "decode_frames" path makes of the same frame from a compact pair: lat / lon / alt with the host
 * libm (parse_ira's expressions), id / timestamp / frequency from the frame record. */
void irdm_frame_unpack(const irdm_frame_packed_t *fr, const irdm_demod_packed_t *f, irdm_decoded_t *out);

/* 3c. IDA reassembly, SBD and ACARS (--acars, --acars-json)            */
/* ------------------------------------------------------------------ */
/* Host C, once per IDA burst and once per message: the reference's ida_reassemble / ida_reassemble_flush
 * (ida_decode.c:669-748), SBD extraction and multi-packet reassembly (sbd_acars.c:1002-1218) and its ACARS printer as it
 * builds without libacars (sbd_acars.c:603-998; no ARINC-622 decoding).  Contexts are opaque, one thread each. */

/* one reassembled IDA message: the arguments of ida_message_cb (ida_decode.h:76-79) */
typedef struct {
    uint8_t data[256];
    int32_t len;
    int32_t direction;         /* ir_direction_t: 1 DL, 2 UL */
    uint64_t timestamp;        /* the last burst's */
    double frequency;          /* the first burst's */
    float magnitude;           /* the last burst's */
    int32_t pad;
} irdm_ida_message_t;

typedef struct irdm_ida_reasm irdm_ida_reasm_t;
irdm_ida_reasm_t *irdm_ida_reasm_create(void);
void irdm_ida_reasm_destroy(irdm_ida_reasm_t *r);
/* Per record in stream order (main.c:357-361): ida_reassemble when b[i].ok, then ida_reassemble_flush at b[i].timestamp.
 * A frame ida_decode() did not take still flushes: give it ok = 0 and the frame's timestamp (irdm_poll_ida leaves that
 * 0).  Completed messages go to out in order, at most one per record: max >= n.  Returns their count, or -1. */
int irdm_ida_reasm_push(irdm_ida_reasm_t *r, const irdm_ida_t *b, int n, irdm_ida_message_t *out, int max);
/* the same from the packed record path's pairs (through irdm_ida_unpack); every frame flushes at its own timestamp */
int irdm_ida_reasm_push_packed(irdm_ida_reasm_t *r, const irdm_demod_packed_t *f, const irdm_ida_packed_t *idas, int n,
                               irdm_ida_message_t *out, int max);

typedef struct {
    int32_t json;              /* 1: --acars-json's lines (messages with errors dropped), 0: the text lines */
    int32_t fixed_origin;      /* 1: the wall clock of the first printed message is origin_sec + origin_nsec; 0: read
                                  CLOCK_REALTIME then (ts_ensure_init, sbd_acars.c:306-313) */
    int64_t origin_sec, origin_nsec;
    const char *station;       /* --station (copied), NULL for none */
} irdm_acars_config_t;

/* acars_print_stats's counters (sbd_acars.c:291-299) */
typedef struct {
    int32_t ida_total, sbd_total, sbd_short, sbd_single, sbd_multi_ok, sbd_multi_frag, sbd_broken;
    int32_t acars_total, acars_errors;
} irdm_acars_stats_t;

typedef struct irdm_acars irdm_acars_t;
irdm_acars_t *irdm_acars_create(const irdm_acars_config_t *cfg);
void irdm_acars_destroy(irdm_acars_t *a);
/* acars_ida_cb for n messages: the lines the reference prints, concatenated in buf (NUL-terminated; a line may hold NUL
 * bytes where the message does, so use the returned length).  At most one line per message of at most
 * IRDM_ACARS_LINE_MAX bytes.  Returns the length, or -1 when cap is too small (the messages are consumed all the same). */
#define IRDM_ACARS_LINE_MAX 8192
long long irdm_acars_feed(irdm_acars_t *a, const irdm_ida_message_t *m, int n, char *buf, size_t cap);
int irdm_acars_stats(const irdm_acars_t *a, irdm_acars_stats_t *out);
/* acars_print_stats's stderr text (sbd_acars.c:1336-1349).  Returns its length, or -1. */
int irdm_acars_format_stats(const irdm_acars_t *a, char *buf, size_t cap);
/* --acars on the packed record path: per frame (main.c:322-361) its IDA line when parsed and idas[i].ok, no RAW line
 * (frame_output_print returns under --acars before it sets t0, frame_output.c:162-168), then the ACARS lines of the
 * messages the frame completes.  State lives in r and a across calls.  cap >= n * (IRDM_RAW_LINE_MAX +
 * IRDM_ACARS_LINE_MAX) always suffices.  Returns the length, or -1. */
long long irdm_format_acars_packed_batch(irdm_ida_reasm_t *r, irdm_acars_t *a, const irdm_demod_packed_t *f,
                                         const irdm_ida_packed_t *idas, int n, int parsed, uint64_t *t0_io, char *buf,
                                         size_t cap);
/* the same from full records and the "decode_ida" path's irdm_ida_t (--save-bursts) */
long long irdm_format_acars_batch(irdm_ida_reasm_t *r, irdm_acars_t *a, const irdm_demod_t *f, const irdm_ida_t *idas,
                                  int n, int parsed, uint64_t *t0_io, char *buf, size_t cap);

/* 3d. Doppler positioning (--position)                                  */
/* ------------------------------------------------------------------ */
/* Host C: the reference's positioning engine (doppler_pos.c) -- per-satellite measurement buffers of decoded IRA frames,
 * channel-frequency and velocity estimation, the motion-based visibility cluster, iterated weighted least squares with
 * height aiding, outlier and per-satellite screening and the solution-jump guard -- with all of its state in one object
 * (one thread each).  Doubles are those of the reference's own build, operation for operation. */

/* doppler_solution_t (doppler_pos.h) */
typedef struct {
    double lat, lon;           /* degrees */
    double alt;                /* metres */
    double hdop;
    int32_t n_measurements, n_satellites, converged, pad;
} irdm_position_t;

typedef struct irdm_doppler irdm_doppler_t;
/* doppler_pos_init + doppler_pos_set_height(height_m) (main.c:597-604) */
irdm_doppler_t *irdm_doppler_create(double height_m);
void irdm_doppler_destroy(irdm_doppler_t *d);
/* doppler_pos_add_measurement(&f->ira, f->frequency, f->timestamp) for a type 1 (IRA) record (main.c:333-343); other
 * records are ignored.  Returns 1 when the measurement was stored, 0 when it was not. */
int irdm_doppler_add(irdm_doppler_t *d, const irdm_decoded_t *f);
/* doppler_pos_solve: 1 and a solution, or 0 (out still holds the satellite and measurement counts).  The solver's
 * unconditional "DOPPLER: ... FAIL" lines are kept for the formatters below and dropped here. */
int irdm_doppler_solve(irdm_doppler_t *d, irdm_position_t *out);
/* --position's schedule runs on stream time: tick T = 10, 20, ... s after start_time_ns (the context's
 * irdm_start_time_ns).  Set before the first batch. */
void irdm_doppler_set_origin(irdm_doppler_t *d, uint64_t start_time_ns);
/* --position for one poll batch, in output order: before the first frame whose timestamp - start_time_ns >= T s, the
 * solve for tick T, printed as the reference's stats thread prints it (main.c:506-519): the POSITION line on success, the
 * waiting line on failure when T % 60 == 0.  Then the frame's IRA record, if any, into the buffers (frames with ok set;
 * frame_decode's failures give type 0).  Returns the stderr bytes (NUL-terminated), or -1 when cap is too small.
 * cap >= 4096 per tick the batch crosses always suffices. */
long long irdm_format_doppler_packed_batch(irdm_doppler_t *d, const irdm_demod_packed_t *f, const irdm_frame_packed_t *fr,
                                           int n, char *buf, size_t cap);
/* the same from the "decode_frames" path's records (--save-bursts) */
long long irdm_format_doppler_batch(irdm_doppler_t *d, const irdm_decoded_t *f, int n, char *buf, size_t cap);
/* the end of the stream at end_ns (the clock of the timestamps: start_time_ns + samples / rate): the ticks up to it not yet
 * run, then one final solve, always printed (its POSITION line, or the waiting line).  Returns the bytes, or -1. */
long long irdm_doppler_finish(irdm_doppler_t *d, uint64_t end_ns, char *buf, size_t cap);

/* --save-bursts (qpsk_demod.c:339-389): writes <dir>/<timestamp>_<freq>_<id>_<DL|UL|UN>.cf32 (the frame's cf32 samples at
 * 250 kHz) and the matching .meta text file for one downmixed frame (info->drop_reason == 0), creating dir if needed.
 * samples: 2 * info->num_samples floats as returned by irdm_poll_frames with "keep_frame_samples" = 1.
 * Returns 0, or -1 (no frame / I/O error, message on stderr as the reference prints). */
int irdm_save_burst(const irdm_frame_info_t *info, const float *samples, const char *dir);

/* 3e. Band-select front end (K0): a wideband capture decimated on the GPU  */
/* ------------------------------------------------------------------ */
/* An object beside the pipeline (no reference counterpart: the reference is given a stream at the detector's rate).  It
 * shifts the band of interest to the centre, low-passes and decimates by an integer D, and writes cf32 at in_rate / D
 * straight into the pipeline's ingest slot (irdm_ingest_ptr), so captures at rates irdm_create refuses -- 25 .. 61.44 MS/s --
 * run through the unchanged pipeline, created as IRDM_FMT_CF32 at irdm_frontend_out_rate with centre frequency
 * capture centre + irdm_frontend_applied_shift_hz:
 *
 *   y[m] = sum_k h[k] r[m D + c - k],  r[n] = x[n] T[(q n) mod 65536],  c = (ntaps - 1) / 2,  r = 0 outside the stream
 *
 *   x  the capture in any IRDM_FMT_*, converted as the pipeline's kernels convert it
 *   q  = round(shift_hz * 65536 / in_rate); T[i] = cos(-2 pi i / 65536) + i sin(-2 pi i / 65536); the phase index comes from
 *      the 64-bit stream position, so the rotator has no drift and does not depend on how the stream is cut
 *   h  the pipeline's own low-pass design (Blackman-Harris), cut-off 0.5 out_rate, transition parameter 0.09 out_rate:
 *      ntaps ~ 44.4 D, flat to 0.42 out_rate, more than 80 dB down from 0.58 out_rate on
 * Centre-aligned: output m sits at capture sample m D, the filter adds no delay.  The arithmetic is a fixed sequence of
 * float operations (tests/frontend_model.c restates it in plain C, bit for bit).  The output does
 * not depend on how the input is cut into feeds; the samples a later output still needs are carried on the device.
 * One thread per object; every call puts the thread on the object's device. */
typedef struct {
    int device;                /* HIP device ordinal (the pipeline's) */
    int in_rate;               /* capture sample rate, Hz */
    int in_format;             /* IRDM_FMT_* of the capture */
    int decim;                 /* D, 2 .. 16; in_rate must be a multiple of it */
    double shift_hz;           /* band centre - capture centre; |shift_hz| <= in_rate / 2 */
} irdm_frontend_config_t;

typedef struct irdm_frontend irdm_frontend_t;
/* NULL (message on stderr) for in_rate / D not an integer, D outside 2 .. 16, an unknown format, a shift beyond half the
 * capture rate, or an output rate irdm_create would refuse. */
irdm_frontend_t *irdm_frontend_create(const irdm_frontend_config_t *cfg);
void irdm_frontend_destroy(irdm_frontend_t *fe);
int irdm_frontend_out_rate(const irdm_frontend_t *fe);
/* q * in_rate / 65536: the shift that is applied, what the pipeline's centre frequency is computed from */
double irdm_frontend_applied_shift_hz(const irdm_frontend_t *fe);
int irdm_frontend_ntaps(const irdm_frontend_t *fe);
/* the taps h[0 .. ntaps-1]; returns ntaps, or -1 when max is too small */
int irdm_frontend_taps(const irdm_frontend_t *fe, float *out, int max);
/* Stage-level entry: the next n_in samples of the capture (device memory, in_format); the outputs they complete -- output m
 * needs input m D + c -- are written to d_out (device memory, cf32).  stream: a hipStream_t as void*; NULL = the front end's
 * own stream, and the call returns when the outputs are written.  Returns the number of outputs, or -1 (more than out_cap
 * among them; nothing is consumed then). */
long long irdm_frontend_run_device(irdm_frontend_t *fe, const void *d_in, size_t n_in, void *d_out, size_t out_cap, void *stream);
/* the end of the stream for the stage-level entry: zeros behind the last sample, ceil(n_in_total / D) outputs in all */
long long irdm_frontend_finish_device(irdm_frontend_t *fe, void *d_out, size_t out_cap, void *stream);
/* The feeder: converts into irdm_ingest_ptr's slot (into a scratch chunk at pipeline_depth 0) and calls irdm_feed_device with
 * whole multiples of the pipeline's feed_block, at most max_chunk_samples at a time; the remainder waits for the next call.
 * p: an IRDM_FMT_CF32 context at irdm_frontend_out_rate on the same device.  n_in is arbitrary.  _device: stream = the
 * producer of d_in or NULL (as irdm_feed_device); d_in must stay unchanged until irdm_frontend_wait_input returns.
 * _host: the buffer (pinned for speed) may be reused when the call returns.  Return the bursts whose records became pollable,
 * or -1. */
int irdm_frontend_feed_device(irdm_frontend_t *fe, irdm_pipeline_t *p, const void *d_in, size_t n_in, void *stream);
int irdm_frontend_feed_host(irdm_frontend_t *fe, irdm_pipeline_t *p, const void *h_in, size_t n_in);
/* the end of the stream: the zero-padded rest, the held-back remainder as the pipeline's last chunk, then irdm_flush(p) */
int irdm_frontend_flush(irdm_frontend_t *fe, irdm_pipeline_t *p);
/* Another capture through the same front end (with irdm_reset of the pipeline behind it): back to its state after
 * irdm_frontend_create -- no carried tail, stream position and output count zero (and with them the rotator's phase index),
 * nothing held back by the feeder, not finished.  Taps, tables and the applied shift stay; nothing is allocated.  Waits for
 * the front end's stream.  0 ok, -1 error. */
int irdm_frontend_reset(irdm_frontend_t *fe);
/* irdm_prime_host behind a front end: the capture's first n_in samples (the format irdm_frontend_feed_host takes) run
 * through K0 / K0r / K0w without a flush -- irdm_frontend_swap_iq, _iq_balance and _scrub applied; saving, input statistics,
 * moments and the scrub's figures off -- until 512 frames of the band are there, and p is primed from the whole frames the
 * front end handed on (F: irdm_primed_frames(p); fewer than one: -1).  Then the front end is as irdm_frontend_reset leaves
 * it: the real run starts at input 0.  The band irdm_frontend_save writes and every figure of the front end are exactly
 * those of the run without priming; the context's records are those of a plain context fed P(y) followed by y, the band
 * of the plain run.  For 512 frames hand over at least ceil((512 N M + ntaps) / L) samples at the ratio L / M.  fe and
 * p must both be fresh (irdm_prime_host's conditions); -1 otherwise. */
int irdm_frontend_prime_host(irdm_frontend_t *fe, irdm_pipeline_t *p, const void *h_in, size_t n_in);
/* A capture taken up at input sample total_in, not at 0: the state that feeding total_in samples of zero codes (all-zero
 * bytes) would have left -- the stream position total_in (the rotator's phase index and the resampler's polyphase schedule
 * with it), every output that those samples complete counted as produced, the carried tail zeros.  Valid only directly
 * after irdm_frontend_create* or irdm_frontend_reset (nothing fed, not finished) and for total_in below IRDM_MAX_POSITION;
 * -1 otherwise, and the object is as it was.  irdm_frontend_save and a change of irdm_frontend_swap_iq, which a stream's
 * first sample closes, come before it.  Host state and one memset of the tail: a front end that is never sought launches
 * exactly what it launched without this entry.  0 ok. */
int irdm_frontend_seek(irdm_frontend_t *fe, uint64_t total_in);
/* host wait until everything enqueued so far has read its input buffer */
int irdm_frontend_wait_input(irdm_frontend_t *fe);
/* irdm_kernel_clock for K0 (always on): the kernel's own spans on the device summed since the last reset.  Waits for the
 * front end's stream. */
int irdm_frontend_kernel_clock(irdm_frontend_t *fe, double *sum_ms, uint64_t *launches, int reset);

/* The rational mode (K0r): output rate = in_rate * L / M, L / M = out_rate / in_rate in lowest terms, for captures whose
 * rate is no integer multiple of a rate the pipeline demodulates at (the pipeline wants a multiple of 250 kHz: 10 samples per
 * symbol after its own integer decimation).
 *
 *   y[m] = sum_n P[m M + C - n L] r[n]   (terms with 0 <= m M + C - n L < Np),  C = (Np - 1) / 2,  r[n] as above
 *
 *   P  the same low-pass design at the rate L * in_rate with gain L: cut-off 0.5 f_min, transition parameter 0.09 f_min,
 *      f_min = min(in_rate, out_rate); Np odd.  For L = 1 these are K0's taps at D = M.  (The design takes the rate as a
 *      float: L * in_rate is formed exactly and rounded once to nearest; exact for the rates the README names.)
 * Output m sits at capture time m M / L input samples: no delay.  A stream of n samples gives ceil(n L / M) outputs.  One
 * accumulator per component from +0, one fused multiply-add per term in ascending n, the zero samples outside the stream
 * included (tests/resample_model.c restates it in plain C, bit for bit).
 * Limits: L <= 125, M <= 768, 24/25 <= M / L <= 16, M != L; out_rate one irdm_create takes; format and shift as above.
 * When in_rate / out_rate is an integer D in 2 .. 16 the object is irdm_frontend_create's: K0's output, bit for bit.
 * Every irdm_frontend_* call above works on the object unchanged in meaning (irdm_frontend_taps returns P). */
typedef struct {
    int device;                /* HIP device ordinal (the pipeline's) */
    int in_rate;               /* capture sample rate, Hz */
    int in_format;             /* IRDM_FMT_* of the capture */
    int out_rate;              /* the rate handed to the pipeline, Hz */
    double shift_hz;           /* band centre - capture centre; |shift_hz| <= in_rate / 2 */
} irdm_frontend_rational_config_t;
/* NULL (message on stderr) for a ratio outside the limits, an unknown format, a shift beyond half the capture rate, or an
 * output rate irdm_create would refuse. */
irdm_frontend_t *irdm_frontend_create_rational(const irdm_frontend_rational_config_t *cfg);
/* The ratio out_rate / in_rate in lowest terms and the limits above on it, without a device: 0 when
 * irdm_frontend_create_rational would take the pair of rates as far as the ratio goes (an integer ratio 2 .. 16 included),
 * -1 with the create call's message on stderr otherwise.  L, M (either may be NULL) are set whenever both rates are positive. */
int irdm_frontend_rational_ratio(int in_rate, int out_rate, int *L, int *M);

/* The rational mode beyond L <= 125 and M <= 768 (K0w): the same function y[m], the same arithmetic, the same prototype from
 * the same design, for 2 <= L <= 4096, M <= 65536, 24/25 <= M / L <= 16 (L != M) and a prototype of at most 2^20 taps -- a
 * clock that is off by a fraction of a per cent (10.025 MS/s declared 10 MS/s: 400/401) and capture rates such as 2.88 MS/s
 * (275/288 to 2.75 MS/s) or 8.01 MS/s (100/801 to 1 MS/s).  Its tile is a run of consecutive outputs and a lane owns whole
 * outputs, so neither a period nor a phase block has to fit anything; the price is one vector load per tap where K0r has
 * scalar loads.  A ratio both kernels take gives the same output bit for bit.
 *
 * irdm_frontend_resampler_ratio: the ratio out_rate / in_rate in lowest terms and the kernel that
 * irdm_frontend_create_resampler would use -- *kernel 0: K0 (an integer ratio 2 .. 16), 1: K0r, 2: K0w -- without a device.
 * 0, or -1 with a message on stderr beyond K0w's limits.  L, M (any of the three may be NULL) are set whenever both rates
 * are positive. */
int irdm_frontend_resampler_ratio(int in_rate, int out_rate, int *L, int *M, int *kernel);
/* The front end for any pair of rates one of the three kernels takes: wherever irdm_frontend_create (an integer ratio) or
 * irdm_frontend_create_rational would make the object it is theirs, bit for bit; K0w otherwise.  NULL (message on stderr)
 * as irdm_frontend_create_rational. */
irdm_frontend_t *irdm_frontend_create_resampler(const irdm_frontend_rational_config_t *cfg);
/* Always K0w, for any ratio in K0w's limits (L >= 2: K0r's ratios included, for tests and measurements). */
irdm_frontend_t *irdm_frontend_create_wide(const irdm_frontend_rational_config_t *cfg);
/* K0w's launch geometry for a pair of rates, without a device: the prototype's length, the outputs per tile (one workgroup),
 * the workgroup's dynamic LDS in bytes and how many workgroups per CU that size is chosen for.  Any pointer may be NULL.
 * 0, or -1 (message) where irdm_frontend_create_wide would refuse the ratio or the prototype. */
int irdm_frontend_wide_geometry(int in_rate, int out_rate, int *ntaps, int *tile_outputs, int *lds_bytes, int *workgroups_per_cu);
/* the ratio in lowest terms: output rate = capture rate * L / M (1 / D for irdm_frontend_create's object).  0 ok, -1 error. */
int irdm_frontend_ratio(const irdm_frontend_t *fe, int *L, int *M);

/* Saving the band: the front end's output stream -- every sample it produces, in order, in either mode, through the
 * stage-level entries and the feeder alike -- handed to a callback as a ci8 / ci16 / cf32 recording at
 * irdm_frontend_out_rate, centred at the capture centre + irdm_frontend_applied_shift_hz.  Per float component x of the
 * cf32 band, with S = 128 (ci8) or 32768 (ci16) and k = (float)gain * S formed once in float:
 *
 *   v = rintf(x * k)   (one rounded product; to nearest, ties to even)     q = clamp(v, -S, S - 1)
 *   NaN -> 0; +-Inf -> the rail of its sign
 *
 * written as interleaved I, Q little-endian int8 / int16.  ci16 holds all 16 bits: such a file is read back as
 * IRDM_FMT_CI16_FULL (IRDM_FMT_CI16 narrows by >> 8 as the reference does).  cf32: the bytes as they are, gain 1.
 * The sink runs on the calling thread, inside irdm_frontend_* calls, in stream order, with at most slot_samples samples at
 * a time; irdm_frontend_flush and irdm_frontend_finish_device deliver everything outstanding before they return.  The bytes
 * delivered are ceil(n_in_total * L / M) samples and do not depend on how the input was cut into feeds, on slot_samples, or
 * on the pipeline behind the feeder.  irdm_frontend_reset drops what has not been delivered and zeroes the statistics; the
 * sink stays installed and nothing is allocated. */
typedef int (*irdm_band_sink_t)(void *user, const void *bytes, size_t n_bytes);   /* non-zero = stop: the call in progress returns -1 */
typedef struct {
    int format;               /* IRDM_FMT_CI8, IRDM_FMT_CI16 (full 16 bits, read back as IRDM_FMT_CI16_FULL) or IRDM_FMT_CF32 */
    float gain;               /* > 0, finite; must be 1 for cf32 */
    size_t slot_samples;      /* 0 = default (4 Mi samples); two pinned host slots of this size (and two on the device) */
    irdm_band_sink_t sink;
    void *user;
} irdm_frontend_save_config_t;
/* before the first sample; NULL cfg = off; -1 mid-stream or on a bad field */
int irdm_frontend_save(irdm_frontend_t *fe, const irdm_frontend_save_config_t *cfg);
/* n_samples: samples requantised (cf32: copied) since creation or the last reset; n_clipped: components whose v fell outside
 * [-S, S - 1] or that were NaN; peak: max |x * k| / S over the finite components, the fraction of full scale before clipping
 * (cf32: n_clipped 0, peak 0 -- no kernel looks at the samples). */
typedef struct { uint64_t n_samples, n_clipped; float peak; } irdm_band_stats_t;
int irdm_frontend_save_stats(irdm_frontend_t *fe, irdm_band_stats_t *out);              /* waits for the front end's streams */
/* stage level: n cf32 samples in device memory (8-byte aligned) -> d_out (format as above; aligned to a sample of it), the
 * statistics of this call alone (stats may be NULL); stream NULL = synchronous (an integer format waits for the stream in
 * either case: the statistics are read back).  0 ok, -1 error. */
int irdm_requantize_device(const void *d_in, size_t n, int format, float gain, void *d_out, irdm_band_stats_t *stats, int device, void *stream);

/* ---- input statistics (irdm_input_stats_t above) ----
 * irdm_set_option(p, "input_stats", 1): every chunk fed from then on is reduced by one extra pass on a side stream of the
 * context (one read of the chunk, beside K1; no record changes).  irdm_input_stats: the statistics of the stream so far --
 * what is in flight is settled first, like irdm_detector_stats.  irdm_reset starts them over; they are not part of
 * irdm_export_state.  Returns 0, or -1 (the option is off included).
 * The front end has the same switch and getter over the CAPTURE's samples in front of its kernel: clipping is a property of
 * the recording, not of the selected band.  irdm_frontend_reset starts them over.
 * Stage level: the statistics of the n samples of `format` at d_in (device memory, aligned to a sample) alone; the pass runs
 * on `stream` (NULL: a stream of its own) and the call is synchronous on return. */
int irdm_input_stats(irdm_pipeline_t *p, irdm_input_stats_t *out);
int irdm_frontend_input_stats_enable(irdm_frontend_t *fe, int on);
int irdm_frontend_input_stats(irdm_frontend_t *fe, irdm_input_stats_t *out);
int irdm_input_stats_device(const void *d_in, size_t n, int format, irdm_input_stats_t *out, int device, void *stream);

/* ---- symbol clock check (irdm_clock_est_t / irdm_symbol_clock_t above) ----
 * irdm_set_option(p, "symbol_clock", 1): every frame that reaches the demodulator from then on gets an estimate of its
 * symbol clock error, by one kernel on the chain's stream that only reads the frames.
 * irdm_poll_symbol_clock: up to `max` per-frame records, one for every frame that reached the demodulator, in the order
 *   of the demodulator's records: those without IRDM_CLOCK_NOT_OK pair one to one with the records of irdm_poll_demods /
 *   irdm_poll_demods_packed.  A frame's record depends on its samples alone, not on pipeline_depth or how the stream was
 *   fed.  Returns the number written (0 with the option off), -1 on error.
 * irdm_symbol_clock: the summary of the stream so far (of the records queued so far: irdm_flush first for the whole
 *   stream).  irdm_reset starts it over.  Returns 0, or -1 (the option never set included).
 * irdm_symbol_clock_batch: the kernel alone on n frames, with the calling convention of irdm_qpsk_demod_batch: samples =
 *   n rows of IRDM_MAX_FRAME_SAMPLES interleaved float pairs, num_samples[i] <= IRDM_MAX_FRAME_SAMPLES.  Works with the
 *   option off.  Returns 0 or -1. */
int irdm_poll_symbol_clock(irdm_pipeline_t *p, irdm_clock_est_t *out, int max);
int irdm_symbol_clock(irdm_pipeline_t *p, irdm_symbol_clock_t *out);
int irdm_symbol_clock_batch(irdm_pipeline_t *p, const float *samples, const int *num_samples, int n, irdm_clock_est_t *out);

/* ---- carrier frequency from the frame's samples (irdm_fine_freq_t / irdm_fine_freq_summary_t above) ----
 * irdm_set_option(p, "fine_freq", 1): every frame that reaches the demodulator from then on gets an estimate of its
 * carrier frequency, by one kernel on the chain's stream that only reads the frames; the demodulator records carry it.
 * irdm_poll_fine_freq: up to `max` per-frame records, one for every frame that reached the demodulator, in the order
 *   of the demodulator's records: those without IRDM_FINE_FREQ_NOT_OK pair one to one with the records of
 *   irdm_poll_demods / irdm_poll_demods_packed.  A frame's record depends on its samples and the downmixer's frequency
 *   alone, not on pipeline_depth or how the stream was fed.  Returns the number written (0 with the option off), -1 on error.
 * irdm_fine_freq: the summary of the stream so far (of the records queued so far: irdm_flush first for the whole
 *   stream).  irdm_reset starts it over.  Returns 0, or -1 (the option never set included).
 * irdm_fine_freq_batch: the kernel alone on n frames, with the calling convention of irdm_symbol_clock_batch: samples =
 *   n rows of IRDM_MAX_FRAME_SAMPLES interleaved float pairs, num_samples[i] <= IRDM_MAX_FRAME_SAMPLES.  freq_hz of a
 *   record is df_hz (there is no downmixer's value).  Works with the option off.  Returns 0 or -1. */
int irdm_poll_fine_freq(irdm_pipeline_t *p, irdm_fine_freq_t *out, int max);
int irdm_fine_freq(irdm_pipeline_t *p, irdm_fine_freq_summary_t *out);
int irdm_fine_freq_batch(irdm_pipeline_t *p, const float *samples, const int *num_samples, int n, irdm_fine_freq_t *out);

/* ---- arrival time from the frame's samples (irdm_fine_time_t / irdm_fine_time_summary_t above) ----
 * irdm_set_option(p, "fine_time", 1): every frame that reaches the demodulator from then on gets an estimate of its
 * symbol timing, by one kernel on the chain's stream that only reads the frames; the demodulator records carry the time.
 * irdm_poll_fine_time: up to `max` per-frame records, one for every frame that reached the demodulator, in the order
 *   of the demodulator's records: those without IRDM_FINE_TIME_NOT_OK pair one to one with the records of
 *   irdm_poll_demods / irdm_poll_demods_packed, and time_ns is that record's timestamp.  A frame's record depends on its
 *   samples, its class (simplex or not), the downmixer's timestamp and the correlator's place alone, not on pipeline_depth or
 *   how the stream was fed.  Returns the number written (0 with the option off), -1 on error.
 * irdm_fine_time: the summary of the stream so far (of the records queued so far: irdm_flush first for the whole
 *   stream).  irdm_reset starts it over.  Returns 0, or -1 (the option never set included).
 * irdm_fine_time_batch: the kernel alone on n frames, with the calling convention of irdm_fine_freq_batch: samples =
 *   n rows of IRDM_MAX_FRAME_SAMPLES interleaved float pairs, num_samples[i] <= IRDM_MAX_FRAME_SAMPLES; simplex[i] != 0:
 *   frame i takes the simplex window (NULL: none does).  tau, s_re, s_im, floor, quality, flags and n of a record are
 *   filled, corr and time_ns are 0 and the ambiguity rule is not applied (there is no correlator).  Works with the option
 *   off.  Returns 0 or -1. */
int irdm_poll_fine_time(irdm_pipeline_t *p, irdm_fine_time_t *out, int max);
int irdm_fine_time(irdm_pipeline_t *p, irdm_fine_time_summary_t *out);
int irdm_fine_time_batch(irdm_pipeline_t *p, const float *samples, const int *num_samples, const int *simplex, int n,
                         irdm_fine_time_t *out);

/* ---- per-burst resampling (option "burst_resample") ----
 * Output m of a decimated row x[0 .. n) is the band-limited interpolation of x at input time m M / L: q = floor(m M / L),
 * ph = (m M) mod L, y[m] = sum_k taps[ph][k] x[q - T/2 + 1 + k] over T = taps_per_phase taps, x zero outside the row,
 * res_len = floor(n L / M) outputs.  The filter adds no delay (an impulse at input i is centred at output i L / M).  The
 * prototype is a windowed sinc designed in binary64 at rate L f_in: flat within 0.01 dB to 50 kHz, 80 dB down from
 * 165 kHz.  Per component the sum is ONE chain of float32 fused multiply-adds in ascending k from 0: a row's result depends
 * on the row and the ratio alone.  Behind the stage frequencies and times are in units of a true 250 kHz; the frame record's
 * dec_len is res_len.
 * irdm_burst_resample_ratio: the ratio in force and the taps per phase; 1 / 1 with 0 taps at a rate on the grid.  0, or -1
 *   with the option off.
 * irdm_burst_resample_taps: the phase-major table, L x taps_per_phase floats, as irdm_frontend_taps: the floats copied,
 *   0 at a rate on the grid, -1 with the option off or cap too small.
 * irdm_burst_resample_batch: the kernel alone, without a context: n rows of interleaved float pairs, row i at
 *   rows + 2 * stride * i with lens[i] <= stride samples, resampled at L / M (7/8 <= L / M <= 8/7, L <= 4096, the table
 *   designed by the same function) into out + 2 * out_stride * i, res_lens[i] <= out_stride samples each.  0 or -1.
 * irdm_burst_resample_design: that table, L x 20 floats phase-major, for a ratio given directly (4096/4097 is no sample
 *   rate's): the floats copied, -1 for a ratio the stage refuses or cap too small.  Host only. */
int irdm_burst_resample_ratio(irdm_pipeline_t *p, int *L, int *M, int *taps_per_phase);
int irdm_burst_resample_taps(irdm_pipeline_t *p, float *out, int cap);
int irdm_burst_resample_design(int L, int M, float *out, int cap);
int irdm_burst_resample_batch(int device, const float *rows, const int *lens, int n, int stride, int L, int M, float *out,
                              int out_stride, int *res_lens);

/* ---- exchanged I and Q (irdm_iq_vote_t / irdm_iq_sense_t above) ----
 * irdm_swap_iq_device: the two components of each of n_samples samples of `format` (IRDM_FMT_*) at d_iq exchanged in
 *   place -- a byte permutation, no conversion: cu8 stays cu8, a NaN stays a NaN; applied twice it is the identity.  d_iq
 *   need only be aligned to a sample.  On `stream` (a hipStream_t) without waiting; stream == NULL: on a stream of the
 *   call's own, complete on return.  Returns 0; -1 for an unknown format, a pointer that is not sample-aligned or a
 *   failed launch; n_samples == 0 launches nothing.
 * irdm_set_option(p, "swap_iq", 1) applies it to every chunk of irdm_feed_host; irdm_frontend_swap_iq (below) to every
 *   capture chunk of irdm_frontend_feed_host.
 * irdm_set_option(p, "iq_sense", 1): every frame whose unique word passes from then on is judged in both senses.
 * irdm_poll_iq_votes: up to `max` per-frame records, one per record of irdm_poll_demods / irdm_poll_demods_packed, in
 *   their order.  A frame's record depends on its bits and LLRs alone.  Returns the number written (0 with the option
 *   off), -1 on error.
 * irdm_iq_sense: the summary of the records queued so far (irdm_flush first for the whole stream); irdm_reset starts it
 *   over.  Returns 0, or -1 (the option never set included).
 * irdm_iq_sense_batch: the kernel alone on n frames (bits, llr, n_bits and direction of each irdm_demod_t are read; an odd
 *   n_bits is rounded down), as irdm_ida_decode_batch.  Works with the option off.  Returns 0 or -1. */
int irdm_swap_iq_device(void *d_iq, size_t n_samples, int format, int device, void *stream);
int irdm_poll_iq_votes(irdm_pipeline_t *p, irdm_iq_vote_t *out, int max);
int irdm_iq_sense(irdm_pipeline_t *p, irdm_iq_sense_t *out);
int irdm_iq_sense_batch(irdm_pipeline_t *p, const irdm_demod_t *in, int n, irdm_iq_vote_t *out);
/* irdm_frontend_swap_iq: option "swap_iq" for a front end -- irdm_frontend_feed_host exchanges the components of every
 *   capture chunk in its staging buffer, in front of K0 / K0r and of the front end's statistics pass, so the band that
 *   irdm_frontend_save writes is the corrected one.  With it on, irdm_frontend_feed_device and irdm_frontend_run_device
 *   return -1 with a line on stderr (they take the caller's buffer as it is).  Returns 0; -1 for a change between the
 *   stream's first chunk and irdm_frontend_reset.  (With irdm_frontend_dc_block, _iq_balance and _scrub, below: exchange, DC,
 *   balance, scrub, in that order, the DC tracker's wire format in effect when both it and the balance are on -- DESIGN.md
 *   section 5, "The host feed's corrections in one place".) */
int irdm_frontend_swap_iq(irdm_frontend_t *fe, int on);

/* ---- non-finite and out-of-range samples (irdm_scrub_stats_t above) ----
 * irdm_scrub_device: the pass alone, on the n_samples samples of `format` (IRDM_FMT_*) at d_iq, a buffer the caller owns;
 *   d_iq need only be aligned to a sample.  limit_log2: 0 .. 127 (IRDM_SCRUB_DEFAULT_LOG2 = 40).  stats == NULL: on
 *   `stream` (a hipStream_t) without waiting; stream == NULL: on a stream of the call's own, complete on return.  With
 *   stats the call waits for the stream and fills them in; first and last are indices into the buffer.  A buffer of more
 *   than 2^31 samples is cut into launches of at most that many.  Returns 0 -- for a format other than cf32 without
 *   touching the buffer (stats: active 0) --; -1 for an unknown format, a pointer that is not aligned to a sample, a
 *   limit outside 0 .. 127 or a failed launch; n_samples == 0 launches nothing.  Applied twice, the second pass changes
 *   and counts nothing.
 * irdm_set_option(p, "scrub", 1) applies it to every chunk of irdm_feed_host; irdm_frontend_scrub to every capture chunk of
 *   irdm_frontend_feed_host.
 * irdm_scrub_stats: the figures of the stream so far, positions in stream coordinates; waits for the feed stream.
 *   irdm_reset starts them over.  They are NOT part of irdm_export_state / irdm_import_state: a context that takes a
 *   stream over counts from zero.  Returns 0, or -1 (the option off included).
 * irdm_frontend_scrub: option "scrub" for a front end -- irdm_frontend_feed_host scrubs every capture chunk in its staging
 *   buffer, behind irdm_frontend_swap_iq's exchange and in front of the front end's statistics pass and K0 / K0r, so the
 *   band that irdm_frontend_save writes is the scrubbed one.  A front end of another capture format takes the switch and
 *   launches nothing.  With it on, irdm_frontend_feed_device and irdm_frontend_run_device return -1 with a line on
 *   stderr.  Returns 0; -1 for a limit outside 0 .. 127 and for a change of either value between the stream's first chunk
 *   and irdm_frontend_reset.
 * irdm_frontend_scrub_stats: as irdm_scrub_stats, positions in capture coordinates (irdm_frontend_seek moves the origin
 *   with the stream position); irdm_frontend_reset starts them over. */
int irdm_scrub_device(void *d_iq, size_t n_samples, int format, int limit_log2, irdm_scrub_stats_t *stats, int device, void *stream);
int irdm_scrub_stats(irdm_pipeline_t *p, irdm_scrub_stats_t *out);
int irdm_frontend_scrub(irdm_frontend_t *fe, int on, int limit_log2);
int irdm_frontend_scrub_stats(irdm_frontend_t *fe, irdm_scrub_stats_t *out);

/* ---- receiver I/Q imbalance: the measurement (irdm_iq_moments_t above) and the correction ----
 * A zero-IF receiver whose arms differ in gain (g) and are not exactly 90 degrees apart (phi) delivers
 *   y_I = x_I,  y_Q = g (x_Q cos phi + x_I sin phi):  every signal at +f leaves an image at -f, image_db down.  The image
 * of a burst is its conjugate, which the demodulator accepts (see "Exchanged I and Q" in the README).
 * irdm_iq_moments: option "iq_moments" -- the sums of the stream so far and the figures derived from them; waits for the
 *   passes in flight.  NOT part of irdm_export_state / irdm_import_state.  Returns 0, or -1 (the option never set included).
 * irdm_iq_moments_device: the pass alone over the n samples of `format` at d_iq (aligned to a sample), complete on
 *   return; on `stream` (a hipStream_t) or, with NULL, on a stream of the call's own.  Launches of at most 2^31 samples.
 *   n == 0 launches nothing and returns 0 with valid 0.  -1 for an unknown format, a misaligned pointer, a failed launch.
 *   out == NULL (with a stream): the launches alone on `stream`, without waiting and without figures -- for timing.
 * irdm_frontend_iq_moments / irdm_frontend_iq_moments_stats: the same for a front end, over the capture in front of
 *   K0 / K0r (behind irdm_frontend_swap_iq, irdm_frontend_iq_balance and irdm_frontend_scrub); the image mirrors about the
 *   capture's centre.  irdm_frontend_reset starts the sums over.
 *
 * irdm_iq_balance_coeffs (host only): alpha = -tan(phi), beta = 1 / (g cos(phi)) with g = 10^(gain_db / 20), computed in
 *   binary64 and rounded once to float.  -1 outside |gain_db| <= 6, |phase_deg| <= 30.  Either pointer may be NULL.
 * irdm_iq_balance_device: the n samples of `format` at d_in (aligned to a sample) become cf32 at d_out_cf32 (aligned to 8
 *   bytes): i' = i, q' = alpha i + beta q -- two rounded binary32 products and one rounded sum, never fused; i, q as the
 *   load stage converts them.  d_out_cf32 == d_in is allowed for the 8-byte formats (in place); any other overlap, an
 *   unknown format, a misaligned pointer and coefficients outside what irdm_iq_balance_coeffs can return give -1.  On
 *   `stream` without waiting, or with NULL on a stream of the call's own, complete on return.
 * irdm_iq_balance: for a context created as IRDM_FMT_CF32, before its first feed.  From then on irdm_feed_host takes
 *   n_samples of wire_format (any IRDM_FMT_*): the host-to-device copy lands in a wire staging buffer (max_chunk samples
 *   of the wire format, allocated by this call; none for a cf32 wire format, which lands where it lands today and is
 *   corrected in place), option "swap_iq" exchanges the components there, the kernel above writes the ring slot or the
 *   staging buffer, and "scrub" and everything else follow on cf32.  A context so set, fed F's bytes, yields bit for bit
 *   every record of a plain cf32 context fed the corrected samples.  The setting survives irdm_reset.  With it on
 *   irdm_feed_device / irdm_feed_begin return -1 with a line on stderr -- correct the buffer with irdm_iq_balance_device
 *   first.  -1 after the stream's first feed, for a context of another format, for a member of a group, for an unknown
 *   wire format and for figures outside the limits.
 * irdm_frontend_iq_balance: the same for a front end created with in_format cf32; irdm_frontend_feed_host then takes
 *   wire_format's bytes and the kernel writes the capture staging buffer. */
int irdm_iq_moments(irdm_pipeline_t *p, irdm_iq_moments_t *out);
int irdm_iq_moments_device(const void *d_iq, size_t n, int format, irdm_iq_moments_t *out, int device, void *stream);
int irdm_frontend_iq_moments(irdm_frontend_t *fe, int on);
int irdm_frontend_iq_moments_stats(irdm_frontend_t *fe, irdm_iq_moments_t *out);
int irdm_iq_balance_coeffs(double gain_db, double phase_deg, float *alpha, float *beta);
int irdm_iq_balance_device(void *d_out_cf32, const void *d_in, size_t n, int format, float alpha, float beta, int device, void *stream);
int irdm_iq_balance(irdm_pipeline_t *p, int wire_format, double gain_db, double phase_deg);
int irdm_frontend_iq_balance(irdm_frontend_t *fe, int wire_format, double gain_db, double phase_deg);

/* ---- a receiver's DC offset: tracked block by block and subtracted (csrc/dc_block.hpp) ----
 * A constant added to every sample is a tone at the capture's centre; the downmix and the demodulator lose the frames of
 * the channel it falls into (the README has the figures).  The rule, for all eight formats alike:
 *   a component c is the float the load stage makes of the sample; q(c) = llrint(c' 2^32) as int64, c' = c clamped to +-64,
 *   a NaN counting 0; the stream is cut into blocks of B = 2^block_log2 samples (12 .. 24, IRDM_DC_DEFAULT_LOG2 = 20) aligned
 *   to the stream position; S_k = the int64 sum of q over block k per arm; m_k = (float)((double)S_k / (B 2^32)); a sample of
 *   block k >= 1 becomes (i - m_{k-1}.i, q - m_{k-1}.q), one rounded binary32 subtraction each, block 0 uses the seed; a NaN
 *   component leaves with its quiet bit set.  Integer sums: the output does not depend on how feeds cut the stream.
 * irdm_dc_mean_host (host only, no device call): out = the mean by that rule of the n <= 2^24 leading samples of `format` at
 *   h_iq, (float)((double)sum q / (n 2^32)) per arm -- what the binary seeds a recording with.  0, or -1.
 * irdm_dc_block_device: n samples of `format` at d_in (aligned to a sample) become cf32 at d_out_cf32 (aligned to 8 bytes;
 *   d_in itself for an 8-byte format, any other overlap is refused), the sample at d_in lying at stream position
 *   first_sample.  state_io carries a stream from call to call: on entry the sums of the block first_sample lies in as far
 *   as earlier calls have seen it (ignored when first_sample is a multiple of B) and the mean that block is corrected by
 *   (the seed, for a stream's first call); on return those of the block first_sample + n lies in.  One stream cut into
 *   calls anywhere gives the bytes and the final state of a single call.  The call works on `stream` (a hipStream_t) or,
 *   with NULL, on a stream of its own, on the current device, and is complete on return.  0, or -1 for an unknown
 *   format, a block length outside 12 .. 24, a misaligned pointer, overlapping buffers, a mean in state_io that is not finite
 *   or lies beyond +-64, or a failed launch; n == 0 launches nothing.
 * irdm_dc_block: for a context created as IRDM_FMT_CF32, before its first feed; it works as irdm_iq_balance does.  From
 *   then on irdm_feed_host takes n_samples of wire_format: they land in a wire staging buffer (none for cf32, which is
 *   corrected where it lands, in the ring slot or the staging buffer), and three launches on the feed's stream write the
 *   corrected cf32 chunk.  Order where a chunk lands: option "swap_iq", then this, then irdm_iq_balance (then on cf32, in
 *   place, whatever its own wire format), then "scrub".  A prefix of irdm_prime_* goes through like any chunk: blocks count
 *   from the start of the prefix.  block_log2 < 0 switches it off.  seed_i, seed_q: what block 0 is corrected by.  Switch,
 *   block length, wire format and seed are configuration and survive irdm_reset; the position, the open block's sums, the
 *   means and the figures are stream state, which irdm_reset starts over; they are NOT part of irdm_export_state /
 *   irdm_import_state.  With it on irdm_feed_device / irdm_feed_begin return -1 with a line on stderr -- correct the
 *   buffer with irdm_dc_block_device first.  -1 after the stream's first feed, for a context of another format, for a
 *   member of a group, for a block length outside 12 .. 24, an unknown wire format and a seed that is not finite or lies
 *   beyond +-64.  Off, nothing is allocated and nothing launched.  Options "dc_block_log2" (12 .. 24) and "dc_block" (1:
 *   irdm_dc_block with a cf32 wire format, that block length and a zero seed; 0: off) reach the same switch.
 * irdm_dc_stats: the figures of the stream so far; waits for the feed stream.  0, or -1 (the option off included).
 * irdm_frontend_dc_block: the same for a front end created with in_format cf32, on the capture in front of K0 / K0r / K0w:
 *   irdm_frontend_feed_host takes wire_format's bytes and the three launches write the capture staging buffer, behind
 *   irdm_frontend_swap_iq's exchange and in front of irdm_frontend_iq_balance, irdm_frontend_scrub, the statistics passes
 *   and the kernel.  The tone is removed before the shift, and irdm_frontend_save writes the corrected band.  Blocks count
 *   from the first sample fed since creation, irdm_frontend_reset or irdm_frontend_seek; irdm_frontend_reset starts the
 *   stream state over and keeps the setting.  With it on irdm_frontend_feed_device and irdm_frontend_run_device return -1
 *   with a line on stderr.  -1 after the capture's first chunk and for the values irdm_dc_block refuses.
 * irdm_frontend_dc_stats: as irdm_dc_stats.
 * irdm_dc_block_time_device (measurement surface: tools/dc_block_rate.py): the three kernels over the n <= 2^26 samples of
 *   `format` at d_in (out of place, or an 8-byte format in place), each launched `reps` times between two events of its
 *   own on a stream of the call's: us[0] the sums pass, us[1] the close pass, us[2] the subtraction, microseconds per
 *   launch.  The output at d_out_cf32 is corrected by means that mean nothing.  0, or -1. */
#define IRDM_DC_DEFAULT_LOG2 20
typedef struct {
    int64_t sum_i, sum_q;          /* the open block's sums of q */
    float   mean_i, mean_q;        /* what the open block is corrected by */
} irdm_dc_state_t;
typedef struct {
    uint64_t n_samples;            /* samples the pass has taken */
    uint64_t n_blocks;             /* whole blocks among them */
    int      block_log2;
    int      wire_format;
    float    seed_i, seed_q;
    float    first_i, first_q;     /* m_0; these and the following: 0 while n_blocks == 0 */
    float    last_i, last_q;       /* the mean of the last whole block */
    float    min_i, max_i, min_q, max_q;
} irdm_dc_stats_t;
int irdm_dc_mean_host(int format, const void *h_iq, size_t n, float out[2]);
int irdm_dc_block_device(int format, void *d_out_cf32, const void *d_in, size_t n, int block_log2, uint64_t first_sample,
                         irdm_dc_state_t *state_io, void *stream);
int irdm_dc_block(irdm_pipeline_t *p, int wire_format, int block_log2, float seed_i, float seed_q);
int irdm_dc_stats(irdm_pipeline_t *p, irdm_dc_stats_t *out);
int irdm_frontend_dc_block(irdm_frontend_t *fe, int wire_format, int block_log2, float seed_i, float seed_q);
int irdm_frontend_dc_stats(irdm_frontend_t *fe, irdm_dc_stats_t *out);
int irdm_dc_block_time_device(int format, void *d_out_cf32, const void *d_in, size_t n, int block_log2, int reps, float us[3]);

/* ---- self-describing recordings: WAV / RF64, SigMF, SDRangel .sdriq (csrc/recording.cpp) ----
 * Host code only, no device call: works without a GPU.  irdm_recording_probe reads the header of `path` and says what the
 * samples are and where they lie.  container: 0 = by the file's extension, compared without case (.wav / .wave / .rf64;
 * .sigmf-meta / .sigmf-data; .sdriq), or one of IRDM_CONTAINER_* to force a kind.  File contents are never sniffed: a raw
 * recording may begin with any bytes.  Returns 0: a container was recognised and *out is filled; 1: not a container (a
 * raw file; *out untouched but for kind = 0); -1: malformed or unsupported, and err (err_cap bytes, may be NULL) says what
 * and where.
 *   WAV / RF64: RIFF..WAVE, or RF64 / BW64 with a ds64 chunk; fmt of 16, 18 or 40 bytes, tag 1 (PCM), 3 (float) or 0xFFFE
 *     (the tag is the first two bytes of the sub-format GUID); two channels (I, Q); 8-bit PCM -> cu8, 16-bit PCM -> ci16-full
 *     (v / 32768), 32-bit PCM -> ci32, 32-bit float -> cf32; anything else is refused with the bit depth in the message.  A
 *     data size of 0 or 0xFFFFFFFF, or one past the end of the file, means "to the end of the file".  The binary auxi chunk
 *     (two SYSTEMTIMEs, then a u32 centre frequency) gives start time and centre when its year lies in 1990..2100;
 *     otherwise the centre comes from _<digits>Hz / _<digits>kHz in the file name.
 *   SigMF: either file of the pair; global core:datatype cf32_le / ci16_le (-> ci16-full) / ci8 / cu8 / ci32_le,
 *     core:sample_rate (a whole number), core:num_channels absent or 1, core:trailing_bytes, core:dataset; captures[0]
 *     core:sample_start 0, core:frequency, core:datetime (ISO 8601 UTC, kept to the nanosecond), core:header_bytes.
 *   .sdriq: a 32-byte header (u32 rate, u64 centre, u64 start in s or -- from 10^11 up -- ms, u32 sample size 16 / 24, u32 0,
 *     u32 CRC-32 of the first 28 bytes); 16 -> ci16-full, 24 -> IRDM_FMT_CI32_24. */
#define IRDM_CONTAINER_NONE  0
#define IRDM_CONTAINER_WAV   1
#define IRDM_CONTAINER_SIGMF 2
#define IRDM_CONTAINER_SDRIQ 3
typedef struct {
    int      kind;                 /* IRDM_CONTAINER_* */
    int      format;               /* IRDM_FMT_* of the samples */
    int      sample_rate;          /* samples per second */
    int      has_center;           /* center_frequency is from the file */
    double   center_frequency;     /* Hz */
    int      has_start;            /* start_time_ns is from the file */
    int      n_captures;           /* SigMF: capture segments in the metadata (the first one's values are used); else 1 */
    uint64_t start_time_ns;        /* UTC, ns since 1970 */
    uint64_t data_offset;          /* the samples are [data_offset, data_offset + data_bytes) of data_path */
    uint64_t data_bytes;           /* rounded down to whole samples */
    char     data_path[4096];      /* the file that holds the samples */
} irdm_recording_info_t;
int irdm_recording_probe(const char *path, int container, irdm_recording_info_t *out, char *err, size_t err_cap);

/* The fine-CFO step's cexpf(i x) (burst_downmix.c:716-717) as the device evaluates it -- glibc's sincosf restated,
 * csrc/libm_port.hpp -- for n arbitrary arguments (test / audit surface: tests/test_gpu_libm.py,
 * tools/check_sincosf_gpu.c compare it with the host's libm).  0 ok, -1 error; NaN where |x| >= 120. */
int irdm_sincosf_probe(int device, const float *x, size_t n, float *re, float *im);

const char *irdm_version(void);

#ifdef __cplusplus
}
#endif
#endif
