/*
 * iridium_sniffer_hip.c -- file-mode command line over the MI355X hot path, plain C99.
 *
 * Mirrors the reference's file-mode surface (options.c:186-551, main.c:223-284, frame_output.c:160-199):
 *     iridium-sniffer-hip -f FILE [-r RATE] [-c FREQ] [--format ci8|cu8|ci16|cf32|ci16-full|sc16q11|ci32|ci32-24] [-d DB]
 *                         [--container wav|sigmf|sdriq|raw] [--probe]
 *                         [--file-info STR] [--no-gardner] [--no-simd] [--chunk SAMPLES] [-v]
 *                         [--parsed] [--acars] [--acars-json] [--station ID] [--position[=HEIGHT_M]]
 *                         [--band-center HZ --decimate D] [--resample-to HZ [--band-center HZ]]
 *                         [-f FILE2 ...] [--files-from LIST] [--start-time SEC[.NNNNNNNNN]] [--out-dir DIR]
 *                         [--spectrum FILE [--spectrum-frames R]]
 *                         [--save-band FILE [--save-format ci8|ci16|cf32] [--save-gain G] [--save-only]]
 *                         [--input-stats] [--diagnostic] [--clock-check] [--fine-freq] [--fine-time] [--iq-check] [--swap-iq] [--scrub[=LOG2]] [--dc-block[=LOG2]]
 *                         [--image-check] [--iq-balance=GAIN_DB,PHASE_DEG] [--burst-resample] [--prime] [--join]
 * IQ file in, iridium-toolkit "RAW:" lines on stdout (IDA: lines with --parsed; ACARS lines instead of RAW ones with
 * --acars / --acars-json, main.c:357-361), "burst_detect: tagged N bursts total" on stderr
 * (burst_detect.c:350-351, the line test-configurations.sh:140 greps); with --position, the Doppler position estimate's
 * "POSITION:" lines on stderr (main.c:506-519), solved every 10 s of stream time instead of wall-clock time.  Everything between the file
 * read and the line printer runs on the GPU through the C-ABI in include/irdm_hip.h; there is no CPU
 * path here (the reference's own --no-gpu binary is the CPU path).
 * --format ci16-full and --format sc16q11 read interleaved int16 at full precision, scaled as the reference's live
 * SoapySDR CS16 (v / 32768) and bladeRF SC16Q11 (v / 2048) paths scale it; ci16 (and a .ci16 / .cs16 file) is the
 * reference's file path, narrowed to 8 bits.  --format cu8 (and a .cu8 / .u8 file) is rtl_sdr's unsigned 8-bit I/Q,
 * (u - 127.5) / 128; the reference reads no such file.
 * --format ci32 and --format ci32-24 read interleaved int32: v / 2^31 (SigMF ci32_le, 32-bit PCM WAV) and 24-bit samples held
 * in int32, v / 2^23 (SDRangel's .sdriq).
 * Self-describing recordings: a FILE ending in .wav / .wave / .rf64, .sigmf-meta / .sigmf-data or .sdriq (compared without
 * case), or any FILE with --container wav|sigmf|sdriq, is probed (irdm_recording_probe) and its header gives the sample
 * format, the rate, the centre frequency and the capture time: -f FILE alone runs it.  --container raw turns probing off for
 * every -f; stdin is always raw (-f - with --container is refused), and so is --format beside a container.  An explicit -r
 * that disagrees with the header wins, with a one-line warning; an explicit -c wins silently; --start-time (or a list entry's
 * START_SEC) wins over the header's time; a header without a centre leaves -c or its default.  A malformed header fails
 * that recording with the probe's message (exit 1; exit 2 when it is the only input) and nothing of it is read as samples.
 * Several recordings must resolve to one format and one rate (exit 2 otherwise); centre and start time are each one's own
 * (irdm_reset), except behind a front end, whose shift is fixed at creation: differing centres are refused there.  A
 * container whose rate is no multiple of 250 kHz, without --resample-to, gets one warning that names the flag.
 * --probe: one line per input on stdout and exit 0, before any device call (-v prints the same line on stderr before a run):
 *     probe: FILE container=wav|sigmf|sdriq|raw format=NAME rate=HZ|- centre=HZ|- start=SEC.NNNNNNNNN|- offset=BYTES bytes=BYTES data=PATH
 * --band-center HZ --decimate D (both or neither): the file is a wideband capture -- -r and -c describe it -- and the band
 * around HZ is shifted to the centre, low-passed and decimated by D (2 .. 16) on the GPU in front of the detector
 * (irdm_frontend_*): a 50 MS/s capture with --decimate 5 runs as a 10 MS/s stream centred at HZ (at the nearest multiple
 * of RATE / 65536 from -c, printed with -v).  --chunk stays in samples of the decimated stream.
 * --resample-to HZ: the same front end in its rational mode (irdm_frontend_create_resampler) -- the capture, described by -r
 * and -c, is resampled on the GPU to HZ = RATE * L / M (L <= 4096, M <= 65536, 24/25 <= M / L <= 16) in front of the detector:
 * for captures whose rate is no multiple of 250 kHz (2.4 MS/s, 11.2 MS/s, 61.44 MS/s ...), which the demodulator cannot
 * follow to the end of a frame, and for a clock that is off (10.025 MS/s declared 10 MS/s: 400/401, what --clock-check
 * suggests).  --band-center is optional with it (without: no shift); --decimate, --gpus N > 1 and HZ =
 * RATE are refused.  --chunk counts samples of the resampled stream.
 * Several recordings in one run: -f more than once and / or --files-from LIST (one "PATH" or "PATH START_SEC[.NNNNNNNNN]"
 * per line).  They go, in the order given, through ONE context, one front end and one pair of pinned buffers, with
 * irdm_reset / irdm_frontend_reset between them: what is paid once per process -- the HIP runtime, the context's device
 * buffers, its filters and rotator rows, the pinned allocations -- is paid once per run.  Every option holds for all of them;
 * each prints exactly what a run of its own prints (its lines, its "tagged N bursts total", its own ACARS and position
 * state and closing lines), to stdout one after the other or, with --out-dir DIR, to DIR/<basename>.out.
 * --start-time is the capture time of the first recording (instead of the wall clock at start: the timestamps, and with
 * them the whole output, then depend on the file alone); a later one starts at the time its list entry carries, else
 * at the wall clock.  A recording that cannot be opened or fails mid-way is reported and the others still run (exit 1).
 * --spectrum FILE: a band survey beside the lines -- the mean and the peak-hold spectrum of every R consecutive FFT frames of
 * the stream the detector sees (behind the front end: of the selected band), reduced on the GPU (option "spectrum_frames",
 * irdm_poll_spectrum), written to FILE: a 64-byte little-endian header -- "IRDMSPEC", u32 version 1, u32 n_bins, u32 R, u32
 * rate, f64 centre frequency, u64 start time in ns, 24 bytes of zeros; rate and centre are the context's, behind a front end
 * the band's -- then per row an irdm_spectrum_row_t (32 bytes), n_bins floats of mean, n_bins floats of peak (bin 0 = -rate / 2,
 * linear |X|^2).  --spectrum-frames R: frames per row, default round(rate / fft_size), about a second, at least 1.  stdout and
 * stderr are what they are without the flag.  With several recordings FILE must be `auto` and --out-dir given: each recording
 * leaves DIR/<basename>.spec.  --gpus N > 1 is refused.
 * --save-band FILE (with --decimate or --resample-to): the selected band, every sample the front end produces, written to FILE
 * beside the normal run (irdm_frontend_save) as a recording at the front end's output rate.  --save-format ci8|ci16|cf32, default
 * by FILE's extension (options.c:536-542: .cf32 .fc32 .cfile / .ci16 .cs16 / .ci8); ci8 and ci16 are round(x * G * 128) and
 * round(x * G * 32768), clipped to the format's range, --save-gain G (default 1, positive; cf32 takes 1 only).  A ci16 file
 * holds all 16 bits: read it back with --format ci16-full.  stdout and stderr are what they are without the flag, except, with
 * -v, a closing "saved band: ..." line that names the -r, -c and --format to read the file with, and, without -v, a warning
 * when components clipped.  --save-only: nothing but the file -- no context, no lines (irdm_frontend_run_device).  With several
 * recordings FILE must be `auto`, --out-dir given and --save-format named: each leaves DIR/<basename>.band.<format>.
 * A FILE ending in .sigmf-data (format by --save-format, default cf32) also gets FILE's .sigmf-meta on close: datatype, the
 * front end's output rate, the band's centre and the start time -- the pair reads back with -f alone.
 * --input-stats: one closing line per recording on stderr, after "tagged N bursts total" -- what the raw samples of the file
 * say about the recording, reduced on the GPU (option "input_stats"; behind a front end: of the capture, not of the band):
 *     input: N samples FMT; I dc %+.5f rms %.2f dBFS peak %.2f dBFS rails %llu (%.4f%%); Q ...; nonfinite %llu
 * dBFS relative to |x| = 1, -inf where there is nothing to take a logarithm of; rails: components at the converter's
 * negative or positive rail, and their share of N.  stdout and the rest of stderr are those of the run without the flag.
 * --diagnostic: the reference's setup check (main.c:444-480) in file form.  Implies --input-stats, suppresses the RAW / IDA
 * lines (frame_output.c:162, :205) and closes each recording with the reference's "Runtime: ... | Bursts: ... | Decoded: ...
 * | Noise: ... | Peak: ..." line and its guidance clause; the elapsed time is the recording's stream time, samples / rate.
 * Both work with --save-only (statistics without a context; no Runtime line: there is no detector) and are refused with
 * --gpus N > 1.
 * --clock-check: one closing line per recording on stderr, directly after "tagged N bursts total" -- the symbol clock error
 * the frames themselves show, estimated on the GPU (option "symbol_clock"), whatever -r said:
 *     clock: N frames; symbol clock %+.2f %% (quartiles %+.2f %% .. %+.2f %%); A not ok, B out of range
 * over the frames whose unique word passed; "clock: N frames; too few to judge" below 5 of them.  From 5 frames and a median
 * of 0.15 % on (between the 0.098 % that does no harm and the 0.25 % from which frames die half way) a clause follows:
 *     -- the samples look like R S/s, not R0: check -r, or --resample-to R0
 * R0 the grid rate the pipeline assumed, R rounded to 0.05 % of it (the estimator's resolution).  Behind a front end the
 * line describes the stream the detector sees; R and R0 are scaled back to the capture's -r.  stdout and the rest of
 * stderr are those of the run without the flag.  Refused with --gpus N > 1 and with --save-only (no context, no frames).
 * --fine-freq: every frame's carrier frequency estimated on the GPU from the frame's own samples (option "fine_freq": the line
 * of the fourth power, to about 1 Hz where the PLL's arithmetic is 10 to 30 Hz off), at the middle of the frame.  The
 * frequency field of every RAW: / IDA: line, and what --position, --acars and --parsed make of it, is then the refined one;
 * a frame whose estimate is out of range (beyond +-250 Hz of the downmixer's value; beyond +-300 Hz the estimator is blind) or
 * invalid keeps the PLL's value.  One closing line per recording on stderr, directly behind "clock:" and in front of "iq:":
 *     freq: N frames refined (K kept the PLL's value: A out of range, B invalid); refined - PLL median %+.0f Hz (quartiles %+.0f .. %+.0f)
 * or "freq: 0 frames".  -v says once "fine freq: carrier frequency from each frame's samples (+-250 Hz of the downmixer's)".
 * --save-bursts .meta files state the downmixer's frequency as before.  Refused with --gpus N > 1 and with --save-only.
 * --fine-time: every frame's arrival time refined on the GPU from the frame's own samples (option "fine_time": the phase of the
 * symbol rate's line in |x|^2, to about 0.3 us).  The time field of every RAW: / IDA: line, and what --position, --acars and
 * --parsed make of it, is then the time of the frame's first symbol -- the unique word's first on a downlink frame -- about
 * 0.73 ms later than without the flag, where it is the time the burst's magnitude crosses a threshold, which wanders by 6 to
 * 60 us with the noise.  A frame whose estimate is ambiguous (further than a quarter of a symbol from the correlator's) or
 * invalid takes the correlator's place instead, so every time of a run means the same.  One closing line per recording on
 * stderr, directly behind "freq:" and in front of "iq:":
 *     time: N frames refined (K kept the correlator's place: A ambiguous, B invalid); line - correlator median %+.2f samples (quartiles %+.2f .. %+.2f)
 * or "time: 0 frames".  At a rate that is no multiple of 250 kHz the frames' samples are not 4 us apart and the estimate
 * inherits the clock error: one warning names --burst-resample, with which nothing more is needed.  -v says once "fine time:
 * arrival time of each frame's first symbol from its samples".  --save-bursts .meta files state the downmixer's timestamp as
 * before.  Refused with --gpus N > 1 and with --save-only.
 * --burst-resample: at a rate that is no multiple of 250 kHz every burst's decimated row is resampled on the GPU to exactly
 * 250 000 samples/s before it is demodulated (option "burst_resample", on every member with --gpus N): frames come out whole,
 * their frequencies and times right, without resampling the whole stream.  With every input kind, behind --band-center /
 * --decimate / --resample-to (the front end's output rate is the rate it applies to), with --prime, --join, batches and
 * --gpus N.  -v says once "burst resample: F_IN -> 250000 samples/s per burst (L/M), 20 taps per phase", or "burst resample:
 * RATE is on the 250 kHz grid; nothing to do"; without -v a run at a rate on the grid prints what the run without the flag
 * prints.  The warning about a container rate off the grid is not printed.  A rate whose L exceeds 4096 exits 2 before
 * anything runs.  --clock-check behind it describes the resampled frames: its clause names RATE (1 + median) against the
 * declared RATE and says "check -r" only.  --save-bursts .meta files then state a true 250 000.
 * --swap-iq: the two components of every sample of every recording of the run are exchanged on the GPU where they arrive
 * (option "swap_iq", irdm_frontend_swap_iq, irdm_swap_iq_device), raw file or container, in front of --band-center /
 * --decimate / --resample-to: for a Q/I WAV, a SigMF file of the other convention, an inverting mixer.  Allowed with
 * --save-only, which then writes the corrected band.  The "input:" line describes the samples as processed: its I is the
 * file's second component (-v says so once).  Refused with --gpus N > 1.
 * --iq-check: one closing line per recording on stderr, after "tagged N bursts total" and a "clock:" line and before the
 * "input:" line -- whether the frames' bits make sense as they are or with I and Q exchanged (option "iq_sense"):
 *     iq: N frames decide (A IDA, B IRA, C IBC): R as recorded, X with I and Q exchanged
 * followed, when 9 in 10 of them say exchanged, by " -- the recording is I/Q-swapped (spectrum inverted): every payload is
 * wrong and every frequency mirrored about -c; run with --swap-iq" (with --swap-iq given: " -- the samples are I/Q-swapped
 * with --swap-iq in effect: remove it"), by " -- undecided" when neither sense has 9 in 10, and replaced by
 * "iq: N frames decide; too few to judge" below 5.  stdout and the rest of stderr are those of the run without the flag.
 * --diagnostic does not imply it.  Refused with --gpus N > 1 and with --save-only.
 * --scrub[=LOG2]: every cf32 sample of every recording of the run with a component that is not finite or lies beyond
 * +-2^LOG2 (0 .. 127, default 40) is zeroed on the GPU where it arrives (option "scrub", irdm_frontend_scrub,
 * irdm_scrub_device), behind --swap-iq's exchange and in front of everything else: one such sample -- the ragged tail of a
 * recorder that was killed, a division by zero upstream, corrupt bytes -- otherwise silences the detector for the rest of
 * the run.  Raw file or container; allowed with --save-only, which then writes the scrubbed band.  One closing line per
 * recording on stderr, after "tagged N bursts total" and the "clock:" and "iq:" lines and before the "input:" line, which
 * describes the samples as processed:
 *     scrub: N samples cf32, limit 2^40; none zeroed
 *     scrub: N samples cf32, limit 2^40; Z zeroed (A non-finite, B out-of-range components), first at sample F (T s), last at L (T s)
 * with positions in samples of the stream the pass sees (the capture in front of a front end) and times to the
 * microsecond at its rate; followed by " -- more than 0.1 % of the recording: is this file cf32 at all? check --format"
 * when that many were zeroed.  A recording of another format gets "scrub: ci16 samples are always finite; nothing to do".
 * stdout and the rest of stderr of a run over a clean file are those of the run without the flag.  --diagnostic does not
 * imply it.  Refused with --gpus N > 1.
 * --image-check: the receiver's I/Q imbalance (option "iq_moments", irdm_frontend_iq_moments: the second moments of every
 * sample of the stream as processed, reduced on the GPU).  A zero-IF receiver whose arms differ in gain and miss quadrature
 * leaves an image at -f of every signal at +f; the image of a strong burst is its conjugate, which the demodulator accepts
 * and prints as a RAW line with a mirrored frequency and a garbage payload.  One closing line per recording on stderr,
 * behind "iq:" and in front of "scrub:" and "input:":
 *     image: N samples; Q/I gain +0.999 dB, phase +4.99 deg: image at -22.8 dB; 10 of 24 frames are images of a stronger frame -- receiver I/Q imbalance: run with --iq-balance=0.999,4.99
 *     image: N samples; Q/I gain +0.000 dB, phase +0.00 deg: image below -60 dB; 0 of 12 frames are images
 *     image: 0 samples; nothing to judge
 * The clause behind "are images" appears when the image lies at -40 dB or above or any frame is an image; with
 * --iq-balance in effect it ends "with --iq-balance in effect: adjust it".  A frame j is an image when some frame i
 * lies within 1 ms of it, mirrors it about the capture's centre (-c) within 500 Hz (|f_i + f_j - 2 c| <= 500) and is at
 * least 10 dB stronger; the count is made on the host over all frames of the recording, whatever --chunk and --depth.
 * stdout and the rest of stderr are those of the run without the flag.  --diagnostic does not imply it.  Refused with
 * --gpus N > 1 and with --save-only.
 * --iq-balance=GAIN_DB,PHASE_DEG (this form only; |GAIN_DB| <= 6, |PHASE_DEG| <= 30): every sample of every recording of
 * the run is corrected on the GPU where it arrives, q' = alpha i + beta q with alpha = -tan(phase), beta = 1 / (gain
 * cos(phase)) (irdm_iq_balance, irdm_frontend_iq_balance, irdm_iq_balance_device): the context or the front end is
 * created as cf32 and takes the file's format as its wire format.  Raw file or container; allowed with --save-only /
 * --save-band, which then write the corrected band.  -v names the option and alpha, beta once.  Every closing line then
 * describes the stream as processed, which is cf32.  Refused with --gpus N > 1.
 * --dc-block[=LOG2] (only the = form takes the value; an integer 12 .. 24, default 20): a receiver's DC offset -- a tone at
 * the capture's centre, which costs every frame of the channel it falls into -- is tracked over aligned blocks of 2^LOG2
 * samples and subtracted on the GPU where the samples arrive (irdm_dc_block, irdm_frontend_dc_block,
 * irdm_dc_block_device): a block is corrected by the mean of the block in front of it, the first block by the seed, which
 * is the mean of the recording's first min(2^LOG2, recording) samples (irdm_dc_mean_host on the kept head, whatever --chunk
 * is; standard input too).  Behind --swap-iq's exchange, in front of --iq-balance, --scrub and any front end (the tone is
 * gone before the shift; --save-band / --save-only write the corrected band).  The context or the front end is created as
 * cf32 and takes the file's format as its wire format.  Every recording of a batch gets its own seed, state and line;
 * --join's parts are one stream.  With --prime the prefix runs through the pass like everything else, blocks counting from
 * the start of the prefix.  -v names the option once.  One closing line per recording on stderr, behind "image:" and in
 * front of "scrub:" and "input:", which then describes the samples as processed:
 *     dc: 3000000 samples cf32, 2 whole blocks of 2^20; seed I +0.03000 Q +0.01800; block means I +0.02999 .. +0.03001, Q +0.01799 .. +0.01801, last I +0.03000 Q +0.01800
 *     dc: 500000 samples cf32, 0 whole blocks of 2^20; seed I +0.03000 Q +0.01800 (the only correction)
 * (--save-only, which keeps no record of the blocks: "...; seed I .. Q ..; last I .. Q ..").  Refused with --gpus N > 1.
 * --prime: the detector finds nothing in a stream's first 512 FFT frames (0.37 to 0.70 s), which fill its noise history; a
 * file is all there, so every recording of the run is primed from its own head first (irdm_prime_host,
 * irdm_frontend_prime_host): the first 512 frames -- of a shorter recording the frames it has, repeated -- go through the
 * detector in front of the recording, and the recording then runs from its sample 0 with a full history.  Raw file,
 * container or standard input (the head, at most 64 MiB, is kept in memory and not read twice), behind --band-center /
 * --decimate / --resample-to (the head goes through the front end), in a batch after each reset.  --start-time and header
 * times still name the recording's first sample.  stdout gains the early frames; every closing line but "tagged" and every
 * side file (--spectrum, --save-band) is what the run without the flag writes.  -v: "primed: 512 frames from the first F".
 * A recording shorter than one frame runs unprimed with a warning.  Refused with --gpus N > 1 and with --save-only.
 * --join: every -f and every --files-from entry is a part of ONE recording, cut by the recorder (SDR#, HDSDR and SDR Console
 * start a new WAV every 2 or 4 GB): the parts' sample regions -- a container's data, a raw file whole -- run one behind the
 * other as one stream: one reset, one output (--out-dir names it after the first part; --spectrum and --save-band take plain
 * names), one set of closing lines, one ACARS / position state, chunks filled across the parts' edges wherever they fall.
 * Format and rate must agree, and the centres wherever headers give them (exit 2).  The start time is the first part's or
 * --start-time; a later part whose own time is more than 1 ms off the stream's gets one warning, no gap is inserted.  The
 * parts are read with one fread() thread.  -f - beside other inputs, --gpus N > 1 and --save-only are refused.  --prime with
 * --join primes from the joined stream's head.
 */
#include <err.h>
#include <errno.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>
#include <pthread.h>
#include <semaphore.h>
#include <sys/stat.h>
#include <sys/types.h>
#include <unistd.h>

#include "irdm_hip.h"

static const char *ext_of(const char *p)
{
    const char *d = strrchr(p, '.');
    return d ? d + 1 : "";
}

/* print every finished frame (frame_output_print, frame_output.c:160-199) and discard the other record queues */
static const char *g_save_dir;

/* --spectrum: the rows finished so far to the recording's .spec file */
static FILE *g_spec;
static float *g_spec_rows;
#define SPEC_POLL 8
static int spectrum_drain(irdm_pipeline_t *p)
{
    if (!g_spec) return 0;
    irdm_spectrum_row_t hdr[SPEC_POLL];
    const size_t n = (size_t)irdm_spectrum_bins(p);
    for (;;) {
        const int k = irdm_poll_spectrum(p, hdr, g_spec_rows, g_spec_rows + SPEC_POLL * n, SPEC_POLL);
        if (k < 0) return -1;
        if (k == 0) return 0;
        for (int i = 0; i < k; i++)
            if (fwrite(&hdr[i], sizeof hdr[i], 1, g_spec) != 1 || fwrite(g_spec_rows + (size_t)i * n, sizeof(float), n, g_spec) != n ||
                fwrite(g_spec_rows + (SPEC_POLL + (size_t)i) * n, sizeof(float), n, g_spec) != n)
                return -1;
    }
}

static int spectrum_open(const char *path, irdm_pipeline_t *p, int R, int rate, double centre)
{
    unsigned char h[64];
    const uint32_t w[4] = { 1u, (uint32_t)irdm_spectrum_bins(p), (uint32_t)R, (uint32_t)rate };
    const uint64_t t0 = irdm_start_time_ns(p);
    memset(h, 0, sizeof h);
    memcpy(h, "IRDMSPEC", 8);
    memcpy(h + 8, w, 16);
    memcpy(h + 24, &centre, 8);
    memcpy(h + 32, &t0, 8);
    g_spec = fopen(path, "wb");
    if (!g_spec) { perror(path); return -1; }
    return fwrite(h, sizeof h, 1, g_spec) == 1 ? 0 : -1;
}
/* where the lines of the recording at hand go: stdout, or with --out-dir its own file */
static FILE *g_out;

/* file reader thread: fills the two pinned buffers alternately.  A regular file is read by `n_slices` helper threads,
 * each with pread() on its own slice of the chunk (one thread copying out of the page cache moves 5-7 GB/s; the H2D copy
 * behind it runs at 50 GB/s); a pipe (stdin) is read with fread() as before. */
#define MAX_SLICES 16
typedef struct {
    int fd;
    char *dst;
    off_t off;
    size_t len, got;
    sem_t go, done;
    volatile int quit;
    pthread_t th;
} slice_t;

/* --join: the sample region of one input, [off, off + bytes) of f (bytes -1: to the end of the stream) */
typedef struct {
    FILE *f;
    off_t off;
    long long bytes;
} seg_t;

typedef struct {
    FILE *f;
    size_t bps, chunk;
    void *buf[2];
    size_t n[2];
    sem_t filled, empty;
    volatile int stop;
    int n_slices;               /* 0: fread */
    off_t pos, size;            /* the slices read [pos, size) of the file */
    long long remain;           /* fread: bytes left of a container's samples (-1: to the end of the stream) */
    /* fread, --prime on standard input: the head that was read for priming, handed out again in front of the stream */
    const char *pre;
    size_t pre_n;
    /* fread, --join: the regions behind the one at hand (f, remain), taken up one after the other in mid-chunk */
    const seg_t *segs;
    int n_seg, seg;
    slice_t sl[MAX_SLICES];
} reader_t;

static void *slice_main(void *arg)
{
    slice_t *s = arg;
    for (;;) {
        sem_wait(&s->go);
        if (s->quit) break;
        size_t g = 0;
        while (g < s->len) {
            const ssize_t r = pread(s->fd, s->dst + g, s->len - g, s->off + (off_t)g);
            if (r <= 0) break;
            g += (size_t)r;
        }
        s->got = g;
        sem_post(&s->done);
    }
    return NULL;
}

/* the next chunk of a regular file into dst: the slices in parallel; returns the samples read */
static size_t read_slices(reader_t *r, void *dst)
{
    size_t want = r->chunk * r->bps;
    if (r->pos >= r->size) return 0;
    if ((off_t)want > r->size - r->pos) want = (size_t)(r->size - r->pos);
    const int T = r->n_slices;
    /* ceil(want / T) rounded up to a page: T slices of `per` bytes always cover `want` (floor here handed out a
     * T + 1-th slice that has no thread when want / T was a multiple of 4096 and want % T != 0); the last slice used
     * takes what is left */
    const size_t per = ((want + (size_t)T - 1) / (size_t)T + 4095) & ~(size_t)4095;
    int used = 0;
    for (size_t o = 0; o < want && used < T; o += per, used++) {
        slice_t *s = &r->sl[used];
        s->dst = (char *)dst + o;
        s->off = r->pos + (off_t)o;
        s->len = (want - o < per || used == T - 1) ? want - o : per;
        sem_post(&s->go);
    }
    size_t got = 0;
    int shortfall = 0;
    for (int i = 0; i < used; i++) {
        sem_wait(&r->sl[i].done);
        if (!shortfall) got += r->sl[i].got;
        if (r->sl[i].got < r->sl[i].len) shortfall = 1;       /* (a file that shrank: what lies before the gap counts) */
    }
    r->pos += (off_t)got;
    return got / r->bps;
}

static void *reader_main(void *arg)
{
    reader_t *r = arg;
    for (int k = 0;; k ^= 1) {
        sem_wait(&r->empty);
        if (r->stop) break;
        if (r->n_slices) {
            r->n[k] = read_slices(r, r->buf[k]);
        } else {
            size_t got = 0;
            if (r->pre_n) {
                got = r->pre_n < r->chunk ? r->pre_n : r->chunk;
                memcpy(r->buf[k], r->pre, got * r->bps);
                r->pre += got * r->bps;
                r->pre_n -= got;
            }
            while (got < r->chunk) {
                size_t want = r->chunk - got;
                if (r->remain >= 0 && (unsigned long long)r->remain / r->bps < want) want = (size_t)((unsigned long long)r->remain / r->bps);
                const size_t g = want ? fread((char *)r->buf[k] + got * r->bps, r->bps, want, r->f) : 0;
                if (r->remain >= 0) r->remain -= (long long)(g * r->bps);
                got += g;
                if (got == r->chunk) break;
                /* this region is used up: the next one goes on in the same chunk (--join), or the stream ends here */
                if (r->seg + 1 >= r->n_seg) break;
                r->seg++;
                r->f = r->segs[r->seg].f;
                r->remain = r->segs[r->seg].bytes;
            }
            r->n[k] = got;
        }
        sem_post(&r->filled);
        if (r->n[k] < r->chunk) {                   /* short read: after it an explicit end marker */
            if (r->n[k] != 0) {
                sem_wait(&r->empty);
                if (!r->stop) { r->n[k ^ 1] = 0; sem_post(&r->filled); }
            }
            break;
        }
    }
    return NULL;
}

/* --gpus N: the stream goes through a group (irdm_group_*: chunk k on GPU k mod N, records merged in stream order by the
 * library); the polls below then read the group's queues */
static irdm_group_t *g_group;
#define irdm_poll_demods_packed(p, o, m) (g_group ? irdm_group_poll_demods_packed(g_group, o, m) : irdm_poll_demods_packed(p, o, m))
#define irdm_poll_demods(p, o, m) (g_group ? irdm_group_poll_demods(g_group, o, m) : irdm_poll_demods(p, o, m))
#define irdm_poll_bursts(p, o, m) (g_group ? irdm_group_poll_bursts(g_group, o, m) : irdm_poll_bursts(p, o, m))
#define irdm_poll_frames(p, o, s, m) (g_group ? irdm_group_poll_frames(g_group, o, s, m) : irdm_poll_frames(p, o, s, m))
#define irdm_poll_ida_packed(p, o, m) (g_group ? irdm_group_poll_ida_packed(g_group, o, m) : irdm_poll_ida_packed(p, o, m))
#define irdm_poll_ida(p, o, m) (g_group ? irdm_group_poll_ida(g_group, o, m) : irdm_poll_ida(p, o, m))
#define irdm_poll_frame_packed(p, o, m) (g_group ? irdm_group_poll_frame_packed(g_group, o, m) : irdm_poll_frame_packed(p, o, m))
#define irdm_poll_decoded(p, o, m) (g_group ? irdm_group_poll_decoded(g_group, o, m) : irdm_poll_decoded(p, o, m))

/* --input-stats / --diagnostic */
static int g_input_stats, g_diag;
/* --clock-check */
static int g_clock;
/* --fine-freq */
static int g_fine;
/* --fine-time */
static int g_ftime;
/* --iq-check, --swap-iq */
static int g_iq, g_swap;
/* --burst-resample */
static int g_burst_resample;
/* --scrub[=LOG2] */
static int g_scrub, g_scrub_log2 = IRDM_SCRUB_DEFAULT_LOG2;
/* --image-check, --iq-balance=G,P */
static int g_image, g_bal;
static double g_bal_gain, g_bal_phase;
/* --image-check: time, frequency and magnitude of every frame of the recording whose unique word was accepted */
typedef struct { uint64_t t; double f; float mag; } img_frame_t;
static img_frame_t *g_img;
static size_t g_n_img, g_cap_img;
static unsigned long long g_n_demods;       /* frames the demodulator accepted, this recording */

static const char *format_name(int fmt)
{
    switch (fmt) {
    case IRDM_FMT_CF32: return "cf32";
    case IRDM_FMT_CI16: return "ci16";
    case IRDM_FMT_CI16_FULL: return "ci16-full";
    case IRDM_FMT_SC16Q11: return "sc16q11";
    case IRDM_FMT_CU8: return "cu8";
    case IRDM_FMT_CI32: return "ci32";
    case IRDM_FMT_CI32_24: return "ci32-24";
    default: return "ci8";
    }
}

/* the closing "input:" line of a recording */
static void input_line(const irdm_input_stats_t *st, int fmt)
{
    const double n = (double)st->n_samples;
    fprintf(stderr, "input: %llu samples %s;", (unsigned long long)st->n_samples, format_name(fmt));
    for (int k = 0; k < 2; k++) {
        const double fin = n - (double)st->n_nonfinite[k];
        const double dc = fin > 0 ? st->sum[k] / fin : 0.0;
        const double ms = fin > 0 ? st->sum_sq[k] / fin : 0.0;
        const unsigned long long rails = (unsigned long long)(st->n_rail_lo[k] + st->n_rail_hi[k]);
        fprintf(stderr, " %c dc %+.5f rms %.2f dBFS peak %.2f dBFS rails %llu (%.4f%%);", k ? 'Q' : 'I', dc,
                ms > 0 ? 10.0 * log10(ms) : -INFINITY, st->abs_max[k] > 0 ? 20.0 * log10((double)st->abs_max[k]) : -INFINITY,
                rails, n > 0 ? 100.0 * (double)rails / n : 0.0);
    }
    fprintf(stderr, " nonfinite %llu\n", (unsigned long long)(st->n_nonfinite[0] + st->n_nonfinite[1]));
}

/* the closing "clock:" line of a recording.  nominal: the rate the detector's stream was taken for (its context's rate);
 * capture: the -r of the file in front of it (the same without a front end) */
static void clock_line(const irdm_symbol_clock_t *sc, double nominal, double capture, int front_end, int per_burst)
{
    if (sc->frames_used < 5) {
        fprintf(stderr, "clock: %llu frames; too few to judge\n", (unsigned long long)sc->frames_used);
        return;
    }
    fprintf(stderr, "clock: %llu frames; symbol clock %+.2f %% (quartiles %+.2f %% .. %+.2f %%); %llu not ok, %llu out of range",
            (unsigned long long)sc->frames_used, 100.0 * sc->median, 100.0 * sc->q25, 100.0 * sc->q75,
            (unsigned long long)sc->frames_not_ok, (unsigned long long)sc->frames_out_of_range);
    if (per_burst && fabs(sc->median) >= 0.0015 - 1e-12) {
        /* --burst-resample at a rate off the grid: the frames were resampled from the declared rate to 250 kHz, so what is
         * left is the error of the declared rate itself, in steps of 0.05 % of it */
        const double step = capture / 2000.0;
        fprintf(stderr, " -- the samples look like %.0f S/s, not %.0f: check -r", floor(capture * (1.0 + sc->median) / step + 0.5) * step,
                capture);
    } else if (fabs(sc->median) >= 0.0015 - 1e-12) {
        /* the grid rate the pipeline assumed and the rate the samples look like, both as rates of the capture; the latter in
         * steps of 0.05 % of the former */
        const double grid = sc->implied_rate_hz / (1.0 + sc->median), scale = capture / nominal;
        const double step = grid * scale / 2000.0;
        const double looks = floor(sc->implied_rate_hz * scale / step + 0.5) * step;
        fprintf(stderr, " -- the samples look like %.0f S/s, not %.0f: check -r", looks, grid * scale);
        if (!front_end) fprintf(stderr, ", or --resample-to %.0f", grid);
    }
    fprintf(stderr, "\n");
}

/* the closing "iq:" line of a recording */
static void iq_line(const irdm_iq_sense_t *q)
{
    const unsigned long long d = q->votes_recorded + q->votes_exchanged;
    if (q->verdict == IRDM_IQ_TOO_FEW) {
        fprintf(stderr, "iq: %llu frames decide; too few to judge\n", d);
        return;
    }
    fprintf(stderr, "iq: %llu frames decide (%llu IDA, %llu IRA, %llu IBC): %llu as recorded, %llu with I and Q exchanged", d,
            (unsigned long long)(q->kind_recorded[2] + q->kind_exchanged[2]), (unsigned long long)(q->kind_recorded[0] + q->kind_exchanged[0]),
            (unsigned long long)(q->kind_recorded[1] + q->kind_exchanged[1]), (unsigned long long)q->votes_recorded,
            (unsigned long long)q->votes_exchanged);
    if (q->verdict == IRDM_IQ_EXCHANGED && g_swap) fprintf(stderr, " -- the samples are I/Q-swapped with --swap-iq in effect: remove it");
    else if (q->verdict == IRDM_IQ_EXCHANGED)
        fprintf(stderr, " -- the recording is I/Q-swapped (spectrum inverted): every payload is wrong and every frequency mirrored about -c; run with --swap-iq");
    else if (q->verdict == IRDM_IQ_MIXED) fprintf(stderr, " -- undecided");
    fprintf(stderr, "\n");
}

/* --dc-block[=LOG2] */
static int g_dc, g_dc_log2 = IRDM_DC_DEFAULT_LOG2;

/* the closing "dc:" line of a recording; range: the smallest and largest block mean are known */
static void dc_line(const irdm_dc_stats_t *st, int fmt, int range)
{
    fprintf(stderr, "dc: %llu samples %s, %llu whole block%s of 2^%d; seed I %+.5f Q %+.5f", (unsigned long long)st->n_samples,
            format_name(fmt), (unsigned long long)st->n_blocks, st->n_blocks == 1 ? "" : "s", st->block_log2, (double)st->seed_i,
            (double)st->seed_q);
    if (!st->n_blocks) fprintf(stderr, " (the only correction)\n");
    else if (!range) fprintf(stderr, "; last I %+.5f Q %+.5f\n", (double)st->last_i, (double)st->last_q);
    else
        fprintf(stderr, "; block means I %+.5f .. %+.5f, Q %+.5f .. %+.5f, last I %+.5f Q %+.5f\n", (double)st->min_i, (double)st->max_i,
                (double)st->min_q, (double)st->max_q, (double)st->last_i, (double)st->last_q);
}

/* the closing "scrub:" line of a recording; rate: that of the stream the pass saw */
static void scrub_line(const irdm_scrub_stats_t *st, int fmt, double rate)
{
    if (!st->active) {
        fprintf(stderr, "scrub: %s samples are always finite; nothing to do\n", format_name(fmt));
        return;
    }
    fprintf(stderr, "scrub: %llu samples %s, limit 2^%d;", (unsigned long long)st->n_samples, format_name(fmt), st->limit_log2);
    if (!st->n_zeroed) {
        fprintf(stderr, " none zeroed\n");
        return;
    }
    fprintf(stderr, " %llu zeroed (%llu non-finite, %llu out-of-range components), first at sample %llu (%.6f s), last at %llu (%.6f s)",
            (unsigned long long)st->n_zeroed, (unsigned long long)st->n_nonfinite, (unsigned long long)st->n_over,
            (unsigned long long)st->first, (double)st->first / rate, (unsigned long long)st->last, (double)st->last / rate);
    if ((double)st->n_zeroed * 1000.0 > (double)st->n_samples)
        fprintf(stderr, " -- more than 0.1 %% of the recording: is this file cf32 at all? check --format");
    fprintf(stderr, "\n");
}

static void image_note(uint64_t t, double f, float mag, int ok)
{
    if (!ok) return;
    if (g_n_img == g_cap_img) {
        g_cap_img = g_cap_img ? 2 * g_cap_img : 4096;
        g_img = realloc(g_img, g_cap_img * sizeof(*g_img));
        if (!g_img) { fprintf(stderr, "--image-check: out of memory\n"); exit(1); }
    }
    g_img[g_n_img].t = t;
    g_img[g_n_img].f = f;
    g_img[g_n_img].mag = mag;
    g_n_img++;
}

static int image_by_time(const void *a, const void *b)
{
    const img_frame_t *x = a, *y = b;
    if (x->t != y->t) return x->t < y->t ? -1 : 1;
    return x->f < y->f ? -1 : (x->f > y->f ? 1 : 0);
}

/* frames that are images of a stronger frame: |t_i - t_j| <= 1 ms, |f_i + f_j - 2 c| <= 500 Hz, mag_j <= mag_i - 10 dB.  Over
 * all frames of the recording, sorted by time: the count does not depend on how the stream was cut or queued. */
static size_t image_count(double centre)
{
    size_t images = 0;
    qsort(g_img, g_n_img, sizeof(*g_img), image_by_time);
    for (size_t j = 0, lo = 0; j < g_n_img; j++) {
        while (g_img[j].t - g_img[lo].t > 1000000u) lo++;
        for (size_t i = lo; i < g_n_img && g_img[i].t <= g_img[j].t + 1000000u; i++)
            if (fabs(g_img[i].f + g_img[j].f - 2.0 * centre) <= 500.0 && g_img[j].mag <= g_img[i].mag - 10.0f) { images++; break; }
    }
    return images;
}

/* the closing "image:" line of a recording */
static void image_line(const irdm_iq_moments_t *m, double centre)
{
    const size_t images = image_count(centre);
    if (!m->n_samples) {
        fprintf(stderr, "image: 0 samples; nothing to judge\n");
        return;
    }
    if (!m->valid) {
        fprintf(stderr, "image: %llu samples; no variance in I or Q; nothing to judge\n", (unsigned long long)m->n_samples);
        return;
    }
    fprintf(stderr, "image: %llu samples; Q/I gain %+.3f dB, phase %+.2f deg: ", (unsigned long long)m->n_samples, m->gain_db, m->phase_deg);
    if (m->image_db >= -60.0) fprintf(stderr, "image at %.1f dB", m->image_db);
    else fprintf(stderr, "image below -60 dB");
    fprintf(stderr, "; %zu of %zu frames are images", images, g_n_img);
    if (m->image_db >= -40.0 || images) {
        fprintf(stderr, " of a stronger frame -- receiver I/Q imbalance: ");
        if (g_bal) fprintf(stderr, "with --iq-balance in effect: adjust it");
        else fprintf(stderr, "run with --iq-balance=%.3f,%.2f", m->gain_db, m->phase_deg);
    }
    fprintf(stderr, "\n");
}

/* the closing "freq:" line of a recording (--fine-freq) */
static void freq_line(const irdm_fine_freq_summary_t *ff)
{
    if (ff->frames_seen - ff->frames_not_ok == 0) {
        fprintf(stderr, "freq: 0 frames\n");
        return;
    }
    fprintf(stderr, "freq: %llu frames refined (%llu kept the PLL's value: %llu out of range, %llu invalid); "
            "refined - PLL median %+.0f Hz (quartiles %+.0f .. %+.0f)\n",
            (unsigned long long)ff->frames_applied, (unsigned long long)(ff->frames_out_of_range + ff->frames_invalid),
            (unsigned long long)ff->frames_out_of_range, (unsigned long long)ff->frames_invalid, ff->median, ff->q25, ff->q75);
}

/* the closing "time:" line of a recording (--fine-time) */
static void time_line(const irdm_fine_time_summary_t *ft)
{
    if (ft->frames_seen - ft->frames_not_ok == 0) {
        fprintf(stderr, "time: 0 frames\n");
        return;
    }
    fprintf(stderr, "time: %llu frames refined (%llu kept the correlator's place: %llu ambiguous, %llu invalid); "
            "line - correlator median %+.2f samples (quartiles %+.2f .. %+.2f)\n",
            (unsigned long long)ft->frames_applied, (unsigned long long)(ft->frames_ambiguous + ft->frames_invalid),
            (unsigned long long)ft->frames_ambiguous, (unsigned long long)ft->frames_invalid, ft->median, ft->q25, ft->q75);
}

/* --diagnostic: the reference's closing status line (main.c:444-480) over the recording's stream time */
static void diagnostic_line(double elapsed, unsigned long det, unsigned long sub, float noise_floor, float peak_signal)
{
    const int runtime = (int)elapsed;
    const double per_min = elapsed > 0 ? det * 60.0 / elapsed : 0;
    const double ok_avg = det > 0 ? 100.0 * sub / det : 0;
    fprintf(stderr, "Runtime: %02d:%02d:%02d  |  Bursts: %lu detected (%.1f/min)  |  Decoded: %lu (ok_avg: %.0f%%)  |  "
                    "Noise: %.1f dBFS/Hz  |  Peak: %.1f dB  ",
            runtime / 3600, runtime % 3600 / 60, runtime % 60, det, per_min, sub, ok_avg, noise_floor, peak_signal);
    if (det == 0 && elapsed > 120) fprintf(stderr, "| No bursts detected - check antenna");
    else if (ok_avg >= 70 && per_min >= 3) fprintf(stderr, "| Setup looks good (gap: %.1f dB)", peak_signal - noise_floor);
    else if (ok_avg < 70 && det > 10) fprintf(stderr, "| Low decode rate - try adjusting gain");
    else if (ok_avg >= 70 && per_min < 3 && elapsed > 60) fprintf(stderr, "| Good decode rate but low burst count");
    fprintf(stderr, "\n");
}

/* --parsed (main.c:322-331): per frame the IDA line where ida_decode() succeeds, the RAW line otherwise */
static int g_parsed;
/* --acars / --acars-json (main.c:357-361): IDA reassembly, SBD and ACARS on the host for the whole stream; RAW lines are
 * suppressed (frame_output.c:162-168) */
static irdm_ida_reasm_t *g_reasm;
static irdm_acars_t *g_acars;
static char g_acars_line[256 * (IRDM_RAW_LINE_MAX + IRDM_ACARS_LINE_MAX)];
/* --position (main.c:333-343, :506-519): every frame's IRA record into the Doppler solver, its POSITION lines on stderr */
static irdm_doppler_t *g_dop;
static char g_dop_text[1 << 20];

static void position_out(long long len)
{
    if (len < 0) { fprintf(stderr, "--position: formatting failed\n"); exit(1); }
    if (len > 0) fwrite(g_dop_text, 1, (size_t)len, stderr);
}

static void drain(irdm_pipeline_t *p, irdm_demod_t *d, const char *file_info, uint64_t *t0, char *line, size_t cap)
{
    int n;
    if (!g_save_dir) {
        /* RAW lines need no LLRs: compact records (hard bits 8 per byte), 176 bytes per frame instead of 4.5 KB */
        static irdm_demod_packed_t dp[256];
        static irdm_ida_packed_t ip[256];
        static irdm_frame_packed_t fp[256];
        while ((n = irdm_poll_demods_packed(p, dp, 256)) > 0) {
            long long len;
            g_n_demods += (unsigned long long)n;
            if (g_image)
                for (int i = 0; i < n; i++) image_note(dp[i].timestamp, dp[i].center_frequency, dp[i].magnitude, dp[i].ok);
            if (g_dop) {
                /* one compact frame_decode() record per compact frame record, decoded on the GPU (option frame_records) */
                if (irdm_poll_frame_packed(p, fp, n) != n) { fprintf(stderr, "--position: frame records out of step\n"); exit(1); }
                position_out(irdm_format_doppler_packed_batch(g_dop, dp, fp, n, g_dop_text, sizeof g_dop_text));
            }
            if (g_acars) {
                if (irdm_poll_ida_packed(p, ip, n) != n) { fprintf(stderr, "--acars: IDA records out of step\n"); exit(1); }
                len = irdm_format_acars_packed_batch(g_reasm, g_acars, dp, ip, n, g_parsed, t0, g_acars_line, sizeof g_acars_line);
                if (len < 0) { fprintf(stderr, "--acars: formatting failed\n"); exit(1); }
                if (len > 0) fwrite(g_acars_line, 1, (size_t)len, g_out);
                continue;
            } else if (g_parsed) {
                /* one compact IDA record per compact frame record, decoded on the GPU (option parsed_records) */
                if (irdm_poll_ida_packed(p, ip, n) != n) { fprintf(stderr, "--parsed: IDA records out of step\n"); exit(1); }
                len = irdm_format_parsed_packed_batch(dp, ip, n, file_info, t0, line, cap);
            } else {
                len = irdm_format_raw_packed_batch(dp, n, file_info, t0, line, cap);   /* one write per batch */
            }
            if (len > 0 && !g_diag) fwrite(line, 1, (size_t)len, g_out);
        }
    }
    if (g_clock) {
        /* (the summary is the library's; the per-frame records are not printed) */
        static irdm_clock_est_t ce[256];
        while (irdm_poll_symbol_clock(p, ce, 256) > 0) {}
    }
    if (g_fine) {
        /* (likewise; the demodulator records carry the refined frequency) */
        static irdm_fine_freq_t ff[256];
        while (irdm_poll_fine_freq(p, ff, 256) > 0) {}
    }
    if (g_ftime) {
        /* (likewise; the demodulator records carry the refined time) */
        static irdm_fine_time_t ft[256];
        while (irdm_poll_fine_time(p, ft, 256) > 0) {}
    }
    if (g_iq) {
        /* (likewise: the summary is the library's) */
        static irdm_iq_vote_t iv[256];
        while (irdm_poll_iq_votes(p, iv, 256) > 0) {}
    }
    static irdm_ida_t ida[256];
    static irdm_decoded_t dec[256];
    while ((n = irdm_poll_demods(p, d, 256)) > 0) {
        long long len = 0;
        g_n_demods += (unsigned long long)n;
        if (g_image)
            for (int i = 0; i < n; i++) image_note(d[i].timestamp, d[i].center_frequency, d[i].magnitude, d[i].ok);
        if (g_dop) {
            /* the full-record path (--save-bursts): option decode_frames, one irdm_decoded_t per frame record */
            if (irdm_poll_decoded(p, dec, n) != n) { fprintf(stderr, "--position: frame records out of step\n"); exit(1); }
            position_out(irdm_format_doppler_batch(g_dop, dec, n, g_dop_text, sizeof g_dop_text));
        }
        if (g_acars) {
            if (irdm_poll_ida(p, ida, n) != n) { fprintf(stderr, "--acars: IDA records out of step\n"); exit(1); }
            len = irdm_format_acars_batch(g_reasm, g_acars, d, ida, n, g_parsed, t0, g_acars_line, sizeof g_acars_line);
            if (len < 0) { fprintf(stderr, "--acars: formatting failed\n"); exit(1); }
            if (len > 0) fwrite(g_acars_line, 1, (size_t)len, g_out);
            continue;
        } else if (g_parsed) {
            /* the full-record path (--save-bursts): option decode_ida, one irdm_ida_t per frame record */
            if (irdm_poll_ida(p, ida, n) != n) { fprintf(stderr, "--parsed: IDA records out of step\n"); exit(1); }
            for (int i = 0; i < n && len >= 0; i++) {
                const int l = ida[i].ok ? irdm_format_ida(&ida[i], t0, line + len, cap - (size_t)len)
                                        : irdm_format_raw(&d[i], file_info, t0, line + len, cap - (size_t)len);
                len = l < 0 ? -1 : len + l;
            }
        } else {
            len = irdm_format_raw_batch(d, n, file_info, t0, line, cap);     /* one write per batch */
        }
        if (len > 0 && !g_diag) fwrite(line, 1, (size_t)len, g_out);
    }
    irdm_burst_t tmp[256];
    while (irdm_poll_bursts(p, tmp, 256) > 0) {}
    if (g_save_dir) {
        /* every frame handed to the demodulator is saved, accepted or not (qpsk_demod.c:443-445, :468-470) */
        static irdm_frame_info_t fi[16];
        static float fs[16 * 2 * IRDM_MAX_FRAME_SAMPLES];
        while ((n = irdm_poll_frames(p, fi, fs, 16)) > 0)
            for (int i = 0; i < n; i++)
                if (fi[i].drop_reason == 0) irdm_save_burst(&fi[i], fs + (size_t)i * 2 * IRDM_MAX_FRAME_SAMPLES, g_save_dir);
    } else {
        irdm_frame_info_t fi[256];
        while (irdm_poll_frames(p, fi, NULL, 256) > 0) {}
    }
}

static double now_s(void)
{
    struct timespec ts;
    clock_gettime(CLOCK_MONOTONIC, &ts);
    return (double)ts.tv_sec + 1e-9 * (double)ts.tv_nsec;
}

/* SEC[.NNNNNNNNN] -> nanoseconds; 0 ok, -1 malformed */
static int parse_time(const char *v, long long *sec, long long *nsec)
{
    char *end;
    *sec = strtoll(v, &end, 10);
    *nsec = 0;
    if (end == v) return -1;
    if (*end == '.') {
        int digits = 0;
        for (end++; *end >= '0' && *end <= '9' && digits < 9; end++, digits++) *nsec = *nsec * 10 + (*end - '0');
        for (; digits < 9; digits++) *nsec *= 10;
    }
    return *end ? -1 : 0;
}

/* the recordings of a run, in the order given */
typedef struct {
    char *path;
    uint64_t start_ns;          /* capture time (--start-time for the first, the list's second column, else a container's
                                 * header); 0: the wall clock */
    /* what irdm_recording_probe said (resolve_input): kind 0 a raw file, > 0 a container, -1 a malformed one (err says why) */
    int kind, fmt, hdr_rate;
    size_t bps;
    double centre;              /* the recording's centre frequency: -c, else the header's, else -c's default */
    irdm_recording_info_t *info;
    char *err;
} input_t;
static input_t *g_in;
static int g_n_in;

static void add_input(const char *path, uint64_t start_ns)
{
    g_in = realloc(g_in, sizeof(*g_in) * (size_t)(g_n_in + 1));
    if (!g_in) errx(1, "out of memory");
    memset(&g_in[g_n_in], 0, sizeof(*g_in));
    if (!(g_in[g_n_in].path = strdup(path))) errx(1, "out of memory");
    g_in[g_n_in++].start_ns = start_ns;
}

/* --files-from LIST: one "PATH" or "PATH START_SEC[.NNNNNNNNN]" per line; empty lines are skipped */
static int read_list(const char *list)
{
    FILE *lf = fopen(list, "r");
    if (!lf) { perror(list); return -1; }
    char ln[4352];
    int no = 0;
    while (fgets(ln, sizeof ln, lf)) {
        no++;
        size_t n = strlen(ln);
        while (n && (ln[n - 1] == '\n' || ln[n - 1] == '\r' || ln[n - 1] == ' ' || ln[n - 1] == '\t')) ln[--n] = 0;
        if (!n) continue;
        uint64_t start_ns = 0;
        char *sp = strrchr(ln, ' ');
        long long sec, nsec;
        /* (a last column that reads as a time is one; a path with blanks and no time stays a path) */
        if (sp && sp[1] && parse_time(sp + 1, &sec, &nsec) == 0 && sec >= 0) {
            start_ns = (uint64_t)sec * 1000000000ULL + (uint64_t)nsec;
            while (sp > ln && (sp[-1] == ' ' || sp[-1] == '\t')) sp--;
            *sp = 0;
        }
        if (!ln[0]) { fprintf(stderr, "%s:%d: no path\n", list, no); fclose(lf); return -1; }
        add_input(ln, start_ns);
    }
    fclose(lf);
    return 0;
}

/* the sample format of a recording: --format, else its extension (options.c:533-544); -1: --format names none */
static int format_of(const char *format, const char *path, size_t *bps)
{
    const int given = format != NULL;
    if (!format) format = ext_of(path);
    *bps = 2;
    if (!strcmp(format, "cf32") || !strcmp(format, "fc32") || !strcmp(format, "cfile")) { *bps = 8; return IRDM_FMT_CF32; }
    if (!strcmp(format, "ci16") || !strcmp(format, "cs16")) { *bps = 4; return IRDM_FMT_CI16; }
    /* full-precision int16 (the reference's SoapySDR CS16 and bladeRF live conversions): by --format only, the extension
     * autodetect above is the reference's */
    if (given && !strcmp(format, "ci16-full")) { *bps = 4; return IRDM_FMT_CI16_FULL; }
    if (given && !strcmp(format, "sc16q11")) { *bps = 4; return IRDM_FMT_SC16Q11; }
    /* rtl_sdr's unsigned bytes: by --format, or by an extension the reference does not know (it would read such a file as
     * ci8, which is never right) */
    if (!strcmp(format, "cu8") || (!given && !strcmp(format, "u8"))) return IRDM_FMT_CU8;
    /* interleaved int32, by --format only */
    if (given && !strcmp(format, "ci32")) { *bps = 8; return IRDM_FMT_CI32; }
    if (given && !strcmp(format, "ci32-24")) { *bps = 8; return IRDM_FMT_CI32_24; }
    return IRDM_FMT_CI8;
}

static const char *container_name(int kind)
{
    return kind == IRDM_CONTAINER_WAV ? "wav" : (kind == IRDM_CONTAINER_SIGMF ? "sigmf" : (kind == IRDM_CONTAINER_SDRIQ ? "sdriq" : "raw"));
}

/* Probe one input (container: -1 by extension, IRDM_CONTAINER_NONE never, else the forced kind) and settle its format, centre
 * and start time: an explicit -c and an explicit start time win over the header. */
static void resolve_input(input_t *in, int container, const char *format, double freq, int freq_given)
{
    in->kind = 0;
    in->centre = freq;
    if (container != IRDM_CONTAINER_NONE && strcmp(in->path, "-") != 0) {
        char msg[1024];
        irdm_recording_info_t *info = calloc(1, sizeof(*info));
        if (!info) errx(1, "out of memory");
        const int rc = irdm_recording_probe(in->path, container < 0 ? 0 : container, info, msg, sizeof msg);
        if (rc == 0) {
            in->kind = info->kind;
            in->info = info;
            in->fmt = info->format;
            in->bps = irdm_format_bytes(info->format);
            in->hdr_rate = info->sample_rate;
            if (info->has_center && !freq_given) in->centre = info->center_frequency;
            if (info->has_start && in->start_ns == 0) in->start_ns = info->start_time_ns;
            return;
        }
        free(info);
        if (rc < 0) {
            in->kind = -1;
            if (!(in->err = strdup(msg))) errx(1, "out of memory");
            return;
        }
    }
    in->fmt = format_of(format, in->path, &in->bps);
}

/* the probe line of an input (--probe: stdout; -v: stderr) */
static void probe_line(FILE *o, const input_t *in, double rate)
{
    char centre[64] = "-", start[64] = "-", r[32] = "-";
    if (in->kind > 0) {
        const irdm_recording_info_t *i = in->info;
        if (i->has_center) snprintf(centre, sizeof centre, "%.0f", i->center_frequency);
        if (i->has_start) snprintf(start, sizeof start, "%llu.%09llu", (unsigned long long)(i->start_time_ns / 1000000000ULL),
                                   (unsigned long long)(i->start_time_ns % 1000000000ULL));
        fprintf(o, "probe: %s container=%s format=%s rate=%d centre=%s start=%s offset=%llu bytes=%llu data=%s\n", in->path,
                container_name(i->kind), format_name(i->format), i->sample_rate, centre, start, (unsigned long long)i->data_offset,
                (unsigned long long)i->data_bytes, i->data_path);
        return;
    }
    struct stat sb;
    unsigned long long size = 0;
    if (strcmp(in->path, "-") != 0 && stat(in->path, &sb) == 0) size = (unsigned long long)sb.st_size;
    if (rate > 0) snprintf(r, sizeof r, "%.0f", rate);
    fprintf(o, "probe: %s container=raw format=%s rate=%s centre=- start=- offset=0 bytes=%llu data=%s\n", in->path, format_name(in->fmt), r,
            size - size % in->bps, in->path);
}

static const char *base_of(const char *p);

/* --save-band: its format by name (--save-format) or by the file's extension (options.c:536-542); -1: neither names one */
static int save_format_of(const char *name, const char *path)
{
    const char *f = name ? name : ext_of(path);
    if (!strcmp(f, "cf32") || (!name && (!strcmp(f, "fc32") || !strcmp(f, "cfile")))) return IRDM_FMT_CF32;
    if (!strcmp(f, "ci16") || (!name && !strcmp(f, "cs16"))) return IRDM_FMT_CI16;
    if (!strcmp(f, "ci8")) return IRDM_FMT_CI8;
    return -1;
}

/* --save-band: the front end's sink.  A short write is remembered, reported once the recording ends, and the rest of the
 * recording's bytes are dropped; the run itself goes on. */
static struct { FILE *f; int failed; } g_band;

static int band_sink(void *user, const void *bytes, size_t n)
{
    (void)user;
    if (g_band.f && !g_band.failed && fwrite(bytes, 1, n, g_band.f) != n) g_band.failed = 1;
    return 0;
}

static const char *save_name(int fmt) { return fmt == IRDM_FMT_CF32 ? "cf32" : (fmt == IRDM_FMT_CI16 ? "ci16" : "ci8"); }

static int has_suffix_nocase(const char *s, const char *suffix)
{
    const size_t n = strlen(s), m = strlen(suffix);
    return n >= m && strcasecmp(s + n - m, suffix) == 0;
}

/* --save-band FILE.sigmf-data: FILE's .sigmf-meta beside it -- what -f FILE.sigmf-data needs to run the band alone.
 * start_ns 0 (no capture time known): no core:datetime. */
static int band_write_meta(const char *save_band, int fmt, int rate, double centre, uint64_t start_ns)
{
    char path[4608];
    const size_t n = strlen(save_band);
    snprintf(path, sizeof path, "%.*s%s", (int)(n - 4), save_band, save_band[n - 4] == 'D' ? "META" : "meta");
    FILE *m = fopen(path, "w");
    if (!m) { perror(path); return 1; }
    fprintf(m, "{\n  \"global\": {\n    \"core:datatype\": \"%s\",\n    \"core:sample_rate\": %d,\n    \"core:version\": \"1.0.0\",\n"
               "    \"core:recorder\": \"iridium-sniffer-hip --save-band\"\n  },\n  \"captures\": [\n    {\n      \"core:sample_start\": 0,\n"
               "      \"core:frequency\": %.17g",
            fmt == IRDM_FMT_CF32 ? "cf32_le" : (fmt == IRDM_FMT_CI16 ? "ci16_le" : "ci8"), rate, centre);
    if (start_ns) {
        const time_t sec = (time_t)(start_ns / 1000000000ULL);
        struct tm tm;
        char day[32];
        gmtime_r(&sec, &tm);
        strftime(day, sizeof day, "%Y-%m-%dT%H:%M:%S", &tm);
        fprintf(m, ",\n      \"core:datetime\": \"%s.%09lluZ\"", day, (unsigned long long)(start_ns % 1000000000ULL));
    }
    fprintf(m, "\n    }\n  ],\n  \"annotations\": []\n}\n");
    return fclose(m) != 0;
}

static int band_open(const char *save_band, const char *out_dir, const char *file, int fmt)
{
    char path[4608];
    if (!strcmp(save_band, "auto")) snprintf(path, sizeof path, "%s/%s.band.%s", out_dir, base_of(file), save_name(fmt));
    else snprintf(path, sizeof path, "%s", save_band);
    g_band.failed = 0;
    g_band.f = fopen(path, "wb");
    if (!g_band.f) { perror(path); return -1; }
    return 0;
}

/* the recording is complete: close it, say what went wrong or, with -v, what was written.  0 ok, 1 the file is not whole */
static int band_close(irdm_frontend_t *fe, const char *file, int fmt, float gain, int verbose, double centre)
{
    int rc = g_band.failed;
    if (fclose(g_band.f) != 0) rc = 1;
    g_band.f = NULL;
    if (rc) fprintf(stderr, "--save-band: %s: writing the band failed\n", file);
    irdm_band_stats_t st;
    if (irdm_frontend_save_stats(fe, &st) != 0) { fprintf(stderr, "--save-band: %s: no statistics\n", file); return 1; }
    if (verbose)
        fprintf(stderr, "saved band: %llu samples %s gain %g, peak %.4f of full scale, %llu components clipped; read with -r %d -c %.17g --format %s\n",
                (unsigned long long)st.n_samples, save_name(fmt), (double)gain, (double)st.peak, (unsigned long long)st.n_clipped,
                irdm_frontend_out_rate(fe), centre, fmt == IRDM_FMT_CI16 ? "ci16-full" : save_name(fmt));
    else if (st.n_clipped)
        fprintf(stderr, "--save-band: %s: %llu of %llu components clipped at gain %g (peak %.4f of full scale)\n", file,
                (unsigned long long)st.n_clipped, 2ULL * (unsigned long long)st.n_samples, (double)gain, (double)st.peak);
    return rc;
}

/* --save-only: every recording through the stage-level entries -- no context, no lines.  step: capture samples per read,
 * cap: the outputs a read can complete. */
static seg_t region_of(FILE *f, const input_t *in, size_t bps);
static size_t read_head(const seg_t *segs, int n_seg, size_t bps, size_t want, char *head);

static int save_only_run(irdm_frontend_t *fe, const char *save_band, const char *out_dir, int fmt, float gain, int verbose,
                         double centre, size_t step, size_t bps, size_t cap, int in_fmt, double rate)
{
    void *h_in = irdm_host_alloc(step * bps), *d_in = irdm_device_alloc(0, step * bps), *d_out = irdm_device_alloc(0, cap * 8);
    /* --iq-balance: the front end is a cf32 one; every read is corrected into d_bal (a cf32 file: in place) */
    /* --dc-block: likewise, in front of the balance; the first block of every recording is read ahead for the seed */
    const int fe_fmt = g_bal || g_dc ? IRDM_FMT_CF32 : in_fmt;
    void *d_bal = (g_bal || g_dc) && in_fmt != IRDM_FMT_CF32 ? irdm_device_alloc(0, step * 8) : d_in;
    const size_t dc_block = (size_t)1 << g_dc_log2;
    char *dc_head = g_dc ? malloc(dc_block * bps) : NULL;
    if (g_dc && !dc_head) { fprintf(stderr, "--dc-block: out of memory\n"); return 1; }
    float bal_a = 0.0f, bal_b = 1.0f;
    if (g_bal) irdm_iq_balance_coeffs(g_bal_gain, g_bal_phase, &bal_a, &bal_b);
    int rc_all = 0;
    if (!h_in || !d_in || !d_out || !d_bal) { fprintf(stderr, "--save-only: allocating the buffers failed\n"); return 1; }
    for (int fi = 0; fi < g_n_in; fi++) {
        const char *file = g_in[fi].path;
        const input_t *in = &g_in[fi];
        if (in->kind < 0) { fprintf(stderr, "%s\n", in->err); rc_all = 1; continue; }
        const char *data = in->kind > 0 ? in->info->data_path : file;
        FILE *f = strcmp(file, "-") ? fopen(data, "rb") : stdin;
        int rc = 0;
        unsigned long long remain = in->kind > 0 ? in->info->data_bytes / bps : ~0ULL;      /* samples left */
        if (!f) { perror(data); rc_all = 1; continue; }
        if (in->kind > 0 && fseeko(f, (off_t)in->info->data_offset, SEEK_SET) != 0) { perror(data); fclose(f); rc_all = 1; continue; }
        if (fi > 0 && irdm_frontend_reset(fe) != 0) { fprintf(stderr, "%s: the front end could not be reset\n", file); rc_all = 1; break; }
        if (band_open(save_band, out_dir, file, fmt) != 0) { if (f != stdin) fclose(f); rc_all = 1; continue; }
        irdm_scrub_stats_t sb = { 0 };                       /* --scrub: the recording's figures, summed over its reads */
        sb.limit_log2 = g_scrub_log2;
        sb.active = fe_fmt == IRDM_FMT_CF32;
        /* --dc-block: the state of the recording's stream, seeded from its head (a pipe's head is handed out again below) */
        irdm_dc_state_t dcs = { 0, 0, 0.0f, 0.0f };
        irdm_dc_stats_t dst;
        memset(&dst, 0, sizeof(dst));
        const char *pre = NULL;
        size_t pre_n = 0;
        if (g_dc) {
            const seg_t seg = region_of(f, in, bps);
            float seed[2] = { 0.0f, 0.0f };
            const size_t got = read_head(&seg, 1, bps, dc_block, dc_head);
            if (seg.bytes < 0) { pre = dc_head; pre_n = got; }
            if (irdm_dc_mean_host(in_fmt, dc_head, got, seed) != 0) rc = 1;
            dcs.mean_i = dst.seed_i = seed[g_swap ? 1 : 0];
            dcs.mean_q = dst.seed_q = seed[g_swap ? 0 : 1];
            dst.block_log2 = g_dc_log2;
        }
        for (;;) {
            const size_t want = remain < step ? (size_t)remain : step;
            size_t r = 0;
            if (pre_n && want) {
                r = pre_n < want ? pre_n : want;
                memcpy(h_in, pre, r * bps);
                pre += r * bps;
                pre_n -= r;
            }
            if (r < want) r += fread((char *)h_in + r * bps, bps, want - r, f);
            if (r == 0) break;
            remain -= r;
            if (irdm_device_upload(d_in, h_in, r * bps) != 0 || (g_swap && irdm_swap_iq_device(d_in, r, in_fmt, 0, NULL) != 0)) { rc = 1; break; }
            if (g_dc) {
                if (irdm_dc_block_device(in_fmt, d_bal, d_in, r, g_dc_log2, dst.n_samples, &dcs, NULL) != 0) { rc = 1; break; }
                /* (the figures of the line: the blocks this read closed end with the mean now in the state) */
                const uint64_t nb = ((dst.n_samples + r) >> g_dc_log2) - (dst.n_samples >> g_dc_log2);
                dst.n_samples += r;
                dst.n_blocks += nb;
                if (nb) { dst.last_i = dcs.mean_i; dst.last_q = dcs.mean_q; }
            }
            if (g_bal && irdm_iq_balance_device(d_bal, g_dc ? d_bal : d_in, r, g_dc ? IRDM_FMT_CF32 : in_fmt, bal_a, bal_b, 0, NULL) != 0) { rc = 1; break; }
            if (g_scrub) {
                irdm_scrub_stats_t one;
                if (irdm_scrub_device(d_bal, r, fe_fmt, g_scrub_log2, &one, 0, NULL) != 0) { rc = 1; break; }
                if (one.n_zeroed) {
                    if (!sb.n_zeroed) sb.first = sb.n_samples + one.first;
                    sb.last = sb.n_samples + one.last;
                }
                sb.n_samples += one.n_samples;
                sb.n_zeroed += one.n_zeroed;
                sb.n_nonfinite += one.n_nonfinite;
                sb.n_over += one.n_over;
            }
            if (irdm_frontend_run_device(fe, d_bal, r, d_out, cap, NULL) < 0) { rc = 1; break; }
            if (r < step) break;
        }
        if (rc == 0 && irdm_frontend_finish_device(fe, d_out, cap, NULL) < 0) rc = 1;
        if (rc) fprintf(stderr, "%s: GPU processing failed\n", file);
        if (band_close(fe, file, fmt, gain, verbose, centre) != 0) rc = 1;
        if (has_suffix_nocase(save_band, ".sigmf-data") && band_write_meta(save_band, fmt, irdm_frontend_out_rate(fe), centre, in->start_ns) != 0) rc = 1;
        if (g_dc) dc_line(&dst, in_fmt, 0);
        if (g_scrub) scrub_line(&sb, fe_fmt, rate);
        if (g_input_stats) {
            irdm_input_stats_t is;
            if (irdm_frontend_input_stats(fe, &is) == 0) input_line(&is, fe_fmt);
            else { fprintf(stderr, "--input-stats: %s: no statistics\n", file); rc = 1; }
        }
        if (f != stdin) fclose(f);
        if (rc) rc_all = 1;
    }
    return rc_all;
}

static const char *base_of(const char *p)
{
    const char *s = strrchr(p, '/');
    return s ? s + 1 : p;
}

/* The sample region of an opened input: a container's [data_offset, data_offset + data_bytes), cut to what the file
 * holds; a raw file whole; whole samples either way.  bytes -1: a pipe, read to its end. */
static seg_t region_of(FILE *f, const input_t *in, size_t bps)
{
    seg_t s = { f, 0, -1 };
    struct stat sb;
    const int regular = f != stdin && fstat(fileno(f), &sb) == 0 && S_ISREG(sb.st_mode);
    if (in->kind > 0) {
        s.off = (off_t)in->info->data_offset;
        s.bytes = (long long)in->info->data_bytes;
        if (regular && (off_t)s.off + (off_t)s.bytes > sb.st_size) s.bytes = sb.st_size > s.off ? (long long)(sb.st_size - s.off) : 0;
    } else if (regular)
        s.bytes = (long long)sb.st_size;
    if (s.bytes > 0) s.bytes -= s.bytes % (long long)bps;
    return s;
}

/* --prime: up to `want` leading samples of the regions into head -- pread() on files, which leaves their read positions
 * alone; standard input is read, and the reader hands those samples out again (reader_t.pre).  Returns the samples read. */
static size_t read_head(const seg_t *segs, int n_seg, size_t bps, size_t want, char *head)
{
    size_t got = 0;
    for (int k = 0; k < n_seg && got < want; k++) {
        if (segs[k].bytes < 0) return k == 0 ? fread(head, bps, want, segs[k].f) : got;     /* (a pipe: only in front) */
        size_t left = want - got, have = (size_t)((unsigned long long)segs[k].bytes / bps), done = 0;
        if (left > have) left = have;
        while (done < left * bps) {
            const ssize_t r = pread(fileno(segs[k].f), head + got * bps + done, left * bps - done, segs[k].off + (off_t)done);
            if (r <= 0) break;
            done += (size_t)r;
        }
        got += done / bps;
        if (done < left * bps) break;
    }
    return got;
}

int main(int argc, char **argv)
{
    const double t_main = now_s();
    int timing = 0;
    const char *file_info = NULL, *format = NULL, *out_dir = NULL;
    double rate = 0, freq = 1622000000.0, db = 0;
    int freq_given = 0, probe_only = 0;
    int container = -1;         /* --container: -1 by extension, IRDM_CONTAINER_NONE raw, else the kind every -f is read as */
    int gardner = 1, verbose = 0, no_simd = 0;
    size_t chunk = (size_t)16 << 20;
    int depth = 1;
    int read_threads = 6;       /* pread() helpers per chunk of a regular file (0: one fread thread) */
    int gpus = 0;               /* --gpus N: one stream across N GPUs of this process (0: one context on device 0) */
    int chunk_given = 0, loopback = 0;
    const char *save_dir = NULL;
    int acars = 0, acars_json = 0, has_origin = 0;
    const char *station = NULL;
    long long origin_sec = 0, origin_nsec = 0;
    uint64_t start_ns = 0;      /* --start-time: the capture time of the first recording (0: the wall clock) */
    int position = 0;
    double position_height = 0;
    int decimate = 0, band_given = 0;      /* --band-center / --decimate: the band-select front end */
    double band_center = 0;
    int resample_to = 0;                   /* --resample-to: the front end's rational mode */
    int rs_l = 0, rs_m = 0;
    const char *spectrum = NULL;           /* --spectrum FILE | auto */
    int spectrum_frames = 0;               /* --spectrum-frames R (0: about a second) */
    const char *save_band = NULL, *save_format = NULL;     /* --save-band FILE | auto, --save-format */
    double save_gain = 1.0;
    int save_gain_given = 0, save_only = 0, save_fmt = -1;
    int prime = 0, join = 0;               /* --prime, --join */
    for (int i = 1; i < argc; i++) {
        const char *a = argv[i];
#define NEXT() (i + 1 < argc ? argv[++i] : (fprintf(stderr, "missing value for %s\n", a), exit(2), ""))
        if (!strcmp(a, "-f") || !strcmp(a, "--file")) add_input(NEXT(), 0);      /* more than once: the recordings in this order */
        else if (!strcmp(a, "--files-from")) { if (read_list(NEXT()) != 0) return 2; }
        else if (!strcmp(a, "--out-dir")) out_dir = NEXT();
        else if (!strcmp(a, "--start-time")) {
            const char *v = NEXT();
            long long sec, nsec;
            if (parse_time(v, &sec, &nsec) != 0 || sec < 0) { fprintf(stderr, "--start-time %s: expected SEC[.NNNNNNNNN]\n", v); return 2; }
            start_ns = (uint64_t)sec * 1000000000ULL + (uint64_t)nsec;
        }
        else if (!strcmp(a, "-r") || !strcmp(a, "--sample-rate")) rate = atof(NEXT());
        else if (!strcmp(a, "-c") || !strcmp(a, "--center-freq")) { freq = atof(NEXT()); freq_given = 1; }
        else if (!strcmp(a, "--container")) {
            const char *v = NEXT();
            if (!strcmp(v, "wav")) container = IRDM_CONTAINER_WAV;
            else if (!strcmp(v, "sigmf")) container = IRDM_CONTAINER_SIGMF;
            else if (!strcmp(v, "sdriq")) container = IRDM_CONTAINER_SDRIQ;
            else if (!strcmp(v, "raw")) container = IRDM_CONTAINER_NONE;
            else { fprintf(stderr, "--container %s: wav, sigmf, sdriq or raw\n", v); return 2; }
        }
        else if (!strcmp(a, "--probe")) probe_only = 1;
        else if (!strcmp(a, "-d") || !strcmp(a, "--threshold")) db = atof(NEXT());
        else if (!strcmp(a, "--format")) format = NEXT();
        else if (!strcmp(a, "--file-info")) file_info = NEXT();
        else if (!strcmp(a, "--chunk")) { chunk = (size_t)atoll(NEXT()); chunk_given = 1; }
        else if (!strcmp(a, "--gpus")) gpus = atoi(NEXT());         /* the reference's thread layout for N > 1 (main.c:667-694) */
        else if (!strcmp(a, "--group-loopback")) loopback = 1;      /* test aid: --gpus 1 hands the detector state to itself over RCCL */
        else if (!strcmp(a, "--no-gardner")) gardner = 0;
        else if (!strcmp(a, "--save-bursts")) save_dir = NEXT();   /* options.c --save-bursts: IQ + .meta per downmixed frame */
        else if (!strcmp(a, "--parsed")) g_parsed = 1;              /* options.c --parsed: IDA lines where they decode */
        else if (!strcmp(a, "--acars")) acars = 1;                  /* options.c:401-408: ACARS from reassembled IDA */
        else if (!strcmp(a, "--acars-json")) acars = acars_json = 1;
        else if (!strcmp(a, "--station")) station = NEXT();         /* options.c --station=ID (getopt takes both forms) */
        else if (!strncmp(a, "--station=", 10)) station = a + 10;
        else if (!strcmp(a, "--position") || !strncmp(a, "--position=", 11)) {
            /* options.c:391-398 (getopt optional_argument: only the --position=H form takes a value); the web map the
             * reference also turns on here is not built */
            position = 1;
            if (a[10] == '=') {
                position_height = atof(a + 11);
                if (position_height < 0 || position_height > 9000)
                    errx(1, "--position height must be 0-9000 m (got %.0f)", position_height);
            }
        }
        else if (!strcmp(a, "--acars-origin")) {
            /* test aid: SEC[.NNNNNNNNN] is the wall clock of the first printed ACARS message instead of CLOCK_REALTIME */
            const char *v = NEXT();
            if (parse_time(v, &origin_sec, &origin_nsec) != 0) { fprintf(stderr, "--acars-origin %s: expected SEC[.NNNNNNNNN]\n", v); return 2; }
            has_origin = 1;
        }
        else if (!strcmp(a, "--acars-udp") || !strncmp(a, "--acars-udp=", 12) || !strcmp(a, "--feed") || !strncmp(a, "--feed=", 7) ||
                 !strcmp(a, "--gsmtap") || !strncmp(a, "--gsmtap=", 9) || !strcmp(a, "--web") || !strncmp(a, "--web=", 6)) {
            fprintf(stderr, "%s: network output is not built in this binary (ACARS goes to stdout with --acars / --acars-json)\n", a);
            return 2;
        }
        else if (!strcmp(a, "--band-center")) { band_center = atof(NEXT()); band_given = 1; }
        else if (!strcmp(a, "--decimate")) decimate = atoi(NEXT());
        else if (!strcmp(a, "--resample-to")) {
            resample_to = atoi(NEXT());
            if (resample_to <= 0) { fprintf(stderr, "--resample-to: a rate in Hz\n"); return 2; }
        }
        else if (!strcmp(a, "--spectrum")) spectrum = NEXT();
        else if (!strcmp(a, "--spectrum-frames")) {
            spectrum_frames = atoi(NEXT());
            if (spectrum_frames < 1 || spectrum_frames > (1 << 20)) { fprintf(stderr, "--spectrum-frames: 1 .. 1048576 frames per row\n"); return 2; }
        }
        else if (!strcmp(a, "--save-band")) save_band = NEXT();
        else if (!strcmp(a, "--save-format")) save_format = NEXT();
        else if (!strcmp(a, "--save-gain")) {
            char *end;
            const char *v = NEXT();
            save_gain = strtod(v, &end);
            save_gain_given = 1;
            if (end == v || *end || !(save_gain > 0) || !(save_gain <= 3.0e38) || !((float)save_gain > 0)) {
                fprintf(stderr, "--save-gain %s: a positive finite number\n", v);
                return 2;
            }
        }
        else if (!strcmp(a, "--save-only")) save_only = 1;
        else if (!strcmp(a, "--input-stats")) g_input_stats = 1;
        else if (!strcmp(a, "--diagnostic")) g_input_stats = g_diag = 1;     /* options.c:376 */
        else if (!strcmp(a, "--clock-check")) g_clock = 1;
        else if (!strcmp(a, "--fine-freq")) g_fine = 1;
        else if (!strcmp(a, "--fine-time")) g_ftime = 1;
        else if (!strcmp(a, "--iq-check")) g_iq = 1;
        else if (!strcmp(a, "--burst-resample")) g_burst_resample = 1;
        else if (!strcmp(a, "--swap-iq")) g_swap = 1;
        else if (!strcmp(a, "--scrub") || !strncmp(a, "--scrub=", 8)) {
            /* (as --position: only the --scrub=LOG2 form takes a value) */
            g_scrub = 1;
            if (a[7] == '=') {
                char *end;
                const long v = strtol(a + 8, &end, 10);
                if (end == a + 8 || *end || v < 0 || v > 127) {
                    fprintf(stderr, "--scrub=%s: the limit's base-2 logarithm, an integer 0 .. 127\n", a + 8);
                    return 2;
                }
                g_scrub_log2 = (int)v;
            }
        }
        else if (!strcmp(a, "--dc-block") || !strncmp(a, "--dc-block=", 11)) {
            /* (as --scrub: only the --dc-block=LOG2 form takes a value) */
            g_dc = 1;
            if (a[10] == '=') {
                char *end;
                const long v = strtol(a + 11, &end, 10);
                if (end == a + 11 || *end || v < 12 || v > 24) {
                    fprintf(stderr, "--dc-block=%s: the block length's base-2 logarithm, an integer 12 .. 24\n", a + 11);
                    return 2;
                }
                g_dc_log2 = (int)v;
            }
        }
        else if (!strcmp(a, "--image-check")) g_image = 1;
        else if (!strcmp(a, "--prime")) prime = 1;
        else if (!strcmp(a, "--join")) join = 1;
        else if (!strcmp(a, "--iq-balance") || !strncmp(a, "--iq-balance=", 13)) {
            /* (the --iq-balance=GAIN_DB,PHASE_DEG form only) */
            char *end = NULL, *end2 = NULL;
            const char *v = a[12] == '=' ? a + 13 : "";
            g_bal_gain = strtod(v, &end);
            if (end != v && *end == ',') g_bal_phase = strtod(end + 1, &end2);
            if (!end2 || end2 == end + 1 || *end2 || irdm_iq_balance_coeffs(g_bal_gain, g_bal_phase, NULL, NULL) != 0) {
                fprintf(stderr, "%s: give --iq-balance=GAIN_DB,PHASE_DEG, two numbers within +-6 dB and +-30 degrees\n", a);
                return 2;
            }
            g_bal = 1;
        }
        else if (!strcmp(a, "--read-threads")) read_threads = atoi(NEXT());
        else if (!strcmp(a, "--depth")) depth = atoi(NEXT());       /* 0: per-chunk latency, 1: throughput (default) */
        else if (!strcmp(a, "-v") || !strcmp(a, "--verbose")) verbose = 1;
        else if (!strcmp(a, "--timing")) timing = 1;                /* start-up and streaming time on stderr */
        else if (!strcmp(a, "--no-simd")) no_simd = 1;              /* options.c:240, :351; main.c:567 simd_init(no_simd) */
        else if (!strcmp(a, "--no-gpu")) {
            fprintf(stderr, "%s: this binary is the GPU path; use the reference binary for the CPU path\n", a);
            return 2;
        } else {
            fprintf(stderr, "unknown option %s\n", a);
            return 2;
        }
    }
    /* the inputs: what each one is (a container's header, or a raw file described by the flags) */
    int first = -1, n_cont = 0, n_named = 0;     /* containers read well; inputs read as containers, malformed ones too */
    if (container > 0)
        for (int k = 0; k < g_n_in; k++)
            if (!strcmp(g_in[k].path, "-")) {
                fprintf(stderr, "-f - with --container: standard input is read as a raw stream\n");
                return 2;
            }
    if (g_n_in > 0 && g_in[0].start_ns == 0) g_in[0].start_ns = start_ns;
    for (int k = 0; k < g_n_in; k++) {
        resolve_input(&g_in[k], container, format, freq, freq_given);
        if (g_in[k].kind > 0) n_cont++;
        if (g_in[k].kind != 0) n_named++;
        if (g_in[k].kind >= 0 && first < 0) first = k;
    }
    if (n_named && format) {
        fprintf(stderr, "--format %s beside a container: the header names the sample format (--container raw reads the file as raw samples)\n", format);
        return 2;
    }
    if (probe_only && g_n_in) {
        int bad = 0;
        for (int k = 0; k < g_n_in; k++) {
            if (g_in[k].kind < 0) { fprintf(stderr, "%s\n", g_in[k].err); bad++; }
            else probe_line(stdout, &g_in[k], rate);
        }
        return bad ? (g_n_in == 1 ? 2 : 1) : 0;
    }
    if (g_n_in && first < 0) {
        for (int k = 0; k < g_n_in; k++) fprintf(stderr, "%s\n", g_in[k].err);
        return g_n_in == 1 ? 2 : 1;
    }
    if (join) {
        /* one recording in parts: every part must be there, and the headers must describe one capture */
        int bad = 0;
        for (int k = 0; k < g_n_in; k++)
            if (g_in[k].kind < 0) { fprintf(stderr, "%s\n", g_in[k].err); bad = 1; }
        if (bad) { fprintf(stderr, "--join: every part must be readable\n"); return 2; }
        for (int k = 0, c0 = -1, r0 = -1; k < g_n_in; k++) {
            if (g_in[k].kind <= 0) continue;
            if (r0 >= 0 && g_in[k].hdr_rate != g_in[r0].hdr_rate) {
                fprintf(stderr, "--join: %s (%d samples/s) and %s (%d samples/s) are not parts of one capture\n", g_in[r0].path,
                        g_in[r0].hdr_rate, g_in[k].path, g_in[k].hdr_rate);
                return 2;
            }
            r0 = k;
            if (!g_in[k].info->has_center) continue;
            if (c0 >= 0 && g_in[k].info->center_frequency != g_in[c0].info->center_frequency) {
                fprintf(stderr, "--join: %s (%.0f Hz) and %s (%.0f Hz) are not parts of one capture\n", g_in[c0].path,
                        g_in[c0].info->center_frequency, g_in[k].path, g_in[k].info->center_frequency);
                return 2;
            }
            c0 = k;
        }
        if (gpus > 1) { fprintf(stderr, "--join: one GPU only (--gpus %d)\n", gpus); return 2; }
        if (save_only) { fprintf(stderr, "--join with --save-only: not supported; run the band's recording through --save-band\n"); return 2; }
    }
    /* the recordings of the run: with --join all inputs are one */
    const int n_rec = join ? (g_n_in > 0) : g_n_in;
    if (g_n_in && rate <= 0) {
        /* no -r: every input carries its rate, and they agree */
        for (int k = 0; k < g_n_in; k++) {
            if (g_in[k].kind < 0) continue;
            if (g_in[k].kind == 0) { rate = 0; break; }
            if (rate > 0 && (int)rate != g_in[k].hdr_rate) {
                fprintf(stderr, "%s (%d samples/s) and %s (%d samples/s): one context takes one sample rate (run them apart)\n", g_in[first].path,
                        g_in[first].hdr_rate, g_in[k].path, g_in[k].hdr_rate);
                return 2;
            }
            rate = g_in[k].hdr_rate;
        }
    } else {
        for (int k = 0; k < g_n_in; k++)
            if (g_in[k].kind > 0 && (double)g_in[k].hdr_rate != rate)
                fprintf(stderr, "warning: %s: -r %.0f overrides the header's %d samples/s\n", g_in[k].path, rate, g_in[k].hdr_rate);
    }
    if (!g_n_in || rate <= 0) {
        fprintf(stderr, "usage: %s -f FILE [-f FILE2 ...] [--files-from LIST] [-r RATE] [-c FREQ] [--format ci8|cu8|ci16|cf32|ci16-full|sc16q11|ci32|ci32-24] [--container wav|sigmf|sdriq|raw] [--probe] [-d DB] [--file-info STR] [--no-simd] [--save-bursts DIR] [--parsed] [--acars] [--acars-json] [--station ID] [--position[=HEIGHT_M]] [--gpus N] [--band-center HZ --decimate D] [--resample-to HZ [--band-center HZ]] [--start-time SEC[.NNNNNNNNN]] [--out-dir DIR] [--spectrum FILE [--spectrum-frames R]] [--save-band FILE [--save-format ci8|ci16|cf32] [--save-gain G] [--save-only]] [--input-stats] [--diagnostic] [--clock-check] [--fine-freq] [--fine-time] [--iq-check] [--swap-iq] [--scrub[=LOG2]] [--dc-block[=LOG2]] [--image-check] [--iq-balance=GAIN_DB,PHASE_DEG] [--burst-resample] [--prime] [--join]\n", argv[0]);
        return 2;
    }
    if (resample_to && decimate) {
        fprintf(stderr, "--resample-to and --decimate: one or the other (--resample-to takes integer ratios as well)\n");
        return 2;
    }
    if (!resample_to && band_given != (decimate != 0)) {
        fprintf(stderr, "--band-center and --decimate go together\n");
        return 2;
    }
    if (resample_to) {
        if (gpus > 1) {
            fprintf(stderr, "--resample-to: one GPU only (--gpus %d)\n", gpus);
            return 2;
        }
        if ((double)(int)rate != rate) {
            fprintf(stderr, "--resample-to: -r %.3f is no whole number of samples per second\n", rate);
            return 2;
        }
        if ((int)rate == resample_to) {
            fprintf(stderr, "--resample-to %d: that is the capture's rate; leave the flag out\n", resample_to);
            return 2;
        }
        /* the library's own check of the ratio (its message), before anything is started */
        if (irdm_frontend_resampler_ratio((int)rate, resample_to, &rs_l, &rs_m, NULL) != 0) return 2;
        gpus = 0;
    }
    if (decimate && gpus > 1) {
        fprintf(stderr, "--band-center / --decimate: one GPU only (--gpus %d)\n", gpus);
        return 2;
    }
    if (decimate) gpus = 0;
    /* several recordings: everything that can be refused is refused before anything is processed */
    if (g_n_in > 1 && gpus > 1) {
        fprintf(stderr, "%d recordings: one GPU only (--gpus %d); a group is not reset between recordings\n", g_n_in, gpus);
        return 2;
    }
    if (g_n_in > 1) gpus = 0;
    if (prime) {
        if (gpus > 1) {
            fprintf(stderr, "--prime: one GPU only (--gpus %d): a member of a group is not primed\n", gpus);
            return 2;
        }
        if (save_only) {
            fprintf(stderr, "--prime with --save-only: no context runs, so there is no detector to prime\n");
            return 2;
        }
        gpus = 0;
    }
    if (spectrum) {
        if (gpus > 1) {
            fprintf(stderr, "--spectrum: one GPU only (--gpus %d)\n", gpus);
            return 2;
        }
        if ((n_rec > 1 || !strcmp(spectrum, "auto")) && (strcmp(spectrum, "auto") != 0 || !out_dir)) {
            fprintf(stderr, "--spectrum with several recordings: give --spectrum auto and --out-dir DIR (DIR/<basename>.spec each)\n");
            return 2;
        }
        gpus = 0;
    } else if (spectrum_frames) {
        fprintf(stderr, "--spectrum-frames goes with --spectrum FILE\n");
        return 2;
    }
    if (g_input_stats) {
        if (gpus > 1) {
            fprintf(stderr, "%s: one GPU only (--gpus %d)\n", g_diag ? "--diagnostic" : "--input-stats", gpus);
            return 2;
        }
        gpus = 0;
    }
    if (g_clock) {
        if (gpus > 1) {
            fprintf(stderr, "--clock-check: one GPU only (--gpus %d)\n", gpus);
            return 2;
        }
        if (save_only) {
            fprintf(stderr, "--clock-check with --save-only: no context runs, so there are no frames to judge\n");
            return 2;
        }
        gpus = 0;
    }
    if (g_fine) {
        if (gpus > 1) {
            fprintf(stderr, "--fine-freq: one GPU only (--gpus %d)\n", gpus);
            return 2;
        }
        if (save_only) {
            fprintf(stderr, "--fine-freq with --save-only: no context runs, so there are no frames to refine\n");
            return 2;
        }
        gpus = 0;
    }
    if (g_ftime) {
        if (gpus > 1) {
            fprintf(stderr, "--fine-time: one GPU only (--gpus %d)\n", gpus);
            return 2;
        }
        if (save_only) {
            fprintf(stderr, "--fine-time with --save-only: no context runs, so there are no frames to refine\n");
            return 2;
        }
        gpus = 0;
    }
    if (g_iq) {
        if (gpus > 1) {
            fprintf(stderr, "--iq-check: one GPU only (--gpus %d)\n", gpus);
            return 2;
        }
        if (save_only) {
            fprintf(stderr, "--iq-check with --save-only: no context runs, so there are no frames to judge\n");
            return 2;
        }
        gpus = 0;
    }
    if (g_swap) {
        if (gpus > 1) {
            fprintf(stderr, "--swap-iq: one GPU only (--gpus %d): a group is fed on the device\n", gpus);
            return 2;
        }
        gpus = 0;
    }
    if (g_scrub) {
        if (gpus > 1) {
            fprintf(stderr, "--scrub: one GPU only (--gpus %d): a group is fed on the device\n", gpus);
            return 2;
        }
        gpus = 0;
    }
    if (g_image) {
        if (gpus > 1) {
            fprintf(stderr, "--image-check: one GPU only (--gpus %d)\n", gpus);
            return 2;
        }
        if (save_only) {
            fprintf(stderr, "--image-check with --save-only: no context runs, so there are no frames to judge\n");
            return 2;
        }
        gpus = 0;
    }
    if (g_bal) {
        if (gpus > 1) {
            fprintf(stderr, "--iq-balance: one GPU only (--gpus %d): a group is fed on the device\n", gpus);
            return 2;
        }
        gpus = 0;
    }
    if (g_dc) {
        if (gpus > 1) {
            fprintf(stderr, "--dc-block: one GPU only (--gpus %d): a group is fed on the device\n", gpus);
            return 2;
        }
        gpus = 0;
    }
    if (save_band) {
        if (!decimate && !resample_to) {
            fprintf(stderr, "--save-band saves the band a front end selects: give --band-center / --decimate or --resample-to\n");
            return 2;
        }
        const int many = n_rec > 1 || !strcmp(save_band, "auto");
        if (many && (strcmp(save_band, "auto") != 0 || !out_dir)) {
            fprintf(stderr, "--save-band with several recordings: give --save-band auto and --out-dir DIR (DIR/<basename>.band.<format> each)\n");
            return 2;
        }
        if (many && !save_format) {
            fprintf(stderr, "--save-band auto: name the format with --save-format ci8|ci16|cf32\n");
            return 2;
        }
        save_fmt = save_format_of(save_format ? save_format : (has_suffix_nocase(save_band, ".sigmf-data") ? "cf32" : NULL), save_band);
        if (save_fmt < 0) {
            if (save_format) fprintf(stderr, "--save-format %s: ci8, ci16 or cf32\n", save_format);
            else fprintf(stderr, "--save-band %s: the extension names no format (.ci8, .ci16, .cs16, .cf32, .fc32, .cfile); give --save-format\n", save_band);
            return 2;
        }
        if (save_fmt == IRDM_FMT_CF32 && (float)save_gain != 1.0f) {
            fprintf(stderr, "--save-gain %g: a cf32 recording holds the samples as they are (gain 1)\n", save_gain);
            return 2;
        }
        if (save_fmt != IRDM_FMT_CF32 && !((float)save_gain * (save_fmt == IRDM_FMT_CI8 ? 128.0f : 32768.0f) <= 3.0e38f)) {
            fprintf(stderr, "--save-gain %g: too large\n", save_gain);
            return 2;
        }
    } else if (save_format || save_gain_given || save_only) {
        fprintf(stderr, "--save-format, --save-gain and --save-only go with --save-band FILE\n");
        return 2;
    }
    const size_t bps = g_in[first].bps;
    const int fmt = g_in[first].fmt;
    /* --iq-balance: the context or the front end is a cf32 one and takes the file's format as its wire format */
    /* --dc-block: likewise */
    const int proc_fmt = g_bal || g_dc ? IRDM_FMT_CF32 : fmt;
    freq = g_in[first].centre;
    for (int k = 0; k < g_n_in; k++) {
        if (g_n_in > 1 && !strcmp(g_in[k].path, "-")) {
            fprintf(stderr, "-f -: stdin only as the sole input (%d recordings given)\n", g_n_in);
            return 2;
        }
        if (g_in[k].kind >= 0 && g_in[k].fmt != fmt) {
            fprintf(stderr, "%s and %s resolve to different sample formats: one context takes one format (give --format, or run them apart)\n",
                    g_in[first].path, g_in[k].path);
            return 2;
        }
        if (g_in[k].kind >= 0 && (decimate || resample_to) && g_in[k].centre != freq) {
            fprintf(stderr, "%s (%.0f Hz) and %s (%.0f Hz): behind a front end every recording has one centre frequency (its shift is fixed; give -c, or run them apart)\n",
                    g_in[first].path, freq, g_in[k].path, g_in[k].centre);
            return 2;
        }
        for (int j = 0; out_dir && !join && j < k; j++)
            if (!strcmp(base_of(g_in[j].path), base_of(g_in[k].path))) {
                fprintf(stderr, "--out-dir: %s and %s would share %s/%s.out\n", g_in[j].path, g_in[k].path, out_dir, base_of(g_in[k].path));
                return 2;
            }
    }
    if (n_cont && !resample_to && !g_burst_resample && (long long)rate % 250000 != 0)
        fprintf(stderr, "warning: %.0f samples/s is no multiple of 250 kHz: frames may decode only in part; resample with --resample-to HZ\n", rate);
    if (verbose)
        for (int k = 0; k < g_n_in; k++) {
            if (g_in[k].kind <= 0) continue;
            probe_line(stderr, &g_in[k], rate);
            if (g_in[k].info->n_captures > 1)
                fprintf(stderr, "%s: %d capture segments, the first one's frequency and time are used\n", g_in[k].path, g_in[k].info->n_captures);
        }
    g_out = stdout;

    /* the front end first: the context behind it runs at its output rate, centred where the applied shift puts it */
    irdm_frontend_t *fe = NULL;
    if (decimate) {
        irdm_frontend_config_t fc;
        memset(&fc, 0, sizeof(fc));
        fc.in_rate = (int)rate;
        fc.in_format = proc_fmt;
        fc.decim = decimate;
        fc.shift_hz = band_center - freq;
        fe = irdm_frontend_create(&fc);
        if (!fe) {
            fprintf(stderr, "irdm_frontend_create failed (no MI355X / bad parameters)\n");
            return 1;
        }
    } else if (resample_to) {
        irdm_frontend_rational_config_t fc;
        memset(&fc, 0, sizeof(fc));
        fc.in_rate = (int)rate;
        fc.in_format = proc_fmt;
        fc.out_rate = resample_to;
        fc.shift_hz = band_given ? band_center - freq : 0.0;
        fe = irdm_frontend_create_resampler(&fc);
        if (!fe) {
            fprintf(stderr, "irdm_frontend_create_resampler failed (no MI355X / bad parameters)\n");
            return 1;
        }
    }
    irdm_config_t c;
    memset(&c, 0, sizeof(c));
    c.center_frequency = fe ? freq + irdm_frontend_applied_shift_hz(fe) : freq;
    c.sample_rate = fe ? irdm_frontend_out_rate(fe) : (int)rate;
    c.threshold_db = (float)db;
    c.format = fe ? IRDM_FMT_CF32 : proc_fmt;
    c.feed_block = 32768;
    c.use_gardner = gardner;
    c.start_time_ns = g_in[first].start_ns;
    /* --burst-resample: the ratio decim 250000 / rate of the context's rate in lowest terms (the library's arithmetic); one
     * whose L the kernel does not take ends the run here, before a context exists */
    long long br_l = 1, br_m = 1;
    if (g_burst_resample) {
        long long decim = (long long)roundf((float)c.sample_rate / 250000.0f);
        if (decim < 1) decim = 1;
        long long x = decim * 250000, y = c.sample_rate;
        while (y) { const long long t = x % y; x = y; y = t; }
        br_l = decim * 250000 / x;
        br_m = c.sample_rate / x;
        if (br_l > 4096) {
            fprintf(stderr, "--burst-resample: %d samples/s needs the ratio %lld/%lld, L = %lld is beyond 4096; resample the stream with --resample-to HZ\n",
                    c.sample_rate, br_l, br_m, br_l);
            return 2;
        }
        if (verbose && br_l != br_m)
            fprintf(stderr, "burst resample: %.10g -> 250000 samples/s per burst (%lld/%lld), 20 taps per phase\n",
                    (double)c.sample_rate / (double)decim, br_l, br_m);
        else if (verbose)
            fprintf(stderr, "burst resample: %d is on the 250 kHz grid; nothing to do\n", c.sample_rate);
    }
    /* (several GPUs: a chunk must hold the samples a member is given from in front of its chunk -- 2 s of signal, the
     * reference's ring -- so the default grows with the rate) */
    if (gpus > 1 && !chunk_given) chunk = (size_t)(2.75 * rate);
    chunk = chunk / 32768 * 32768;
    if (chunk == 0) chunk = 32768;
    c.max_chunk_samples = chunk;
    c.pipeline_depth = depth;
    if (gpus < 0 || gpus > 64) { fprintf(stderr, "--gpus %d\n", gpus); return 2; }
    if (save_band) {
        irdm_frontend_save_config_t sc;
        memset(&sc, 0, sizeof(sc));
        sc.format = save_fmt;
        sc.gain = (float)save_gain;
        sc.sink = band_sink;
        if (irdm_frontend_save(fe, &sc) != 0) {
            fprintf(stderr, "--save-band: the library refused the recording\n");
            return 1;
        }
    }
    if (g_input_stats && fe && irdm_frontend_input_stats_enable(fe, 1) != 0) {
        fprintf(stderr, "--input-stats: the library refused the statistics\n");
        return 1;
    }
    if (g_swap && verbose)
        fprintf(stderr, "--swap-iq: I and Q of every sample are exchanged on the GPU; I of the \"input:\" line is the file's second component\n");
    if (g_swap && fe && !save_only && irdm_frontend_swap_iq(fe, 1) != 0) {
        fprintf(stderr, "--swap-iq: the library refused the exchange\n");
        return 1;
    }
    if (g_bal && verbose) {
        float a = 0.0f, b = 1.0f;
        irdm_iq_balance_coeffs(g_bal_gain, g_bal_phase, &a, &b);
        fprintf(stderr, "--iq-balance: Q/I gain %+.3f dB, phase %+.2f deg: q' = %.9g i + %.9g q on the GPU, %s in, cf32 from there on; "
                        "the closing lines describe the corrected stream\n", g_bal_gain, g_bal_phase, (double)a, (double)b, format_name(fmt));
    }
    if (g_bal && fe && !save_only && irdm_frontend_iq_balance(fe, fmt, g_bal_gain, g_bal_phase) != 0) {
        fprintf(stderr, "--iq-balance: the library refused the correction\n");
        return 1;
    }
    if (g_dc && verbose)
        fprintf(stderr, "--dc-block: the DC offset is tracked over blocks of 2^%d samples and subtracted on the GPU, %s in, cf32 from "
                        "there on; each recording is seeded from its own head; the closing lines describe the corrected stream\n",
                g_dc_log2, format_name(fmt));
    if (g_image && fe && irdm_frontend_iq_moments(fe, 1) != 0) {
        fprintf(stderr, "--image-check: the library refused the measurement\n");
        return 1;
    }
    if (g_scrub && verbose)
        fprintf(stderr, "--scrub: cf32 samples with a component that is not finite or beyond +-2^%d are zeroed on the GPU; the "
                        "\"input:\" line describes what is left\n", g_scrub_log2);
    if (g_scrub && fe && !save_only && irdm_frontend_scrub(fe, 1, g_scrub_log2) != 0) {
        fprintf(stderr, "--scrub: the library refused the pass\n");
        return 1;
    }
    if (save_only) {
        const size_t so_step = resample_to ? (chunk * (size_t)rs_m + (size_t)rs_l - 1) / (size_t)rs_l : chunk * (size_t)decimate;
        if (out_dir && mkdir(out_dir, 0777) != 0 && errno != EEXIST) { perror(out_dir); return 1; }
        const int rc = save_only_run(fe, save_band, out_dir, save_fmt, (float)save_gain, verbose, c.center_frequency, so_step, bps,
                                     chunk + (size_t)irdm_frontend_ntaps(fe) + 64, fmt, rate);
        fflush(stderr);
        _exit(rc);
    }
    if (gpus > irdm_device_count()) {
        fprintf(stderr, "--gpus %d: this host has %d GPU%s\n", gpus, irdm_device_count(), irdm_device_count() == 1 ? "" : "s");
        return 2;
    }
    irdm_pipeline_t *p;
    if (gpus > 0) {
        g_group = irdm_group_create(&c, gpus, NULL);
        if (!g_group) {
            fprintf(stderr, "irdm_group_create failed (%d MI355X asked for / RCCL / bad parameters)\n", gpus);
            return 1;
        }
        if (loopback && irdm_group_set_option(g_group, "group_loopback", 1) != 0) {
            fprintf(stderr, "--group-loopback: refused (chunk smaller than the overlap, or no RCCL)\n");
            return 1;
        }
        p = irdm_group_member(g_group, 0);
    } else {
        p = irdm_create(&c);
        if (!p) {
            fprintf(stderr, "irdm_create failed (no MI355X / bad parameters)\n");
            return 1;
        }
    }
#define SET_OPTION(key, v) (g_group ? irdm_group_set_option(g_group, key, v) : irdm_set_option(p, key, v))
    /* --no-simd: the reference points its eleven dispatched kernels at simd_generic.c instead of simd_avx2.c
     * (simd_generic.c:33-57); here the same switch selects the kernels that follow the generic file's operation order */
    if (no_simd && SET_OPTION("fir_order", 0) != 0) {
        fprintf(stderr, "--no-simd: the library refused fir_order 0\n");
        return 1;
    }
    if (save_dir) SET_OPTION("keep_frame_samples", 1);
    else SET_OPTION("packed_records", 1);
    if ((g_parsed || acars) && SET_OPTION(save_dir ? "decode_ida" : "parsed_records", 1) != 0) {
        fprintf(stderr, "%s: the library refused the IDA decoder\n", g_parsed ? "--parsed" : "--acars");
        return 1;
    }
    if (position && SET_OPTION(save_dir ? "decode_frames" : "frame_records", 1) != 0) {
        fprintf(stderr, "--position: the library refused the frame decoder\n");
        return 1;
    }
    if (spectrum) {
        if (!spectrum_frames) {
            spectrum_frames = (int)((double)c.sample_rate / (double)irdm_fft_size(p) + 0.5);
            if (spectrum_frames < 1) spectrum_frames = 1;
        }
        g_spec_rows = malloc(sizeof(float) * 2 * SPEC_POLL * (size_t)irdm_spectrum_bins(p));
        if (!g_spec_rows || irdm_set_option(p, "spectrum_frames", spectrum_frames) != 0) {
            fprintf(stderr, "--spectrum: the library refused %d frames per row\n", spectrum_frames);
            return 1;
        }
    }
    if (g_input_stats && !fe && irdm_set_option(p, "input_stats", 1) != 0) {
        fprintf(stderr, "--input-stats: the library refused the statistics\n");
        return 1;
    }
    if (g_burst_resample && SET_OPTION("burst_resample", 1) != 0) {
        fprintf(stderr, "--burst-resample: the library refused the option\n");
        return 1;
    }
    if (g_clock && irdm_set_option(p, "symbol_clock", 1) != 0) {
        fprintf(stderr, "--clock-check: the library refused the estimator\n");
        return 1;
    }
    if (g_fine && irdm_set_option(p, "fine_freq", 1) != 0) {
        fprintf(stderr, "--fine-freq: the library refused the estimator\n");
        return 1;
    }
    if (g_fine && verbose) fprintf(stderr, "fine freq: carrier frequency from each frame's samples (+-250 Hz of the downmixer's)\n");
    if (g_ftime && irdm_set_option(p, "fine_time", 1) != 0) {
        fprintf(stderr, "--fine-time: the library refused the estimator\n");
        return 1;
    }
    if (g_ftime && !g_burst_resample && c.sample_rate % 250000 != 0)
        fprintf(stderr, "warning: --fine-time at %d samples/s, no multiple of 250 kHz: the frames' samples are not 4 us apart and the "
                        "refined times inherit the clock error; add --burst-resample\n", c.sample_rate);
    if (g_ftime && verbose) fprintf(stderr, "fine time: arrival time of each frame's first symbol from its samples\n");
    if (g_iq && irdm_set_option(p, "iq_sense", 1) != 0) {
        fprintf(stderr, "--iq-check: the library refused the check\n");
        return 1;
    }
    if (g_swap && !fe && irdm_set_option(p, "swap_iq", 1) != 0) {
        fprintf(stderr, "--swap-iq: the library refused the exchange\n");
        return 1;
    }
    if (g_scrub && !fe && (irdm_set_option(p, "scrub_limit_log2", g_scrub_log2) != 0 || irdm_set_option(p, "scrub", 1) != 0)) {
        fprintf(stderr, "--scrub: the library refused the pass\n");
        return 1;
    }
    if (g_bal && !fe && irdm_iq_balance(p, fmt, g_bal_gain, g_bal_phase) != 0) {
        fprintf(stderr, "--iq-balance: the library refused the correction\n");
        return 1;
    }
    if (g_image && !fe && irdm_set_option(p, "iq_moments", 1) != 0) {
        fprintf(stderr, "--image-check: the library refused the measurement\n");
        return 1;
    }
    g_save_dir = save_dir;
    /* a group is fed a super-step at a time: one chunk per member */
    /* (behind a front end the reader's chunk is D -- or M / L -- pipeline chunks of capture samples) */
    const size_t step = resample_to ? (chunk * (size_t)rs_m + (size_t)rs_l - 1) / (size_t)rs_l
                                    : chunk * (size_t)(gpus > 0 ? gpus : 1) * (size_t)(fe ? decimate : 1);
    if (out_dir && mkdir(out_dir, 0777) != 0 && errno != EEXIST) { perror(out_dir); return 1; }

    /* Two pinned read buffers and a reader thread per recording (the reference's spewer thread, main.c:223-284): the file
     * read of chunk k+1 overlaps the H2D copy and GPU work of chunk k; the H2D copy itself is DMA that overlaps chunk
     * k-1's detector scan.  The buffers serve every recording of the run. */
    void *pinned[2];
    for (int i = 0; i < 2; i++) {
        pinned[i] = irdm_host_alloc(step * bps);
        if (!pinned[i]) { fprintf(stderr, "irdm_host_alloc failed\n"); return 1; }
    }
    irdm_demod_t *d = malloc(sizeof(*d) * 256);
    static char line[256 * IRDM_RAW_LINE_MAX];
    int rc_all = 0;
    FILE *f = NULL;
    double t_down = 0;
    seg_t *segs = calloc((size_t)g_n_in, sizeof(*segs));
    if (!d || !segs) { fprintf(stderr, "out of memory\n"); return 1; }
    /* --prime: the capture samples that complete 512 frames in front of the detector (behind a front end: at its ratio, with
     * its taps; the library takes no more of them than it needs) */
    size_t head_cap = 0, prime_cap = 0;
    char *head = NULL;
    if (prime) {
        const size_t H = (size_t)512 * (size_t)irdm_fft_size(p);
        prime_cap = !fe ? H : (resample_to ? (H * (size_t)rs_m + (size_t)irdm_frontend_ntaps(fe)) / (size_t)rs_l + 2
                                           : H * (size_t)decimate + (size_t)irdm_frontend_ntaps(fe) + 2);
    }
    /* --dc-block: the first block, which the seed is the mean of, is kept the same way */
    head_cap = g_dc && ((size_t)1 << g_dc_log2) > prime_cap ? (size_t)1 << g_dc_log2 : prime_cap;
    if (head_cap && !(head = malloc(head_cap * bps))) { fprintf(stderr, "%s: out of memory\n", prime ? "--prime" : "--dc-block"); return 1; }
    for (int fi = 0; fi < n_rec; fi++) {
        const char *file = g_in[fi].path;
        const double t_file = now_s();
        double reset_ms = 0;
        int rc = 0;
        unsigned long long fed = 0;
        const input_t *in = &g_in[fi];
        /* (a malformed header: the probe's message, and nothing of the file is read as samples) */
        if (in->kind < 0) { fprintf(stderr, "%s\n", in->err); rc_all = 1; f = NULL; continue; }
        const char *data = in->kind > 0 ? in->info->data_path : file;
        g_n_demods = 0;
        g_n_img = 0;
        f = strcmp(file, "-") ? fopen(data, "rb") : stdin;
        if (!f) { perror(data); rc_all = 1; continue; }
        if (fi > 0) {
            /* the context and the front end as they were created, for this recording's centre frequency and capture time */
            if ((fe && irdm_frontend_reset(fe) != 0) || irdm_reset(p, fe ? c.center_frequency : in->centre, in->start_ns) != 0) {
                fprintf(stderr, "%s: the context could not be reset\n", file);
                fclose(f);
                rc_all = 1;
                break;
            }
            reset_ms = (now_s() - t_file) * 1e3;
            if (verbose) fprintf(stderr, "%s: context reset in %.3f ms\n", file, reset_ms);
        }
        if (out_dir) {
            char path[4608];
            snprintf(path, sizeof path, "%s/%s.out", out_dir, base_of(file));
            g_out = fopen(path, "w");
            if (!g_out) { perror(path); fclose(f); g_out = stdout; rc_all = 1; continue; }
        }
        if (spectrum) {
            char path[4608];
            if (!strcmp(spectrum, "auto")) snprintf(path, sizeof path, "%s/%s.spec", out_dir, base_of(file));
            else snprintf(path, sizeof path, "%s", spectrum);
            if (spectrum_open(path, p, spectrum_frames, c.sample_rate, c.center_frequency) != 0) {
                if (g_spec) fclose(g_spec);
                g_spec = NULL;
                if (out_dir) { fclose(g_out); g_out = stdout; }
                fclose(f);
                rc_all = 1;
                continue;
            }
        }
        if (save_band && band_open(save_band, out_dir, file, save_fmt) != 0) {
            if (g_spec) { fclose(g_spec); g_spec = NULL; }
            if (out_dir) { fclose(g_out); g_out = stdout; }
            fclose(f);
            rc_all = 1;
            continue;
        }
        /* the host-side objects of a recording: its line printer's t0, its IDA reassembly and ACARS state, its solver */
        if (acars) {
            irdm_acars_config_t ac;
            memset(&ac, 0, sizeof(ac));
            ac.json = acars_json;
            ac.station = station;
            ac.fixed_origin = has_origin;
            ac.origin_sec = origin_sec;
            ac.origin_nsec = origin_nsec;
            g_reasm = irdm_ida_reasm_create();
            g_acars = irdm_acars_create(&ac);
            if (!g_reasm || !g_acars) { fprintf(stderr, "--acars: out of memory\n"); return 1; }
            /* main.c:617-629, without the network endpoints this binary does not build */
            fprintf(stderr, "ACARS: enabled (%s output%s)\n", acars_json ? "JSON" : "text", station ? ", station set" : "");
        }
        if (position) {
            g_dop = irdm_doppler_create(position_height);
            if (!g_dop) { fprintf(stderr, "--position: out of memory\n"); return 1; }
            /* stream time: the frames' timestamps count from the context's start time */
            irdm_doppler_set_origin(g_dop, irdm_start_time_ns(p));
            fprintf(stderr, "Doppler positioning: enabled (height aiding: %.0f m)\n", position_height);     /* main.c:597-605 */
        }
        /* the recording's time origin: a primed context's own lies 512 frames earlier */
        const uint64_t rec_t0 = irdm_start_time_ns(p);
        /* the recording's sample regions: its own, or with --join every input's, one behind the other */
        int n_seg = 1;
        segs[0] = region_of(f, in, bps);
        if (join) {
            unsigned long long before = segs[0].bytes > 0 ? (unsigned long long)segs[0].bytes / bps : 0;
            for (int k = 1; k < g_n_in; k++) {
                const input_t *part = &g_in[k];
                const char *pd = part->kind > 0 ? part->info->data_path : part->path;
                FILE *pf = fopen(pd, "rb");
                if (!pf) { perror(pd); return 1; }
                segs[k] = region_of(pf, part, bps);
                if (part->start_ns) {
                    /* the part's own time against the stream's: said once, no gap is inserted */
                    const double late = ((double)part->start_ns - (double)rec_t0) * 1e-9 - (double)before / rate;
                    if (fabs(late) > 1e-3)
                        fprintf(stderr, "warning: --join: %s starts %.6f s %s than the stream has got to; the parts are joined without a gap\n",
                                part->path, fabs(late), late > 0 ? "later" : "earlier");
                }
                before += segs[k].bytes > 0 ? (unsigned long long)segs[k].bytes / bps : 0;
            }
            n_seg = g_n_in;
        }
        if (verbose && fi == 0) fprintf(stderr, "%s: fft_size=%d chunk=%zu samples, %d GPU%s\n", irdm_version(), irdm_fft_size(p), chunk,
                             gpus > 0 ? gpus : 1, gpus > 1 ? "s" : "");
        if (verbose && fi == 0 && fe && resample_to)
            fprintf(stderr, "front end: %d -> %d samples/s (%d/%d), %d taps, shift %.3f Hz applied (%.3f asked), centre %.3f Hz\n", (int)rate,
                    irdm_frontend_out_rate(fe), rs_l, rs_m, irdm_frontend_ntaps(fe), irdm_frontend_applied_shift_hz(fe),
                    band_given ? band_center - freq : 0.0, c.center_frequency);
        else if (verbose && fi == 0 && fe)
        fprintf(stderr, "front end: %d -> %d samples/s, %d taps, shift %.3f Hz applied (%.3f asked), centre %.3f Hz\n", (int)rate,
                    irdm_frontend_out_rate(fe), irdm_frontend_ntaps(fe), irdm_frontend_applied_shift_hz(fe), band_center - freq,
                    c.center_frequency);
        reader_t rd;
        memset(&rd, 0, sizeof(rd));
        rd.f = f;
        rd.bps = bps;
        rd.chunk = step;
        rd.remain = -1;
        if (in->kind > 0) {
            /* a container: [data_offset, data_offset + data_bytes) of the data file, for the fread path here and the slices below */
            rd.remain = (long long)in->info->data_bytes;
            if (fseeko(f, (off_t)in->info->data_offset, SEEK_SET) != 0) { perror(data); return 1; }
        }
        if (join) {
            /* the regions one behind the other, read with fread(): a chunk is filled across their edges */
            rd.segs = segs;
            rd.n_seg = n_seg;
            rd.remain = segs[0].bytes;
            for (int k = 1; k < n_seg; k++)
                if (segs[k].off && fseeko(segs[k].f, segs[k].off, SEEK_SET) != 0) { perror(g_in[k].path); return 1; }
        }
        size_t head_got = 0;
        if (head_cap) {
            head_got = read_head(segs, n_seg, bps, head_cap, head);
            if (segs[0].bytes < 0) { rd.pre = head; rd.pre_n = head_got; }
        }
        if (g_dc) {
            /* the seed: the mean of the recording's first block (of a shorter recording: of all of it), in the sense the pass
             * sees the samples in; set before anything of the recording, a --prime prefix included, reaches the GPU */
            float seed[2] = { 0.0f, 0.0f };
            const size_t nb = head_got < ((size_t)1 << g_dc_log2) ? head_got : (size_t)1 << g_dc_log2;
            if (irdm_dc_mean_host(fmt, head, nb, seed) != 0 ||
                (fe ? irdm_frontend_dc_block(fe, fmt, g_dc_log2, seed[g_swap ? 1 : 0], seed[g_swap ? 0 : 1])
                    : irdm_dc_block(p, fmt, g_dc_log2, seed[g_swap ? 1 : 0], seed[g_swap ? 0 : 1])) != 0) {
                fprintf(stderr, "--dc-block: the library refused the pass\n");
                return 1;
            }
        }
        if (prime) {
            /* the detector's history from the recording's own head, before the recording itself is fed from its sample 0 */
            const size_t got = head_got < prime_cap ? head_got : prime_cap;
            if ((fe ? irdm_frontend_prime_host(fe, p, head, got) : irdm_prime_host(p, head, got)) != 0) {
                if (irdm_sample_count(p) != 0 || irdm_primed_samples(p) != 0) {
                    fprintf(stderr, "burst_detect: GPU processing failed\n");
                    rc = 1;
                } else
                    fprintf(stderr, "warning: --prime: %s is shorter than one FFT frame; it runs unprimed\n", file);
            } else if (verbose)
                fprintf(stderr, "primed: 512 frames from the first %d\n", irdm_primed_frames(p));
        }
        rd.buf[0] = pinned[0];
        rd.buf[1] = pinned[1];
        sem_init(&rd.filled, 0, 0);
        sem_init(&rd.empty, 0, 2);
        {
            struct stat sb;
            if (!join && f != stdin && read_threads > 0 && fstat(fileno(f), &sb) == 0 && S_ISREG(sb.st_mode)) {
                rd.n_slices = read_threads > MAX_SLICES ? MAX_SLICES : read_threads;
                rd.size = sb.st_size - sb.st_size % (off_t)bps;
                if (in->kind > 0) {
                    rd.pos = (off_t)in->info->data_offset;
                    rd.size = (off_t)(in->info->data_offset + in->info->data_bytes);
                    if (rd.size > sb.st_size) rd.size = rd.pos + (sb.st_size > rd.pos ? (sb.st_size - rd.pos) / (off_t)bps * (off_t)bps : 0);
                }
                for (int i = 0; i < rd.n_slices; i++) {
                    rd.sl[i].fd = fileno(f);
                    sem_init(&rd.sl[i].go, 0, 0);
                    sem_init(&rd.sl[i].done, 0, 0);
                    if (pthread_create(&rd.sl[i].th, NULL, slice_main, &rd.sl[i]) != 0) { rd.n_slices = i; break; }
                }
            }
        }
        pthread_t th;
        if (pthread_create(&th, NULL, reader_main, &rd) != 0) { fprintf(stderr, "pthread_create failed\n"); return 1; }
        const double t_ready = now_s();
        uint64_t t0 = 0;
        for (int k = 0;; k ^= 1) {
            sem_wait(&rd.filled);
            const size_t r = rd.n[k];
            if (r == 0) break;                          /* end of file */
            if (rc == 0 && (fe ? irdm_frontend_feed_host(fe, p, rd.buf[k], r)
                               : g_group ? irdm_group_feed_host(g_group, rd.buf[k], r) : irdm_feed_host(p, rd.buf[k], r)) < 0) {
                fprintf(stderr, "burst_detect: GPU processing failed\n");
                rc = 1;
            }
            fed += r;
            sem_post(&rd.empty);                        /* irdm_feed_host has consumed the buffer when it returns */
            if (rc == 0) drain(p, d, file_info, &t0, line, sizeof line);
            if (rc == 0 && spectrum_drain(p) != 0) { fprintf(stderr, "--spectrum: writing the rows failed\n"); rc = 1; }
            if (r < step) { rd.stop = 1; sem_post(&rd.empty); break; }    /* ragged last chunk = end of stream */
        }
        rd.stop = 1;
        sem_post(&rd.empty);
        pthread_join(th, NULL);
        for (int i = 0; i < rd.n_slices; i++) {
            rd.sl[i].quit = 1;
            sem_post(&rd.sl[i].go);
            pthread_join(rd.sl[i].th, NULL);
        }
        if (rc == 0 && (fe ? irdm_frontend_flush(fe, p) : g_group ? irdm_group_flush(g_group) : irdm_flush(p)) < 0) { fprintf(stderr, "burst_detect: GPU processing failed\n"); rc = 1; }
        drain(p, d, file_info, &t0, line, sizeof line);
        fflush(g_out);
        if (g_spec) {
            if (rc == 0 && spectrum_drain(p) != 0) { fprintf(stderr, "--spectrum: writing the rows failed\n"); rc = 1; }
            if (fclose(g_spec) != 0) { fprintf(stderr, "--spectrum: writing the rows failed\n"); rc = 1; }
            g_spec = NULL;
        }
        if (g_dop && rc == 0)          /* the ticks up to the stream's end (samples / rate), then the final solve */
            position_out(irdm_doppler_finish(g_dop, rec_t0 + (uint64_t)((double)fed / rate * 1e9), g_dop_text,
                                             sizeof g_dop_text));
        if (timing) {
            const double t_done = now_s();
            if (fi == 0)
                fprintf(stderr, "irdm timing: startup %.3f s (HIP initialisation + device context), stream %.3f s for %llu samples = %.1f Msamples/s\n",
                        t_ready - t_main, t_done - t_ready, fed, t_done > t_ready ? fed / (t_done - t_ready) / 1e6 : 0.0);
            else
                fprintf(stderr, "irdm timing: %s: reset %.3f ms (context and front end back to their created state), stream %.3f s for %llu samples = %.1f Msamples/s\n",
                        file, reset_ms, t_done - t_ready, fed, t_done > t_ready ? fed / (t_done - t_ready) / 1e6 : 0.0);
        }
        fprintf(stderr, "burst_detect: tagged %lu bursts total\n",
                (unsigned long)(g_group ? (uint64_t)irdm_group_get_stat(g_group, "tagged") : irdm_tagged_bursts(p)));
        if (g_clock) {
            irdm_symbol_clock_t sc;
            if (irdm_symbol_clock(p, &sc) == 0) clock_line(&sc, (double)c.sample_rate, rate, fe != NULL, br_l != br_m);
            else { fprintf(stderr, "--clock-check: %s: no estimate\n", file); rc = 1; }
        }
        if (g_fine) {
            irdm_fine_freq_summary_t ff;
            if (irdm_fine_freq(p, &ff) == 0) freq_line(&ff);
            else { fprintf(stderr, "--fine-freq: %s: no estimate\n", file); rc = 1; }
        }
        if (g_ftime) {
            irdm_fine_time_summary_t ft;
            if (irdm_fine_time(p, &ft) == 0) time_line(&ft);
            else { fprintf(stderr, "--fine-time: %s: no estimate\n", file); rc = 1; }
        }
        if (g_iq) {
            irdm_iq_sense_t iq;
            if (irdm_iq_sense(p, &iq) == 0) iq_line(&iq);
            else { fprintf(stderr, "--iq-check: %s: no verdict\n", file); rc = 1; }
        }
        if (g_image) {
            irdm_iq_moments_t im;
            if ((fe ? irdm_frontend_iq_moments_stats(fe, &im) : irdm_iq_moments(p, &im)) == 0) image_line(&im, fe ? freq : in->centre);
            else { fprintf(stderr, "--image-check: %s: no figures\n", file); rc = 1; }
        }
        if (g_dc) {
            irdm_dc_stats_t ds;
            if ((fe ? irdm_frontend_dc_stats(fe, &ds) : irdm_dc_stats(p, &ds)) == 0) dc_line(&ds, fmt, 1);
            else { fprintf(stderr, "--dc-block: %s: no figures\n", file); rc = 1; }
        }
        if (g_scrub) {
            irdm_scrub_stats_t sb;
            if ((fe ? irdm_frontend_scrub_stats(fe, &sb) : irdm_scrub_stats(p, &sb)) == 0) scrub_line(&sb, proc_fmt, rate);
            else { fprintf(stderr, "--scrub: %s: no figures\n", file); rc = 1; }
        }
        if (g_acars) {
            char st[512];
            if (irdm_acars_format_stats(g_acars, st, sizeof st) > 0) fputs(st, stderr);      /* main.c:805-806 */
        }
        if (save_band && band_close(fe, file, save_fmt, (float)save_gain, verbose, c.center_frequency) != 0) rc = 1;
        if (save_band && has_suffix_nocase(save_band, ".sigmf-data") &&
            band_write_meta(save_band, save_fmt, irdm_frontend_out_rate(fe), c.center_frequency, rec_t0) != 0) rc = 1;
        if (g_input_stats) {
            irdm_input_stats_t is;
            if ((fe ? irdm_frontend_input_stats(fe, &is) : irdm_input_stats(p, &is)) == 0) input_line(&is, proc_fmt);
            else { fprintf(stderr, "--input-stats: %s: no statistics\n", file); rc = 1; }
        }
        if (g_diag) {
            irdm_detector_stats_t ds;
            if (irdm_detector_stats(p, &ds) == 0)
                diagnostic_line((double)fed / rate, (unsigned long)irdm_tagged_bursts(p), (unsigned long)g_n_demods,
                                ds.noise_floor_dbfs_hz, ds.peak_signal_db);
            else { fprintf(stderr, "--diagnostic: %s: no detector statistics\n", file); rc = 1; }
        }
        if (rc) rc_all = 1;
        if (fi + 1 == n_rec) break;         /* (the last recording's objects go with the process, below) */
        if (out_dir) { fclose(g_out); g_out = stdout; }
        irdm_acars_destroy(g_acars);
        irdm_ida_reasm_destroy(g_reasm);
        irdm_doppler_destroy(g_dop);
        g_acars = NULL;
        g_reasm = NULL;
        g_dop = NULL;
        if (f != stdin) fclose(f);
        f = NULL;
    }
    fflush(g_out);
    /* Everything is printed and flushed.  Giving 5-9 GB of device memory, the pinned buffers and the HIP runtime back piece
     * by piece took 0.2 s of a 0.77 s run; the process is about to end and the kernel reclaims all of it at once, so the
     * binary leaves here unless IRDM_CLEAN_EXIT=1 asks for the orderly teardown (leak checkers, embedding tests). */
    const char *ce = getenv("IRDM_CLEAN_EXIT");
    if (!(ce && ce[0] == '1')) {
        fflush(stderr);
        _exit(rc_all);
    }
    t_down = now_s();
    irdm_frontend_destroy(fe);
    if (g_group) irdm_group_destroy(g_group);
    else irdm_destroy(p);
    irdm_host_free(pinned[0]);
    irdm_host_free(pinned[1]);
    free(d);
    irdm_acars_destroy(g_acars);
    irdm_ida_reasm_destroy(g_reasm);
    irdm_doppler_destroy(g_dop);
    if (f && f != stdin) fclose(f);
    if (g_out && g_out != stdout) fclose(g_out);
    if (timing) fprintf(stderr, "irdm timing: teardown %.3f s\n", now_s() - t_down);
    return rc_all;
}
