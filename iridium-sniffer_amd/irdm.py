"""ctypes view of the C-ABI in include/irdm_hip.h (libirdm_hip.so, gfx950).

Host-side mirror used by tests, bench.py and __graft_entry__: the same entry
points a C host binds.  There is no CPU fallback here: if the
HIP library is missing or no GPU is present, creation fails loudly.
"""
import ctypes as C
import os
import subprocess

import numpy as np

PKG_DIR = os.path.dirname(os.path.abspath(__file__))
# IRDM_LIB: another build of the same library (A/B timing of kernel variants on one GPU box)
LIB_PATH = os.environ.get("IRDM_LIB") or os.path.join(PKG_DIR, "libirdm_hip.so")

FMT_CI8, FMT_CI16, FMT_CF32 = 0, 1, 2
# full-precision int16 I/Q (include/irdm_hip.h): records equal a cf32 context's on v.astype(np.float32) * FMT_SCALE[fmt]
FMT_CI16_FULL, FMT_SC16Q11 = 3, 4
FMT_SCALE = {FMT_CI16_FULL: 1.0 / 32768.0, FMT_SC16Q11: 1.0 / 2048.0}
# rtl_sdr's unsigned 8-bit I/Q (offset binary): records equal a cf32 context's on convert_cu8(u)
FMT_CU8 = 6
# 32-bit integer I/Q, interleaved int32 I, Q: records equal a cf32 context's on v.astype(np.float32) * np.float32(FMT_SCALE[fmt])
# (FMT_CI32: SigMF ci32_le, 32-bit PCM WAV; FMT_CI32_24: 24-bit samples held in int32, SDRangel's .sdriq)
FMT_CI32, FMT_CI32_24 = 8, 9
FMT_SCALE.update({FMT_CI32: 2.0 ** -31, FMT_CI32_24: 2.0 ** -23})
# irdm_recording_probe: container kinds
CONTAINER_NONE, CONTAINER_WAV, CONTAINER_SIGMF, CONTAINER_SDRIQ = 0, 1, 2, 3


def convert_ci32(v, fmt=FMT_CI32):
    """interleaved int32 I, Q -> complex64 as the load stage converts them: (float)v, rounded to nearest even, times 2^-31
    (FMT_CI32) or 2^-23 (FMT_CI32_24)"""
    v = np.ascontiguousarray(v, np.int32)
    return (v.astype(np.float32) * np.float32(FMT_SCALE[fmt])).view(np.complex64)


def convert_cu8(u):
    """interleaved uint8 I, Q -> complex64 as the load stage converts them: (u - 127.5) / 128 = (2u - 255) / 256, exact"""
    u = np.ascontiguousarray(u, np.uint8)
    x = (u.astype(np.float32) - np.float32(127.5)) / np.float32(128.0)
    return x.view(np.complex64)
MAX_FRAME_SAMPLES = 4440
MAX_BITS = 896


class Config(C.Structure):
    _fields_ = [("center_frequency", C.c_double), ("sample_rate", C.c_int),
                ("threshold_db", C.c_float), ("format", C.c_int), ("feed_block", C.c_int),
                ("use_gardner", C.c_int), ("start_time_ns", C.c_uint64), ("device", C.c_int),
                ("max_chunk_samples", C.c_size_t), ("max_bursts_per_chunk", C.c_int),
                ("pipeline_depth", C.c_int)]


class Burst(C.Structure):
    _fields_ = [("id", C.c_uint64), ("start", C.c_uint64), ("stop", C.c_uint64),
                ("last_active", C.c_uint64), ("center_bin", C.c_int32),
                ("magnitude", C.c_float), ("noise", C.c_float), ("peak_rel", C.c_float),
                ("base_sum", C.c_float), ("num_samples", C.c_uint64),
                ("avail_end", C.c_uint64)]


class FrameInfo(C.Structure):
    _fields_ = [("id", C.c_uint64), ("timestamp", C.c_uint64),
                ("center_frequency", C.c_double), ("sample_rate", C.c_float),
                ("samples_per_symbol", C.c_float), ("direction", C.c_int32),
                ("magnitude", C.c_float), ("noise", C.c_float), ("uw_start", C.c_float),
                ("num_samples", C.c_int32), ("dec_len", C.c_int32), ("start", C.c_int32),
                ("center_offset", C.c_float), ("uw_start_idx", C.c_int32),
                ("corr_re", C.c_float), ("corr_im", C.c_float), ("drop_reason", C.c_int32),
                ("demod_ok", C.c_int32), ("demod_direction", C.c_int32)]


class Demod(C.Structure):
    _fields_ = [("id", C.c_uint64), ("timestamp", C.c_uint64),
                ("center_frequency", C.c_double), ("direction", C.c_int32),
                ("magnitude", C.c_float), ("noise", C.c_float), ("confidence", C.c_int32),
                ("level", C.c_float), ("n_symbols", C.c_int32),
                ("n_payload_symbols", C.c_int32), ("n_bits", C.c_int32), ("ok", C.c_int32),
                ("total_phase", C.c_float), ("bits", C.c_uint8 * MAX_BITS),
                ("llr", C.c_float * MAX_BITS)]


class DemodPacked(C.Structure):
    """irdm_demod_packed_t: the frame without LLRs, hard bits 8 per byte (MSB first)"""
    _fields_ = [("id", C.c_uint64), ("timestamp", C.c_uint64),
                ("center_frequency", C.c_double), ("direction", C.c_int32),
                ("magnitude", C.c_float), ("noise", C.c_float), ("confidence", C.c_int32),
                ("level", C.c_float), ("n_symbols", C.c_int32),
                ("n_payload_symbols", C.c_int32), ("n_bits", C.c_int32), ("ok", C.c_int32),
                ("total_phase", C.c_float), ("bits", C.c_uint8 * (MAX_BITS // 8))]


class Decoded(C.Structure):
    _fields_ = [("type", C.c_int32), ("sat_id", C.c_int32), ("beam_id", C.c_int32), ("pos_xyz", C.c_int32 * 3),
                ("alt", C.c_int32), ("n_pages", C.c_int32), ("lat", C.c_double), ("lon", C.c_double),
                ("page_tmsi", C.c_uint32 * 12), ("page_msc", C.c_int32 * 12), ("timeslot", C.c_int32),
                ("sv_blocking", C.c_int32), ("bc_type", C.c_int32), ("iri_time", C.c_uint32),
                ("bch_len", C.c_int32), ("pad", C.c_int32), ("id", C.c_uint64), ("timestamp", C.c_uint64),
                ("frequency", C.c_double)]


class Ida(C.Structure):
    _fields_ = [("ok", C.c_int32), ("ft", C.c_int32), ("lcw_ft", C.c_int32), ("lcw_code", C.c_int32),
                ("ec_lcw", C.c_int32), ("lcw3_val", C.c_uint32), ("da_ctr", C.c_int32), ("da_len", C.c_int32),
                ("cont", C.c_int32), ("crc_ok", C.c_int32), ("stored_crc", C.c_uint32), ("computed_crc", C.c_uint32),
                ("fixederrs", C.c_int32), ("payload_len", C.c_int32), ("bch_len", C.c_int32), ("direction", C.c_int32),
                ("payload", C.c_uint8 * 32), ("bch_stream", C.c_uint8 * 256), ("lcw_header", C.c_char * 128),
                ("id", C.c_uint64), ("timestamp", C.c_uint64), ("frequency", C.c_double), ("magnitude", C.c_float),
                ("noise", C.c_float), ("level", C.c_float), ("confidence", C.c_int32), ("n_symbols", C.c_int32),
                ("pad", C.c_int32)]


class IdaPacked(C.Structure):
    """irdm_ida_packed_t: ida_decode()'s fields for one packed frame (option parsed_records); bch_stream 8 bits per byte"""
    _fields_ = [("ok", C.c_int32), ("lcw3_val", C.c_uint32), ("ft", C.c_uint8), ("lcw_ft", C.c_uint8),
                ("lcw_code", C.c_uint8), ("ec_lcw", C.c_uint8), ("da_ctr", C.c_uint8), ("da_len", C.c_uint8),
                ("cont", C.c_uint8), ("crc_ok", C.c_uint8), ("stored_crc", C.c_uint16), ("computed_crc", C.c_uint16),
                ("fixederrs", C.c_uint8), ("payload_len", C.c_uint8), ("bch_len", C.c_uint16),
                ("payload", C.c_uint8 * 32), ("bch_stream", C.c_uint8 * 32)]


class FramePacked(C.Structure):
    """irdm_frame_packed_t: frame_decode()'s fields for one packed frame (option frame_records), in narrow types"""
    _fields_ = [("type", C.c_uint8), ("sat_id", C.c_uint8), ("beam_id", C.c_uint8), ("n_pages", C.c_uint8),
                ("pos_xyz", C.c_int16 * 3), ("bch_len", C.c_uint16), ("timeslot", C.c_uint8), ("sv_blocking", C.c_uint8),
                ("bc_type", C.c_uint8), ("pad", C.c_uint8), ("iri_time", C.c_uint32), ("page_tmsi", C.c_uint32 * 12),
                ("page_msc", C.c_uint8 * 12)]


class SpectrumRow(C.Structure):
    """irdm_spectrum_row_t: header of one row of the waterfall (option spectrum_frames)"""
    _fields_ = [("row", C.c_uint64), ("first_frame", C.c_uint64), ("timestamp_ns", C.c_uint64), ("n_frames", C.c_uint32),
                ("n_bins", C.c_uint32)]


class Position(C.Structure):
    """irdm_position_t: doppler_solution_t"""
    _fields_ = [("lat", C.c_double), ("lon", C.c_double), ("alt", C.c_double), ("hdop", C.c_double),
                ("n_measurements", C.c_int32), ("n_satellites", C.c_int32), ("converged", C.c_int32), ("pad", C.c_int32)]


class IdaMessage(C.Structure):
    """irdm_ida_message_t: one reassembled IDA message (ida_message_cb's arguments)"""
    _fields_ = [("data", C.c_uint8 * 256), ("len", C.c_int32), ("direction", C.c_int32), ("timestamp", C.c_uint64),
                ("frequency", C.c_double), ("magnitude", C.c_float), ("pad", C.c_int32)]


class AcarsConfig(C.Structure):
    _fields_ = [("json", C.c_int32), ("fixed_origin", C.c_int32), ("origin_sec", C.c_int64), ("origin_nsec", C.c_int64),
                ("station", C.c_char_p)]


class AcarsStats(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("ida_total", "sbd_total", "sbd_short", "sbd_single", "sbd_multi_ok",
                                         "sbd_multi_frag", "sbd_broken", "acars_total", "acars_errors")]


class FrontendConfig(C.Structure):
    """irdm_frontend_config_t: the band-select front end (csrc/frontend.cpp)"""
    _fields_ = [("device", C.c_int), ("in_rate", C.c_int), ("in_format", C.c_int), ("decim", C.c_int),
                ("shift_hz", C.c_double)]


class FrontendRationalConfig(C.Structure):
    """irdm_frontend_rational_config_t: the front end's rational mode (csrc/resample.cpp)"""
    _fields_ = [("device", C.c_int), ("in_rate", C.c_int), ("in_format", C.c_int), ("out_rate", C.c_int),
                ("shift_hz", C.c_double)]


BAND_SINK = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_size_t)


class FrontendSaveConfig(C.Structure):
    """irdm_frontend_save_config_t: the band as a recording (csrc/frontend.cpp)"""
    _fields_ = [("format", C.c_int), ("gain", C.c_float), ("slot_samples", C.c_size_t), ("sink", BAND_SINK),
                ("user", C.c_void_p)]


class BandStats(C.Structure):
    """irdm_band_stats_t"""
    _fields_ = [("n_samples", C.c_uint64), ("n_clipped", C.c_uint64), ("peak", C.c_float)]


class InputStats(C.Structure):
    """irdm_input_stats_t (option input_stats): [0] = I, [1] = Q"""
    _fields_ = [("n_samples", C.c_uint64), ("n_rail_lo", C.c_uint64 * 2), ("n_rail_hi", C.c_uint64 * 2),
                ("n_nonfinite", C.c_uint64 * 2), ("code_min", C.c_int32 * 2), ("code_max", C.c_int32 * 2),
                ("sum", C.c_double * 2), ("sum_sq", C.c_double * 2), ("abs_max", C.c_float * 2)]


CLOCK_INVALID, CLOCK_OUT_OF_RANGE, CLOCK_NOT_OK = 1, 2, 4


class ClockEst(C.Structure):
    """irdm_clock_est_t (option symbol_clock): eps and quality of one frame, flags CLOCK_*"""
    _fields_ = [("id", C.c_uint64), ("eps", C.c_float), ("quality", C.c_float), ("flags", C.c_uint32), ("n", C.c_uint32)]


class SymbolClock(C.Structure):
    """irdm_symbol_clock_t (irdm_symbol_clock): the summary of the stream so far; median and quartiles are fractions"""
    _fields_ = [("frames_used", C.c_uint64), ("frames_not_ok", C.c_uint64), ("frames_out_of_range", C.c_uint64),
                ("median", C.c_double), ("q25", C.c_double), ("q75", C.c_double), ("implied_rate_hz", C.c_double),
                ("frames_invalid", C.c_uint64)]


IQ_IRA, IQ_IBC, IQ_IDA = 1, 2, 4
IQ_TOO_FEW, IQ_AS_RECORDED, IQ_EXCHANGED, IQ_MIXED = 0, 1, 2, 3


class IqVote(C.Structure):
    """irdm_iq_vote_t (option iq_sense): the predicates IQ_* that hold on a frame's bits as recorded and with I and Q exchanged"""
    _fields_ = [("id", C.c_uint64), ("recorded", C.c_uint8), ("exchanged", C.c_uint8), ("pad", C.c_uint16), ("n_bits", C.c_uint32)]


class IqSense(C.Structure):
    """irdm_iq_sense_t (irdm_iq_sense): the votes of the stream so far (kind index 0 IRA, 1 IBC, 2 IDA) and the verdict IQ_*"""
    _fields_ = [("frames", C.c_uint64), ("votes_recorded", C.c_uint64), ("votes_exchanged", C.c_uint64), ("votes_both", C.c_uint64),
                ("kind_recorded", C.c_uint64 * 3), ("kind_exchanged", C.c_uint64 * 3), ("kind_both", C.c_uint64 * 3),
                ("verdict", C.c_int32), ("pad", C.c_int32)]


SCRUB_DEFAULT_LOG2 = 40


class ScrubStats(C.Structure):
    """irdm_scrub_stats_t (option scrub): what the pass has zeroed; first / last are stream positions, valid when n_zeroed > 0"""
    _fields_ = [("n_samples", C.c_uint64), ("n_zeroed", C.c_uint64), ("n_nonfinite", C.c_uint64), ("n_over", C.c_uint64),
                ("first", C.c_uint64), ("last", C.c_uint64), ("limit_log2", C.c_int32), ("active", C.c_int32)]


class IqMoments(C.Structure):
    """irdm_iq_moments_t (option iq_moments): the second moments of I and Q and the imbalance derived from them"""
    _fields_ = [("n_samples", C.c_uint64), ("n_used", C.c_uint64), ("sum_i", C.c_double), ("sum_q", C.c_double),
                ("sum_ii", C.c_double), ("sum_qq", C.c_double), ("sum_iq", C.c_double), ("gain_db", C.c_double),
                ("phase_deg", C.c_double), ("image_db", C.c_double), ("valid", C.c_int), ("reserved", C.c_int)]


DC_DEFAULT_LOG2 = 20


class DcState(C.Structure):
    """irdm_dc_state_t (irdm_dc_block_device): the open block's sums and the mean it is corrected by"""
    _fields_ = [("sum_i", C.c_int64), ("sum_q", C.c_int64), ("mean_i", C.c_float), ("mean_q", C.c_float)]


class DcStats(C.Structure):
    """irdm_dc_stats_t (irdm_dc_block): samples, whole blocks, the seed, and the first, last, smallest and largest block mean"""
    _fields_ = [("n_samples", C.c_uint64), ("n_blocks", C.c_uint64), ("block_log2", C.c_int), ("wire_format", C.c_int),
                ("seed_i", C.c_float), ("seed_q", C.c_float), ("first_i", C.c_float), ("first_q", C.c_float),
                ("last_i", C.c_float), ("last_q", C.c_float), ("min_i", C.c_float), ("max_i", C.c_float),
                ("min_q", C.c_float), ("max_q", C.c_float)]


FINE_FREQ_INVALID, FINE_FREQ_OUT_OF_RANGE, FINE_FREQ_NOT_OK = 1, 2, 4


class FineFreq(C.Structure):
    """irdm_fine_freq_t (option fine_freq): the carrier frequency of one frame from its own samples, flags FINE_FREQ_*"""
    _fields_ = [("id", C.c_uint64), ("freq_hz", C.c_double), ("df_hz", C.c_float), ("quality", C.c_float),
                ("flags", C.c_uint32), ("n", C.c_uint32)]


FINE_TIME_INVALID, FINE_TIME_AMBIGUOUS, FINE_TIME_NOT_OK = 1, 2, 4


class FineTime(C.Structure):
    """irdm_fine_time_t (option fine_time): the time of one frame's sample 0 from its own samples, flags FINE_TIME_*"""
    _fields_ = [("id", C.c_uint64), ("time_ns", C.c_uint64), ("tau", C.c_double), ("s_re", C.c_double), ("s_im", C.c_double),
                ("floor", C.c_double), ("corr", C.c_float), ("quality", C.c_float), ("flags", C.c_uint32), ("n", C.c_uint32)]


class FineTimeSummary(C.Structure):
    """irdm_fine_time_summary_t (irdm_fine_time): the summary of the stream so far; median and quartiles of tau - corr in samples"""
    _fields_ = [("frames_seen", C.c_uint64), ("frames_applied", C.c_uint64), ("frames_not_ok", C.c_uint64),
                ("frames_ambiguous", C.c_uint64), ("frames_invalid", C.c_uint64),
                ("median", C.c_double), ("q25", C.c_double), ("q75", C.c_double)]


class FineFreqSummary(C.Structure):
    """irdm_fine_freq_summary_t (irdm_fine_freq): the summary of the stream so far; median and quartiles of refined - PLL in Hz"""
    _fields_ = [("frames_seen", C.c_uint64), ("frames_applied", C.c_uint64), ("frames_not_ok", C.c_uint64),
                ("frames_out_of_range", C.c_uint64), ("frames_invalid", C.c_uint64),
                ("median", C.c_double), ("q25", C.c_double), ("q75", C.c_double)]


class RecordingInfo(C.Structure):
    """irdm_recording_info_t (irdm_recording_probe)"""
    _fields_ = [("kind", C.c_int), ("format", C.c_int), ("sample_rate", C.c_int), ("has_center", C.c_int),
                ("center_frequency", C.c_double), ("has_start", C.c_int), ("n_captures", C.c_int),
                ("start_time_ns", C.c_uint64), ("data_offset", C.c_uint64), ("data_bytes", C.c_uint64),
                ("data_path", C.c_char * 4096)]


ACARS_LINE_MAX = 8192
RAW_LINE_MAX = 1280
_lib = None


def recording_probe(path, container=CONTAINER_NONE):
    """irdm_recording_probe (host code only, no GPU needed): (rc, RecordingInfo, message) -- rc 0 a container was recognised,
    1 not a container (a raw file), -1 malformed or unsupported, and the message says what and where"""
    info = RecordingInfo()
    err = C.create_string_buffer(1024)
    rc = lib().irdm_recording_probe(os.fsencode(str(path)), int(container), C.byref(info), err, len(err))
    return rc, info, err.value.decode(errors="replace")


def build(force=False):
    """hipcc --offload-arch=gfx950 ... -> iridium-sniffer_amd/libirdm_hip.so (in-tree)."""
    if force or not os.path.exists(LIB_PATH):
        subprocess.check_call(["make", "-s", "-C", PKG_DIR, "-j8"])
    return LIB_PATH


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError("libirdm_hip.so is not built (run __graft_entry__.build()); "
                               "there is no CPU fallback for the product path")
        L = C.CDLL(LIB_PATH)
        L.gpu_burst_fft_create.restype = C.c_void_p
        L.gpu_burst_fft_create.argtypes = [C.c_int, C.c_int, C.POINTER(C.c_float)]
        L.gpu_burst_fft_destroy.argtypes = [C.c_void_p]
        L.gpu_burst_fft_process.argtypes = [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_int]
        L.gpu_burst_fft_process_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        L.irdm_create.restype = C.c_void_p
        L.irdm_create.argtypes = [C.POINTER(Config)]
        L.irdm_destroy.argtypes = [C.c_void_p]
        L.irdm_feed_device.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
        L.irdm_feed_host.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
        L.irdm_flush.argtypes = [C.c_void_p]
        if hasattr(L, "irdm_reset"):                       # (IRDM_LIB may name an older build, for A/B timing)
            L.irdm_reset.argtypes = [C.c_void_p, C.c_double, C.c_uint64]
        if hasattr(L, "irdm_advance"):
            L.irdm_advance.argtypes = [C.c_void_p]
        if hasattr(L, "irdm_prime_host"):
            L.irdm_prime_host.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
            L.irdm_prime_device.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
            L.irdm_primed_samples.argtypes = [C.c_void_p]
            L.irdm_primed_samples.restype = C.c_uint64
            L.irdm_primed_frames.argtypes = [C.c_void_p]
            L.irdm_start_time_ns.argtypes = [C.c_void_p]
            L.irdm_start_time_ns.restype = C.c_uint64
            if hasattr(L, "irdm_frontend_prime_host"):
                L.irdm_frontend_prime_host.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]
        if hasattr(L, "irdm_poll_spectrum"):
            L.irdm_spectrum_bins.argtypes = [C.c_void_p]
            L.irdm_poll_spectrum.argtypes = [C.c_void_p, C.POINTER(SpectrumRow), C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_int]
        if hasattr(L, "irdm_input_stats"):
            L.irdm_input_stats.argtypes = [C.c_void_p, C.POINTER(InputStats)]
            L.irdm_input_stats_device.argtypes = [C.c_void_p, C.c_size_t, C.c_int, C.POINTER(InputStats), C.c_int, C.c_void_p]
        if hasattr(L, "irdm_symbol_clock"):
            L.irdm_poll_symbol_clock.argtypes = [C.c_void_p, C.POINTER(ClockEst), C.c_int]
            L.irdm_symbol_clock.argtypes = [C.c_void_p, C.POINTER(SymbolClock)]
            L.irdm_symbol_clock_batch.argtypes = [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_int), C.c_int, C.POINTER(ClockEst)]
        if hasattr(L, "irdm_burst_resample_batch"):
            L.irdm_burst_resample_ratio.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]
            L.irdm_burst_resample_taps.argtypes = [C.c_void_p, C.POINTER(C.c_float), C.c_int]
            L.irdm_burst_resample_design.argtypes = [C.c_int, C.c_int, C.POINTER(C.c_float), C.c_int]
            L.irdm_burst_resample_batch.argtypes = [C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_int), C.c_int, C.c_int, C.c_int,
                                                    C.c_int, C.POINTER(C.c_float), C.c_int, C.POINTER(C.c_int)]
        if hasattr(L, "irdm_iq_sense"):
            L.irdm_swap_iq_device.argtypes = [C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.c_void_p]
            L.irdm_poll_iq_votes.argtypes = [C.c_void_p, C.POINTER(IqVote), C.c_int]
            L.irdm_iq_sense.argtypes = [C.c_void_p, C.POINTER(IqSense)]
            L.irdm_iq_sense_batch.argtypes = [C.c_void_p, C.POINTER(Demod), C.c_int, C.POINTER(IqVote)]
        if hasattr(L, "irdm_scrub_device"):
            L.irdm_scrub_device.argtypes = [C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.POINTER(ScrubStats), C.c_int, C.c_void_p]
            L.irdm_scrub_stats.argtypes = [C.c_void_p, C.POINTER(ScrubStats)]
        if hasattr(L, "irdm_iq_moments_device"):
            L.irdm_iq_moments.argtypes = [C.c_void_p, C.POINTER(IqMoments)]
            L.irdm_iq_moments_device.argtypes = [C.c_void_p, C.c_size_t, C.c_int, C.POINTER(IqMoments), C.c_int, C.c_void_p]
            L.irdm_iq_balance_coeffs.argtypes = [C.c_double, C.c_double, C.POINTER(C.c_float), C.POINTER(C.c_float)]
            L.irdm_iq_balance_device.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_float, C.c_float, C.c_int, C.c_void_p]
            L.irdm_iq_balance.argtypes = [C.c_void_p, C.c_int, C.c_double, C.c_double]
        if hasattr(L, "irdm_dc_block_device"):
            L.irdm_dc_mean_host.argtypes = [C.c_int, C.c_void_p, C.c_size_t, C.POINTER(C.c_float)]
            L.irdm_dc_block_device.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_uint64, C.POINTER(DcState),
                                               C.c_void_p]
            L.irdm_dc_block.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_float]
            L.irdm_dc_stats.argtypes = [C.c_void_p, C.POINTER(DcStats)]
            L.irdm_dc_block_time_device.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.POINTER(C.c_float)]
        if hasattr(L, "irdm_fine_freq"):
            L.irdm_poll_fine_freq.argtypes = [C.c_void_p, C.POINTER(FineFreq), C.c_int]
            L.irdm_fine_freq.argtypes = [C.c_void_p, C.POINTER(FineFreqSummary)]
            L.irdm_fine_freq_batch.argtypes = [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_int), C.c_int, C.POINTER(FineFreq)]
        if hasattr(L, "irdm_fine_time"):
            L.irdm_poll_fine_time.argtypes = [C.c_void_p, C.POINTER(FineTime), C.c_int]
            L.irdm_fine_time.argtypes = [C.c_void_p, C.POINTER(FineTimeSummary)]
            L.irdm_fine_time_batch.argtypes = [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_int,
                                               C.POINTER(FineTime)]
        if hasattr(L, "irdm_recording_probe"):
            L.irdm_recording_probe.argtypes = [C.c_char_p, C.c_int, C.POINTER(RecordingInfo), C.c_char_p, C.c_size_t]
        if hasattr(L, "irdm_format_bytes"):
            L.irdm_format_bytes.argtypes = [C.c_int]
            L.irdm_format_bytes.restype = C.c_size_t
        L.irdm_host_alloc.argtypes = [C.c_size_t]
        L.irdm_host_alloc.restype = C.c_void_p
        L.irdm_host_free.argtypes = [C.c_void_p]
        L.irdm_host_free.restype = None
        L.irdm_feed_begin.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
        L.irdm_feed_end.argtypes = [C.c_void_p]
        L.irdm_ingest_ptr.argtypes = [C.c_void_p, C.c_size_t]
        L.irdm_ingest_ptr.restype = C.c_void_p
        L.irdm_ring_ptr.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
        L.irdm_ring_ptr.restype = C.c_void_p
        L.irdm_export_state_device.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
        L.irdm_export_state_device.restype = C.c_longlong
        L.irdm_import_state_device.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
        L.irdm_state_head_bytes.argtypes = [C.c_void_p]
        L.irdm_state_head_bytes.restype = C.c_size_t
        L.irdm_import_state_head_device.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
        L.irdm_expect_history.argtypes = [C.c_void_p, C.c_void_p]
        L.irdm_import_state_history_device.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
        L.irdm_seed_history_device.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint64]
        L.irdm_device_alloc.argtypes = [C.c_int, C.c_size_t]
        L.irdm_device_alloc.restype = C.c_void_p
        L.irdm_device_free.argtypes = [C.c_void_p]
        L.irdm_device_free.restype = None
        L.irdm_device_upload.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
        L.irdm_device_copy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
        L.irdm_poll_bursts.argtypes = [C.c_void_p, C.POINTER(Burst), C.c_int]
        L.irdm_poll_frames.argtypes = [C.c_void_p, C.POINTER(FrameInfo), C.POINTER(C.c_float), C.c_int]
        L.irdm_poll_demods.argtypes = [C.c_void_p, C.POINTER(Demod), C.c_int]
        L.irdm_poll_demods_packed.argtypes = [C.c_void_p, C.POINTER(DemodPacked), C.c_int]
        L.irdm_poll_decoded.argtypes = [C.c_void_p, C.POINTER(Decoded), C.c_int]
        L.irdm_poll_ida.argtypes = [C.c_void_p, C.POINTER(Ida), C.c_int]
        L.irdm_poll_ida_packed.argtypes = [C.c_void_p, C.POINTER(IdaPacked), C.c_int]
        L.irdm_ida_unpack.argtypes = [C.POINTER(IdaPacked), C.POINTER(DemodPacked), C.POINTER(Ida)]
        L.irdm_poll_frame_packed.argtypes = [C.c_void_p, C.POINTER(FramePacked), C.c_int]
        L.irdm_frame_unpack.argtypes = [C.POINTER(FramePacked), C.POINTER(DemodPacked), C.POINTER(Decoded)]
        L.irdm_ida_unpack.restype = None
        L.irdm_format_ida.argtypes = [C.POINTER(Ida), C.POINTER(C.c_uint64), C.c_char_p, C.c_size_t]
        L.irdm_format_parsed_packed_batch.argtypes = [C.POINTER(DemodPacked), C.POINTER(IdaPacked), C.c_int, C.c_char_p,
                                                      C.POINTER(C.c_uint64), C.c_char_p, C.c_size_t]
        L.irdm_format_parsed_packed_batch.restype = C.c_longlong
        L.irdm_ida_decode_batch.argtypes = [C.c_void_p, C.POINTER(Demod), C.c_int, C.c_int, C.POINTER(Ida)]
        L.irdm_frame_decode_batch.argtypes = [C.c_void_p, C.POINTER(Demod), C.c_int, C.c_int, C.POINTER(Decoded)]
        L.irdm_ida_packed_batch.argtypes = [C.c_void_p, C.POINTER(Demod), C.c_int, C.POINTER(IdaPacked)]
        L.irdm_frame_packed_batch.argtypes = [C.c_void_p, C.POINTER(Demod), C.c_int, C.POINTER(FramePacked)]
        L.irdm_tagged_bursts.argtypes = [C.c_void_p]
        L.irdm_tagged_bursts.restype = C.c_uint64
        L.irdm_sample_count.argtypes = [C.c_void_p]
        L.irdm_sample_count.restype = C.c_uint64
        L.irdm_fft_size.argtypes = [C.c_void_p]
        L.irdm_set_stream_origin.argtypes = [C.c_void_p, C.c_double, C.c_uint64]
        L.irdm_last_magnitudes.argtypes = [C.c_void_p, C.POINTER(C.c_float), C.c_size_t]
        L.irdm_baseline_sum.argtypes = [C.c_void_p, C.POINTER(C.c_float)]
        L.irdm_burst_samples.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_float), C.c_size_t]
        L.irdm_downmix_burst.argtypes = [C.c_void_p, C.POINTER(Burst), C.POINTER(C.c_float), C.c_size_t,
                                         C.POINTER(FrameInfo), C.POINTER(C.c_float)]
        L.irdm_qpsk_demod_batch.argtypes = [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_int),
                                            C.POINTER(C.c_int), C.c_int, C.POINTER(Demod)]
        L.irdm_qpsk_demod_packed_batch.argtypes = [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_int),
                                                   C.POINTER(C.c_int), C.c_int, C.c_int, C.POINTER(DemodPacked),
                                                   C.POINTER(Demod)]
        L.irdm_state_bytes.argtypes = [C.c_void_p]
        L.irdm_state_bytes.restype = C.c_size_t
        L.irdm_export_state.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
        L.irdm_export_state.restype = C.c_longlong
        L.irdm_import_state.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
        L.irdm_seed_history.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint64]
        L.irdm_set_option.argtypes = [C.c_void_p, C.c_char_p, C.c_int]
        L.irdm_get_stat.argtypes = [C.c_void_p, C.c_char_p]
        L.irdm_get_stat.restype = C.c_int64
        L.irdm_last_timings.argtypes = [C.c_void_p, C.POINTER(C.c_float), C.c_int]
        L.irdm_kernel_clock.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_uint64), C.POINTER(C.c_double), C.c_int]
        L.irdm_format_raw.argtypes = [C.POINTER(Demod), C.c_char_p, C.POINTER(C.c_uint64), C.c_char_p, C.c_size_t]
        L.irdm_version.restype = C.c_char_p
        # a group: one stream across several GPUs of this process (csrc/group.cpp)
        L.irdm_group_create.restype = C.c_void_p
        L.irdm_group_create.argtypes = [C.POINTER(Config), C.c_int, C.POINTER(C.c_int)]
        L.irdm_group_destroy.argtypes = [C.c_void_p]
        L.irdm_group_destroy.restype = None
        L.irdm_group_size.argtypes = [C.c_void_p]
        L.irdm_group_member.argtypes = [C.c_void_p, C.c_int]
        L.irdm_group_member.restype = C.c_void_p
        L.irdm_group_set_option.argtypes = [C.c_void_p, C.c_char_p, C.c_int]
        L.irdm_group_get_stat.argtypes = [C.c_void_p, C.c_char_p]
        L.irdm_group_get_stat.restype = C.c_int64
        for name in ("irdm_group_stage_host", "irdm_group_stage_device", "irdm_group_feed_host", "irdm_group_feed_device"):
            getattr(L, name).argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
        L.irdm_group_flush.argtypes = [C.c_void_p]
        L.irdm_group_poll_bursts.argtypes = [C.c_void_p, C.POINTER(Burst), C.c_int]
        L.irdm_group_poll_frames.argtypes = [C.c_void_p, C.POINTER(FrameInfo), C.POINTER(C.c_float), C.c_int]
        L.irdm_group_poll_demods.argtypes = [C.c_void_p, C.POINTER(Demod), C.c_int]
        L.irdm_group_poll_demods_packed.argtypes = [C.c_void_p, C.POINTER(DemodPacked), C.c_int]
        L.irdm_group_poll_decoded.argtypes = [C.c_void_p, C.POINTER(Decoded), C.c_int]
        L.irdm_group_poll_ida.argtypes = [C.c_void_p, C.POINTER(Ida), C.c_int]
        L.irdm_group_poll_ida_packed.argtypes = [C.c_void_p, C.POINTER(IdaPacked), C.c_int]
        L.irdm_group_poll_frame_packed.argtypes = [C.c_void_p, C.POINTER(FramePacked), C.c_int]
        L.irdm_chunks_complete.argtypes = [C.c_void_p]
        L.irdm_chunks_complete.restype = C.c_uint64
        L.irdm_required_overlap.argtypes = [C.c_void_p]
        L.irdm_required_overlap.restype = C.c_size_t
        L.irdm_max_chunk_samples.argtypes = [C.c_void_p]
        L.irdm_max_chunk_samples.restype = C.c_size_t
        L.irdm_bytes_per_sample.argtypes = [C.c_void_p]
        L.irdm_bytes_per_sample.restype = C.c_size_t
        L.irdm_wait_ingest.argtypes = [C.c_void_p]
        if hasattr(L, "irdm_doppler_create"):              # (csrc/doppler.cpp; the emulated test build leaves it out)
            L.irdm_doppler_create.restype = C.c_void_p
            L.irdm_doppler_create.argtypes = [C.c_double]
            L.irdm_doppler_destroy.argtypes = [C.c_void_p]
            L.irdm_doppler_add.argtypes = [C.c_void_p, C.POINTER(Decoded)]
            L.irdm_doppler_solve.argtypes = [C.c_void_p, C.POINTER(Position)]
            L.irdm_doppler_set_origin.argtypes = [C.c_void_p, C.c_uint64]
            L.irdm_format_doppler_packed_batch.restype = C.c_longlong
            L.irdm_format_doppler_packed_batch.argtypes = [C.c_void_p, C.POINTER(DemodPacked), C.POINTER(FramePacked),
                                                           C.c_int, C.c_char_p, C.c_size_t]
            L.irdm_format_doppler_batch.restype = C.c_longlong
            L.irdm_format_doppler_batch.argtypes = [C.c_void_p, C.POINTER(Decoded), C.c_int, C.c_char_p, C.c_size_t]
            L.irdm_doppler_finish.restype = C.c_longlong
            L.irdm_doppler_finish.argtypes = [C.c_void_p, C.c_uint64, C.c_char_p, C.c_size_t]
        if hasattr(L, "irdm_ida_reasm_create"):            # (csrc/acars.cpp; the emulated test build leaves it out)
            L.irdm_ida_reasm_create.restype = C.c_void_p
            L.irdm_ida_reasm_create.argtypes = []
            L.irdm_ida_reasm_destroy.argtypes = [C.c_void_p]
            L.irdm_ida_reasm_push.argtypes = [C.c_void_p, C.POINTER(Ida), C.c_int, C.POINTER(IdaMessage), C.c_int]
            L.irdm_ida_reasm_push_packed.argtypes = [C.c_void_p, C.POINTER(DemodPacked), C.POINTER(IdaPacked), C.c_int,
                                                     C.POINTER(IdaMessage), C.c_int]
            L.irdm_acars_create.restype = C.c_void_p
            L.irdm_acars_create.argtypes = [C.POINTER(AcarsConfig)]
            L.irdm_acars_destroy.argtypes = [C.c_void_p]
            L.irdm_acars_feed.restype = C.c_longlong
            L.irdm_acars_feed.argtypes = [C.c_void_p, C.POINTER(IdaMessage), C.c_int, C.c_char_p, C.c_size_t]
            L.irdm_acars_stats.argtypes = [C.c_void_p, C.POINTER(AcarsStats)]
            L.irdm_acars_format_stats.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t]
            for name, rec, ida in (("irdm_format_acars_packed_batch", DemodPacked, IdaPacked),
                                   ("irdm_format_acars_batch", Demod, Ida)):
                getattr(L, name).restype = C.c_longlong
                getattr(L, name).argtypes = [C.c_void_p, C.c_void_p, C.POINTER(rec), C.POINTER(ida), C.c_int, C.c_int,
                                             C.POINTER(C.c_uint64), C.c_char_p, C.c_size_t]
        if hasattr(L, "irdm_frontend_create"):             # (csrc/frontend.cpp)
            L.irdm_device_download.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
            L.irdm_frontend_create.restype = C.c_void_p
            L.irdm_frontend_create.argtypes = [C.POINTER(FrontendConfig)]
            L.irdm_frontend_destroy.argtypes = [C.c_void_p]
            L.irdm_frontend_destroy.restype = None
            L.irdm_frontend_out_rate.argtypes = [C.c_void_p]
            L.irdm_frontend_applied_shift_hz.argtypes = [C.c_void_p]
            L.irdm_frontend_applied_shift_hz.restype = C.c_double
            L.irdm_frontend_ntaps.argtypes = [C.c_void_p]
            L.irdm_frontend_taps.argtypes = [C.c_void_p, C.POINTER(C.c_float), C.c_int]
            L.irdm_frontend_run_device.restype = C.c_longlong
            L.irdm_frontend_run_device.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p]
            L.irdm_frontend_finish_device.restype = C.c_longlong
            L.irdm_frontend_finish_device.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
            L.irdm_frontend_feed_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
            L.irdm_frontend_feed_host.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]
            L.irdm_frontend_flush.argtypes = [C.c_void_p, C.c_void_p]
            L.irdm_frontend_wait_input.argtypes = [C.c_void_p]
            if hasattr(L, "irdm_frontend_reset"):
                L.irdm_frontend_reset.argtypes = [C.c_void_p]
            if hasattr(L, "irdm_frontend_seek"):
                L.irdm_frontend_seek.argtypes = [C.c_void_p, C.c_uint64]
            L.irdm_frontend_kernel_clock.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_uint64), C.c_int]
            if hasattr(L, "irdm_frontend_save"):
                L.irdm_frontend_save.argtypes = [C.c_void_p, C.POINTER(FrontendSaveConfig)]
                L.irdm_frontend_save_stats.argtypes = [C.c_void_p, C.POINTER(BandStats)]
                L.irdm_requantize_device.argtypes = [C.c_void_p, C.c_size_t, C.c_int, C.c_float, C.c_void_p, C.POINTER(BandStats),
                                                     C.c_int, C.c_void_p]
            if hasattr(L, "irdm_frontend_input_stats"):
                L.irdm_frontend_input_stats_enable.argtypes = [C.c_void_p, C.c_int]
                L.irdm_frontend_input_stats.argtypes = [C.c_void_p, C.POINTER(InputStats)]
            if hasattr(L, "irdm_frontend_swap_iq"):
                L.irdm_frontend_swap_iq.argtypes = [C.c_void_p, C.c_int]
            if hasattr(L, "irdm_frontend_scrub"):
                L.irdm_frontend_scrub.argtypes = [C.c_void_p, C.c_int, C.c_int]
                L.irdm_frontend_scrub_stats.argtypes = [C.c_void_p, C.POINTER(ScrubStats)]
            if hasattr(L, "irdm_frontend_iq_moments"):
                L.irdm_frontend_iq_moments.argtypes = [C.c_void_p, C.c_int]
                L.irdm_frontend_iq_moments_stats.argtypes = [C.c_void_p, C.POINTER(IqMoments)]
                L.irdm_frontend_iq_balance.argtypes = [C.c_void_p, C.c_int, C.c_double, C.c_double]
            if hasattr(L, "irdm_frontend_dc_block"):
                L.irdm_frontend_dc_block.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_float]
                L.irdm_frontend_dc_stats.argtypes = [C.c_void_p, C.POINTER(DcStats)]
            if hasattr(L, "irdm_frontend_create_rational"):    # (csrc/resample.cpp)
                L.irdm_frontend_create_rational.restype = C.c_void_p
                L.irdm_frontend_create_rational.argtypes = [C.POINTER(FrontendRationalConfig)]
                L.irdm_frontend_ratio.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int)]
                L.irdm_frontend_rational_ratio.argtypes = [C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]
            if hasattr(L, "irdm_frontend_create_wide"):        # (csrc/resample_wide.cpp)
                for name in ("irdm_frontend_create_wide", "irdm_frontend_create_resampler"):
                    getattr(L, name).restype = C.c_void_p
                    getattr(L, name).argtypes = [C.POINTER(FrontendRationalConfig)]
                L.irdm_frontend_resampler_ratio.argtypes = [C.c_int, C.c_int] + [C.POINTER(C.c_int)] * 3
                L.irdm_frontend_wide_geometry.argtypes = [C.c_int, C.c_int] + [C.POINTER(C.c_int)] * 4
        _lib = L
    return _lib


def _fp(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def host_alloc(nbytes):
    """Pinned host buffer (irdm_host_alloc) as (pointer, numpy uint8 view); release with host_free(pointer)."""
    L = lib()
    ptr = L.irdm_host_alloc(nbytes)
    if not ptr:
        raise MemoryError("irdm_host_alloc(%d) failed" % nbytes)
    view = np.ctypeslib.as_array((C.c_uint8 * nbytes).from_address(ptr))
    return ptr, view


def device_buffer(array, device=0):
    """Copy a numpy array into a device buffer allocated by the library (irdm_device_alloc + irdm_device_upload);
    returns the device pointer, release with device_free(pointer)."""
    L = lib()
    a = np.ascontiguousarray(array)
    ptr = L.irdm_device_alloc(device, a.nbytes)
    if not ptr:
        raise MemoryError("irdm_device_alloc(%d) failed" % a.nbytes)
    if L.irdm_device_upload(ptr, a.ctypes.data_as(C.c_void_p), a.nbytes) != 0:
        L.irdm_device_free(ptr)
        raise RuntimeError("irdm_device_upload failed")
    return ptr


def device_download(array, ptr):
    """Copy array.nbytes from the device address ptr into the (contiguous) numpy array (irdm_device_download)."""
    if lib().irdm_device_download(array.ctypes.data_as(C.c_void_p), C.c_void_p(ptr), array.nbytes) != 0:
        raise RuntimeError("irdm_device_download failed")


def device_free(ptr):
    lib().irdm_device_free(ptr)


def requantize_device(d_in, n, fmt, gain, d_out, device=0, stream=None):
    """irdm_requantize_device: n cf32 samples at the device address d_in -> d_out as ci8 / ci16 (FMT_CI16: all 16 bits) / cf32;
    returns (n_samples, n_clipped, peak) of this call"""
    st = BandStats()
    if lib().irdm_requantize_device(C.c_void_p(d_in), n, fmt, float(gain), C.c_void_p(d_out), C.byref(st), device,
                                    C.c_void_p(stream or 0)) != 0:
        raise RuntimeError("irdm_requantize_device failed")
    return int(st.n_samples), int(st.n_clipped), np.float32(st.peak)


def input_stats_device(d_in, n, fmt, device=0, stream=None):
    """irdm_input_stats_device: the InputStats of the n samples of format fmt at the device address d_in alone"""
    st = InputStats()
    if lib().irdm_input_stats_device(C.c_void_p(d_in), n, fmt, C.byref(st), device, C.c_void_p(stream or 0)) != 0:
        raise RuntimeError("irdm_input_stats_device failed")
    return st


def swap_iq_device(d_iq, n, fmt, device=0, stream=None):
    """irdm_swap_iq_device: I and Q of the n samples of format fmt at the device address d_iq exchanged in place; returns
    the call's result (0, or -1 for an unknown format or a pointer that is not sample-aligned)"""
    return int(lib().irdm_swap_iq_device(C.c_void_p(d_iq), n, fmt, device, C.c_void_p(stream or 0)))


def scrub_device(d_iq, n, fmt, limit_log2=SCRUB_DEFAULT_LOG2, stats=True, device=0, stream=None):
    """irdm_scrub_device: every cf32 sample of the n at the device address d_iq with a component that is not finite or beyond
    +-2^limit_log2 zeroed in place.  Returns (rc, ScrubStats with positions relative to the buffer, or None without stats):
    rc 0, or -1 for an unknown format, a pointer that is not sample-aligned or a limit outside 0 .. 127"""
    st = ScrubStats() if stats else None
    rc = int(lib().irdm_scrub_device(C.c_void_p(d_iq), n, fmt, limit_log2, C.byref(st) if stats else None, device,
                                     C.c_void_p(stream or 0)))
    return rc, st


def iq_moments_device(d_iq, n, fmt, device=0, stream=None, stats=True):
    """irdm_iq_moments_device: (rc, IqMoments) of the n samples of format fmt at the device address d_iq alone; stats False
    (with a stream): the launches alone, without waiting -- (rc, None)"""
    st = IqMoments() if stats else None
    rc = int(lib().irdm_iq_moments_device(C.c_void_p(d_iq), n, fmt, C.byref(st) if stats else None, device, C.c_void_p(stream or 0)))
    return rc, st


def iq_balance_coeffs(gain_db, phase_deg):
    """irdm_iq_balance_coeffs: (alpha, beta) as np.float32 for a Q arm gain_db above the I arm and phase_deg off quadrature;
    None outside |gain_db| <= 6, |phase_deg| <= 30"""
    a, b = C.c_float(), C.c_float()
    if lib().irdm_iq_balance_coeffs(float(gain_db), float(phase_deg), C.byref(a), C.byref(b)) != 0:
        return None
    return np.float32(a.value), np.float32(b.value)


def iq_balance_device(d_out, d_in, n, fmt, alpha, beta, device=0, stream=None):
    """irdm_iq_balance_device: the n samples of format fmt at d_in become cf32 at d_out, i' = i, q' = alpha i + beta q;
    returns the call's result (0 or -1)"""
    return int(lib().irdm_iq_balance_device(C.c_void_p(d_out), C.c_void_p(d_in), n, fmt, float(alpha), float(beta), device,
                                            C.c_void_p(stream or 0)))


def dc_mean_host(fmt, raw, n):
    """irdm_dc_mean_host: (mean_i, mean_q) as np.float32 of the n leading samples of format fmt in the array `raw`, by the
    rule of irdm_dc_block; None where the call refuses"""
    raw = np.ascontiguousarray(raw)
    out = (C.c_float * 2)()
    if lib().irdm_dc_mean_host(fmt, raw.ctypes.data_as(C.c_void_p), n, out) != 0:
        return None
    return np.float32(out[0]), np.float32(out[1])


def dc_block_device(fmt, d_out, d_in, n, block_log2, first_sample, state, stream=None):
    """irdm_dc_block_device: the n samples of format fmt at d_in, which lie at stream position first_sample, become cf32 at
    d_out less the mean of the block in front of their own; state (a DcState) carries the stream from call to call.
    Returns the call's result (0 or -1)"""
    return int(lib().irdm_dc_block_device(fmt, C.c_void_p(d_out), C.c_void_p(d_in), n, block_log2, first_sample, C.byref(state),
                                          C.c_void_p(stream or 0)))


def dc_block_time_device(fmt, d_out, d_in, n, block_log2, reps):
    """irdm_dc_block_time_device: microseconds per launch of the sums pass, the close pass and the subtraction over the n
    resident samples of format fmt at d_in; None where the call refuses"""
    us = (C.c_float * 3)()
    if lib().irdm_dc_block_time_device(fmt, C.c_void_p(d_out), C.c_void_p(d_in), n, block_log2, reps, us) != 0:
        return None
    return float(us[0]), float(us[1]), float(us[2])


def host_free(ptr):
    lib().irdm_host_free(C.c_void_p(ptr))


class GpuBurstFFT:
    """gpu_burst_fft_* (opencl/burst_fft.h:35-47)."""

    def __init__(self, fft_size, batch_size, window):
        self.L = lib()
        self.n, self.batch = fft_size, batch_size
        w = np.ascontiguousarray(window, np.float32)
        self.h = self.L.gpu_burst_fft_create(fft_size, batch_size, _fp(w))
        if not self.h:
            raise RuntimeError("gpu_burst_fft_create failed (no GPU?)")

    def process(self, frames):
        """frames: complex64 [count, n] -> float32 [count, n] (mag^2, DC-shifted); raises on -1."""
        x = np.ascontiguousarray(frames, np.complex64)
        count = x.shape[0]
        out = np.empty((count, self.n), np.float32)
        rc = self.L.gpu_burst_fft_process(self.h, _fp(x.view(np.float32)), _fp(out), count)
        if rc != 0:
            raise RuntimeError("gpu_burst_fft_process returned %d" % rc)
        return out

    def process_rc(self, frames, count):
        x = np.ascontiguousarray(frames, np.complex64)
        out = np.empty((max(count, 1), self.n), np.float32)
        return self.L.gpu_burst_fft_process(self.h, _fp(x.view(np.float32)), _fp(out), count)

    def close(self):
        if self.h:
            self.L.gpu_burst_fft_destroy(self.h)
            self.h = None

    def __del__(self):
        self.close()


def burst_resample_design(L, M, taps_per_phase=20):
    """irdm_burst_resample_design: the phase-major table of the ratio L / M as a float32 array [L, taps_per_phase]"""
    out = np.empty(L * taps_per_phase, np.float32)
    if lib().irdm_burst_resample_design(L, M, _fp(out), len(out)) != len(out):
        raise RuntimeError("irdm_burst_resample_design failed")
    return out.reshape(L, taps_per_phase)


def burst_resample_batch(rows, L, M, device=0):
    """irdm_burst_resample_batch: rows = list of complex64 arrays, resampled at L / M by burst_resample_kernel alone (no
    context); returns the list of resampled rows (floor(len L / M) samples each)"""
    n = len(rows)
    stride = max([len(r) for r in rows] + [1])
    out_stride = stride * L // M + 1
    buf = np.zeros((max(n, 1), 2 * stride), np.float32)
    lens = np.zeros(max(n, 1), np.int32)
    for i, r in enumerate(rows):
        r = np.ascontiguousarray(r, np.complex64)
        lens[i] = len(r)
        buf[i, :2 * len(r)] = r.view(np.float32)
    out = np.zeros((max(n, 1), 2 * out_stride), np.float32)
    res = np.zeros(max(n, 1), np.int32)
    ip = C.POINTER(C.c_int)
    if lib().irdm_burst_resample_batch(device, _fp(buf), lens.ctypes.data_as(ip), n, stride, L, M, _fp(out), out_stride,
                                       res.ctypes.data_as(ip)) != 0:
        raise RuntimeError("irdm_burst_resample_batch failed")
    return [out[i, :2 * res[i]].copy().view(np.complex64) for i in range(n)]


class Pipeline:
    """irdm_* batched detect -> downmix -> demod context."""

    def __init__(self, sample_rate, fmt=FMT_CF32, center_frequency=1622000000.0, threshold_db=0.0,
                 feed_block=0, use_gardner=1, start_time_ns=1700000000 * 10**9, device=0,
                 max_chunk_samples=0, max_bursts_per_chunk=0, pipeline_depth=0):
        self.L = lib()
        self.cfg = Config(center_frequency, int(sample_rate), threshold_db, fmt, feed_block,
                          use_gardner, start_time_ns, device, max_chunk_samples, max_bursts_per_chunk,
                          pipeline_depth)
        self.h = self.L.irdm_create(C.byref(self.cfg))
        if not self.h:
            raise RuntimeError("irdm_create failed (no GPU, or bad config)")
        self.fmt = fmt
        self.fft_size = self.L.irdm_fft_size(self.h)

    def set_option(self, key, value):
        if self.L.irdm_set_option(self.h, key.encode(), int(value)) != 0:
            raise ValueError("unknown option %r" % key)

    def stat(self, key):
        return int(self.L.irdm_get_stat(self.h, key.encode()))

    def input_stats(self):
        """irdm_input_stats (option input_stats): the InputStats of the stream's raw samples so far"""
        st = InputStats()
        if self.L.irdm_input_stats(self.h, C.byref(st)) != 0:
            raise RuntimeError("irdm_input_stats failed (option input_stats never set?)")
        return st

    def iq_moments(self):
        """irdm_iq_moments (option iq_moments): the IqMoments of the stream so far"""
        st = IqMoments()
        if self.L.irdm_iq_moments(self.h, C.byref(st)) != 0:
            raise RuntimeError("irdm_iq_moments failed (option iq_moments never set?)")
        return st

    def iq_balance(self, wire_fmt, gain_db, phase_deg):
        """irdm_iq_balance: from now on feed_host takes wire_fmt's samples and corrects them into the cf32 context"""
        if self.L.irdm_iq_balance(self.h, wire_fmt, float(gain_db), float(phase_deg)) != 0:
            raise RuntimeError("irdm_iq_balance refused (not a cf32 context, the stream has begun, or figures outside the limits)")
        self.wire_fmt = wire_fmt

    def dc_block(self, wire_fmt=FMT_CF32, block_log2=DC_DEFAULT_LOG2, seed=(0.0, 0.0)):
        """irdm_dc_block: from now on feed_host takes wire_fmt's samples, tracks their DC offset over blocks of 2^block_log2
        samples and subtracts it into the cf32 context; block_log2 < 0 switches it off"""
        if self.L.irdm_dc_block(self.h, wire_fmt, block_log2, float(seed[0]), float(seed[1])) != 0:
            raise RuntimeError("irdm_dc_block refused (not a cf32 context, the stream has begun, or values outside the limits)")
        if block_log2 >= 0:
            self.wire_fmt = wire_fmt

    def dc_stats(self):
        """irdm_dc_stats: the DcStats of the stream so far"""
        st = DcStats()
        if self.L.irdm_dc_stats(self.h, C.byref(st)) != 0:
            raise RuntimeError("irdm_dc_stats failed (irdm_dc_block off?)")
        return st

    def feed_host(self, iq):
        iq = np.ascontiguousarray(iq)
        n = len(iq) if getattr(self, "wire_fmt", self.fmt) == FMT_CF32 else len(iq) // 2
        rc = self.L.irdm_feed_host(self.h, iq.ctypes.data_as(C.c_void_p), n)
        if rc < 0:
            raise RuntimeError("irdm_feed_host failed")
        return rc

    def prime_host(self, iq):
        """irdm_prime_host: the detector's 512-frame history filled from the recording's leading samples iq (the array
        feed_host takes), tiled when they are fewer than 512 frames, before the recording itself is fed; returns the whole
        frames used.  Only on a fresh stream: after creation or reset(), before the first feed."""
        iq = np.ascontiguousarray(iq)
        n = len(iq) if getattr(self, "wire_fmt", self.fmt) == FMT_CF32 else len(iq) // 2
        if self.L.irdm_prime_host(self.h, iq.ctypes.data_as(C.c_void_p), n) != 0:
            raise RuntimeError("irdm_prime_host refused (not a fresh stream, a member of a group, or less than one frame)")
        return self.primed_frames

    def prime_device(self, ptr, n_samples, stream=None):
        """irdm_prime_device: prime_host from a device buffer"""
        if self.L.irdm_prime_device(self.h, C.c_void_p(ptr), n_samples, C.c_void_p(stream or 0)) != 0:
            raise RuntimeError("irdm_prime_device refused (not a fresh stream, a member of a group, or less than one frame)")
        return self.primed_frames

    @property
    def primed_samples(self):
        """samples of the priming prefix in front of the recording (512 frames), 0: not primed"""
        return int(self.L.irdm_primed_samples(self.h))

    @property
    def primed_frames(self):
        """whole frames of the recording's head the prefix was tiled from, 0: not primed"""
        return int(self.L.irdm_primed_frames(self.h))

    @property
    def start_time_ns(self):
        """irdm_start_time_ns: the stream's time origin (a primed stream: that of the prefix's first sample)"""
        return int(self.L.irdm_start_time_ns(self.h))

    def poll_decoded(self):
        """irdm_poll_decoded: one Decoded per polled Demod (option "decode_frames" = 1)."""
        return self._poll(self.L.irdm_poll_decoded, Decoded)

    def poll_ida(self):
        """irdm_poll_ida: one Ida per polled Demod (option "decode_ida" = 1)."""
        return self._poll(self.L.irdm_poll_ida, Ida)

    def ida_decode_batch(self, demods, use_llr=True):
        """irdm_ida_decode_batch: ida_decode() for a list of Demod records (direction field = demodulator's)."""
        n = len(demods)
        arr = (Demod * max(n, 1))(*demods)
        out = (Ida * max(n, 1))()
        if self.L.irdm_ida_decode_batch(self.h, arr, n, 1 if use_llr else 0, out) != 0:
            raise RuntimeError("irdm_ida_decode_batch failed")
        return [out[i] for i in range(n)]

    def frame_decode_batch(self, demods, use_llr=True):
        """irdm_frame_decode_batch: frame_decode() for a list of Demod records."""
        n = len(demods)
        arr = (Demod * max(n, 1))(*demods)
        out = (Decoded * max(n, 1))()
        if self.L.irdm_frame_decode_batch(self.h, arr, n, 1 if use_llr else 0, out) != 0:
            raise RuntimeError("irdm_frame_decode_batch failed")
        return [out[i] for i in range(n)]

    def ida_packed_batch(self, demods):
        """irdm_ida_packed_batch: ida_packed_kernel for a list of Demod records (even n_bits; LLRs and direction used)."""
        n = len(demods)
        arr = (Demod * max(n, 1))(*demods)
        out = (IdaPacked * max(n, 1))()
        if self.L.irdm_ida_packed_batch(self.h, arr, n, out) != 0:
            raise RuntimeError("irdm_ida_packed_batch failed")
        return [out[i] for i in range(n)]

    def frame_packed_batch(self, demods):
        """irdm_frame_packed_batch: frame_packed_kernel for a list of Demod records (even n_bits; LLRs used)."""
        n = len(demods)
        arr = (Demod * max(n, 1))(*demods)
        out = (FramePacked * max(n, 1))()
        if self.L.irdm_frame_packed_batch(self.h, arr, n, out) != 0:
            raise RuntimeError("irdm_frame_packed_batch failed")
        return [out[i] for i in range(n)]

    def feed_host_ptr(self, ptr, n_samples):
        """irdm_feed_host on a raw host pointer (e.g. a pinned buffer from host_alloc)."""
        rc = self.L.irdm_feed_host(self.h, C.c_void_p(ptr), n_samples)
        if rc < 0:
            raise RuntimeError("irdm_feed_host failed")
        return rc

    def feed_device(self, ptr, n_samples, stream=None):
        rc = self.L.irdm_feed_device(self.h, C.c_void_p(ptr), n_samples, C.c_void_p(stream or 0))
        if rc < 0:
            raise RuntimeError("irdm_feed_device failed")
        return rc

    def feed_begin(self, ptr, n_samples, stream=None):
        """K1 + history-ring copy of a device-resident chunk (what does not depend on the detector state)."""
        if self.L.irdm_feed_begin(self.h, C.c_void_p(ptr), n_samples, C.c_void_p(stream or 0)) != 0:
            raise RuntimeError("irdm_feed_begin failed")

    def feed_end(self):
        rc = self.L.irdm_feed_end(self.h)
        if rc < 0:
            raise RuntimeError("irdm_feed_end failed")
        return rc

    def ingest_ptr(self, n_samples):
        """Device address the next chunk may be written to in place (its slot of the history ring), or None."""
        return self.L.irdm_ingest_ptr(self.h, n_samples)

    def ring(self):
        """(device address, length in samples) of the history ring."""
        n = C.c_uint64(0)
        ptr = self.L.irdm_ring_ptr(self.h, C.byref(n))
        return ptr, int(n.value)

    def state_bytes(self):
        return int(self.L.irdm_state_bytes(self.h))

    def export_state_device(self, dptr, cap):
        if self.L.irdm_export_state_device(self.h, C.c_void_p(dptr), cap) < 0:
            raise RuntimeError("irdm_export_state_device failed")

    def state_head_bytes(self):
        return int(self.L.irdm_state_head_bytes(self.h))

    def import_state_head_device(self, dptr, n):
        if self.L.irdm_import_state_head_device(self.h, C.c_void_p(dptr), n) != 0:
            raise RuntimeError("irdm_import_state_head_device failed")

    def expect_history(self, dptr):
        """True: the scan the next feed_end enqueues waits on the device until import_state_history_device(dptr, n) says
        the history has arrived at dptr"""
        return bool(self.L.irdm_expect_history(self.h, C.c_void_p(dptr)))

    def import_state_history_device(self, dptr, n):
        if self.L.irdm_import_state_history_device(self.h, C.c_void_p(dptr), n) != 0:
            raise RuntimeError("irdm_import_state_history_device failed")

    def import_state_device(self, dptr, n):
        if self.L.irdm_import_state_device(self.h, C.c_void_p(dptr), n) != 0:
            raise RuntimeError("irdm_import_state_device failed")

    def seed_history_device(self, dptr, n_samples, abs_start):
        if self.L.irdm_seed_history_device(self.h, C.c_void_p(dptr), n_samples, abs_start) != 0:
            raise RuntimeError("irdm_seed_history_device failed")

    def flush(self):
        rc = self.L.irdm_flush(self.h)
        if rc < 0:
            raise RuntimeError("irdm_flush failed")
        return rc

    def reset(self, center_frequency=None, start_time_ns=None):
        """irdm_reset: the context as irdm_create returned it, for another stream (defaults: the centre frequency and
        start time this Pipeline was made with; start_time_ns 0 = now).  Every queue is emptied."""
        cf = self.cfg.center_frequency if center_frequency is None else float(center_frequency)
        t0 = self.cfg.start_time_ns if start_time_ns is None else int(start_time_ns)
        if self.L.irdm_reset(self.h, cf, t0) != 0:
            raise RuntimeError("irdm_reset refused (a feed begun and not ended, or a member of a group)")

    def advance(self):
        """irdm_flush without the waiting: the scan in flight settled, its bursts' chain enqueued, finished records out"""
        rc = self.L.irdm_advance(self.h)
        if rc < 0:
            raise RuntimeError("irdm_advance failed")
        return rc

    def _poll(self, fn, typ, chunk=256):
        out = []
        buf = (typ * chunk)()
        while True:
            n = fn(self.h, buf, chunk)
            if n <= 0:
                break
            out += [typ.from_buffer_copy(buf[i]) for i in range(n)]
        return out

    def _poll_raw(self, fn, typ, chunk):
        """Drain a result queue into one numpy byte matrix [n, sizeof(typ)] (no per-record objects)."""
        size = C.sizeof(typ)
        parts = []
        while True:
            buf = np.empty((chunk, size), np.uint8)
            n = fn(self.h, buf.ctypes.data_as(C.POINTER(typ)), chunk)
            if n <= 0:
                break
            parts.append(buf[:n])
            if n < chunk:
                break
        return np.concatenate(parts) if parts else np.empty((0, size), np.uint8)

    def poll_bursts_raw(self, chunk=4096):
        return self._poll_raw(self.L.irdm_poll_bursts, Burst, chunk)

    def poll_demods_raw(self, chunk=2048):
        return self._poll_raw(self.L.irdm_poll_demods, Demod, chunk)

    def poll_demods_packed_raw(self, chunk=8192):
        """option packed_records 1: [n, 176] bytes, irdm_demod_packed_t records"""
        return self._poll_raw(self.L.irdm_poll_demods_packed, DemodPacked, chunk)

    def poll_demods_packed(self):
        return self._poll(self.L.irdm_poll_demods_packed, DemodPacked)

    def poll_ida_packed(self):
        """option parsed_records 1: one IdaPacked per polled DemodPacked, in the same order"""
        return self._poll(self.L.irdm_poll_ida_packed, IdaPacked)

    def poll_frame_packed(self):
        """option frame_records 1: one FramePacked per polled DemodPacked, in the same order"""
        return self._poll(self.L.irdm_poll_frame_packed, FramePacked)

    def poll_symbol_clock(self):
        """option symbol_clock 1: one ClockEst per frame that reached the demodulator, in the order of the demod records"""
        return self._poll(self.L.irdm_poll_symbol_clock, ClockEst)

    def poll_symbol_clock_raw(self, chunk=4096):
        """the same as one numpy byte matrix [n, 24]"""
        return self._poll_raw(self.L.irdm_poll_symbol_clock, ClockEst, chunk)

    def symbol_clock(self):
        """irdm_symbol_clock (option symbol_clock): the SymbolClock summary of the stream so far"""
        st = SymbolClock()
        if self.L.irdm_symbol_clock(self.h, C.byref(st)) != 0:
            raise RuntimeError("irdm_symbol_clock failed (option symbol_clock never set?)")
        return st

    def _frames_batch(self, fn, Rec, frames, what, extra=False):
        """a stage call that takes frames (list of complex64 arrays, <= 4440 samples) and gives one Rec per frame; extra: one
        int per frame, handed over behind the lengths (None: a null pointer; False: the call has no such argument)"""
        n = len(frames)
        buf = np.zeros((max(n, 1), 2 * MAX_FRAME_SAMPLES), np.float32)
        ns = np.zeros(max(n, 1), np.int32)
        for i, f in enumerate(frames):
            f = np.ascontiguousarray(f, np.complex64)
            ns[i] = len(f)
            buf[i, :2 * len(f)] = f.view(np.float32)
        out = (Rec * max(n, 1))()
        args = [self.h, _fp(buf), ns.ctypes.data_as(C.POINTER(C.c_int))]
        if extra is None:
            args.append(None)
        elif extra is not False:
            ex = np.zeros(max(n, 1), np.int32)
            ex[:n] = extra
            args.append(ex.ctypes.data_as(C.POINTER(C.c_int)))
        if fn(*args, n, out) != 0:
            raise RuntimeError(what + " failed")
        return [Rec.from_buffer_copy(out[i]) for i in range(n)]

    def symbol_clock_batch(self, frames):
        """irdm_symbol_clock_batch: frames = list of complex64 arrays (<= 4440 samples); returns a list of ClockEst"""
        return self._frames_batch(self.L.irdm_symbol_clock_batch, ClockEst, frames, "irdm_symbol_clock_batch")

    def burst_resample_ratio(self):
        """irdm_burst_resample_ratio (option burst_resample): (L, M, taps_per_phase); (1, 1, 0) at a rate on the 250 kHz grid"""
        l, m, t = C.c_int(0), C.c_int(0), C.c_int(0)
        if self.L.irdm_burst_resample_ratio(self.h, C.byref(l), C.byref(m), C.byref(t)) != 0:
            raise RuntimeError("irdm_burst_resample_ratio failed (option burst_resample off?)")
        return l.value, m.value, t.value

    def burst_resample_taps(self):
        """irdm_burst_resample_taps: the phase-major table as a float32 array [L, taps_per_phase] ([0, 0] on the grid)"""
        l, _, t = self.burst_resample_ratio()
        if t == 0:
            return np.zeros((0, 0), np.float32)
        out = np.empty(l * t, np.float32)
        if self.L.irdm_burst_resample_taps(self.h, _fp(out), l * t) != l * t:
            raise RuntimeError("irdm_burst_resample_taps failed")
        return out.reshape(l, t)

    def poll_iq_votes(self):
        """option iq_sense 1: one IqVote per demodulator record, in their order"""
        return self._poll(self.L.irdm_poll_iq_votes, IqVote)

    def poll_iq_votes_raw(self, chunk=4096):
        """the same as one numpy byte matrix [n, 16]"""
        return self._poll_raw(self.L.irdm_poll_iq_votes, IqVote, chunk)

    def iq_sense(self):
        """irdm_iq_sense (option iq_sense): the IqSense summary of the stream so far"""
        st = IqSense()
        if self.L.irdm_iq_sense(self.h, C.byref(st)) != 0:
            raise RuntimeError("irdm_iq_sense failed (option iq_sense never set?)")
        return st

    def scrub_stats(self):
        """irdm_scrub_stats (option scrub): the ScrubStats of the stream so far, positions in stream coordinates"""
        st = ScrubStats()
        if self.L.irdm_scrub_stats(self.h, C.byref(st)) != 0:
            raise RuntimeError("irdm_scrub_stats failed (option scrub off?)")
        return st

    def iq_sense_batch(self, demods):
        """irdm_iq_sense_batch: the sense kernel for a list of Demod records (bits, llr, n_bits and direction are read)"""
        n = len(demods)
        arr = (Demod * max(n, 1))(*demods)
        out = (IqVote * max(n, 1))()
        if self.L.irdm_iq_sense_batch(self.h, arr, n, out) != 0:
            raise RuntimeError("irdm_iq_sense_batch failed")
        return [IqVote.from_buffer_copy(out[i]) for i in range(n)]

    def poll_fine_freq(self):
        """option fine_freq 1: one FineFreq per frame that reached the demodulator, in the order of the demod records"""
        return self._poll(self.L.irdm_poll_fine_freq, FineFreq)

    def poll_fine_freq_raw(self, chunk=4096):
        """the same as one numpy byte matrix [n, 32]"""
        return self._poll_raw(self.L.irdm_poll_fine_freq, FineFreq, chunk)

    def fine_freq(self):
        """irdm_fine_freq (option fine_freq): the FineFreqSummary of the stream so far"""
        st = FineFreqSummary()
        if self.L.irdm_fine_freq(self.h, C.byref(st)) != 0:
            raise RuntimeError("irdm_fine_freq failed (option fine_freq never set?)")
        return st

    def fine_freq_batch(self, frames):
        """irdm_fine_freq_batch: frames = list of complex64 arrays (<= 4440 samples); returns a list of FineFreq"""
        return self._frames_batch(self.L.irdm_fine_freq_batch, FineFreq, frames, "irdm_fine_freq_batch")

    def poll_fine_time(self):
        """option fine_time 1: one FineTime per frame that reached the demodulator, in the order of the demod records"""
        return self._poll(self.L.irdm_poll_fine_time, FineTime)

    def poll_fine_time_raw(self, chunk=4096):
        """the same as one numpy byte matrix [n, 64]"""
        return self._poll_raw(self.L.irdm_poll_fine_time, FineTime, chunk)

    def fine_time(self):
        """irdm_fine_time (option fine_time): the FineTimeSummary of the stream so far"""
        st = FineTimeSummary()
        if self.L.irdm_fine_time(self.h, C.byref(st)) != 0:
            raise RuntimeError("irdm_fine_time failed (option fine_time never set?)")
        return st

    def fine_time_batch(self, frames, simplex=None):
        """irdm_fine_time_batch: frames = list of complex64 arrays (<= 4440 samples), simplex = one flag per frame (None: all 0);
        returns a list of FineTime"""
        return self._frames_batch(self.L.irdm_fine_time_batch, FineTime, frames, "irdm_fine_time_batch",
                                  extra=None if simplex is None else [int(bool(v)) for v in simplex])

    def poll_spectrum(self, chunk=64):
        """option spectrum_frames: (headers, mean, peak) of the rows finished so far -- a list of SpectrumRow and two float32
        arrays [rows][n_bins], bin 0 at -fs/2, linear |X|^2"""
        n = self.L.irdm_spectrum_bins(self.h)
        hdr = (SpectrumRow * chunk)()
        mean, peak = np.empty((chunk, n), np.float32), np.empty((chunk, n), np.float32)
        hs, ms, ps = [], [np.empty((0, n), np.float32)], [np.empty((0, n), np.float32)]
        while True:
            k = self.L.irdm_poll_spectrum(self.h, hdr, _fp(mean), _fp(peak), chunk)
            if k < 0:
                raise RuntimeError("irdm_poll_spectrum failed")
            if k == 0:
                break
            hs += [SpectrumRow.from_buffer_copy(hdr[i]) for i in range(k)]
            ms.append(mean[:k].copy())
            ps.append(peak[:k].copy())
        return hs, np.concatenate(ms), np.concatenate(ps)

    def drop_frames(self, chunk=4096):
        """Discard queued frame records (metadata only path)."""
        buf = (FrameInfo * chunk)()
        total = 0
        while True:
            n = self.L.irdm_poll_frames(self.h, buf, None, chunk)
            if n <= 0:
                break
            total += n
            if n < chunk:
                break
        return total

    def poll_bursts(self):
        return self._poll(self.L.irdm_poll_bursts, Burst)

    def poll_demods(self):
        return self._poll(self.L.irdm_poll_demods, Demod)

    def poll_frames(self, chunk=64):
        infos, samples = [], []
        buf = (FrameInfo * chunk)()
        sb = np.zeros((chunk, 2 * MAX_FRAME_SAMPLES), np.float32)
        while True:
            n = self.L.irdm_poll_frames(self.h, buf, _fp(sb), chunk)
            if n <= 0:
                break
            for i in range(n):
                fi = FrameInfo.from_buffer_copy(buf[i])
                infos.append(fi)
                samples.append(sb[i, :2 * fi.num_samples].copy().view(np.complex64))
        return infos, samples

    def downmix_burst(self, info, samples):
        """burst_downmix_process for one burst (host samples, complex64) -> (FrameInfo, complex64 frame | None)."""
        x = np.ascontiguousarray(samples, np.complex64)
        fi = FrameInfo()
        out = np.zeros(2 * MAX_FRAME_SAMPLES, np.float32)
        rc = self.L.irdm_downmix_burst(self.h, C.byref(info), _fp(x.view(np.float32)), len(x), C.byref(fi), _fp(out))
        if rc < 0:
            raise RuntimeError("irdm_downmix_burst failed")
        return fi, (out[:2 * fi.num_samples].view(np.complex64).copy() if rc == 1 else None)

    @staticmethod
    def _frame_rows(frames, directions, pad):
        n = len(frames)
        buf = np.full((n, 2 * MAX_FRAME_SAMPLES), pad, np.float32)
        ns = np.zeros(n, np.int32)
        for i, f in enumerate(frames):
            f = np.ascontiguousarray(f, np.complex64)
            ns[i] = len(f)
            buf[i, :2 * len(f)] = f.view(np.float32)
        return buf, ns, np.ascontiguousarray(directions, np.int32)

    def qpsk_demod_batch(self, frames, directions, pad=0.0):
        """frames: list of complex64 arrays (<= 4440 samples), each row filled up with `pad`; returns list of Demod."""
        n = len(frames)
        buf, ns, dirs = self._frame_rows(frames, directions, pad)
        out = (Demod * n)()
        rc = self.L.irdm_qpsk_demod_batch(self.h, _fp(buf), ns.ctypes.data_as(C.POINTER(C.c_int)),
                                          dirs.ctypes.data_as(C.POINTER(C.c_int)), n, out)
        if rc != 0:
            raise RuntimeError("irdm_qpsk_demod_batch failed")
        return [Demod.from_buffer_copy(out[i]) for i in range(n)]

    def qpsk_demod_packed_batch(self, frames, directions, keep_bits):
        """the same frames on the packed record path; returns (list of DemodPacked, list of Demod | None: keep_bits 0)."""
        n = len(frames)
        buf, ns, dirs = self._frame_rows(frames, directions, 0.0)
        packed = (DemodPacked * n)()
        full = (Demod * n)() if keep_bits else None
        rc = self.L.irdm_qpsk_demod_packed_batch(self.h, _fp(buf), ns.ctypes.data_as(C.POINTER(C.c_int)),
                                                 dirs.ctypes.data_as(C.POINTER(C.c_int)), n, int(keep_bits), packed, full)
        if rc != 0:
            raise RuntimeError("irdm_qpsk_demod_packed_batch failed")
        return ([DemodPacked.from_buffer_copy(packed[i]) for i in range(n)],
                [Demod.from_buffer_copy(full[i]) for i in range(n)] if keep_bits else None)

    def export_state(self):
        n = self.L.irdm_state_bytes(self.h)
        buf = np.empty(n, np.uint8)
        if self.L.irdm_export_state(self.h, buf.ctypes.data_as(C.c_void_p), n) != n:
            raise RuntimeError("irdm_export_state failed")
        return buf

    def import_state(self, buf):
        buf = np.ascontiguousarray(buf, np.uint8)
        if self.L.irdm_import_state(self.h, buf.ctypes.data_as(C.c_void_p), len(buf)) != 0:
            raise RuntimeError("irdm_import_state failed")

    def seed_history(self, iq_tail, abs_start):
        iq_tail = np.ascontiguousarray(iq_tail)
        n = len(iq_tail) if self.fmt == FMT_CF32 else len(iq_tail) // 2
        if self.L.irdm_seed_history(self.h, iq_tail.ctypes.data_as(C.c_void_p), n, abs_start) != 0:
            raise RuntimeError("irdm_seed_history failed")

    def last_magnitudes(self, max_frames):
        out = np.zeros((max_frames, self.fft_size), np.float32)
        n = self.L.irdm_last_magnitudes(self.h, _fp(out), max_frames)
        return out[:n]

    def baseline_sum(self):
        out = np.zeros(self.fft_size, np.float32)
        self.L.irdm_baseline_sum(self.h, _fp(out))
        return out

    def burst_samples(self, i, n):
        out = np.zeros(2 * n, np.float32)
        got = self.L.irdm_burst_samples(self.h, i, _fp(out), n)
        if got < 0:
            raise RuntimeError("irdm_burst_samples failed")
        return out[:2 * got].view(np.complex64)

    def kernel_clock(self, which, reset=False):
        """(sum of the launches' device spans in ms, launches, last span in ms) of the decimator (0) / K1 (1); option
        kernel_clock must be on"""
        sm, n, last = C.c_double(0), C.c_uint64(0), C.c_double(0)
        if self.L.irdm_kernel_clock(self.h, which, C.byref(sm), C.byref(n), C.byref(last), 1 if reset else 0) != 0:
            raise RuntimeError("irdm_kernel_clock failed")
        return sm.value, int(n.value), last.value

    def timings(self):
        t = (C.c_float * 6)()
        self.L.irdm_last_timings(self.h, t, 6)
        return dict(zip(["fft_mag", "scan", "fir", "post", "demod", "total"], [float(v) for v in t]))

    @property
    def tagged(self):
        return self.L.irdm_tagged_bursts(self.h)

    @property
    def sample_count(self):
        return self.L.irdm_sample_count(self.h)

    def close(self):
        if self.h:
            self.L.irdm_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Frontend:
    """irdm_frontend_*: band select in front of a Pipeline -- shift by shift_hz, low-pass, decimate by decim.  The pipeline
    behind it is a cf32 context at out_rate, centred at the capture centre + applied_shift_hz."""

    def __init__(self, in_rate, fmt, decim, shift_hz=0.0, device=0, out_rate=None, maker="rational"):
        self.L = lib()
        if out_rate is None:
            self.cfg = FrontendConfig(device, int(in_rate), fmt, int(decim), float(shift_hz))
            self.h = self.L.irdm_frontend_create(C.byref(self.cfg))
        else:
            self.cfg = FrontendRationalConfig(device, int(in_rate), fmt, int(out_rate), float(shift_hz))
            self.h = getattr(self.L, "irdm_frontend_create_" + maker)(C.byref(self.cfg))
        if not self.h:
            raise RuntimeError("irdm_frontend_create%s failed (no GPU, or bad config)" % ("" if out_rate is None else "_" + maker))
        self.fmt = fmt
        self.out_rate = self.L.irdm_frontend_out_rate(self.h)
        self.applied_shift_hz = self.L.irdm_frontend_applied_shift_hz(self.h)
        self.ntaps = self.L.irdm_frontend_ntaps(self.h)

    @classmethod
    def rational(cls, in_rate, fmt, out_rate, shift_hz=0.0, device=0):
        """irdm_frontend_create_rational: resample to out_rate = in_rate * L / M (an integer ratio 2 .. 16 gives the
        integer front end)"""
        return cls(in_rate, fmt, None, shift_hz, device, out_rate=out_rate)

    @classmethod
    def resampler(cls, in_rate, fmt, out_rate, shift_hz=0.0, device=0):
        """irdm_frontend_create_resampler: the integer front end, K0r or K0w, whichever takes out_rate / in_rate"""
        return cls(in_rate, fmt, None, shift_hz, device, out_rate=out_rate, maker="resampler")

    @classmethod
    def wide(cls, in_rate, fmt, out_rate, shift_hz=0.0, device=0):
        """irdm_frontend_create_wide: K0w, for any ratio with 2 <= L <= 4096, M <= 65536, 24/25 <= M / L <= 16"""
        return cls(in_rate, fmt, None, shift_hz, device, out_rate=out_rate, maker="wide")

    @staticmethod
    def resampler_ratio(in_rate, out_rate):
        """irdm_frontend_resampler_ratio: (L, M, kernel) -- kernel 0 K0, 1 K0r, 2 K0w -- or None beyond K0w's limits"""
        l, m, k = C.c_int(0), C.c_int(0), C.c_int(-1)
        if lib().irdm_frontend_resampler_ratio(int(in_rate), int(out_rate), C.byref(l), C.byref(m), C.byref(k)) != 0:
            return None
        return l.value, m.value, k.value

    @staticmethod
    def wide_geometry(in_rate, out_rate):
        """irdm_frontend_wide_geometry: dict(ntaps, tile, lds_bytes, wg_per_cu) of K0w at out_rate / in_rate (no device)"""
        v = [C.c_int(0) for _ in range(4)]
        if lib().irdm_frontend_wide_geometry(int(in_rate), int(out_rate), *[C.byref(x) for x in v]) != 0:
            raise RuntimeError("irdm_frontend_wide_geometry refused %d -> %d" % (in_rate, out_rate))
        return dict(zip(("ntaps", "tile", "lds_bytes", "wg_per_cu"), (x.value for x in v)))

    @property
    def ratio(self):
        """(L, M): output rate = capture rate * L / M; (1, D) for the integer front end"""
        l, m = C.c_int(0), C.c_int(0)
        if self.L.irdm_frontend_ratio(self.h, C.byref(l), C.byref(m)) != 0:
            raise RuntimeError("irdm_frontend_ratio failed")
        return l.value, m.value

    def taps(self):
        out = np.empty(self.ntaps, np.float32)
        if self.L.irdm_frontend_taps(self.h, _fp(out), self.ntaps) != self.ntaps:
            raise RuntimeError("irdm_frontend_taps failed")
        return out

    def iq_moments_enable(self, on=True):
        """irdm_frontend_iq_moments: the second moments of the capture's samples in front of the kernel"""
        if self.L.irdm_frontend_iq_moments(self.h, 1 if on else 0) != 0:
            raise RuntimeError("irdm_frontend_iq_moments failed")

    def iq_moments(self):
        """irdm_frontend_iq_moments_stats: the IqMoments of the capture so far"""
        st = IqMoments()
        if self.L.irdm_frontend_iq_moments_stats(self.h, C.byref(st)) != 0:
            raise RuntimeError("irdm_frontend_iq_moments_stats failed (never switched on?)")
        return st

    def iq_balance(self, wire_fmt, gain_db, phase_deg):
        """irdm_frontend_iq_balance: from now on feed_host takes wire_fmt's samples and corrects them into the cf32 capture"""
        if self.L.irdm_frontend_iq_balance(self.h, wire_fmt, float(gain_db), float(phase_deg)) != 0:
            raise RuntimeError("irdm_frontend_iq_balance refused (not a cf32 front end, the capture has begun, or figures outside the limits)")
        self.wire_fmt = wire_fmt

    def dc_block(self, wire_fmt=FMT_CF32, block_log2=DC_DEFAULT_LOG2, seed=(0.0, 0.0)):
        """irdm_frontend_dc_block: from now on feed_host takes wire_fmt's samples, tracks their DC offset over blocks of
        2^block_log2 samples and subtracts it into the cf32 capture; block_log2 < 0 switches it off"""
        if self.L.irdm_frontend_dc_block(self.h, wire_fmt, block_log2, float(seed[0]), float(seed[1])) != 0:
            raise RuntimeError("irdm_frontend_dc_block refused (not a cf32 front end, the capture has begun, or values outside the limits)")
        if block_log2 >= 0:
            self.wire_fmt = wire_fmt

    def dc_stats(self):
        """irdm_frontend_dc_stats: the DcStats of the capture so far"""
        st = DcStats()
        if self.L.irdm_frontend_dc_stats(self.h, C.byref(st)) != 0:
            raise RuntimeError("irdm_frontend_dc_stats failed (irdm_frontend_dc_block off?)")
        return st

    def feed_host(self, pipeline, x):
        x = np.ascontiguousarray(x)
        n = len(x) if getattr(self, "wire_fmt", self.fmt) == FMT_CF32 else len(x) // 2
        rc = self.L.irdm_frontend_feed_host(self.h, pipeline.h, x.ctypes.data_as(C.c_void_p), n)
        if rc < 0:
            raise RuntimeError("irdm_frontend_feed_host failed")
        return rc

    def feed_device(self, pipeline, ptr, n_samples, stream=None):
        rc = self.L.irdm_frontend_feed_device(self.h, pipeline.h, C.c_void_p(ptr), n_samples, C.c_void_p(stream or 0))
        if rc < 0:
            raise RuntimeError("irdm_frontend_feed_device failed")
        return rc

    def wait_input(self):
        if self.L.irdm_frontend_wait_input(self.h) != 0:
            raise RuntimeError("irdm_frontend_wait_input failed")

    def prime_host(self, pipeline, x):
        """irdm_frontend_prime_host: the capture's leading samples x through the kernel, the pipeline primed from the band's
        whole frames, the front end reset; returns the frames used"""
        x = np.ascontiguousarray(x)
        n = len(x) if getattr(self, "wire_fmt", self.fmt) == FMT_CF32 else len(x) // 2
        if self.L.irdm_frontend_prime_host(self.h, pipeline.h, x.ctypes.data_as(C.c_void_p), n) != 0:
            raise RuntimeError("irdm_frontend_prime_host refused (front end or pipeline not fresh, or less than one frame of band)")
        return pipeline.primed_frames

    def reset(self):
        """irdm_frontend_reset: back to the state after creation, for another capture (taps, tables and shift stay)"""
        if self.L.irdm_frontend_reset(self.h) != 0:
            raise RuntimeError("irdm_frontend_reset failed")

    def seek(self, total_in):
        """irdm_frontend_seek: directly after creation or reset, take the capture up at input sample total_in -- the state
        that feeding total_in samples of zero codes would have left"""
        if self.L.irdm_frontend_seek(self.h, int(total_in)) != 0:
            raise RuntimeError("irdm_frontend_seek refused (samples already fed, or a position from 2^53 on)")

    def flush(self, pipeline):
        rc = self.L.irdm_frontend_flush(self.h, pipeline.h)
        if rc < 0:
            raise RuntimeError("irdm_frontend_flush failed")
        return rc

    def save(self, fmt, sink=None, gain=1.0, slot_samples=0):
        """irdm_frontend_save: the band as a ci8 / ci16 / cf32 recording.  sink(bytes) is called with each piece in stream
        order (return a true value to stop); without one the pieces collect in self.saved.  fmt None: saving off."""
        if fmt is None:
            if self.L.irdm_frontend_save(self.h, None) != 0:
                raise RuntimeError("irdm_frontend_save failed")
            self._sink = None
            return
        saved = []
        take = sink if sink is not None else saved.append

        def call(user, ptr, n):
            return 1 if take(C.string_at(ptr, n)) else 0
        cb = BAND_SINK(call)
        cfg = FrontendSaveConfig(fmt, float(gain), int(slot_samples), cb, None)
        if self.L.irdm_frontend_save(self.h, C.byref(cfg)) != 0:
            raise RuntimeError("irdm_frontend_save failed (mid-stream, or a bad field)")
        self.saved = saved
        self._sink = cb              # (the library calls it for as long as the front end lives)

    def swap_iq(self, on=True):
        """irdm_frontend_swap_iq: feed_host exchanges I and Q of every capture chunk in front of the kernel"""
        if self.L.irdm_frontend_swap_iq(self.h, 1 if on else 0) != 0:
            raise RuntimeError("irdm_frontend_swap_iq failed")

    def scrub(self, on=True, limit_log2=SCRUB_DEFAULT_LOG2):
        """irdm_frontend_scrub: feed_host zeroes the non-finite and out-of-range samples of every cf32 capture chunk in
        front of the kernel"""
        if self.L.irdm_frontend_scrub(self.h, 1 if on else 0, limit_log2) != 0:
            raise RuntimeError("irdm_frontend_scrub failed")

    def scrub_stats(self):
        """irdm_frontend_scrub_stats: the ScrubStats of the capture so far, positions in capture coordinates"""
        st = ScrubStats()
        if self.L.irdm_frontend_scrub_stats(self.h, C.byref(st)) != 0:
            raise RuntimeError("irdm_frontend_scrub_stats failed (never switched on?)")
        return st

    def input_stats_enable(self, on=True):
        """irdm_frontend_input_stats_enable: statistics of the capture's samples in front of the kernel"""
        if self.L.irdm_frontend_input_stats_enable(self.h, 1 if on else 0) != 0:
            raise RuntimeError("irdm_frontend_input_stats_enable failed")

    def input_stats(self):
        """irdm_frontend_input_stats: the InputStats of the capture so far"""
        st = InputStats()
        if self.L.irdm_frontend_input_stats(self.h, C.byref(st)) != 0:
            raise RuntimeError("irdm_frontend_input_stats failed (never enabled?)")
        return st

    def save_stats(self):
        """irdm_frontend_save_stats: (n_samples, n_clipped, peak as a fraction of full scale)"""
        st = BandStats()
        if self.L.irdm_frontend_save_stats(self.h, C.byref(st)) != 0:
            raise RuntimeError("irdm_frontend_save_stats failed")
        return int(st.n_samples), int(st.n_clipped), np.float32(st.peak)

    def kernel_clock(self, reset=False):
        """(sum of K0's device spans in ms, launches) since the last reset"""
        sm, n = C.c_double(0), C.c_uint64(0)
        if self.L.irdm_frontend_kernel_clock(self.h, C.byref(sm), C.byref(n), 1 if reset else 0) != 0:
            raise RuntimeError("irdm_frontend_kernel_clock failed")
        return sm.value, int(n.value)

    def close(self):
        if self.h:
            self.L.irdm_frontend_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Group:
    """irdm_group_*: ONE stream across n_gpus GPUs of this process, chunk k on member k mod n_gpus, the detector's state
    handed from member to member with RCCL (csrc/group.cpp).  The polls return the members' records merged in stream
    order -- what one Pipeline fed with the same samples returns."""
    _poll = Pipeline._poll            # (fn(self.h, buffer, max): the group's polls have the pipeline's shape)

    def __init__(self, sample_rate, n_gpus, devices=None, fmt=FMT_CF32, center_frequency=1622000000.0, threshold_db=0.0,
                 feed_block=0, use_gardner=1, start_time_ns=1700000000 * 10**9, max_chunk_samples=0,
                 max_bursts_per_chunk=0, pipeline_depth=1):
        self.L = lib()
        self.cfg = Config(center_frequency, int(sample_rate), threshold_db, fmt, feed_block, use_gardner, start_time_ns, 0,
                          max_chunk_samples, max_bursts_per_chunk, pipeline_depth)
        devs = (C.c_int * n_gpus)(*devices) if devices is not None else None
        self.g = self.L.irdm_group_create(C.byref(self.cfg), n_gpus, devs)
        if not self.g:
            raise RuntimeError("irdm_group_create failed (devices, RCCL, or bad config)")
        self.h = self.g                   # (Pipeline's poll helpers call fn(self.h, ...))
        self.fmt = fmt
        self.n_gpus = n_gpus
        self.fft_size = self.L.irdm_fft_size(self.L.irdm_group_member(self.g, 0))
        self.chunk = int(self.L.irdm_max_chunk_samples(self.L.irdm_group_member(self.g, 0)))

    def member(self, i):
        return self.L.irdm_group_member(self.g, i)

    def set_option(self, key, value):
        if self.L.irdm_group_set_option(self.g, key.encode(), int(value)) != 0:
            raise ValueError("option %r refused" % key)

    def stat(self, key):
        return int(self.L.irdm_group_get_stat(self.g, key.encode()))

    def _samples(self, iq):
        return len(iq) if self.fmt == FMT_CF32 else len(iq) // 2

    def stage_host(self, iq):
        if self.L.irdm_group_stage_host(self.g, iq.ctypes.data_as(C.c_void_p), self._samples(iq)) != 0:
            raise RuntimeError("irdm_group_stage_host failed")

    def feed_host(self, iq):
        """iq: a C-contiguous array of at most n_gpus chunks; it must stay alive until the call returns (and, if it was
        staged first, from the stage call on)"""
        rc = self.L.irdm_group_feed_host(self.g, iq.ctypes.data_as(C.c_void_p), self._samples(iq))
        if rc < 0:
            raise RuntimeError("irdm_group_feed_host failed")
        return rc

    def stage_device(self, ptr, n_samples):
        if self.L.irdm_group_stage_device(self.g, C.c_void_p(ptr), n_samples) != 0:
            raise RuntimeError("irdm_group_stage_device failed")

    def feed_device(self, ptr, n_samples, stream=None):
        rc = self.L.irdm_group_feed_device(self.g, C.c_void_p(ptr), n_samples)
        if rc < 0:
            raise RuntimeError("irdm_group_feed_device failed")
        return rc

    def flush(self):
        rc = self.L.irdm_group_flush(self.g)
        if rc < 0:
            raise RuntimeError("irdm_group_flush failed")
        return rc

    def poll_bursts(self):
        return self._poll(self.L.irdm_group_poll_bursts, Burst)

    def poll_demods(self):
        return self._poll(self.L.irdm_group_poll_demods, Demod)

    def poll_demods_packed(self):
        return self._poll(self.L.irdm_group_poll_demods_packed, DemodPacked)

    def poll_decoded(self):
        return self._poll(self.L.irdm_group_poll_decoded, Decoded)

    def poll_ida(self):
        return self._poll(self.L.irdm_group_poll_ida, Ida)

    def poll_ida_packed(self):
        return self._poll(self.L.irdm_group_poll_ida_packed, IdaPacked)

    def poll_frame_packed(self):
        return self._poll(self.L.irdm_group_poll_frame_packed, FramePacked)

    def poll_frames(self, chunk=64):
        infos, samples = [], []
        buf = (FrameInfo * chunk)()
        sb = np.zeros((chunk, 2 * MAX_FRAME_SAMPLES), np.float32)
        while True:
            n = self.L.irdm_group_poll_frames(self.g, buf, _fp(sb), chunk)
            if n <= 0:
                break
            for i in range(n):
                fi = FrameInfo.from_buffer_copy(buf[i])
                infos.append(fi)
                samples.append(sb[i, :2 * fi.num_samples].copy().view(np.complex64))
        return infos, samples

    @property
    def tagged(self):
        return self.stat("tagged")

    def close(self):
        if self.g:
            self.L.irdm_group_destroy(self.g)
            self.g = self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def format_raw(demods, file_info="golden"):
    """frame_output_print for a list of Demod records (t0 from the first, frame_output.c:144-158)."""
    L = lib()
    t0 = C.c_uint64(0)
    buf = C.create_string_buffer(4096)
    out = []
    for d in demods:
        n = L.irdm_format_raw(C.byref(d), file_info.encode() if file_info else None, C.byref(t0), buf, 4096)
        if n < 0:
            raise RuntimeError("irdm_format_raw failed")
        out.append(buf.value.decode())
    return out


def ida_unpack(ida_packed, demod_packed):
    """irdm_ida_unpack: the Ida record the decode_ida path makes of the same frame"""
    out = Ida()
    lib().irdm_ida_unpack(C.byref(ida_packed), C.byref(demod_packed), C.byref(out))
    return out


def frame_unpack(frame_packed, demod_packed):
    """irdm_frame_unpack: the Decoded record the decode_frames path makes of the same frame"""
    out = Decoded()
    lib().irdm_frame_unpack(C.byref(frame_packed), C.byref(demod_packed), C.byref(out))
    return out


def format_ida(idas, t0=0):
    """frame_output_print_ida for a list of Ida records (ok != 0), t0 shared along the list; returns the lines"""
    L = lib()
    t = C.c_uint64(t0)
    buf = C.create_string_buffer(4096)
    out = []
    for b in idas:
        n = L.irdm_format_ida(C.byref(b), C.byref(t), buf, 4096)
        if n < 0:
            raise RuntimeError("irdm_format_ida failed")
        out.append(buf.raw[:n].decode("latin-1"))
    return out


def format_parsed_packed_batch(demods, idas, file_info=None, t0=0):
    """irdm_format_parsed_packed_batch: --parsed's text for paired DemodPacked / IdaPacked lists"""
    L = lib()
    n = len(demods)
    assert len(idas) == n
    arr = (DemodPacked * max(n, 1))(*demods)
    ida = (IdaPacked * max(n, 1))(*idas)
    cap = max(n, 1) * 1280
    buf = C.create_string_buffer(cap)
    t = C.c_uint64(t0)
    rc = L.irdm_format_parsed_packed_batch(arr, ida, n, file_info.encode() if file_info else None, C.byref(t), buf, cap)
    if rc < 0:
        raise RuntimeError("irdm_format_parsed_packed_batch failed")
    return buf.raw[:rc].decode("latin-1")


def format_raw_batch(demods, file_info="golden"):
    """irdm_format_raw_batch: all lines in one buffer (one write per batch); returns the text."""
    L = lib()
    L.irdm_format_raw_batch.restype = C.c_longlong
    n = len(demods)
    arr = (Demod * n)(*demods)
    cap = max(n, 1) * 1280
    buf = C.create_string_buffer(cap)
    t0 = C.c_uint64(0)
    rc = L.irdm_format_raw_batch(arr, n, file_info.encode() if file_info else None, C.byref(t0), buf, cap)
    if rc < 0:
        raise RuntimeError("irdm_format_raw_batch failed")
    return buf.raw[:rc].decode()


def save_burst(info, samples, dirname):
    """irdm_save_burst: the reference's --save-bursts file pair for one frame (qpsk_demod.c:339-389)."""
    L = lib()
    L.irdm_save_burst.argtypes = [C.POINTER(FrameInfo), C.POINTER(C.c_float), C.c_char_p]
    s = np.ascontiguousarray(samples, np.float32)
    return L.irdm_save_burst(C.byref(info), s.ctypes.data_as(C.POINTER(C.c_float)), dirname.encode())


# ---------------------------------------------------------------- --acars (csrc/acars.cpp) ----
class IdaReassembler:
    """irdm_ida_reasm_*: ida_reassemble + ida_reassemble_flush per frame record, state across calls"""

    def __init__(self):
        self._L = lib()
        self._h = self._L.irdm_ida_reasm_create()
        if not self._h:
            raise MemoryError("irdm_ida_reasm_create")

    def push(self, idas):
        """Ida records in stream order (ok 0 with the frame's timestamp: a frame that only flushes) -> IdaMessage list"""
        n = len(idas)
        arr = (Ida * max(n, 1))(*idas)
        out = (IdaMessage * max(n, 1))()
        k = self._L.irdm_ida_reasm_push(self._h, arr, n, out, max(n, 1))
        if k < 0:
            raise RuntimeError("irdm_ida_reasm_push failed")
        return [out[i] for i in range(k)]

    def push_packed(self, demods, idas):
        n = len(demods)
        assert len(idas) == n
        d = (DemodPacked * max(n, 1))(*demods)
        i = (IdaPacked * max(n, 1))(*idas)
        out = (IdaMessage * max(n, 1))()
        k = self._L.irdm_ida_reasm_push_packed(self._h, d, i, n, out, max(n, 1))
        if k < 0:
            raise RuntimeError("irdm_ida_reasm_push_packed failed")
        return [out[j] for j in range(k)]

    def close(self):
        if self._h:
            self._L.irdm_ida_reasm_destroy(self._h)
            self._h = None

    def __del__(self):
        self.close()


class AcarsPrinter:
    """irdm_acars_*: SBD extraction + ACARS lines for reassembled IDA messages; origin (sec, nsec) fixes the wall clock"""

    def __init__(self, json=False, station=None, origin=None):
        self._L = lib()
        self._station = station.encode() if station is not None else None
        cfg = AcarsConfig(1 if json else 0, 1 if origin is not None else 0, origin[0] if origin else 0,
                          origin[1] if origin else 0, self._station)
        self._h = self._L.irdm_acars_create(C.byref(cfg))
        if not self._h:
            raise MemoryError("irdm_acars_create")

    def feed(self, msgs):
        """IdaMessage list -> the printed bytes"""
        n = len(msgs)
        arr = (IdaMessage * max(n, 1))(*msgs)
        cap = max(n, 1) * ACARS_LINE_MAX
        buf = C.create_string_buffer(cap)
        k = self._L.irdm_acars_feed(self._h, arr, n, buf, cap)
        if k < 0:
            raise RuntimeError("irdm_acars_feed failed")
        return buf.raw[:k]

    def stats(self):
        s = AcarsStats()
        self._L.irdm_acars_stats(self._h, C.byref(s))
        return {n: getattr(s, n) for n, _ in AcarsStats._fields_}

    def stats_text(self):
        buf = C.create_string_buffer(1024)
        k = self._L.irdm_acars_format_stats(self._h, buf, 1024)
        if k < 0:
            raise RuntimeError("irdm_acars_format_stats failed")
        return buf.raw[:k]

    def format_packed_batch(self, reasm, demods, idas, parsed=False, t0=None):
        """irdm_format_acars_packed_batch: --acars's stdout bytes for paired DemodPacked / IdaPacked records;
        t0: a c_uint64 shared across calls (the IDA line printer's)"""
        n = len(demods)
        assert len(idas) == n
        d = (DemodPacked * max(n, 1))(*demods)
        i = (IdaPacked * max(n, 1))(*idas)
        cap = max(n, 1) * (RAW_LINE_MAX + ACARS_LINE_MAX)
        buf = C.create_string_buffer(cap)
        t = t0 if t0 is not None else C.c_uint64(0)
        k = self._L.irdm_format_acars_packed_batch(reasm._h, self._h, d, i, n, 1 if parsed else 0, C.byref(t), buf, cap)
        if k < 0:
            raise RuntimeError("irdm_format_acars_packed_batch failed")
        return buf.raw[:k]

    def close(self):
        if self._h:
            self._L.irdm_acars_destroy(self._h)
            self._h = None

    def __del__(self):
        self.close()


# ---------------------------------------------------------------- --position (csrc/doppler.cpp) ----
class Doppler:
    """irdm_doppler_*: the Doppler positioning engine, state across calls; origin: the stream's start_time_ns"""

    def __init__(self, height_m=0.0, origin=0):
        self._L = lib()
        self._h = self._L.irdm_doppler_create(float(height_m))
        if not self._h:
            raise MemoryError("irdm_doppler_create")
        self._L.irdm_doppler_set_origin(self._h, origin)

    def add(self, decoded):
        return self._L.irdm_doppler_add(self._h, C.byref(decoded))

    def solve(self):
        """(return value, Position)"""
        s = Position()
        r = self._L.irdm_doppler_solve(self._h, C.byref(s))
        return r, s

    def _text(self, fn, *args, cap):
        buf = C.create_string_buffer(cap)
        k = fn(self._h, *args, buf, cap)
        if k < 0:
            raise RuntimeError(fn.__name__ + " failed")
        return buf.raw[:k].decode()

    def format_batch(self, decoded, cap=1 << 20):
        """irdm_format_doppler_batch: the stderr text of one batch of Decoded records"""
        n = len(decoded)
        return self._text(self._L.irdm_format_doppler_batch, (Decoded * max(n, 1))(*decoded), n, cap=cap)

    def format_packed_batch(self, demods, frames, cap=1 << 20):
        n = len(demods)
        assert len(frames) == n
        return self._text(self._L.irdm_format_doppler_packed_batch, (DemodPacked * max(n, 1))(*demods),
                          (FramePacked * max(n, 1))(*frames), n, cap=cap)

    def finish(self, end_ns, cap=1 << 20):
        return self._text(self._L.irdm_doppler_finish, C.c_uint64(end_ns), cap=cap)

    def close(self):
        if self._h:
            self._L.irdm_doppler_destroy(self._h)
            self._h = None

    def __del__(self):
        self.close()
