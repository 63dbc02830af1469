"""TEST INFRASTRUCTURE: the truth the symbol timing tests share (tests/test_fine_time_model.py, tests/fine_time_checks.py): the
scenes are those of tests/fine_freq_scenes.py; the truth of a downlink frame is the time of the centre of its unique word's
first symbol, raw sample start + (5 + 16) fs / 25000 of its burst (siggen.make_burst: symbol k is centred on sample
(k + 5) fs / 25000, and 16 preamble symbols stand in front of the unique word)."""
import numpy as np

import fine_freq_scenes as sc
import siggen

START_NS, CENTER, OUT_RATE = sc.START_NS, sc.CENTER, sc.OUT_RATE
SIMPLEX_ABOVE = 1626000000.0           # a frame whose downmixer's frequency is above it is a simplex one (BurstWork::simplex)


def truth_ns(truth, fs, timestamp_ns, center_frequency):
    """the true time [ns, float] of the frame's sample 0: of the burst on the channel of center_frequency whose unique word
    lies nearest to timestamp_ns (the unrefined timestamp is within 1 ms of it)"""
    best = None
    for b in truth:
        if abs(CENTER + b["freq_hz"] - center_frequency) > 2000.0:
            continue
        t = START_NS + (b["start"] + (5 + 16) * fs / siggen.SYMBOL_RATE) / fs * 1e9
        if best is None or abs(t - timestamp_ns) < abs(best - timestamp_ns):
            best = t
    assert best is not None and abs(best - timestamp_ns) < 2e6, (timestamp_ns, center_frequency, best)
    return best


def burst_start_ns(truth, fs, timestamp_ns, center_frequency):
    """the time [ns] of that burst's first sample"""
    return truth_ns(truth, fs, timestamp_ns, center_frequency) - (5 + 16) / siggen.SYMBOL_RATE * 1e9


def oracle_frames(*key):
    """[dict(x, simplex, timestamp, uw_start, c, truth, burst)] of the frames of standard scene `key` = (fs, seed, amp) whose
    unique word passed on the CPU oracle: samples, the downmixer's timestamp [ns], the correlator's peak and its correction"""
    r, truth, fs = sc.oracle("standard", *key)
    frames = {f.id: f for f in r.frames if f.drop_reason == 0}
    out = []
    for d in r.demods:
        f = frames[d.id]
        assert d.timestamp == f.timestamp and d.direction == 1
        x = np.array(f.samples[:2 * f.num_samples], np.float32).view(np.complex64)
        out.append(dict(x=x, simplex=f.center_frequency > SIMPLEX_ABOVE, timestamp=int(f.timestamp), uw_start=int(f.uw_start_idx),
                        c=float(f.uw_start), truth=truth_ns(truth, fs, f.timestamp, f.center_frequency),
                        burst=burst_start_ns(truth, fs, f.timestamp, f.center_frequency)))
    return out
