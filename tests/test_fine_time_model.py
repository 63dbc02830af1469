"""The symbol timing estimator of option fine_time as tests/fine_time_model.py states it, on the CPU oracle's frames against
the time the scenes' bursts were generated at (no GPU, no library: the model alone).

Measured with the committed model, in us, over the frames whose unique word passed.  "printed" is the timestamp without the
option less the burst's first sample: its mean, and the largest deviation of a frame from that mean.  "correlator" and "line"
are the refined time (the timestamp + (uw_start + delta) / 250 kHz, delta the correlator's parabola correction or the
line's tau) less the centre of the unique word's first symbol: the largest error, and for the line mean / std / largest.

    scene                      frames  printed         correlator  line
    2 MHz, seed 3, amp 0.05    16      +86.0,  7.4     1.02        -0.03 / 0.18 / 0.26
    2 MHz, seed 5, amp 0.05    16      +88.6,  6.4     0.51        -0.02 / 0.14 / 0.26
    2 MHz, seed 3, amp 0.01    16      +100.3, 61.2    3.07        -0.14 / 0.65 / 1.54
    10 MHz, seed 3, amp 0.05   16      +86.1,  6.5     1.02        -0.10 / 0.20 / 0.51

The bounds asserted -- 0.52 / 0.52 / 3.08 / 1.02 us -- are twice the line's maxima.  |tau - c| stays within 0.79 samples;
quality runs from 3.2 to 32."""
import numpy as np
import pytest

import fine_time_model as tm
import fine_time_scenes as ts

SCENES = [((2_000_000, 3, 0.05), 0.52), ((2_000_000, 5, 0.05), 0.52), ((2_000_000, 3, 0.01), 3.08), ((10_000_000, 3, 0.05), 1.02)]


def errors(key):
    """per frame, in us: the unrefined timestamp less the burst's first sample, the correlator's and the line's error"""
    fr = ts.oracle_frames(*key)
    printed, e_corr, e_line = [], [], []
    for f in fr:
        tau, quality, flags, n = tm.estimate(f["x"], f["simplex"])
        d, flags = tm.delta(tau, flags, f["c"])
        assert flags == 0 and n == len(f["x"]) and d == tau, (flags, n, tau, f["c"], quality)
        printed.append((f["timestamp"] - f["burst"]) * 1e-3)
        e_corr.append((tm.refined_ns(f["timestamp"], f["uw_start"], f["c"]) - f["truth"]) * 1e-3)
        e_line.append((tm.refined_ns(f["timestamp"], f["uw_start"], d) - f["truth"]) * 1e-3)
    printed, e_corr, e_line = np.array(printed), np.array(e_corr), np.array(e_line)
    print("%s: %d frames, printed %+.1f dev %.1f us, correlator max %.2f us, line mean %+.2f std %.2f max %.2f us" %
          (key, len(fr), printed.mean(), np.abs(printed - printed.mean()).max(), np.abs(e_corr).max(), e_line.mean(), e_line.std(),
           np.abs(e_line).max()))
    return printed, e_corr, e_line


@pytest.mark.parametrize("key,bound", SCENES)
def test_scenes(key, bound):
    """every frame whose unique word passed carries no flag and is within the bound of truth; the correlator alone is worse on
    the scene's maximum; the unrefined timestamp wanders by more than 5 us about its own mean offset"""
    printed, e_corr, e_line = errors(key)
    assert len(e_line) >= 14
    assert np.abs(e_line).max() <= bound, e_line
    assert np.abs(e_corr).max() > np.abs(e_line).max(), (e_corr, e_line)
    assert np.abs(printed - printed.mean()).max() > 5.0, printed


def tone(tau, n=1310):
    """a frame whose |x|^2 is 1 + cos(2 pi (k - tau) / sps) / 2: maxima at tau + 10 k samples"""
    k = np.arange(n, dtype=np.float64)
    return np.sqrt(1.0 + 0.5 * np.cos(2.0 * np.pi * (k - tau) / tm.SPS)).astype(np.complex64)


def test_tau_lands_and_wraps_at_half_a_symbol():
    """on synthetic frames tau is the place of the symbol centre nearest to sample 0, in [-sps / 2, sps / 2): 4.9 and -4.9 are
    found as they are, 5.0 is -5.0 and 5.1 is -4.9"""
    for place, want in ((0.0, 0.0), (2.5, 2.5), (-2.5, -2.5), (4.9, 4.9), (-4.9, -4.9), (5.0, -5.0), (5.1, -4.9), (-5.1, 4.9),
                        (12.0, 2.0)):
        tau, q, flags, n = tm.estimate(tone(place))
        assert flags == 0 and q > 100 and -5.0 <= tau < 5.0       # (the floor of a pure line is its own side lobes')
        d = abs(tau - want)
        assert min(d, 10.0 - d) < 1e-6, (place, tau, want)        # (the frame's floats: 6e-8 of a sample's power)
        if abs(want) < 4.95:
            assert d < 1e-6, (place, tau, want)
    # the window: a simplex frame's line is that of its first 800 samples
    x = np.concatenate([tone(1.0, 800), tone(3.0, 510)])
    assert abs(tm.estimate(x, True)[0] - 1.0) < 1e-6 and 1.0 < tm.estimate(x, False)[0] < 3.0
    assert tm.window(1910) == 1310 and tm.window(1910, True) == 800 and tm.window(700) == 700 and tm.window(4440, True) == 800
    # no estimate
    for bad in (np.zeros(700, np.complex64), tone(0.0, 63), np.ones(64, np.complex64)):
        assert tm.estimate(bad)[2] == tm.INVALID
    nan = tone(0.0)
    nan[1309] = np.nan
    assert tm.estimate(nan, True)[2] == tm.INVALID


def test_host_rule():
    """ambiguous beyond a quarter of a symbol from the correlator's correction; a flagged record keeps the correlator's place"""
    assert tm.delta(1.0, 0, 0.5) == (1.0, 0) and tm.delta(3.0, 0, 0.5) == (3.0, 0)
    assert tm.delta(3.1, 0, 0.5) == (0.5, tm.AMBIGUOUS) and tm.delta(-2.1, 0, 0.5) == (0.5, tm.AMBIGUOUS)
    assert tm.delta(0.0, tm.INVALID, 0.25) == (0.25, tm.INVALID)
    assert tm.refined_ns(1000, 189, 0.5) == 1000 + 758000 and tm.refined_ns(10**6, 0, -0.6) == 10**6 - 2400
    assert tm.refined_ns(10**6, 0, -0.0001) == 10**6 and tm.refined_ns(10**6, 0, -0.0004) == 10**6 - 2


def test_histogram_quantiles():
    """the summary's quartiles are bin centres of 0.01-sample bins over +-2.5 samples; what lies beyond falls into the ends"""
    d = [-1.204, -0.032, 0.004, 0.006, 0.75, 2.5, -2.5, 7.0, -7.0]
    counts = np.bincount([tm.bin_of(v) for v in d], minlength=tm.NBINS)
    assert len(counts) == tm.NBINS == 501 and counts[0] == 2 and counts[-1] == 2
    assert tm.bin_of(0.004) == 250 and tm.bin_of(0.006) == 251 and tm.bin_of(-2.5) == 0 and tm.bin_of(2.5) == 500
    assert tm.quantile(counts, 0.5) == tm.BIN0 + 250 * tm.BIN_W and tm.quantile(counts, 0.25) == tm.BIN0 + 130 * tm.BIN_W
    assert tm.quantile(counts, 0.75) == tm.BIN0 + 325 * tm.BIN_W and tm.quantile(counts, 1.0) == tm.BIN0 + 500 * tm.BIN_W
    assert tm.quantile(np.zeros(tm.NBINS), 0.5) == 0.0
