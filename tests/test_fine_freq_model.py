"""The carrier frequency estimator of option fine_freq as tests/fine_freq_model.py states it, on the CPU oracle's frames
against the frequency the scenes were generated at (no GPU, no library: the model alone).

Measured with the committed model, error against truth in Hz, rms / max over the frames whose unique word passed:

    scene                                    frames  downmixer      + PLL (printed)  model
    2 MHz, seed 3, amp 0.05                  16      7.45 / 14.39   14.66 / 32.99    0.74 / 1.56
    2 MHz, seed 5, amp 0.05                  16      9.58 / 21.32   10.02 / 17.12    0.75 / 2.19
    2 MHz, seed 3, amp 0.01                  16      40.44 / 74.39  11.95 / 30.12    2.30 / 5.26
    12 bursts drifting +-390 Hz/s, seed 3    12      6.02 / 12.42   6.69 / 15.98     0.67 / 1.37
    12 bursts drifting +-390 Hz/s, seed 5    11      8.84 / 18.78   13.29 / 26.82    0.77 / 1.93

The bounds asserted -- 4 / 4 / 10 Hz and 4 Hz -- are about twice these maxima (fine_freq_scenes.py generates the drifting
scenes; their truth is the frequency at the middle of the frame)."""
import numpy as np
import pytest

import fine_freq_model as fm
import fine_freq_scenes as sc

STANDARD = [((2_000_000, 3, 0.05), 4.0), ((2_000_000, 5, 0.05), 4.0), ((2_000_000, 3, 0.01), 10.0)]
DRIFTING = [((3,), 4.0), ((5,), 4.0)]


def errors(kind, key):
    fr = sc.oracle_frames(kind, *key)
    e_pll, e_model = [], []
    for x, f_dm, f_pll, truth in fr:
        df, quality, flags, n = fm.estimate(x)
        assert flags == 0 and n == len(x) and quality > 5, (flags, n, quality)
        e_pll.append(f_pll - truth)
        e_model.append(f_dm + df - truth)
    e_pll, e_model = np.abs(e_pll), np.abs(e_model)
    print("%s %s: %d frames, PLL max %.2f Hz, model rms %.2f max %.2f Hz" %
          (kind, key, len(fr), e_pll.max(), np.sqrt(np.mean(e_model ** 2)), e_model.max()))
    return e_pll, e_model


@pytest.mark.parametrize("key,bound", STANDARD)
def test_standard_scenes(key, bound):
    """every frame within the bound of truth, where the printed frequency is off by more than 15 Hz on at least one"""
    e_pll, e_model = errors("standard", key)
    assert len(e_model) >= 14
    assert e_model.max() <= bound, e_model
    assert e_pll.max() > 15.0, e_pll


@pytest.mark.parametrize("key,bound", DRIFTING)
def test_drifting_scenes(key, bound):
    """a linear drift of +-390 Hz/s (3 Hz over a frame): within the bound of the frequency at the middle of the frame"""
    e_pll, e_model = errors("drifting", key)
    assert len(e_model) >= 10
    assert e_model.max() <= bound, e_model


def test_histogram_quantiles():
    """the summary's quartiles are bin centres of 1 Hz bins over +-500 Hz"""
    d = [-12.4, -3.2, 0.4, 0.6, 7.5, 600.0, -600.0]
    counts = np.bincount([fm.bin_of(v) for v in d], minlength=fm.NBINS)
    assert counts[0] == 1 and counts[-1] == 1 and fm.bin_of(0.4) == 500 and fm.bin_of(0.6) == 501
    assert fm.quantile(counts, 0.5) == 0.0 and fm.quantile(counts, 0.75) == 8.0 and fm.quantile(counts, 0.25) == -12.0 and fm.quantile(np.zeros(fm.NBINS), 0.5) == 0.0
