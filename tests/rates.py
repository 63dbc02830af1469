"""TEST INFRASTRUCTURE: what a context is at a sample rate -- the dispatch rules of the product restated (create.cpp:
rate_supported and the detector constants; scan_band.hip: band_scan_supported; scan_host.cpp: scan_pick; downmix.hip:
fir_reg_path, fir_tile_row) -- the streams the rate tests run, and the assertions they share
(tests/test_pipeline_emul.py under the emulation, tests/test_gpu_rates.py on the card: both assert that the scan this
restatement names is the one whose counter moved, and that the context's FFT size is the one given here)."""
import numpy as np

import siggen

# every class of rate irdm_create accepts: the front ends' output rates on 25 / 30.72 / 50 / 61.44 MS/s captures, the
# edges of acceptance, one rate per FFT size and scan form
GPU_RATES = (725_000, 1_500_000, 2_500_000, 3_000_000, 5_000_000, 6_250_000, 7_680_000, 8_000_000, 10_240_000,
             12_500_000, 15_360_000, 16_000_000, 20_000_000, 22_600_000)
EMUL_RATES = (725_000, 1_500_000, 2_500_000, 5_000_000, 6_250_000, 10_240_000, 12_500_000, 16_000_000, 20_000_000)

K_MAX_ACTIVE = 1024          # types.hpp
K_FIR_TAPS = 801
K_FIR_TILE_OUT = 128         # types.hpp


def fft_size(fs):
    return 1 << int(round(np.log2(fs / 1000.0)))


def describe(fs):
    """dict(n, width, max_bursts, supported, decim, scan, decimator, band_w, fir_lds_bytes)"""
    n = fft_size(fs)
    width = 40000 // max(fs // n, 1)
    max_bursts = int(np.float32(np.float32(fs) / np.float32(40000)) * np.float32(0.8))
    supported = not (n < 1024 or n > 16384 or max_bursts + n // max(width, 1) + 8 > K_MAX_ACTIVE)
    hw = width // 2
    band_w = 128 if hw <= 20 else 256
    n_bands = n // band_w
    gap = (int(fs * 16e-3) + n - 1) // n
    band = (2048 <= n <= 16384 and 1 <= n_bands <= 64 and hw >= 1 and 2 * hw + 8 <= band_w // 2 and 1 <= gap < 64
            and 0 < max_bursts <= K_MAX_ACTIVE - 64)
    scan = "band" if band else ("wave" if n >= 2048 else "dense")
    decim = int(round(fs / 250000.0))
    row = K_FIR_TILE_OUT + K_FIR_TAPS // decim + 2
    while row & 15 != 1:
        row += 1
    return dict(n=n, width=width, max_bursts=max_bursts, supported=supported, decim=decim, scan=scan, band_w=band_w,
                decimator="register" if decim in (40, 48) else "any-M", fir_lds_bytes=8 * row * decim)


def stream(fs, bursts=6):
    """the rate tests' stream: the priming frames, then 0.45 s with `bursts` frames on random channels"""
    n = int(520 * fft_size(fs) + 0.45 * fs) // 32768 * 32768
    return siggen.standard_scene(fs, n, bursts, seed=fs // 1000)[0]


def chunks_of(n, parts):
    blocks = n // 32768
    cuts = [blocks * (i + 1) // parts for i in range(parts)]
    out, prev = [], 0
    for c in cuts:
        if c > prev:
            out.append((c - prev) * 32768)
            prev = c
    if n % 32768:
        out[-1] += n % 32768
    return out


def check_counts(summary, min_bursts=5, min_demods=4):
    """no comparison of empty lists: what parity.compare() returned for the run"""
    assert summary["bursts"] >= min_bursts and summary["demods"] >= min_demods and summary["frames"] >= min_demods, summary


def check_scan(stats, fs, scan=None):
    """the scan the dispatch rules give at this rate ran, and nothing fell back (stats: parity.run_gpu()["stats"])"""
    scan = scan or describe(fs)["scan"]
    if scan == "band":
        assert stats["band_chunks"] >= 1, (fs, stats)
    elif scan == "wave":
        assert stats["band_chunks"] == 0 and stats["scan_fast_chunks"] >= 1, (fs, stats)
    else:
        assert stats["band_chunks"] == 0 and stats["scan_fast_chunks"] == 0, (fs, stats)
    assert stats["scan_fallbacks"] == 0, (fs, stats)
