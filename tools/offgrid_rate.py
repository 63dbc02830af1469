#!/usr/bin/env python3
"""Share of whole frames when the pipeline is fed at a rate off the 250 kHz grid, on the CPU oracle (no GPU): the rows of
the README's table "Sample rates off the 250 kHz grid".  The scene is siggen.standard_scene's (1 s, 30 bursts, seed 3,
amp 0.05, noise 0.002) with the pulse evaluated at the rate's fractional samples per symbol
(tests/resample_model.py make_burst_fractional), so rates that are no multiple of 25 kHz -- 10.24 MHz = 61.44 MS/s / 6 --
can be rendered.  "whole": every payload bit of the frame right.

  python3 tools/offgrid_rate.py 10000000 10240000 10025000 11200000
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "iridium-sniffer_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))


def scene(fs, seed=3, n_bursts=30):
    import resample_model as rm
    import siggen
    n = int(1.0 * fs) // 32768 * 32768
    rng = np.random.default_rng(seed + 1000)
    first = 520 * (1 << int(round(np.log2(fs / 1000.0))))
    starts = np.sort(rng.integers(0, n - first - int(0.05 * fs), size=n_bursts)) + first
    half_ch = int((fs / 2 - 60e3) // (1e6 / 24.0))
    g = np.random.default_rng(seed)
    iq = (g.standard_normal(n, dtype=np.float32) + 1j * g.standard_normal(n, dtype=np.float32)).astype(np.complex64) * np.float32(0.002)
    expect = []
    for s in starts:
        payload = rng.integers(0, 4, size=int(rng.integers(119, 180))).tolist()
        ch = int(rng.integers(-half_ch, half_ch + 1)) or 1
        quads = siggen.frame_quadrants(payload)
        sig = rm.make_burst_fractional(fs, quads, siggen.channel_freq(ch), g.uniform(0, 2 * np.pi))
        e = min(n, s + len(sig))
        iq[s:e] += sig[:e - s]
        expect.append(siggen.quadrants_to_bits(quads[16:]))
    return iq, expect


def main():
    import orc
    import resample_model as rm
    for fs in [int(a) for a in sys.argv[1:]] or [10_000_000, 10_240_000]:
        x, expect = scene(fs)
        r = orc.run_stream(x, fs)
        decim = int(round(fs / 250000.0))
        print("%d Hz: decimated rate %.0f, clock error %+.3f %%, %d frames, %d of %d payloads whole" %
              (fs, fs / decim, (fs / decim / 250000.0 - 1) * 100, len(r.demods), rm.whole_payloads(r.demods, expect), len(expect)))


if __name__ == "__main__":
    main()
