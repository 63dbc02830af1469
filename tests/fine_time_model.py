"""TEST INFRASTRUCTURE: the symbol timing estimator of csrc/fine_time.hpp (option "fine_time") in float64 numpy.

|x|^2 of a frame carries a spectral line at the symbol rate, and the phase of that line is the symbol timing (Oerder and
Meyr).  The frame is x[n], n = 0 .. N - 1, at a nominal sps = 10 samples per symbol:
    W     = min(N, 131 sps), or min(N, 80 sps) for a simplex burst: the part of a frame that holds signal whatever its length
    p[n]  = re re + im im in binary64 from the float pair, p' = p - mean(p) over the window
    S(f)  = sum_{n < W} p'[n] exp(-2 pi i f n), the phase the fraction of f n;  f0 = 1 / sps
    tau   = -arg S(f0) / 2 pi * sps in [-sps / 2, sps / 2): the distance in samples from x[0] to the nearest symbol centre
    floor = mean of |S(f_j)|^2 over f_j = f0 (1 + 0.02 j), j = +-2 .. +-9;  quality = |S(f0)|^2 / floor
The kernel's record is (Re S(f0), Im S(f0), floor, flags, n); arg, tau and quality are taken on the host from it
(tau_of_record).  A frame shorter than 64 or longer than 4440 samples, with a sample that is not finite, with |S(f0)|^2
not above 0 or with the floor's sum above 1e300 is invalid: every number of its record is 0.

Host side, per frame that reached the demodulator, with c the correlator's parabola correction (uw_corr): the record is
ambiguous where |tau - c| > sps / 4; delta = tau where the record carries no flag, else c; the time of the frame's sample 0
is the downmixer's timestamp + llrint((uw_start + delta) 1e9 / out_rate)."""
import math

import numpy as np

F_OUT = 250000.0
SPS = 10.0
WIN_NORMAL, WIN_SIMPLEX = 131, 80          # symbols
FLOOR_J = [j for j in range(-9, 10) if abs(j) >= 2]
FLOOR_STEP = 0.02
MIN_SAMPLES, MAX_SAMPLES = 64, 4440
INVALID, AMBIGUOUS, NOT_OK = 1, 2, 4
BIN0, BIN_W, NBINS = -2.5, 0.01, 501        # the summary's histogram of tau - c: 0.01-sample bins over +-2.5 samples


def window(n, simplex=False, sps=SPS):
    return min(n, int((WIN_SIMPLEX if simplex else WIN_NORMAL) * sps))


def line(p, f):
    """S(f) for the frequencies f [cycles per sample] over p"""
    ph = np.outer(np.asarray(f, np.float64), np.arange(len(p), dtype=np.float64))
    ph -= np.floor(ph)
    return np.exp(-2j * np.pi * ph) @ p


def record(x, simplex=False, sps=SPS):
    """(Re S(f0), Im S(f0), floor, flags, n) of one frame: the kernel's record"""
    x = np.asarray(x, np.complex64)
    n = len(x)
    if n < MIN_SAMPLES or n > MAX_SAMPLES:
        return 0.0, 0.0, 0.0, INVALID, n
    if not (np.isfinite(x.real).all() and np.isfinite(x.imag).all()):
        return 0.0, 0.0, 0.0, INVALID, n
    w = window(n, simplex, sps)
    re, im = x.real[:w].astype(np.float64), x.imag[:w].astype(np.float64)
    p = re * re + im * im
    p = p - p.sum() / w
    f0 = 1.0 / sps
    with np.errstate(all="ignore"):
        s = line(p, [f0] + [f0 * (1.0 + FLOOR_STEP * j) for j in FLOOR_J])
        pw = s.real ** 2 + s.imag ** 2
    if not pw[0] > 0 or not pw[1:].sum() <= 1e300:
        return 0.0, 0.0, 0.0, INVALID, n
    return float(s[0].real), float(s[0].imag), float(pw[1:].sum() / len(FLOOR_J)), 0, n


def tau_of_record(re, im, floor, sps=SPS):
    """(tau [samples], quality) of a record without a flag, as the host takes them"""
    tau = -math.atan2(im, re) / (2.0 * math.pi) * sps
    if tau >= 0.5 * sps:            # (atan2 gives -pi for an imaginary part of -0)
        tau -= sps
    return tau, (re * re + im * im) / floor


def estimate(x, simplex=False, sps=SPS):
    """(tau, quality, flags, n) of one frame"""
    re, im, floor, flags, n = record(x, simplex, sps)
    if flags:
        return 0.0, 0.0, flags, n
    tau, q = tau_of_record(re, im, floor, sps)
    return tau, q, 0, n


def delta(tau, flags, c, sps=SPS):
    """(delta, flags) of the host's rule: the line's place, or the correlator's where the record is flagged or ambiguous"""
    if not flags & INVALID and abs(tau - c) > sps / 4.0:
        flags |= AMBIGUOUS
    return (c if flags else tau), flags


def refined_ns(timestamp_ns, uw_start, d, f_out=F_OUT):
    """the time of the frame's sample 0: llrint rounds to even, as round() does"""
    return int(timestamp_ns) + int(round((uw_start + d) * 1e9 / f_out))


def bin_of(d):
    """the histogram bin of a difference tau - c [samples]"""
    k = math.floor((float(d) - BIN0) / BIN_W + 0.5)
    return int(min(max(k, 0), NBINS - 1))


def quantile(counts, q):
    """the centre [samples] of the bin that holds the ceil(q N)-th smallest of the N differences counted"""
    total = int(np.sum(counts))
    if total == 0:
        return 0.0
    want = max(1, int(np.ceil(q * total)))
    k = int(np.searchsorted(np.cumsum(counts), want))
    return BIN0 + k * BIN_W
