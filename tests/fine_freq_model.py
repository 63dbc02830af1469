"""TEST INFRASTRUCTURE: the carrier frequency estimator of csrc/fine_freq.hpp (option "fine_freq") in float64 numpy.

The fourth power of a QPSK frame carries a spectral line at four times the frame's residual carrier offset.  The frame is
x[n], n = 0 .. N - 1, at f_o samples per second (the context's out_rate, 250 000):
    y[n]  = x[n]^4 in binary64 from the float pair: a = re re - im im, b = 2 re im, y = (a a - b b) + i 2 a b, every product
            and difference rounded separately
    P(g)  = |sum_n y[n] exp(-2 pi i g n / f_o)|^2, the phase the fraction of g n / f_o
    coarse: g_k = -1000 + 20 k Hz, k = 0 .. 100; k_c the first maximum
    fine:   h_j = g_kc + 4 (j - 5), j = 0 .. 10; j* the first maximum; 0 < j* < 10: g* = h_j* + 4 * 0.5 (a - c) / (a - 2 b + c)
            over (a, b, c) = P(h_{j* - 1 .. j* + 1}); otherwise g* = h_j*
    df = g* / 4 Hz, quality = P(g_kc) / mean_k P(g_k) over the 101 coarse points
The same sum is taken at GUARD more points of the coarse step beyond either edge (+-1020 .. +-1200 Hz).  They enter nothing
else: if one of them exceeds P(g_kc), or k_c is 0 or 100, the frame is out of range and df is the edge of that side, +-250 Hz.
A frame shorter than 64 or longer than 4440 samples, with a sample that is not finite, without a coarse P above 0 or with a
sum of the coarse P above 1e300 is invalid: df = quality = 0.

The estimate is the frequency at the middle of the frame: a linear drift leaves the line's centre there.  A frame more than
+-300 Hz from the downmixer's value is not seen: its line is beyond the guard points, and the grid shows the modulation."""
import numpy as np

F_OUT = 250000.0
G0, STEP, NK = -1000.0, 20.0, 101
GUARD = 10
FINE_STEP, NFINE = 4.0, 11
MIN_SAMPLES, MAX_SAMPLES = 64, 4440
INVALID, OUT_OF_RANGE, NOT_OK = 1, 2, 4
EDGE = 250.0
BIN0, NBINS = -500, 1001           # the summary's histogram: 1 Hz bins over +-500 Hz


def fourth(x):
    """y = x^4 of a complex64 frame, as the kernel forms it"""
    x = np.asarray(x, np.complex64)
    re, im = x.real.astype(np.float64), x.imag.astype(np.float64)
    a = re * re - im * im
    b = 2.0 * (re * im)
    return (a * a - b * b) + 1j * (2.0 * (a * b))


def power(y, g, f_out=F_OUT):
    """P(g) for the frequencies g [Hz] over y"""
    ph = np.outer(np.asarray(g, np.float64), np.arange(len(y), dtype=np.float64)) / f_out
    ph -= np.floor(ph)
    s = np.exp(-2j * np.pi * ph) @ y
    return s.real ** 2 + s.imag ** 2


def estimate(x, f_out=F_OUT):
    """(df, quality, flags, n) of one frame"""
    x = np.asarray(x, np.complex64)
    n = len(x)
    if n < MIN_SAMPLES or n > MAX_SAMPLES:
        return 0.0, 0.0, INVALID, n
    if not (np.isfinite(x.real).all() and np.isfinite(x.imag).all()):
        return 0.0, 0.0, INVALID, n
    y = fourth(x)
    with np.errstate(all="ignore"):
        Pg = power(y, G0 + STEP * np.arange(-GUARD, NK + GUARD), f_out)
    P = Pg[GUARD:GUARD + NK]
    if not np.isfinite(P).all() or not P.max() > 0 or not P.sum() <= 1e300:
        return 0.0, 0.0, INVALID, n
    kc = int(np.argmax(P))
    q = float(P[kc] / (P.sum() / NK))
    lo, hi = Pg[:GUARD].max(), Pg[GUARD + NK:].max()
    if max(lo, hi) > P[kc]:
        return (-EDGE if lo >= hi else EDGE), q, OUT_OF_RANGE, n
    if kc == 0 or kc == NK - 1:
        return (-EDGE if kc == 0 else EDGE), q, OUT_OF_RANGE, n
    h = (G0 + STEP * kc) + FINE_STEP * (np.arange(NFINE) - 5.0)
    Pf = power(y, h, f_out)
    j = int(np.argmax(Pf))
    g = h[j]
    if 0 < j < NFINE - 1:
        a, b, c = Pf[j - 1], Pf[j], Pf[j + 1]
        g = h[j] + FINE_STEP * (0.5 * (a - c) / (a - 2.0 * b + c))
    return float(g / 4.0), q, 0, n


def bin_of(d):
    """the histogram bin of a difference refined - PLL [Hz]"""
    k = int(np.floor(float(d) - BIN0 + 0.5))
    return min(max(k, 0), NBINS - 1)


def quantile(counts, q):
    """the centre [Hz] of the bin that holds the ceil(q N)-th smallest of the N differences counted"""
    total = int(np.sum(counts))
    if total == 0:
        return 0.0
    want = max(1, int(np.ceil(q * total)))
    k = int(np.searchsorted(np.cumsum(counts), want))
    return float(BIN0 + k)
