"""TEST INFRASTRUCTURE: the symbol clock estimator of csrc/symbol_clock.hpp (option "symbol_clock") in float64 numpy, and the
frames the kernel tests share.

|x|^2 of a downmixed frame carries a spectral line at the symbol rate.  With a nominal sps samples per symbol and a clock
error eps the line sits at 1 / (sps (1 + eps)) cycles per sample:
    p[n]  = re^2 + im^2,  p' = p - mean(p)
    P[k]  = |sum_n p'[n] exp(-2 pi i f_k n)|^2,  f_k = 1 / (sps (1 + eps_k)),  eps_k = -0.08 + 0.001 k,  k = 0 .. 160
    k*    = the first maximum;  0 < k* < 160: eps = eps_0 + (k* + d) 0.001 with d = 0.5 (a - c) / (a - 2 b + c) over
            (a, b, c) = P[k* - 1 .. k* + 1];  otherwise out of range and eps = eps_k*
    quality = P[k*] / mean_k P[k]
A line beyond the grid leaves no maximum at its edge once it is further out than its own main lobe (1 / n cycles per
sample): the grid then shows the frame's modulation.  So the same sum is taken at GUARD more points of the same step on
either side (eps = -11 % .. -8.1 % and +8.1 % .. +11 %); if one of them exceeds P[k*] the frame is out of range as well, and
eps is the edge of the grid on that side.  The guard points enter nothing else: k*, quality and the eps of a frame that is
not flagged are those of the 161 points.
A frame shorter than 64 samples, all zero (no P above 0) or with a sample that is not finite is invalid: eps = quality = 0."""
import numpy as np

EPS0, STEP, NK = -0.08, 0.001, 161
GUARD = 30                         # points beyond either edge that only flag a frame
MIN_SAMPLES, MAX_SAMPLES = 64, 4440
INVALID, OUT_OF_RANGE, NOT_OK = 1, 2, 4
BIN, NBINS = 1e-4, 1601            # the histogram of the summary: 0.01 % bins over +-8 %


def grid(sps=10.0, guard=0):
    eps = EPS0 + STEP * np.arange(-guard, NK + guard)
    return eps, 1.0 / (float(sps) * (1.0 + eps))


def spectrum(x, sps=10.0, guard=0):
    """P[k] of one frame (complex64 [n]), k = -guard .. 160 + guard; None if a sample is not finite"""
    x = np.asarray(x, np.complex64)
    p = x.real.astype(np.float64) ** 2 + x.imag.astype(np.float64) ** 2
    if not np.isfinite(p).all():
        return None
    p = p - p.mean()
    _, f = grid(sps, guard)
    ph = np.outer(f, np.arange(len(p), dtype=np.float64))
    ph -= np.floor(ph)
    s = np.exp(-2j * np.pi * ph) @ p
    return s.real ** 2 + s.imag ** 2


def estimate(x, sps=10.0):
    """(eps, quality, flags, n) of one frame"""
    n = len(x)
    if n < MIN_SAMPLES:
        return 0.0, 0.0, INVALID, n
    Pg = spectrum(x, sps, GUARD)
    P = None if Pg is None else Pg[GUARD:GUARD + NK]
    if P is None or not np.isfinite(P).all() or not P.max() > 0:
        return 0.0, 0.0, INVALID, n
    k = int(np.argmax(P))
    q = float(P[k] / P.mean())
    lo, hi = Pg[:GUARD].max(), Pg[GUARD + NK:].max()
    if max(lo, hi) > P[k]:
        return (EPS0 if lo >= hi else EPS0 + (NK - 1) * STEP), q, OUT_OF_RANGE, n
    if 0 < k < NK - 1:
        a, b, c = P[k - 1], P[k], P[k + 1]
        return EPS0 + (k + 0.5 * (a - c) / (a - 2.0 * b + c)) * STEP, q, 0, n
    return EPS0 + k * STEP, q, OUT_OF_RANGE, n


def bin_of(eps):
    """the histogram bin of an estimate (a float, as the record holds it)"""
    return int(np.floor((float(eps) + 0.08) / BIN + 0.5))


def quantile(counts, q):
    """the centre of the bin that holds the ceil(q N)-th smallest of the N estimates counted"""
    total = int(np.sum(counts))
    if total == 0:
        return 0.0
    want = max(1, int(np.ceil(q * total)))
    k = int(np.searchsorted(np.cumsum(counts), want))
    return -0.08 + k * BIN


def truth(fs):
    """the clock error the detector sees of a scene generated at fs with whole samples per symbol"""
    decim = int(round(fs / 250000))
    return (fs // 25000) / (10.0 * decim) - 1.0
