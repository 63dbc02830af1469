"""TEST INFRASTRUCTURE: the per-burst resampler (option "burst_resample", csrc/burst_resample.hpp) restated in numpy.

  design(L, M)          the prototype of csrc/host_design.cpp design_resample_proto() in binary64, operation for operation
                        (math.sin / math.cos: the C library's, as the product calls them), as the phase-major float32 table
  resample_f32(x, L, M) the kernel's arithmetic: per component one chain of float32 fused multiply-adds over the T taps in
                        ascending input index, starting from 0 -- bit for bit
  resample_f64(x, L, M) the same interpolation with the binary64 prototype in binary64: the reference the float32 result
                        is held against

Output m of a row x[0 .. n) at ratio L / M is the band-limited interpolation of x at input time m M / L:
  q = floor(m M / L), ph = (m M) mod L, y[m] = sum_k taps[ph][k] x[q - T/2 + 1 + k], x zero outside the row,
  taps[ph][k] = P[(k - T/2 + 1) L - ph], P the prototype at rate L f_in centred on 0; res_len = floor(n L / M).
"""
import math

import numpy as np

T = 20                      # taps per phase (kBrTaps)
MAX_L = 4096                # kBrMaxL
OUT_RATE = 250000
CUTOFF = 107500.0           # Hz: midway between the 50 kHz the passband is flat to and the 165 kHz the stopband begins at


def ratio(fs, decim=None):
    """L / M = decim 250000 / fs in lowest terms."""
    if decim is None:
        decim = max(1, int(np.float32(np.round(np.float32(fs) / np.float32(OUT_RATE)))))
    g = math.gcd(decim * OUT_RATE, fs)
    return decim * OUT_RATE // g, fs // g


def proto64(L, M, taps=T):
    """P[j], j = -T L / 2 + 1 .. T L / 2, as a float64 array indexed j + T L / 2 - 1."""
    n = L * taps
    half = n // 2
    omega = 2.0 * math.pi * CUTOFF / (float(OUT_RATE) * float(M))     # the row rate is 250000 M / L
    out = [0.0] * n
    total = 0.0
    for i in range(n):
        j = i - half + 1
        if j == 0:
            h = omega / math.pi
        else:
            h = math.sin(omega * j) / (math.pi * j)
        x = float(i + 1) / float(n)
        w = (0.35875 - 0.48829 * math.cos(2.0 * math.pi * x) + 0.14128 * math.cos(4.0 * math.pi * x)
             - 0.01168 * math.cos(6.0 * math.pi * x))
        out[i] = h * w
        total += out[i]
    scale = float(L) / total
    return np.array([v * scale for v in out], dtype=np.float64)


def phase_major(p, L, taps=T):
    """table[ph][k] = P[(k - T/2 + 1) L - ph]"""
    half = L * taps // 2
    k = np.arange(taps)[None, :]
    ph = np.arange(L)[:, None]
    j = (k - taps // 2 + 1) * L - ph
    return p[j + half - 1]


_cache = {}


def design64(L, M):
    if ("d", L, M) not in _cache:
        _cache[("d", L, M)] = phase_major(proto64(L, M), L)
    return _cache[("d", L, M)]


def design(L, M):
    if ("f", L, M) not in _cache:
        _cache[("f", L, M)] = design64(L, M).astype(np.float32)
    return _cache[("f", L, M)]


def prototype_of(table):
    """the phase-major table back as P[j], j = -T L / 2 + 1 .. T L / 2"""
    L, taps = table.shape
    p = np.zeros(L * taps, table.dtype)
    k = np.arange(taps)[None, :]
    ph = np.arange(L)[:, None]
    p[(k - taps // 2 + 1) * L - ph + L * taps // 2 - 1] = table
    return p


def res_len(n, L, M):
    return n * L // M


def _gather(x, L, M):
    n = len(x)
    m = np.arange(res_len(n, L, M), dtype=np.int64)
    q = (m * M) // L
    ph = (m * M) % L
    idx = q[:, None] - T // 2 + 1 + np.arange(T, dtype=np.int64)[None, :]
    ok = (idx >= 0) & (idx < n)
    xs = np.where(ok, x[np.clip(idx, 0, max(n - 1, 0))], 0)
    return xs, ph


def _fma32(a, b, c):
    """float32 fma(a, b, c) of float32 arrays, correctly rounded: the product is exact in binary64, the sum is rounded to
    odd there (53 >= 2 * 24 + 2 bits) and then once to float32"""
    p = a.astype(np.float64) * b.astype(np.float64)
    c = c.astype(np.float64)
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)                         # TwoSum: p + c = s + err exactly
    even = (s.view(np.int64) & 1) == 0
    fix = (err != 0) & even
    toward = np.where(err > 0, np.inf, -np.inf)
    s = np.where(fix, np.nextafter(s, toward), s)
    return s.astype(np.float32)


def resample_f32(x, L, M):
    x = np.asarray(x, dtype=np.complex64)
    taps = design(L, M)
    xs, ph = _gather(x, L, M)
    re = np.zeros(len(ph), dtype=np.float32)
    im = np.zeros(len(ph), dtype=np.float32)
    xr = np.ascontiguousarray(xs.real).astype(np.float32)
    xi = np.ascontiguousarray(xs.imag).astype(np.float32)
    for k in range(T):
        t = taps[ph, k]
        re = _fma32(t, xr[:, k], re)
        im = _fma32(t, xi[:, k], im)
    return (re + 1j * im).astype(np.complex64)


def resample_f64(x, L, M):
    x = np.asarray(x, dtype=np.complex128)
    taps = design64(L, M)
    xs, ph = _gather(x, L, M)
    return np.sum(taps[ph] * xs, axis=1)


def response_db(L, M, freqs_hz):
    """|H(f)| in dB of the float32 table read as the prototype at rate L f_in, f_in = 250000 M / L (gain L taken out)"""
    f_in = float(OUT_RATE) * M / L
    taps = design(L, M).astype(np.float64)
    k = np.arange(T)[None, :]
    ph = np.arange(L)[:, None]
    j = ((k - T // 2 + 1) * L - ph).ravel()
    p = taps.ravel()
    out = []
    for f in freqs_hz:
        w = 2.0 * math.pi * f / (L * f_in)
        out.append(abs(np.sum(p * np.exp(-1j * w * j))) / L)
    return 20.0 * np.log10(np.maximum(np.array(out), 1e-300))
