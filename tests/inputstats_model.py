"""TEST INFRASTRUCTURE: a model of irdm_input_stats_t (include/irdm_hip.h) in Python integers (the integer formats) and
math.fsum (cf32), and the comparison of a struct the library filled against it.

Integer formats: x = c * 2^-K with an integer c; sum and sum_sq are the exact integer totals divided by the power of two,
which Python's int / int rounds once -- the struct's doubles must equal them bit for bit.  cf32: x and x^2 are exact doubles,
fsum gives their correctly rounded sums; the library sums the same exact terms in some order, so its error is at most
n 2^-53 times the sum of the terms' magnitudes (the bound of any-order recursive summation of n exact terms, to first order;
the terms of sum_sq are all positive, so that bound is relative)."""
import math
import struct

import numpy as np

import irdm

# format -> (K, negative rail, positive rail) on the file's codes
INT_FORMATS = {irdm.FMT_CI8: (7, -128, 127), irdm.FMT_CU8: (8, 0, 255), irdm.FMT_CI16: (7, -32768, 32767),
               irdm.FMT_CI16_FULL: (15, -32768, 32767), irdm.FMT_SC16Q11: (11, -2048, 2047)}
NAMES = {irdm.FMT_CI8: "ci8", irdm.FMT_CI16: "ci16", irdm.FMT_CF32: "cf32", irdm.FMT_CI16_FULL: "ci16-full",
         irdm.FMT_SC16Q11: "sc16q11", irdm.FMT_CU8: "cu8"}
DTYPES = {irdm.FMT_CI8: np.int8, irdm.FMT_CU8: np.uint8, irdm.FMT_CI16: np.int16, irdm.FMT_CI16_FULL: np.int16,
          irdm.FMT_SC16Q11: np.int16, irdm.FMT_CF32: np.complex64}
FORMATS = tuple(sorted(DTYPES))


def n_samples(x, fmt):
    return len(x) if fmt == irdm.FMT_CF32 else len(x) // 2


def _int_sum(a):
    """the exact sum of an int64 array as a Python integer (pieces small enough that int64 cannot overflow)"""
    return sum(int(a[i:i + 65536].sum()) for i in range(0, len(a), 65536))


def model(x, fmt):
    """the fields of irdm_input_stats_t for the raw samples x (interleaved codes, or complex64)"""
    n = n_samples(x, fmt)
    m = dict(n_samples=n, n_rail_lo=[0, 0], n_rail_hi=[0, 0], n_nonfinite=[0, 0], code_min=[0, 0], code_max=[0, 0],
             sum=[0.0, 0.0], sum_sq=[0.0, 0.0], abs_max=[np.float32(0), np.float32(0)])
    if n == 0:
        return m
    if fmt == irdm.FMT_CF32:
        v = np.ascontiguousarray(x, np.complex64).view(np.float32)
        for k in range(2):
            c = v[k::2]
            fin = np.isfinite(c)
            f = c[fin].astype(np.float64)
            m["n_nonfinite"][k] = int((~fin).sum())
            m["n_rail_lo"][k] = int((f <= -1.0).sum())
            m["n_rail_hi"][k] = int((f >= 1.0).sum())
            m["sum"][k] = math.fsum(f)
            m["sum_sq"][k] = math.fsum(f * f)
            m["abs_max"][k] = np.float32(np.abs(f).max()) if len(f) else np.float32(0)
            m["sum_abs_%d" % k] = math.fsum(np.abs(f))
        return m
    K, lo, hi = INT_FORMATS[fmt]
    codes = np.asarray(x).astype(np.int64)
    for k in range(2):
        v = codes[k::2]
        c = 2 * v - 255 if fmt == irdm.FMT_CU8 else (v >> 8 if fmt == irdm.FMT_CI16 else v)
        m["n_rail_lo"][k] = int((v <= lo).sum())
        m["n_rail_hi"][k] = int((v >= hi).sum())
        m["code_min"][k], m["code_max"][k] = int(v.min()), int(v.max())
        m["sum"][k] = _int_sum(c) / (1 << K)
        m["sum_sq"][k] = _int_sum(c * c) / (1 << (2 * K))
        m["abs_max"][k] = np.float32(int(np.abs(c).max()) / (1 << K))
    return m


def fields(st):
    """an irdm.InputStats as the model's dict"""
    return dict(n_samples=int(st.n_samples), n_rail_lo=list(st.n_rail_lo), n_rail_hi=list(st.n_rail_hi),
                n_nonfinite=list(st.n_nonfinite), code_min=list(st.code_min), code_max=list(st.code_max), sum=list(st.sum),
                sum_sq=list(st.sum_sq), abs_max=[np.float32(v) for v in st.abs_max])


def _bits64(v):
    return struct.pack("<d", v)


def check(st, m, fmt, what=""):
    """the struct against the model: integer formats every field, doubles by their bits; cf32 counts and abs_max exactly,
    the sums within the any-order summation bound"""
    g = fields(st)
    for key in ("n_samples", "n_rail_lo", "n_rail_hi", "n_nonfinite", "code_min", "code_max"):
        assert g[key] == m[key], (what, key, g[key], m[key])
    for k in range(2):
        assert np.float32(g["abs_max"][k]).tobytes() == np.float32(m["abs_max"][k]).tobytes(), (what, "abs_max", k, g["abs_max"], m["abs_max"])
        if fmt != irdm.FMT_CF32:
            assert _bits64(g["sum"][k]) == _bits64(m["sum"][k]), (what, "sum", k, g["sum"][k], m["sum"][k])
            assert _bits64(g["sum_sq"][k]) == _bits64(m["sum_sq"][k]), (what, "sum_sq", k, g["sum_sq"][k], m["sum_sq"][k])
        else:
            n = m["n_samples"]
            assert abs(g["sum_sq"][k] - m["sum_sq"][k]) <= n * 2.0 ** -53 * m["sum_sq"][k], (what, "sum_sq", k, g["sum_sq"][k], m["sum_sq"][k])
            assert abs(g["sum"][k] - m["sum"][k]) <= n * 2.0 ** -53 * m.get("sum_abs_%d" % k, 0.0), (what, "sum", k, g["sum"][k], m["sum"][k])


def random_input(fmt, n, seed):
    """n samples spread over the whole code range (cf32: about +-1.5, so both rails are met)"""
    rng = np.random.default_rng(seed)
    if fmt == irdm.FMT_CF32:
        return ((rng.standard_normal(n) + 1j * rng.standard_normal(n)) * 0.5).astype(np.complex64)
    info = np.iinfo(DTYPES[fmt])
    lo, hi = (-2100, 2100) if fmt == irdm.FMT_SC16Q11 else (info.min, info.max + 1)
    return rng.integers(lo, hi, 2 * n).astype(DTYPES[fmt])


def with_rails_at_the_ends(x, fmt):
    """the first sample at the negative rail (I) / positive rail (Q), the last the other way round"""
    x = x.copy()
    if n_samples(x, fmt) == 0:
        return x
    if fmt == irdm.FMT_CF32:
        x[0] = np.complex64(-1.0 + 1.0j)
        x[-1] = np.complex64(1.0 - 1.0j)
        return x
    _, lo, hi = INT_FORMATS[fmt]
    x[0], x[1] = lo, hi
    x[-2], x[-1] = hi, lo
    return x


def special_cf32(n, seed):
    """NaN, +-Inf, +-1.0 exactly, values next to +-1.0 and subnormals scattered through a random stream"""
    rng = np.random.default_rng(seed)
    v = (rng.standard_normal(2 * n) * 0.3).astype(np.float32)
    specials = np.array([np.nan, np.inf, -np.inf, 1.0, -1.0, np.nextafter(np.float32(1), np.float32(0)),
                         np.nextafter(np.float32(-1), np.float32(0)), 1e-40, -1e-45, 1.4e-45, 0.0, -0.0, 3.5, -7.25], np.float32)
    idx = rng.choice(2 * n, size=min(2 * n, 4 * len(specials)), replace=False)
    v[idx] = np.resize(specials, len(idx))
    return v.view(np.complex64)


class DeviceInput:
    """x in device memory at an address `off` samples past a 16-byte boundary"""

    def __init__(self, x, fmt, off=0, device=0):
        raw = np.ascontiguousarray(x).view(np.uint8)
        bps = 8 if fmt == irdm.FMT_CF32 else raw.itemsize * (2 * np.dtype(DTYPES[fmt]).itemsize)
        pad = np.zeros(len(raw) + 64, np.uint8)
        self.base = irdm.device_buffer(pad, device)
        self.ptr = self.base + (-self.base) % 16 + off * bps
        assert (self.ptr - off * bps) % 16 == 0
        if len(raw):
            import ctypes as C
            assert irdm.lib().irdm_device_upload(C.c_void_p(self.ptr), raw.ctypes.data_as(C.c_void_p), raw.nbytes) == 0
        self.n = n_samples(x, fmt)

    def close(self):
        irdm.device_free(self.base)
