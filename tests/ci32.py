"""Helpers of the int32 format tests (tests/test_gpu_ci32.py, tests/ci32_emul_run.py, tests/test_gpu_containers.py).

The contract (include/irdm_hip.h, IRDM_FMT_CI32 / IRDM_FMT_CI32_24): a context in either format produces exactly the records
of a cf32 context fed v.astype(np.float32) * np.float32(scale), scale 2^-31 / 2^-23.  run / same_records / chunks_of are
those of tests/formats16.py, which take any interleaved integer format.

The input-statistics model of tests/inputstats_model.py is extended here, by import, with the two formats: c = v, K = 31 /
23, rails INT32_MIN / INT32_MAX and v <= -2^23 / v >= 2^23 - 1.  Its sums of squares are formed in int64 pieces, which
2^62-sized squares overflow, so model() below sums the two 32-bit halves of every square apart and joins them as Python
integers."""
import numpy as np

import inputstats_model as im
import irdm
import siggen

FORMATS = (irdm.FMT_CI32, irdm.FMT_CI32_24)
NAMES = {irdm.FMT_CI32: "ci32", irdm.FMT_CI32_24: "ci32-24"}
I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1
# scene scale: x * SCALE[fmt] is the file's code.  Format 8: the converted stream is 8 x the scene, whose noise is then about
# 2^25 rms -- nearly every value needs more than 24 bits and (float)v rounds.  Format 9: 24-bit values, the converted stream
# 4 x the scene as in the int16 and cu8 tests.
SCALE = {irdm.FMT_CI32: 2.0 ** 34, irdm.FMT_CI32_24: 2.0 ** 25}
RANGE = {irdm.FMT_CI32: (I32_MIN, I32_MAX), irdm.FMT_CI32_24: (-2 ** 23, 2 ** 23 - 1)}

im.INT_FORMATS.update({irdm.FMT_CI32: (31, I32_MIN, I32_MAX), irdm.FMT_CI32_24: (23, -2 ** 23, 2 ** 23 - 1)})
im.NAMES.update(NAMES)
im.DTYPES.update({irdm.FMT_CI32: np.int32, irdm.FMT_CI32_24: np.int32})


def to_ci32(iq, fmt):
    """interleaved int32: clip(round(x * SCALE[fmt])) to the format's range"""
    x = np.empty(2 * len(iq), dtype=np.float64)
    x[0::2] = iq.real
    x[1::2] = iq.imag
    lo, hi = RANGE[fmt]
    return np.clip(np.round(x * SCALE[fmt]), lo, hi).astype(np.int32)


def converted(v, fmt):
    """interleaved int32 -> the cf32 stream a context in format fmt sees"""
    return irdm.convert_ci32(v, fmt)


def ci32_scene(fs, secs, nb, seed, fmt):
    n = int(secs * fs) // 32768 * 32768
    iq, _ = siggen.standard_scene(fs, n, nb, seed=seed)
    return to_ci32(iq, fmt)


def with_extremes(v):
    """INT32_MIN and INT32_MAX among the first samples of a format-8 stream (before the detector's history has filled)"""
    v = v.copy()
    v[10], v[11], v[12], v[13] = I32_MIN, I32_MAX, I32_MAX, I32_MIN
    return v


def model(x, fmt):
    """inputstats_model.model for the int32 formats, the sums as Python integers"""
    K, lo, hi = im.INT_FORMATS[fmt]
    n = len(x) // 2
    m = dict(n_samples=n, n_rail_lo=[0, 0], n_rail_hi=[0, 0], n_nonfinite=[0, 0], code_min=[0, 0], code_max=[0, 0],
             sum=[0.0, 0.0], sum_sq=[0.0, 0.0], abs_max=[np.float32(0), np.float32(0)])
    if n == 0:
        return m
    codes = np.asarray(x, np.int32).astype(np.int64)
    for k in range(2):
        v = codes[k::2]
        sq = v * v                                          # <= 2^62
        total_sq = (im._int_sum(sq >> 32) << 32) + im._int_sum(sq & 0xffffffff)
        m["n_rail_lo"][k] = int((v <= lo).sum())
        m["n_rail_hi"][k] = int((v >= hi).sum())
        m["code_min"][k], m["code_max"][k] = int(v.min()), int(v.max())
        m["sum"][k] = im._int_sum(v) / (1 << K)
        m["sum_sq"][k] = total_sq / (1 << (2 * K))
        m["abs_max"][k] = np.float32(int(np.abs(v).max()) / (1 << K))
    return m


def stats_input(fmt, n, seed):
    """n samples over the whole code range (format 9: somewhat past its rails), the first sample at the negative (I) and
    positive (Q) rail, the last the other way round"""
    rng = np.random.default_rng(seed)
    lo, hi = RANGE[fmt]
    if fmt == irdm.FMT_CI32_24:
        x = rng.integers(lo - 2 ** 20, hi + 2 ** 20, 2 * n).astype(np.int32)
    else:
        x = rng.integers(lo, hi, 2 * n, endpoint=True).astype(np.int32)
    if n:
        x[0], x[1] = lo, hi
        x[-2], x[-1] = hi, lo
    return x
