"""TEST INFRASTRUCTURE: receiver I/Q imbalance restated in numpy -- the correction of csrc/iq_balance.hpp in plain float32,
the moments of csrc/iq_moments.hpp in float64 with their derivation, the conversion of the eight device formats as the
pipeline's load stage does it, the impairment the tests plant, and the binary's rule for "this frame is an image"."""
import math

import numpy as np

import irdm

FORMATS = {irdm.FMT_CI8: (np.int8, 2), irdm.FMT_CU8: (np.uint8, 2), irdm.FMT_CI16: (np.int16, 4), irdm.FMT_CI16_FULL: (np.int16, 4),
           irdm.FMT_SC16Q11: (np.int16, 4), irdm.FMT_CF32: (np.float32, 8), irdm.FMT_CI32: (np.int32, 8),
           irdm.FMT_CI32_24: (np.int32, 8)}                 # format -> component type, bytes per sample
MAX_GAIN_DB, MAX_PHASE_DEG = 6.0, 30.0


def convert(raw, fmt):
    """raw: the bytes of a buffer of format fmt (any array; viewed as bytes).  Returns float32 [2 n], I and Q interleaved, as
    load_iq<fmt> (csrc/common.hpp) converts: every step exact, but (float)v of the int32 formats, which rounds to nearest even
    as astype(float32) does"""
    v = np.ascontiguousarray(raw).view(np.uint8).view(FORMATS[fmt][0])
    if fmt == irdm.FMT_CF32:
        return v.copy()
    if fmt == irdm.FMT_CI8:
        return v.astype(np.float32) / np.float32(128)
    if fmt == irdm.FMT_CU8:
        return (v.astype(np.float32) - np.float32(127.5)) / np.float32(128)
    if fmt == irdm.FMT_CI16:
        return (v >> 8).astype(np.float32) / np.float32(128)
    scale = {irdm.FMT_CI16_FULL: 2.0**-15, irdm.FMT_SC16Q11: 2.0**-11, irdm.FMT_CI32: 2.0**-31, irdm.FMT_CI32_24: 2.0**-23}[fmt]
    return v.astype(np.float32) * np.float32(scale)


def coeffs(gain_db, phase_deg):
    """alpha = -tan(phi), beta = 1 / (g cos(phi)), g = 10^(gain_db / 20): binary64 (the C library's functions), rounded once
    to float32; None outside the limits"""
    if not (abs(gain_db) <= MAX_GAIN_DB and abs(phase_deg) <= MAX_PHASE_DEG):
        return None
    g, phi = math.pow(10.0, gain_db / 20.0), phase_deg * (math.pi / 180.0)
    return np.float32(-math.tan(phi)), np.float32(1.0 / (g * math.cos(phi)))


def balance(x, alpha, beta):
    """x: float32 [2 n] interleaved (any bit patterns).  i' = i (its bits), q' = fl(fl(alpha i) + fl(beta q)) in float32"""
    x = np.ascontiguousarray(x, np.float32)
    y = x.copy()
    with np.errstate(all="ignore"):
        a = np.float32(alpha) * x[0::2]
        b = np.float32(beta) * x[1::2]
        y[1::2] = a + b
    return y


def impair(x, gain_db, phase_deg, dc=(0.003, -0.002)):
    """x: float32 [2 n] interleaved.  y_I = x_I + dc_I, y_Q = g (x_Q cos phi + x_I sin phi) + dc_Q, formed in float64 and
    rounded to float32"""
    g, phi = 10.0 ** (gain_db / 20.0), math.radians(phase_deg)
    c = np.asarray(x, np.float64).reshape(-1, 2)
    y = np.empty_like(c)
    y[:, 0] = c[:, 0] + dc[0]
    y[:, 1] = g * (c[:, 1] * math.cos(phi) + c[:, 0] * math.sin(phi)) + dc[1]
    return y.astype(np.float32).reshape(-1)


def image_level_db(gain_db, phase_deg):
    """20 log10(|1 - g e^{j phi}| / |1 + g e^{-j phi}|)"""
    g, phi = 10.0 ** (gain_db / 20.0), math.radians(phase_deg)
    return 20.0 * math.log10(abs(1 - g * complex(math.cos(phi), math.sin(phi))) / abs(1 + g * complex(math.cos(phi), -math.sin(phi))))


def derive(n_used, s):
    """s = (sum i, sum q, sum ii, sum qq, sum iq): (valid, gain_db, phase_deg, image_db) from the central moments"""
    if n_used < 2:
        return 0, 0.0, 0.0, 0.0
    N = float(n_used)
    mi, mq = s[0] / N, s[1] / N
    cii, cqq, ciq = s[2] / N - mi * mi, s[3] / N - mq * mq, s[4] / N - mi * mq
    if not (cii > 0.0 and cqq > 0.0):
        return 0, 0.0, 0.0, 0.0
    r = math.sqrt(cii * cqq)
    if not abs(ciq) < r:
        return 0, 0.0, 0.0, 0.0
    g, sp = math.sqrt(cqq / cii), ciq / r
    cp = math.sqrt(1.0 - sp * sp)
    num, den = math.hypot(1.0 - g * cp, g * sp), math.hypot(1.0 + g * cp, g * sp)
    img = 20.0 * math.log10(num / den) if num > 0.0 else -120.0
    return 1, 10.0 * math.log10(cqq / cii), math.degrees(math.asin(sp)), max(img, -120.0)


def moments(x):
    """x: float32 [2 n] interleaved.  The record of csrc/iq_moments.hpp in float64: a sample with a component that is not
    finite is left out; `abs` holds the sums of the terms' magnitudes, which bound the effect of the order of addition"""
    c = np.ascontiguousarray(x, np.float32).reshape(-1, 2)
    ok = np.isfinite(c).all(axis=1)
    d = c[ok].astype(np.float64)
    i, q = d[:, 0], d[:, 1]
    terms = (i, q, i * i, q * q, i * q)
    s = tuple(float(t.sum()) for t in terms)
    valid, gain_db, phase_deg, image_db = derive(len(d), s)
    return dict(n_samples=len(c), n_used=len(d), sums=s, abs=tuple(float(np.abs(t).sum()) for t in terms), valid=valid,
                gain_db=gain_db, phase_deg=phase_deg, image_db=image_db)


def count_images(frames, centre):
    """frames: (timestamp in ns, centre frequency in Hz, magnitude in dB, ok) per frame.  A frame j with ok is an image when
    some frame i with ok lies within 1 ms of it, mirrors it about `centre` within 500 Hz and is at least 10 dB stronger.
    Returns (images, frames with ok)."""
    ok = [f for f in frames if f[3]]
    images = 0
    for tj, fj, mj, _ in ok:
        images += any(abs(int(ti) - int(tj)) <= 1_000_000 and abs(fi + fj - 2.0 * centre) <= 500.0 and mj <= mi - 10.0
                      for ti, fi, mi, _ in ok)
    return images, len(ok)


def frames_of(demods):
    return [(int(d.timestamp), float(d.center_frequency), float(d.magnitude), int(d.ok)) for d in demods]


def image_line(m, images, n_ok, balanced=False):
    """the binary's closing line for the moments m (a dict as moments() returns, or an irdm.IqMoments)"""
    get = (lambda k: m[k]) if isinstance(m, dict) else (lambda k: getattr(m, k))
    if not get("n_samples"):
        return "image: 0 samples; nothing to judge"
    if not get("valid"):
        return "image: %d samples; no variance in I or Q; nothing to judge" % get("n_samples")
    level = "image at %.1f dB" % get("image_db") if get("image_db") >= -60.0 else "image below -60 dB"
    line = "image: %d samples; Q/I gain %+.3f dB, phase %+.2f deg: %s; %d of %d frames are images" % (
        get("n_samples"), get("gain_db"), get("phase_deg"), level, images, n_ok)
    if get("image_db") >= -40.0 or images:
        line += " of a stronger frame -- receiver I/Q imbalance: "
        line += ("with --iq-balance in effect: adjust it" if balanced else
                 "run with --iq-balance=%.3f,%.2f" % (get("gain_db"), get("phase_deg")))
    return line
