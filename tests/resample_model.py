"""TEST INFRASTRUCTURE: loader of tests/resample_model.c (the arithmetic contract of the front end's rational mode in plain
C), the float64 evaluation of the same formula, the prototype's design from the oracle's restatement, the ctypes driver of
irdm_frontend_create_rational that the resampling tests share, and their signal scenes."""
import ctypes as C
import math
import os
import subprocess

import numpy as np

import frontend_model as fm
import irdm

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "resample_model.c")
# (in_rate, out_rate) of the tested ratios and their L / M
PAIRS = {(5, 28): (56_000_000, 10_000_000), (25, 24): (2_400_000, 2_500_000), (5, 6): (2_400_000, 2_000_000),
         (25, 64): (30_720_000, 12_000_000), (25, 128): (61_440_000, 12_000_000), (125, 128): (12_288_000, 12_000_000),
         (125, 768): (61_440_000, 10_000_000)}
# every pair the README names (capture rate, resampled rate)
NAMED = [(61_440_000, 12_000_000), (61_440_000, 10_000_000), (30_720_000, 12_000_000), (56_000_000, 10_000_000),
         (12_288_000, 12_000_000), (2_048_000, 2_000_000), (2_560_000, 2_500_000), (2_400_000, 2_500_000),
         (2_400_000, 2_000_000), (11_200_000, 10_000_000)]
# what irdm_frontend_create_rational refuses: (name, (in_rate, format, out_rate[, shift_hz]), the message on stderr); each
# trips exactly one check (100/801 has L <= 125, 10 MS/s at 8.01 is inside the M / L range)
REFUSALS = (("L", (2_048_000, 0, 2_032_000), "ratio 127/128; L <= 125 and M <= 768"),
            ("M", (8_010_000, 0, 1_000_000), "ratio 100/801; L <= 125 and M <= 768"),
            ("ratio_hi", (34_000_000, 0, 2_000_000), "(ratio 1/17): M / L must lie in 24/25 .. 16"),
            ("ratio_lo", (2_000_000, 0, 2_500_000), "(ratio 5/4): M / L must lie in 24/25 .. 16"),
            ("same", (2_000_000, 0, 2_000_000), "(ratio 1/1): M / L must lie in 24/25 .. 16"),
            ("out_rate", (56_000_000, 0, 25_000_000), "output rate 25000000 (56000000 * 25 / 56) is not one the pipeline takes"),
            ("out_rate_integer", (61_440_000, 0, 30_720_000), "output rate 30720000 (61440000 / 2) is not one the pipeline takes"),
            ("format", (2_400_000, 7, 2_500_000), "unknown sample format 7"),
            ("shift", (2_400_000, 0, 2_500_000, 1.3e6), "shift 1300000.0 Hz is beyond half the capture rate 2400000"))
_lib = None


def ratio(in_rate, out_rate):
    g = math.gcd(in_rate, out_rate)
    return out_rate // g, in_rate // g


def lib():
    global _lib
    if _lib is None:
        fma = fm._cpu_has_fma()
        so = os.path.join(HERE, "_build", "resample_model_fma.so" if fma else "resample_model.so")
        if not os.path.exists(so) or os.path.getmtime(so) < os.path.getmtime(SRC):
            os.makedirs(os.path.dirname(so), exist_ok=True)
            subprocess.check_call(["gcc", "-O2", "-std=gnu99", "-fPIC", "-shared", "-ffp-contract=off", "-fopenmp"] +
                                  (["-mfma"] if fma else []) + ["-o", so, SRC, "-lm"])
        L = C.CDLL(so)
        L.rs_model_run.restype = C.c_longlong
        L.rs_model_run.argtypes = [C.c_int, C.c_void_p, C.c_longlong, C.c_int, C.c_int, C.c_longlong, C.POINTER(C.c_float),
                                   C.c_int, C.POINTER(C.c_float)]
        _lib = L
    return _lib


def n_outputs(n, L, M):
    return (n * L + M - 1) // M


def run(x, fmt, L, M, q, taps):
    """the model on a whole stream: complex64 [ceil(n L / M)]"""
    x = np.ascontiguousarray(x)
    n = fm.n_samples(x, fmt)
    p = np.ascontiguousarray(taps, np.float32)
    out = np.empty(2 * n_outputs(n, L, M), np.float32)
    got = lib().rs_model_run(fmt, x.ctypes.data_as(C.c_void_p), n, L, M, q, fm._fp(p), len(p), fm._fp(out))
    assert got == len(out) // 2, got
    return out.view(np.complex64)


def run_float64(x, fmt, L, M, q, taps):
    """the same formula in float64 on the same float taps and the same float table: y[m] = (P * upsampled r)[m M + C]"""
    xf = fm.to_float(x, fmt)
    n = len(xf)
    T = fm.table().astype(np.complex128)
    idx = ((q % 65536) * (np.arange(n, dtype=np.int64) % 65536)) % 65536
    r = xf * T[idx]
    p = np.asarray(taps, np.float32).astype(np.float64)
    c = (len(p) - 1) // 2
    up = np.zeros(n * L, np.complex128)
    up[::L] = r
    from numpy.fft import fft, ifft
    nfft = 1 << int(np.ceil(np.log2(len(up) + len(p))))
    full = ifft(fft(up, nfft) * fft(p, nfft))[:len(up) + len(p) - 1]
    m = np.arange(n_outputs(n, L, M))
    return full[m * M + c]


def phase_tap_sums(taps, L, M):
    """per phase r = m mod L: (taps of the branch, sum of their magnitudes)"""
    p = np.asarray(taps, np.float32).astype(np.float64)
    c = (len(p) - 1) // 2
    out = []
    for r in range(L):
        b = (r * M + c) % L
        br = p[b::L]
        out.append((len(br), float(np.abs(br).sum())))
    return out


def design_taps(in_rate, out_rate):
    """the prototype from the oracle's restatement of the same design: what irdm_frontend_taps returns for the rational
    mode (asserted where a library front end exists).  The rate L * in_rate must be exact as a float (asserted)."""
    import orc
    lo = orc.lib()
    lo.orc_lpf_taps.restype = C.c_int
    lo.orc_lpf_taps.argtypes = [C.POINTER(C.c_float), C.c_int, C.c_float, C.c_float, C.c_float, C.c_float]
    L, M = ratio(in_rate, out_rate)
    rate = L * in_rate
    assert int(np.float32(rate)) == rate, rate
    f_min = np.float32(min(in_rate, out_rate))
    out = np.zeros(65536, np.float32)
    n = lo.orc_lpf_taps(fm._fp(out), len(out), float(L), float(np.float32(rate)), float(np.float32(0.5) * f_min),
                        float(np.float32(0.09) * f_min))
    assert 0 < n <= len(out) and n % 2 == 1
    return out[:n].copy()


def response(taps, L, M, nfft=1 << 21):
    """of the prototype at the rate L in_rate, in units of f_min = min(in, out) = that rate / max(L, M): pass-band ripple
    (dB, peak deviation from the gain L up to 0.42 f_min) and the least attenuation (dB below the gain L) from 0.58 f_min
    to half the rate"""
    H = np.abs(np.fft.rfft(np.asarray(taps, np.float32).astype(np.float64), nfft)) / L
    f = np.arange(len(H)) / nfft * max(L, M)
    mag_db = 20.0 * np.log10(np.maximum(H, 1e-300))
    return dict(ripple_db=float(np.abs(mag_db[f <= 0.42]).max()), atten_db=float(-mag_db[f >= 0.58].max()))


class Stage:
    """irdm_frontend_run_device / _finish_device of a rational front end on device buffers the library allocates"""

    def __init__(self, in_rate, fmt, out_rate, shift_hz=0.0, device=0):
        self.fe = irdm.Frontend.rational(in_rate, fmt, out_rate, shift_hz, device)
        self.fmt, self.device = fmt, device
        self.L, self.M = self.fe.ratio

    def run(self, x, feeds):
        """x cut into feeds (sample counts; their sum = the stream); returns every output, flush included"""
        lib_ = irdm.lib()
        n = fm.n_samples(x, self.fmt)
        assert sum(feeds) == n
        cap = max(feeds) * self.L // self.M + self.fe.ntaps // self.M + 8
        d_out = lib_.irdm_device_alloc(self.device, cap * 8)
        host = np.empty(cap, np.complex64)
        parts, pos = [], 0

        def take(k):
            if k < 0:
                raise RuntimeError("front end failed")
            if k:
                irdm.device_download(host[:k], d_out)
                parts.append(host[:k].copy())
        try:
            for f in feeds:
                part = np.ascontiguousarray(fm._slice(x, self.fmt, pos, pos + f))
                d_in = irdm.device_buffer(part if len(part) else np.zeros(2, part.dtype), self.device)
                try:
                    take(lib_.irdm_frontend_run_device(self.fe.h, C.c_void_p(d_in), f, C.c_void_p(d_out), cap, None))
                finally:
                    irdm.device_free(d_in)
                pos += f
            take(lib_.irdm_frontend_finish_device(self.fe.h, C.c_void_p(d_out), cap, None))
        finally:
            lib_.irdm_device_free(d_out)
        return np.concatenate(parts) if parts else np.empty(0, np.complex64)

    def reset(self):
        self.fe.reset()

    def close(self):
        self.fe.close()


def ragged_feeds(n, ntaps, L, extra=(9973,)):
    """n samples in feeds of 1, one less than the taps of a phase, a prime, ... in turn"""
    return fm.ragged_feeds(n, max(2, -(-ntaps // L)), extra)


def run_composed(x, in_rate, fmt, out_rate, shift_hz, feeds, depth, max_chunk, feed="host", center=1622000000.0):
    """The capture through a rational front end's irdm_frontend_feed_* + flush into a cf32 pipeline at out_rate; returns
    (the record queues in the shape parity.run_gpu returns them, the applied shift)."""
    fe = irdm.Frontend.rational(in_rate, fmt, out_rate, shift_hz)
    p = irdm.Pipeline(fe.out_rate, fmt=irdm.FMT_CF32, center_frequency=center + fe.applied_shift_hz,
                      max_chunk_samples=max_chunk, max_bursts_per_chunk=1024, pipeline_depth=depth)
    try:
        p.set_option("keep_frame_samples", 1)
        pos = 0
        for f in feeds:
            part = np.ascontiguousarray(fm._slice(x, fmt, pos, pos + f))
            if feed == "host":
                fe.feed_host(p, part)
            else:
                d_in = irdm.device_buffer(part if len(part) else np.zeros(2, part.dtype))
                try:
                    fe.feed_device(p, d_in, f)
                    fe.wait_input()
                finally:
                    irdm.device_free(d_in)
            pos += f
        assert pos == fm.n_samples(x, fmt)
        fe.flush(p)
        bursts = p.poll_bursts()
        infos, samples = p.poll_frames()
        demods = p.poll_demods()
        return dict(bursts=bursts, infos=infos, samples=samples, demods=demods, packed=[], tagged=p.tagged,
                    n_samples=p.sample_count), fe.applied_shift_hz
    finally:
        p.close()
        fe.close()


# ---- the signal scenes: a capture at a rate off the 250 kHz grid, bursts spaced in time, all within 0.40 f_min of the centre ----
SCENES = {
    "11.2->10": dict(in_rate=11_200_000, out_rate=10_000_000, secs=0.72, seed=112, channels=(-90, -60, -31, -7, 22, 48, 75, 95)),
    "2.4->2.5": dict(in_rate=2_400_000, out_rate=2_500_000, secs=1.0, seed=24, channels=(-22, -15, -9, -3, 4, 10, 16, 22)),
}


def offgrid_scene(name, fmt=irdm.FMT_CF32):
    """(capture at in_rate, expected hard bits per burst in time order).  The symbols run at 25 ksym/s in capture time
    (the capture rates are multiples of 25 kHz), so the pipeline fed at in_rate sees a symbol clock off by
    in_rate / round(in_rate / 250000) / 250000 - 1, and after resampling an exact one."""
    import siggen
    s = SCENES[name]
    fs = s["in_rate"]
    f_min = min(s["in_rate"], s["out_rate"])
    n = int(s["secs"] * fs) // 32768 * 32768
    rng = np.random.default_rng(s["seed"])
    bursts, expect = [], []
    k_n = len(s["channels"])
    for k, ch in enumerate(s["channels"]):
        f = siggen.channel_freq(ch)
        assert abs(f) <= 0.40 * f_min, (name, ch)
        payload = list(rng.integers(0, 4, 150))
        start = int((0.42 + (s["secs"] - 0.47) * k / k_n) * fs)
        bursts.append(dict(start=start, freq_hz=f, payload=payload, amp=0.05))
        expect.append(siggen.quadrants_to_bits(siggen.frame_quadrants(payload)[16:]))
    iq, _ = siggen.make_stream(fs, n, bursts, seed=s["seed"])
    if fmt == irdm.FMT_CI8:
        return siggen.to_ci8(iq), expect
    return iq, expect


def whole_payloads(demods, expect):
    """how many of the expected payloads some frame carries whole (as its leading hard bits)"""
    found = 0
    for e in expect:
        for d in demods:
            if d.n_bits >= len(e) and [int(b) for b in d.bits[:len(e)]] == e:
                found += 1
                break
    return found


def make_burst_fractional(fs, quads, freq_hz, phase, amp=0.05, alpha=0.4, span=5):
    """siggen.make_burst for a rate that is no multiple of 25 kHz: the root-raised-cosine pulse evaluated at the fractional
    sample instants t = n / fs - k / 25000 (float64)."""
    import siggen
    sps = fs / siggen.SYMBOL_RATE
    sym = np.exp(1j * (np.pi / 4 + np.asarray(quads, dtype=np.float64) * np.pi / 2))
    nsym = len(sym)
    n_tot = int(np.ceil((nsym + 2 * span - 1) * sps)) + 1
    sig = np.zeros(n_tot, np.complex128)
    # the unit-energy normalisation of the integer pulse at the nearest integer sps, scaled like siggen's
    ref = siggen.rrc_pulse(int(round(sps)), alpha, span) / np.sqrt(int(round(sps)))
    peak = ref.max()

    def rrc(t):
        t = np.asarray(t, np.float64)
        out = np.empty_like(t)
        with np.errstate(divide="ignore", invalid="ignore"):
            out = (np.sin(np.pi * t * (1 - alpha)) + 4 * alpha * t * np.cos(np.pi * t * (1 + alpha))) / \
                  (np.pi * t * (1 - (4 * alpha * t) ** 2))
        out[np.abs(t) < 1e-9] = 1.0 - alpha + 4 * alpha / np.pi
        sing = np.abs(np.abs(t) - 1 / (4 * alpha)) < 1e-7
        out[sing] = alpha / np.sqrt(2) * ((1 + 2 / np.pi) * np.sin(np.pi / (4 * alpha)) + (1 - 2 / np.pi) * np.cos(np.pi / (4 * alpha)))
        return out
    scale = peak / (1.0 - alpha + 4 * alpha / np.pi)
    for k in range(nsym):
        centre = (k + span) * sps
        lo, hi = max(0, int(np.ceil(centre - span * sps))), min(n_tot - 1, int(np.floor(centre + span * sps)))
        idx = np.arange(lo, hi + 1)
        sig[idx] += sym[k] * scale * rrc((idx - centre) / sps)
    n = np.arange(n_tot, dtype=np.float64)
    return (amp * sig * np.exp(1j * (2 * np.pi * freq_hz / fs * n + phase))).astype(np.complex64)
