"""TEST INFRASTRUCTURE: loader of tests/frontend_model.c (the band-select front end's arithmetic contract in plain C), the
float64 evaluation of the same formula, and the ctypes driver of irdm_frontend_* that the front-end tests share."""
import ctypes as C
import os
import subprocess

import numpy as np

import irdm

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "frontend_model.c")
D_LIST = (2, 3, 4, 5, 6, 8, 16)
FORMATS = (irdm.FMT_CI8, irdm.FMT_CI16, irdm.FMT_CF32, irdm.FMT_CI16_FULL, irdm.FMT_SC16Q11)
NAMES = {irdm.FMT_CI8: "ci8", irdm.FMT_CI16: "ci16", irdm.FMT_CF32: "cf32", irdm.FMT_CI16_FULL: "ci16-full",
         irdm.FMT_SC16Q11: "sc16q11"}
_lib = None


def _cpu_has_fma():
    try:
        return " fma " in open("/proc/cpuinfo").read()
    except OSError:
        return False


def lib():
    """the model, built with -ffp-contract=off (fmaf where the source says fmaf, nowhere else).  With FMA hardware the
    calls are inlined (-mfma: the same correctly rounded operation, a hundred times faster than the libm call)."""
    global _lib
    if _lib is None:
        fma = _cpu_has_fma()
        so = os.path.join(HERE, "_build", "frontend_model_fma.so" if fma else "frontend_model.so")
        if not os.path.exists(so) or os.path.getmtime(so) < os.path.getmtime(SRC):
            os.makedirs(os.path.dirname(so), exist_ok=True)
            subprocess.check_call(["gcc", "-O2", "-std=gnu99", "-fPIC", "-shared", "-ffp-contract=off", "-fopenmp"] +
                                  (["-mfma"] if fma else []) + ["-o", so, SRC, "-lm"])
        L = C.CDLL(so)
        L.fe_model_run.restype = C.c_longlong
        L.fe_model_run.argtypes = [C.c_int, C.c_void_p, C.c_longlong, C.c_int, C.c_longlong, C.POINTER(C.c_float), C.c_int,
                                   C.POINTER(C.c_float), C.POINTER(C.c_float)]
        L.fe_model_table.argtypes = [C.POINTER(C.c_float)]
        _lib = L
    return _lib


def _fp(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def n_samples(x, fmt):
    return len(x) if fmt == irdm.FMT_CF32 else len(x) // 2


def table():
    t = np.empty(2 * 65536, np.float32)
    lib().fe_model_table(_fp(t))
    return t.view(np.complex64)


def quantise(shift_hz, fs_in):
    return int(np.round(shift_hz * 65536.0 / fs_in))


def run(x, fmt, D, q, taps, want_rot=False):
    """the model on a whole stream: complex64 [ceil(n / D)] (and r[n] with want_rot)"""
    x = np.ascontiguousarray(x)
    n = n_samples(x, fmt)
    h = np.ascontiguousarray(taps, np.float32)
    out = np.empty(2 * ((n + D - 1) // D), np.float32)
    rot = np.empty(2 * n, np.float32) if want_rot else None
    got = lib().fe_model_run(fmt, x.ctypes.data_as(C.c_void_p), n, D, q, _fp(h), len(h), _fp(out), _fp(rot) if want_rot else None)
    assert got == len(out) // 2, got
    y = out.view(np.complex64)
    return (y, rot.view(np.complex64)) if want_rot else y


def to_float(x, fmt):
    """the capture as complex128, converted as the load stage converts it (every conversion is exact in float)"""
    if fmt == irdm.FMT_CF32:
        return np.asarray(x, np.complex64).astype(np.complex128)
    v = np.asarray(x, np.int8 if fmt == irdm.FMT_CI8 else np.int16).astype(np.float64)
    if fmt == irdm.FMT_CI8:
        v = v / 128.0
    elif fmt == irdm.FMT_CI16:
        v = np.floor(v / 256.0) / 128.0
    else:
        v = v * irdm.FMT_SCALE[fmt]
    return v[0::2] + 1j * v[1::2]


def run_float64(x, fmt, D, q, taps):
    """the same formula in float64 on the same float taps and the same float table"""
    xf = to_float(x, fmt)
    n = len(xf)
    T = table().astype(np.complex128)
    idx = ((q % 65536) * (np.arange(n, dtype=np.int64) % 65536)) % 65536
    r = xf * T[idx]
    h = np.asarray(taps, np.float32).astype(np.float64)
    c = (len(h) - 1) // 2
    full = np.convolve(r, h)                 # full[i] = sum_k h[k] r[i - k]
    m = np.arange((n + D - 1) // D)
    return full[m * D + c]


def random_capture(fmt, n, seed):
    rng = np.random.default_rng(seed)
    if fmt == irdm.FMT_CF32:
        return (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(np.complex64) * np.float32(0.25)
    if fmt == irdm.FMT_CI8:
        return rng.integers(-128, 128, 2 * n, dtype=np.int8)
    hi = 2048 if fmt == irdm.FMT_SC16Q11 else 32768
    return rng.integers(-hi, hi, 2 * n, dtype=np.int16)


# ---- the library's front end (irdm_frontend_*), GPU or emulated: whichever build irdm.lib() loads ----
def _slice(x, fmt, a, b):
    return x[a:b] if fmt == irdm.FMT_CF32 else x[2 * a:2 * b]


class Stage:
    """irdm_frontend_run_device / _finish_device on device buffers the library allocates"""

    def __init__(self, fs_in, fmt, D, shift_hz=0.0, device=0):
        self.fe = irdm.Frontend(fs_in, fmt, D, shift_hz, device)
        self.fmt, self.D, self.device = fmt, D, device

    def run(self, x, feeds):
        """x cut into feeds (sample counts; their sum = the stream); returns every output, flush included"""
        L = irdm.lib()
        n = n_samples(x, self.fmt)
        assert sum(feeds) == n
        cap = max(max(feeds) // self.D + 2, (self.fe.ntaps // self.D) + 4)
        d_out = L.irdm_device_alloc(self.device, cap * 8)
        host = np.empty(cap, np.complex64)
        parts, pos = [], 0

        def take(k):
            if k < 0:
                raise RuntimeError("front end failed")
            if k:
                # (device memory is host memory under the emulation; on the GPU the copy back goes through torch-free ctypes)
                irdm.device_download(host[:k], d_out)
                parts.append(host[:k].copy())
        try:
            for f in feeds:
                part = np.ascontiguousarray(_slice(x, self.fmt, pos, pos + f))
                d_in = irdm.device_buffer(part if len(part) else np.zeros(2, part.dtype), self.device)
                try:
                    take(L.irdm_frontend_run_device(self.fe.h, C.c_void_p(d_in), f, C.c_void_p(d_out), cap, None))
                finally:
                    irdm.device_free(d_in)
                pos += f
            take(L.irdm_frontend_finish_device(self.fe.h, C.c_void_p(d_out), cap, None))
        finally:
            L.irdm_device_free(d_out)
        return np.concatenate(parts) if parts else np.empty(0, np.complex64)

    def close(self):
        self.fe.close()


def same_bits(a, b):
    a = np.ascontiguousarray(a, np.complex64).view(np.uint32)
    b = np.ascontiguousarray(b, np.complex64).view(np.uint32)
    return a.shape == b.shape and bool(np.array_equal(a, b))


def run_composed(x, fs_in, fmt, D, shift_hz, feeds, depth, max_chunk, feed="host", center=1622000000.0):
    """The capture through irdm_frontend_feed_* + flush into a cf32 pipeline at fs_in / D; returns (the record queues in
    the shape parity.run_gpu returns them, the applied shift)."""
    fe = irdm.Frontend(fs_in, fmt, D, shift_hz)
    p = irdm.Pipeline(fe.out_rate, fmt=irdm.FMT_CF32, center_frequency=center + fe.applied_shift_hz,
                      max_chunk_samples=max_chunk, max_bursts_per_chunk=1024, pipeline_depth=depth)
    try:
        p.set_option("keep_frame_samples", 1)
        pos = 0
        for f in feeds:
            part = np.ascontiguousarray(_slice(x, fmt, pos, pos + f))
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
        assert pos == n_samples(x, fmt)
        fe.flush(p)
        bursts = p.poll_bursts()
        infos, samples = p.poll_frames()
        demods = p.poll_demods()
        return dict(bursts=bursts, infos=infos, samples=samples, demods=demods, packed=[], tagged=p.tagged,
                    n_samples=p.sample_count), fe.applied_shift_hz
    finally:
        p.close()
        fe.close()


def ragged_feeds(n, ntaps, extra=(9973,)):
    """n samples in feeds of 1, ntaps - 1, a prime, ... in turn"""
    sizes, out, k = (1, ntaps - 1) + tuple(extra), [], 0
    while n > 0:
        f = min(n, sizes[k % len(sizes)])
        out.append(f)
        n -= f
        k += 1
    return out


def block_feeds(n, block):
    return [block] * (n // block) + ([n % block] if n % block else [])


def response(taps, D, nfft=1 << 18):
    """pass-band ripple (dB, peak deviation from unity over |f| <= 0.42 fs_out) and stop-band attenuation (dB, the least over
    0.58 fs_out <= |f| <= fs_in / 2) of real taps at decimation D"""
    H = np.abs(np.fft.rfft(np.asarray(taps, np.float32).astype(np.float64), nfft))
    f = np.arange(len(H)) / nfft * D                 # in units of fs_out
    mag_db = 20.0 * np.log10(np.maximum(H, 1e-300))
    return dict(ripple_db=float(np.abs(mag_db[f <= 0.42]).max()), atten_db=float(-mag_db[f >= 0.58].max()))


# ---- the signal scene of the wideband tests: a 50 MHz capture, the band 11 MHz above its centre, D = 5 ----
SCENE = dict(fs_in=50_000_000, D=5, shift_hz=11_000_000.0, secs=0.75, seed=50, n_inband=6,
             inband_channels=(-90, -55, -20, 15, 50, 85),          # +-3.75 MHz: inside 0.42 fs_out of the band centre
             outband_hz=(6.5e6, -7.0e6, 8.2e6))                    # 0.65 / 0.70 / 0.82 fs_out from the band centre

# ... and two whose output rate is not 10 MHz (optional keys: fmt, default ci8; start0 / step, the first in-band burst's
# start and the spacing in seconds, default 0.45 / 0.045 -- the first burst lies behind the 530 priming frames AT THE OUTPUT
# RATE: 0.424 s at 10.24 MHz, 0.695 s at 12.5 MHz).  In-band channels within 0.42 fs_out of the band centre, the strong
# out-of-band carriers 0.65 / 0.70 / 0.82 fs_out from it.
SCENE_61M44_D6 = dict(fs_in=61_440_000, D=6, shift_hz=9_000_000.0, secs=0.70, seed=61, n_inband=7, fmt=irdm.FMT_CI16,
                      start0=0.44, step=0.035,
                      inband_channels=(-100, -65, -30, 5, 40, 75, 100),       # +-4.17 MHz of 4.30 MHz
                      outband_hz=(6.656e6, -7.168e6, 8.397e6))
SCENE_50M_D4 = dict(fs_in=50_000_000, D=4, shift_hz=-8_000_000.0, secs=0.98, seed=54, n_inband=6, fmt=irdm.FMT_CI8,
                    start0=0.71, step=0.04,
                    inband_channels=(-120, -75, -30, 15, 60, 120),            # +-5.0 MHz of 5.25 MHz
                    outband_hz=(8.125e6, -8.75e6, 10.25e6))


def wideband_scene(scene=None):
    """(capture in the scene's format, expected hard bits per in-band burst in time order, q).  Every strong out-of-band
    burst lies on top of an in-band one in time and would alias into the band without the filter.  Without a scene:
    SCENE, the same bytes as ever (tests/test_frontend_emul.py pins their digest)."""
    import siggen
    s = SCENE if scene is None else scene
    fs = s["fs_in"]
    n = int(s["secs"] * fs) // 32768 * 32768
    q = quantise(s["shift_hz"], fs)
    applied = q * fs / 65536.0
    rng = np.random.default_rng(s["seed"])
    start0, step = s.get("start0", 0.45), s.get("step", 0.045)
    bursts, expect = [], []
    for k, ch in enumerate(s["inband_channels"]):
        payload = list(rng.integers(0, 4, 150))
        start = int((start0 + step * k) * fs)
        bursts.append(dict(start=start, freq_hz=applied + siggen.channel_freq(ch), payload=payload, amp=0.05))
        expect.append(siggen.quadrants_to_bits(siggen.frame_quadrants(payload)[16:]))
    for k, off in enumerate(s["outband_hz"]):
        bursts.append(dict(start=bursts[2 * k]["start"] + 5000, freq_hz=applied + off + 1234.0,
                           payload=list(rng.integers(0, 4, 150)), amp=0.2))
    iq, _ = siggen.make_stream(fs, n, bursts, seed=s["seed"])
    fmt = s.get("fmt", irdm.FMT_CI8)
    assert fmt in (irdm.FMT_CI8, irdm.FMT_CI16)
    return (siggen.to_ci8(iq) if fmt == irdm.FMT_CI8 else siggen.to_ci16(iq)), expect, q


def check_scene_demods(demods, expect):
    """every in-band payload, in time order, as the hard bits of exactly one frame; nothing else"""
    assert len(demods) == len(expect), (len(demods), len(expect))
    for d, e in zip(sorted(demods, key=lambda d: d.timestamp), expect):
        got = [int(b) for b in d.bits[:d.n_bits]]
        assert d.n_bits >= len(e), (d.n_bits, len(e))
        assert got[:len(e)] == e


def design_taps(fs_in, D):
    """the front end's taps from the oracle's restatement of the same design (fir_filter.c:143-182): what
    irdm_frontend_taps returns (asserted where a library front end exists)"""
    import orc
    L = orc.lib()
    L.orc_lpf_taps.restype = C.c_int
    L.orc_lpf_taps.argtypes = [C.POINTER(C.c_float), C.c_int, C.c_float, C.c_float, C.c_float, C.c_float]
    out = np.zeros(1024, np.float32)
    fs_out = fs_in // D
    n = L.orc_lpf_taps(_fp(out), 1024, 1.0, float(fs_in), 0.5 * fs_out, 0.09 * fs_out)
    assert 0 < n <= 1024
    return out[:n].copy()
