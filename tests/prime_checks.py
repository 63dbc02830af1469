"""TEST INFRASTRUCTURE: the checks of irdm_prime_host / irdm_prime_device (csrc/feed.cpp) that the GPU test
(tests/test_gpu_prime.py) and the CPU-emulation test (tests/prime_emul_run.py) share.  The reference of every comparison is
the CPU oracle run over P||x with start time T0': P the 512-frame prefix tiled from the recording's own head, built here in
numpy from the contract's text, never by the library."""
import ctypes as C
import functools

import numpy as np

import irdm
import orc
import parity
import siggen

FS = 2_000_000
T0 = 1700000000 * 10**9
CHUNK = 262_144
HISTORY = 512


def fft_size(fs):
    return 1 << int(round(np.log2(fs / 1000.0)))


def cf32_floats(iq):
    return np.ascontiguousarray(iq).view(np.float32).reshape(-1)


def per(fmt):
    """array elements per sample"""
    return 1 if fmt == irdm.FMT_CF32 else 2


def prefix(x, fs, fmt=irdm.FMT_CF32):
    """(P, F): frame k of P is frame k mod F of x, k = 0 .. 511, F = min(512, whole frames of x)"""
    N = fft_size(fs) * per(fmt)
    F = min(HISTORY, len(x) // N)
    assert F >= 1
    frames = np.asarray(x[:F * N]).reshape(F, N)
    return np.ascontiguousarray(frames[np.arange(HISTORY) % F].reshape(-1)), F


def shifted_origin(fs, t0=T0):
    """T0' = T0 - floor(H 10^9 / rate)"""
    return t0 - HISTORY * fft_size(fs) * 10**9 // fs


def oracle_primed(x, fs, fmt=irdm.FMT_CF32, **kw):
    """the oracle over P || x with start time T0'"""
    P, _ = prefix(x, fs, fmt)
    return orc.run_stream(np.concatenate([P, x]), fs, fmt=fmt, start_time_ns=shifted_origin(fs), **kw)


@functools.lru_cache(maxsize=None)
def scene(name):
    """"full": siggen.standard_scene(2 MHz, 3 000 000 samples, 16 bursts, seed 3, first_start=40 000) -- 6 of its bursts
    start inside the first 512 frames; "excerpt": 700 000 samples of it (341 frames) from 100 000 samples before its first
    burst, with 6 bursts.  (samples, the oracle's records over P || x, the oracle's over x alone)"""
    iq, truth = siggen.standard_scene(FS, 3_000_000, 16, 3, first_start=40_000)
    if name == "excerpt":
        a = min(t["start"] for t in truth) - 100_000
        iq = np.ascontiguousarray(iq[a:a + 700_000])
    iq.setflags(write=False)
    return iq, oracle_primed(iq, FS), orc.run_stream(iq, FS)


def chunks_of(n, chunk):
    return [chunk] * (n // chunk) + ([n % chunk] if n % chunk else [])


def collect(p, depth, packed=False):
    if depth:
        p.flush()
    bursts = p.poll_bursts()
    infos, samples = p.poll_frames()
    return dict(bursts=bursts, infos=infos, samples=samples, demods=p.poll_demods(),
                packed=p.poll_demods_packed() if packed else [], tagged=p.tagged, n_samples=p.sample_count)


def feed(p, x, fmt, chunk):
    parity.feed_chunks(p, x, fmt, chunks_of(len(x) // per(fmt), chunk))


def prime(p, x, fs, fmt, how="host"):
    """prime p from the head of x (at most 512 frames of it are handed over) and check the getters"""
    H = HISTORY * fft_size(fs)
    head = np.ascontiguousarray(x[:H * per(fmt)])
    F = min(HISTORY, len(head) // per(fmt) // fft_size(fs))
    t0 = p.start_time_ns
    assert (p.primed_samples, p.primed_frames) == (0, 0)
    if how == "host":
        assert p.prime_host(head) == F
    else:
        d = irdm.device_buffer(head)
        try:
            assert p.prime_device(d, len(head) // per(fmt)) == F
        finally:
            irdm.device_free(d)
    assert (p.primed_samples, p.primed_frames, p.start_time_ns, p.sample_count) == (H, F, t0 - H * 10**9 // fs, H)
    return H, F


def run_primed(x, fs, fmt=irdm.FMT_CF32, depth=0, max_chunk=CHUNK, chunk=None, options=(), how="host", before=None, after=None,
               packed=False):
    """a context primed from x's head, then fed x in chunks of `chunk` samples (default: max_chunk, or 1 Mi samples when
    max_chunk is the library's default 0); the record queues in the shape parity.compare takes"""
    p = irdm.Pipeline(fs, fmt=fmt, max_chunk_samples=max_chunk, max_bursts_per_chunk=1024, pipeline_depth=depth, start_time_ns=T0)
    try:
        p.set_option("packed_records" if packed else "keep_frame_samples", 1)
        for k, v in options:
            p.set_option(k, v)
        if before:
            before(p)
        H, F = prime(p, x, fs, fmt, how)
        feed(p, x, fmt, chunk or max_chunk or (1 << 20))
        out = collect(p, depth, packed)
        assert out["n_samples"] == H + len(x) // per(fmt)
        if after:
            after(p, out)
        return out
    finally:
        p.close()


def records_bytes(out):
    return (b"".join(bytes(b) for b in out["bursts"]), b"".join(bytes(f) for f in out["infos"]), b"".join(bytes(d) for d in out["demods"]),
            b"".join(np.ascontiguousarray(s).tobytes() for s in out["samples"]), b"".join(bytes(q) for q in out["packed"]))


def good_frames(ref):
    return sum(1 for d in ref.demods if d.ok)


def scene_case(name, depth):
    """A primed context fed the scene equals the oracle over P || x in every field parity.compare compares; the oracle
    finds 16 bursts / 16 ok frames ("full") or 6 / 6 ("excerpt") there and 10 / 10 or 0 / 0 in x alone.  irdm_prime_host
    after the feeds returns -1 and changes nothing.  After irdm_reset the stream is unprimed, irdm_prime_host after its
    first feed returns -1, and the context gives the plain run's records (the oracle's over x)."""
    x, ref, ref_plain = scene(name)
    want, want_plain = {"full": ((16, 16), (10, 10)), "excerpt": ((6, 6), (0, 0))}[name]
    assert (len(ref.bursts), good_frames(ref)) == want and (len(ref_plain.bursts), good_frames(ref_plain)) == want_plain
    res = {}

    def after(p, out):
        L = irdm.lib()
        H = p.primed_samples
        head = np.ascontiguousarray(x[:H])
        # primed and fed: refused, nothing changed
        state = (p.primed_samples, p.primed_frames, p.start_time_ns, p.sample_count)
        assert L.irdm_prime_host(p.h, head.ctypes.data_as(C.c_void_p), len(head)) == -1
        assert (p.primed_samples, p.primed_frames, p.start_time_ns, p.sample_count) == state
        p.reset(start_time_ns=T0)
        assert (p.primed_samples, p.primed_frames, p.start_time_ns, p.sample_count, p.tagged) == (0, 0, T0, 0, 0)
        # less than one frame: refused; then a first feed, and the call is refused for good
        assert L.irdm_prime_host(p.h, head.ctypes.data_as(C.c_void_p), p.fft_size - 1) == -1
        sizes = chunks_of(len(x), CHUNK)
        parity.feed_chunks(p, x, irdm.FMT_CF32, sizes[:1])
        assert L.irdm_prime_host(p.h, head.ctypes.data_as(C.c_void_p), len(head)) == -1
        assert (p.primed_samples, p.primed_frames, p.start_time_ns, p.sample_count) == (0, 0, T0, sizes[0])
        parity.feed_chunks(p, x, irdm.FMT_CF32, sizes[1:], off=sizes[0])
        plain = collect(p, depth)
        s = parity.compare(plain, ref_plain) if ref_plain.bursts else None
        assert (len(plain["bursts"]), len(plain["demods"]), plain["tagged"]) == (want_plain[0], want_plain[1], ref_plain.n_tagged)
        res["plain"] = dict(bursts=len(plain["bursts"]), demods=len(plain["demods"]), compared=s is not None)

    out = run_primed(x, FS, depth=depth, after=after)
    s = parity.compare(out, ref)
    print("primed %s depth %d: %s; plain after reset: %s" % (name, depth, s, res["plain"]))
    assert (s["bursts"], s["demods"], s["frames"]) == (want[0], want[1], want[1])
    return dict(primed=dict(bursts=s["bursts"], demods=s["demods"]), plain=res["plain"])


# ---------------------------------------------------------------- the rates of the GPU test ----
@functools.lru_cache(maxsize=None)
def rate_stream(fs, fmt):
    """(x, oracle over P || x): the smallest scene tests/rates.py builds at the rate; at 16 MHz its last 500 frames, so that
    the prefix is tiled (the scene's bursts all lie behind its frame 520: the cut keeps them)"""
    import rates
    iq = rates.stream(fs)
    if fs == 16_000_000:
        iq = np.ascontiguousarray(iq[len(iq) - 500 * fft_size(fs):])
    x = iq if fmt == irdm.FMT_CF32 else siggen.to_ci8(iq)
    x.setflags(write=False)
    ref = oracle_primed(x, fs, fmt)
    assert len(ref.bursts) >= 5 and len(ref.demods) >= 4, (fs, len(ref.bursts), len(ref.demods))
    return x, ref


# ---------------------------------------------------------------- options on the chunk path ----
BALANCE = (1.5, 8.0)            # dB, degrees


@functools.lru_cache(maxsize=None)
def spoiled_excerpt():
    """the excerpt as a receiver with its Q arm 1.5 dB up and 8 degrees off quadrature and I and Q exchanged on the wire would
    have recorded it, with NaN / Inf / 1e30 written into the noise in front of its first burst -- inside the head the prefix
    is tiled from, and so in P as well; interleaved floats"""
    x = scene("excerpt")[0]
    alpha, beta = irdm.iq_balance_coeffs(*BALANCE)
    i, q = x.real.astype(np.float32), x.imag.astype(np.float32)
    qd = ((q - alpha * i) / beta).astype(np.float32)            # (the inverse of the correction q' = alpha i + beta q)
    w = np.empty(2 * len(x), np.float32)
    w[0::2], w[1::2] = qd, i
    for k, v in ((3, "nan"), (2 * 40_001, "inf"), (2 * 40_001 + 1, "-inf"), (2 * 90_000, 1e30)):
        w[k] = np.float32(v)
    w.setflags(write=False)
    return w


def chunk_options(p):
    p.set_option("swap_iq", 1)
    p.set_option("scrub", 1)
    p.iq_balance(irdm.FMT_CF32, *BALANCE)


def options_case(depth):
    """swap_iq, irdm_iq_balance and scrub on together: the primed context fed the wire samples w gives, byte for byte, the
    records of a plain context with the same three on, created with start time T0' and fed P(w) || w -- the contract as it
    is written -- and finds the excerpt's 6 frames; irdm_scrub_stats counts w alone, positions in w"""
    w = spoiled_excerpt().view(np.complex64)
    seen = {}

    def after(p, out):
        st = p.scrub_stats()
        seen["scrub"] = (int(st.n_samples), int(st.n_zeroed), int(st.first), int(st.last))

    on = run_primed(w, FS, depth=depth, before=chunk_options, after=after)
    P, F = prefix(w, FS)
    assert F == 700_000 // 2048
    p = irdm.Pipeline(FS, fmt=irdm.FMT_CF32, max_chunk_samples=CHUNK, max_bursts_per_chunk=1024, pipeline_depth=depth,
                      start_time_ns=shifted_origin(FS))
    try:
        p.set_option("keep_frame_samples", 1)
        chunk_options(p)
        feed(p, np.concatenate([P, w]), irdm.FMT_CF32, CHUNK)
        plain = collect(p, depth)
        st = p.scrub_stats()
        # (the plain context has scrubbed P as well: the primed one reports the recording alone)
        assert int(st.n_samples) == len(P) + len(w) and int(st.n_zeroed) > 3
    finally:
        p.close()
    for k, name in enumerate(("bursts", "frames", "demods", "frame samples")):
        assert records_bytes(on)[k] == records_bytes(plain)[k], (name, depth)
    assert on["tagged"] == plain["tagged"] and len(on["demods"]) == 6 and all(d.ok for d in on["demods"]), len(on["demods"])
    assert seen["scrub"] == (len(w), 3, 1, 90_000), seen
    return dict(demods=len(on["demods"]))


# ---------------------------------------------------------------- the side passes ----
SPECTRUM_R = 100


def side_options(p):
    for k, v in (("input_stats", 1), ("iq_moments", 1), ("scrub", 1), ("spectrum_frames", SPECTRUM_R)):
        p.set_option(k, v)


def side_results(p):
    """every side pass's result, as bytes and rows"""
    p.flush()
    hdrs, mean, peak = p.poll_spectrum()
    return dict(input=bytes(p.input_stats()), moments=bytes(p.iq_moments()), scrub=bytes(p.scrub_stats()),
                rows=[(h.row, h.first_frame, h.timestamp_ns, h.n_frames, h.n_bins) for h in hdrs], mean=mean.tobytes(), peak=peak.tobytes())


def side_case(depth):
    """input_stats, iq_moments, scrub and spectrum_frames on: their results on a primed context fed x equal, exactly, those of
    a plain context with start time T0 fed x alone -- counts, sums, the scrub's first / last, every spectrum row's number,
    first_frame, timestamp_ns and bins; x is the excerpt with two bad samples in it"""
    x = cf32_floats(scene("excerpt")[0]).copy()
    x[2 * 1234] = np.float32("nan")
    x[2 * 650_000 + 1] = np.float32(1e30)
    x = x.view(np.complex64)
    got = {}

    def after(p, out):
        got["primed"] = side_results(p)

    run_primed(x, FS, depth=depth, before=side_options, after=after)
    p = irdm.Pipeline(FS, fmt=irdm.FMT_CF32, max_chunk_samples=CHUNK, max_bursts_per_chunk=1024, pipeline_depth=depth, start_time_ns=T0)
    try:
        side_options(p)
        feed(p, x, irdm.FMT_CF32, CHUNK)
        got["plain"] = side_results(p)
    finally:
        p.close()
    a, b = got["primed"], got["plain"]
    print("side passes depth %d: rows %s" % (depth, b["rows"]))
    assert len(b["rows"]) == -(-(700_000 // 2048) // SPECTRUM_R) and b["rows"][0][1:3] == (0, T0)
    st = irdm.ScrubStats.from_buffer_copy(b["scrub"])
    assert (int(st.n_samples), int(st.n_zeroed), int(st.first), int(st.last)) == (700_000, 2, 1234, 650_000)
    for k in a:
        assert a[k] == b[k], (k, depth)
    return dict(rows=len(a["rows"]))

