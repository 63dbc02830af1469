"""TEST INFRASTRUCTURE: the band requantiser's arithmetic contract (csrc/frontend.hip, requant_kernel) restated in numpy, and the
checks of irdm_requantize_device / irdm_frontend_save that the emulated and the GPU tests share (whichever build irdm.lib()
loads).

Per float component x of the cf32 band, S = 128 (ci8) or 32768 (ci16), k = float32(float32(gain) * float32(S)):
    v = rint(x * k) in float32 (to nearest, ties to even);  q = clip(v, -S, S - 1);  NaN -> 0;  +-Inf -> the rail of its sign
    n_clipped: components with v outside [-S, S - 1] or NaN;  peak = max |x * k| / S over the components with x finite."""
import numpy as np

import irdm

SCALE = {irdm.FMT_CI8: 128, irdm.FMT_CI16: 32768}
DTYPE = {irdm.FMT_CI8: np.int8, irdm.FMT_CI16: np.int16}
BYTES = {irdm.FMT_CI8: 2, irdm.FMT_CI16: 4, irdm.FMT_CF32: 8}
GAINS = (1.0, 0.37, 64.0)
OFFSETS = (0, 1, 3)
KERNEL_SIZES = (0, 1, 2, 3, 63, 64, 65, 255, 257, (1 << 16) + 7)


def quantise(y, fmt, gain):
    """(the recording's bytes, (n_samples, n_clipped, peak)) of the complex64 band y; cf32: the bytes as they are"""
    y = np.ascontiguousarray(y, np.complex64)
    if fmt == irdm.FMT_CF32:
        assert gain == 1.0
        return y.tobytes(), (len(y), 0, np.float32(0))
    S = SCALE[fmt]
    x = y.view(np.float32)
    k = np.float32(np.float32(gain) * np.float32(S))
    with np.errstate(all="ignore"):
        p = x * k
        assert p.dtype == np.float32
        v = np.rint(p)
        nan = np.isnan(v)
        clipped = nan | (v < -S) | (v > S - 1)
        q = np.clip(np.where(nan, np.float32(0), v), -S, S - 1).astype(DTYPE[fmt])
        fin = np.isfinite(x)
        peak = np.float32(np.abs(p[fin]).max()) / np.float32(S) if fin.any() else np.float32(0)
    return q.astype("<i%d" % q.itemsize).tobytes(), (len(y), int(clipped.sum()), np.float32(peak))


def special_values(fmt, gain):
    """the components every kernel case of at least 64 samples holds: ties, rails, overflow, NaN, +-Inf, denormals, +-0"""
    S = SCALE[fmt]
    k = np.float32(np.float32(gain) * np.float32(S))
    with np.errstate(all="ignore"):
        v = [np.float32(t) / k for t in (0.5, -0.5, 1.5, -1.5, 2.5, -2.5, S - 1, S - 0.5, S, -S, -S - 0.5)]
    v += [np.float32(3.0e38), np.float32(-3.0e38),                      # the product overflows float for every k > 1.2
          np.float32(np.nan), np.float32(np.inf), np.float32(-np.inf),
          np.float32(1e-45), np.float32(-1e-45), np.float32(1.1e-38), np.float32(-5e-39),      # denormals (and the least normal)
          np.float32(0.0), np.float32(-0.0)]
    return np.array(v, np.float32)


def kernel_input(n, fmt, gain, seed):
    """n samples: random components of a few times full scale over gain, the special values written over the front (as many
    as fit) and, from 64 samples on, once more over the end, so that they meet the scalar head and tail as well as the body"""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal(2 * n) * (1.5 / gain)).astype(np.float32)
    sp = special_values(fmt, gain)
    m = min(len(sp), 2 * n)
    x[:m] = sp[:m]
    if n >= 64:
        x[2 * n - len(sp):] = sp[::-1]
    return x.view(np.complex64)


def same_stats(got, want):
    return got[0] == want[0] and got[1] == want[1] and np.float32(got[2]).view(np.uint32) == np.float32(want[2]).view(np.uint32)


def check_kernel(sizes=KERNEL_SIZES, device=0):
    """irdm_requantize_device against quantise(): bytes and statistics exactly equal, both integer formats, the gains, input
    and output each at sample offsets 0, 1 and 3 of a larger buffer; nothing written outside the output.  Returns the
    number of calls compared."""
    calls = 0
    for fmt in (irdm.FMT_CI8, irdm.FMT_CI16):
        bps = BYTES[fmt]
        for gain in GAINS:
            for n in sizes:
                x = kernel_input(n + 3, fmt, gain, seed=n + fmt)
                d_in = irdm.device_buffer(x if len(x) else np.zeros(1, np.complex64), device)
                guard = np.full((n + 8) * bps, 0x5a, np.uint8)
                try:
                    for a in OFFSETS:
                        want, wstats = quantise(x[a:a + n], fmt, gain)
                        for b in OFFSETS:
                            d_out = irdm.device_buffer(guard, device)
                            try:
                                stats = irdm.requantize_device(d_in + 8 * a, n, fmt, gain, d_out + bps * b, device)
                                got = np.empty_like(guard)
                                irdm.device_download(got, d_out)
                            finally:
                                irdm.device_free(d_out)
                            body = got[bps * b:bps * (b + n)].tobytes()
                            assert body == want, (fmt, gain, n, a, b, first_difference(body, want, fmt))
                            assert (got[:bps * b] == 0x5a).all() and (got[bps * (b + n):] == 0x5a).all(), (fmt, gain, n, a, b)
                            assert same_stats(stats, wstats), (fmt, gain, n, a, b, stats, wstats)
                            calls += 1
                finally:
                    irdm.device_free(d_in)
    return calls


def first_difference(got, want, fmt):
    if len(got) != len(want):
        return "lengths %d, %d" % (len(got), len(want))
    dt = np.uint8 if fmt == irdm.FMT_CF32 else DTYPE[fmt]
    g, w = np.frombuffer(got, dt), np.frombuffer(want, dt)
    bad = np.nonzero(g != w)[0]
    return "%d differ, first at component %d: %r, model %r" % (len(bad), bad[0], g[bad[0]], w[bad[0]])


def run_saved(stage, x, feeds, fmt_out, gain=1.0, slot_samples=0):
    """stage: a frontend_model.Stage or resample_model.Stage not yet fed.  The capture through it with saving on; returns
    (the stage's outputs, the sink's bytes concatenated, the largest piece in bytes, irdm_frontend_save_stats)."""
    stage.fe.save(fmt_out, gain=gain, slot_samples=slot_samples)
    y = stage.run(x, feeds)
    pieces = stage.fe.saved
    return y, b"".join(pieces), max([len(p) for p in pieces] or [0]), stage.fe.save_stats()


def check_saved(make_stage, x, want_y, feeds_list, cases, slot_samples):
    """cases: (fmt_out, gain) pairs.  For every case and cut into feeds: the stage's outputs are the model's, the sink's
    bytes are quantise(model), no piece exceeds slot_samples, and the statistics and the sample count match."""
    import frontend_model as fm
    n = 0
    for fmt_out, gain in cases:
        want, wstats = quantise(want_y, fmt_out, gain)
        for feeds in feeds_list:
            st = make_stage()
            try:
                y, got, largest, stats = run_saved(st, x, feeds, fmt_out, gain, slot_samples)
            finally:
                st.close()
            assert fm.same_bits(y, want_y)
            assert got == want, (fmt_out, gain, feeds[:4], first_difference(got, want, fmt_out))
            assert largest <= (slot_samples or 4 << 20) * BYTES[fmt_out]
            assert same_stats(stats, wstats), (fmt_out, gain, stats, wstats)
            n += 1
    return n


def run_composed_saved(x, fs_in, fmt, D, shift_hz, feeds, depth, max_chunk, feed, fmt_out, gain=1.0, slot_samples=0,
                       center=1622000000.0):
    """frontend_model.run_composed with saving on: (the record queues, the applied shift, the sink's bytes, the statistics)"""
    import frontend_model as fm
    fe = irdm.Frontend(fs_in, fmt, D, shift_hz)
    p = irdm.Pipeline(fe.out_rate, fmt=irdm.FMT_CF32, center_frequency=center + fe.applied_shift_hz,
                      max_chunk_samples=max_chunk, max_bursts_per_chunk=1024, pipeline_depth=depth)
    try:
        p.set_option("keep_frame_samples", 1)
        fe.save(fmt_out, gain=gain, slot_samples=slot_samples)
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
        return (dict(bursts=bursts, infos=infos, samples=samples, demods=demods, packed=[], tagged=p.tagged,
                     n_samples=p.sample_count), fe.applied_shift_hz, b"".join(fe.saved), fe.save_stats())
    finally:
        p.close()
        fe.close()
