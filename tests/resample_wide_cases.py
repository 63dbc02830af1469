"""TEST INFRASTRUCTURE: the assertions on the front end's wide-ratio kernel K0w (csrc/resample_wide.hip,
csrc/resample_wide.cpp) that tests/test_gpu_resample_wide.py makes on the GPU and tests/test_resample_wide_emul.py, through
tests/resample_wide_emul_run.py, on the CPU emulation: whichever build irdm.lib() has loaded.  The reference is the plain C
model of the arithmetic contract (tests/resample_model.c), bit for bit."""
import numpy as np

import farpos
import frontend_model as fm
import irdm
import resample_model as rm

# (L, M) -> (capture rate, resampled rate, input samples of the test stream, K0w's outputs per tile).  The tile is what
# irdm_frontend_wide_geometry reports (asserted).  Every stream gives more than 3 tiles; m mod L wraps inside a tile
# because L < tile, and at 4000/4001 inside the tile [2048, 4096) and every second tile after it; the ragged feeds put
# launch boundaries inside tiles.
PAIRS = {(127, 128): (2_048_000, 2_032_000, 40_000, 2048), (400, 401): (10_025_000, 10_000_000, 40_000, 2048),
         (275, 288): (2_880_000, 2_750_000, 40_000, 2048), (100, 801): (8_010_000, 1_000_000, 300_000, 256),
         (4000, 4001): (10_002_500, 10_000_000, 40_000, 2048)}
FORMATS = (irdm.FMT_CI8, irdm.FMT_CF32, irdm.FMT_SC16Q11)
Q_LIST = (0, 14418, -32768)
# ratios K0r takes as well
SHARED = {(25, 28): (11_200_000, 10_000_000), (125, 128): (12_288_000, 12_000_000), (125, 768): (61_440_000, 10_000_000)}
# what irdm_frontend_create_resampler refuses: (name, (in_rate, format, out_rate), the message on stderr)
REFUSALS = (("L", (10_250_000, 0, 10_247_500), "ratio 4099/4100; L <= 4096 and M <= 65536 are built"),
            ("ratio_hi", (34_000_000, 0, 2_000_000), "(ratio 1/17): M / L must lie in 24/25 .. 16"),
            ("ratio_lo", (2_000_000, 0, 2_500_000), "(ratio 5/4): M / L must lie in 24/25 .. 16"),
            ("same", (2_000_000, 0, 2_000_000), "(ratio 1/1): M / L must lie in 24/25 .. 16"),
            ("out_rate", (25_062_500, 0, 25_000_000), "output rate 25000000 (25062500 * 400 / 401) is not one the pipeline takes"))
# eight bursts at 10 025 000 S/s, made as rm.SCENES["11.2->10"] is: a recording declared 10 MS/s whose clock runs 0.25 % fast
# (the seed is one at which the oracle alone finds all eight whole on the float64-resampled stream and not all of them
# natively: tests/test_resample_wide_emul.py asserts both)
SCENE = dict(in_rate=10_025_000, out_rate=10_000_000, secs=0.72, seed=1002, channels=(-90, -60, -31, -7, 22, 48, 75, 95))


class Stage(rm.Stage):
    """rm.Stage on irdm_frontend_create_wide (maker "wide") or another maker of the resampling front end"""

    def __init__(self, in_rate, fmt, out_rate, shift_hz=0.0, device=0, maker="wide"):
        self.fe = irdm.Frontend(in_rate, fmt, None, shift_hz, device, out_rate=out_rate, maker=maker)
        self.fmt, self.device = fmt, device
        self.L, self.M = self.fe.ratio


def differ(got, want):
    if len(got) != len(want):
        return (len(got), len(want))
    bad = np.nonzero(got.view(np.uint64) != want.view(np.uint64))[0]
    return "%d outputs differ, first at %d" % (len(bad), bad[0]) if len(bad) else None


def check_pair(pair, fmt, q):
    """the stream whole and in ragged feeds (1 sample, one less than the taps of a phase, a prime, in turn) = the model"""
    L, M = pair
    fi, fo, n, tile = PAIRS[pair]
    geo = irdm.Frontend.wide_geometry(fi, fo)
    assert geo["tile"] == tile and rm.n_outputs(n, L, M) > 3 * tile and (L < tile or 2 * tile > L), geo
    shift = q * fi / 65536.0
    assert fm.quantise(shift, fi) == q
    x = fm.random_capture(fmt, n, seed=1000 * L + M + fmt)
    st = Stage(fi, fmt, fo, shift)
    assert st.fe.ratio == (L, M) and st.fe.out_rate == fo and st.fe.ntaps == geo["ntaps"]
    taps = st.fe.taps()
    want = rm.run(x, fmt, L, M, q, taps)
    whole = st.run(x, [n])
    st.close()
    assert differ(whole, want) is None, (pair, fm.NAMES[fmt], q, "whole", differ(whole, want))
    feeds = rm.ragged_feeds(n, len(taps), L, (9973,))
    assert 1 in feeds and any(1 < f < len(taps) / L for f in feeds)
    st = Stage(fi, fmt, fo, shift)
    got = st.run(x, feeds)
    st.close()
    assert differ(got, want) is None, (pair, fm.NAMES[fmt], q, "ragged", differ(got, want))
    return len(want)


def check_shared(pair):
    """irdm_frontend_create_wide = irdm_frontend_create_rational bit for bit at a ratio both take (and both = the model)"""
    L, M = pair
    fi, fo = SHARED[pair]
    n = 60 * M + 40_000
    out = {}
    for fmt, q in ((irdm.FMT_CI8, 14418), (irdm.FMT_CF32, -32768)):
        x = fm.random_capture(fmt, n, seed=L + M + fmt)
        shift = q * fi / 65536.0
        res = []
        for maker in ("wide", "rational"):
            st = Stage(fi, fmt, fo, shift, maker=maker)
            assert st.fe.ratio == (L, M)
            taps = st.fe.taps()
            res.append((taps, st.run(x, rm.ragged_feeds(n, len(taps), L, (9973,)))))
            st.close()
        assert np.array_equal(res[0][0].view(np.uint32), res[1][0].view(np.uint32))
        assert differ(res[0][1], res[1][1]) is None, (pair, fmt, differ(res[0][1], res[1][1]))
        assert differ(res[0][1], rm.run(x, fmt, L, M, q, res[0][0])) is None
        out[fm.NAMES[fmt]] = len(res[0][1])
    return out


def check_nonfinite():
    """a cf32 stream at 400/401 with one NaN and one +Inf sample: the outputs that are not finite are the model's, I and Q
    each (an Inf next to an output's window must not reach it: a tap index outside the prototype is no term), and every
    other output equals the model bit for bit"""
    fi, fo, n, _ = PAIRS[(400, 401)]
    q = 14418
    x = fm.random_capture(irdm.FMT_CF32, n, seed=31)
    x[12_345] = np.complex64(complex(np.nan, 0.25))
    x[23_456] = np.complex64(complex(np.inf, -0.125))
    st = Stage(fi, irdm.FMT_CF32, fo, q * fi / 65536.0)
    taps = st.fe.taps()
    got = st.run(x, rm.ragged_feeds(n, len(taps), 400, (9973,)))
    st.close()
    want = rm.run(x, irdm.FMT_CF32, 400, 401, q, taps)
    assert len(got) == len(want)
    counts = {}
    for name, g, w in (("I", got.real, want.real), ("Q", got.imag, want.imag)):
        bad_g, bad_w = ~np.isfinite(g), ~np.isfinite(w)
        assert np.array_equal(bad_g, bad_w), (name, int(bad_g.sum()), int(bad_w.sum()))
        assert np.array_equal(g[~bad_w].view(np.uint32), w[~bad_w].view(np.uint32)), name
        counts[name] = int(bad_w.sum())
    # (about one filter length of outputs around each of the two samples, and no more)
    assert all(2 * (len(taps) // 400 - 1) <= c <= 2 * (len(taps) // 400 + 1) for c in counts.values()), counts
    return counts


def check_seek(power=44, r=12_345, n=100_000):
    """tests/test_gpu_farpos.py's check_frontend for K0w at 400/401: sought to P = r modulo 65536 M above 2^44 and run on n
    samples in ragged feeds = the model on zeros(r) ++ x from the output on that those r samples leave incomplete"""
    L, M = 400, 401
    fi, fo = PAIRS[(L, M)][:2]
    out = {}
    for fmt, q in ((irdm.FMT_CF32, 14418), (irdm.FMT_CI8, -9000)):
        x = fm.random_capture(fmt, n, seed=7000 + 10 * M + fmt)
        st = Stage(fi, fmt, fo, q * fi / 65536.0)
        try:
            taps = st.fe.taps()
            P = farpos.fe_seek_position(power, M, n, r)
            assert P % farpos.fe_period(M) == r and P >= 1 << power and r * L > len(taps)
            st.fe.seek(P)
            got = st.run(x, rm.ragged_feeds(n, len(taps), L, (9973, 65537)))
        finally:
            st.close()
        want = rm.run(farpos.lead_in(x, fmt, r), fmt, L, M, q, taps)[farpos.fe_outputs(r, L, M, len(taps)):]
        assert len(got) > n * L // M - len(taps)
        assert differ(got, want) is None, (fm.NAMES[fmt], P, differ(got, want))
        out[fm.NAMES[fmt]] = len(got)
    return out


def check_resampler():
    """irdm_frontend_create_resampler: the integer front end at 50 -> 10 MS/s, irdm_frontend_create_rational's output at
    25/28, K0w's ratio and kernel numbers from irdm_frontend_resampler_ratio"""
    fe = irdm.Frontend.resampler(50_000_000, irdm.FMT_CI8, 10_000_000)
    assert fe.ratio == (1, 5) and fe.ntaps == 223
    fe.close()
    assert irdm.Frontend.resampler_ratio(50_000_000, 10_000_000) == (1, 5, 0)
    assert irdm.Frontend.resampler_ratio(11_200_000, 10_000_000) == (25, 28, 1)
    assert irdm.Frontend.resampler_ratio(61_440_000, 10_000_000) == (125, 768, 1)
    for (L, M), (fi, fo, _, _) in PAIRS.items():
        assert irdm.Frontend.resampler_ratio(fi, fo) == (L, M, 2)
    fi, fo = SHARED[(25, 28)]
    n = 50_000
    x = fm.random_capture(irdm.FMT_CI8, n, seed=5)
    res = []
    for maker in ("resampler", "rational"):
        st = Stage(fi, irdm.FMT_CI8, fo, 150_000.0, maker=maker)
        res.append(st.run(x, [n]))
        st.close()
    assert differ(res[0], res[1]) is None
    fi, fo = PAIRS[(400, 401)][:2]
    fe = irdm.Frontend.resampler(fi, irdm.FMT_CF32, fo)
    assert fe.ratio == (400, 401) and fe.out_rate == fo
    fe.close()
    return len(res[0])


def check_save_band():
    """irdm_frontend_save, cf32, behind 400/401: the saved bytes are the model's outputs"""
    fi, fo, n, _ = PAIRS[(400, 401)]
    x = fm.random_capture(irdm.FMT_CI8, n, seed=77)
    st = Stage(fi, irdm.FMT_CI8, fo, 0.0)
    st.fe.save(irdm.FMT_CF32, slot_samples=4096)
    taps = st.fe.taps()
    got = st.run(x, rm.ragged_feeds(n, len(taps), 400, (9973,)))
    saved = b"".join(st.fe.saved)
    st.close()
    want = rm.run(x, irdm.FMT_CI8, 400, 401, 0, taps)
    assert differ(got, want) is None
    assert saved == want.tobytes()
    return len(saved)


def run_composed(x, in_rate, fmt, out_rate, shift_hz, feeds, depth, max_chunk, feed="host", center=1622000000.0):
    """rm.run_composed behind irdm_frontend_create_resampler: the capture through irdm_frontend_feed_* + flush into a cf32
    pipeline at out_rate; returns (the record queues in the shape parity.run_gpu returns them, the applied shift)"""
    fe = irdm.Frontend.resampler(in_rate, fmt, out_rate, shift_hz)
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


def float64_resample(x, L, M, taps):
    """y[m] = sum_n P[m M + C - n L] x[n] in float64, phase by phase (no shift): the reference stream of the end-to-end test"""
    p = np.asarray(taps, np.float32).astype(np.float64)
    x = np.asarray(x).astype(np.complex128)
    Np, n = len(p), len(x)
    c = (Np - 1) // 2
    m = np.arange(rm.n_outputs(n, L, M), dtype=np.int64)
    hi = (m * M + c) // L                                   # the last input of output m; its tap index is (m M + c) mod L
    k = (m * M + c) % L
    y = np.zeros(len(m), np.complex128)
    for i in range(-(-Np // L)):
        ok = (k < Np) & (hi >= 0) & (hi < n)
        y[ok] += p[k[ok]] * x[hi[ok]]
        hi -= 1
        k += L
    return y.astype(np.complex64)


def scene(fmt=irdm.FMT_CF32):
    """(capture at 10 025 000 S/s, the expected hard bits per burst in time order): rm.offgrid_scene's construction -- the
    symbols run at 25 ksym/s in capture time, 401 samples each -- on SCENE"""
    import siggen
    s = SCENE
    fs = s["in_rate"]
    n = int(s["secs"] * fs) // 32768 * 32768
    rng = np.random.default_rng(s["seed"])
    bursts, expect = [], []
    for k, ch in enumerate(s["channels"]):
        f = siggen.channel_freq(ch)
        assert abs(f) <= 0.40 * s["out_rate"], ch
        payload = list(rng.integers(0, 4, 150))
        start = int((0.42 + (s["secs"] - 0.47) * k / len(s["channels"])) * fs)
        bursts.append(dict(start=start, freq_hz=f, payload=payload, amp=0.05))
        expect.append(siggen.quadrants_to_bits(siggen.frame_quadrants(payload)[16:]))
    iq, _ = siggen.make_stream(fs, n, bursts, seed=s["seed"])
    return (siggen.to_ci8(iq) if fmt == irdm.FMT_CI8 else iq), expect


def frames_whole(demods, ref_demods):
    """every frame of ref_demods appears in demods with every bit right"""
    have = {(d.n_bits, bytes(int(b) for b in d.bits[:d.n_bits])) for d in demods}
    return all((d.n_bits, bytes(int(b) for b in d.bits[:d.n_bits])) in have for d in ref_demods)
