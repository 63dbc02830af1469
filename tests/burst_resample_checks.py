"""TEST INFRASTRUCTURE: the checks of the per-burst resampler (option "burst_resample") that the CPU emulation
(tests/burst_resample_emul_run.py) and the GPU tests (tests/test_gpu_burst_resample.py) share.

Stage level: irdm_burst_resample_batch against tests/burst_resample_model.py.
Pipeline level: eight-burst scenes at rates off the 250 kHz grid (the construction of resample_model.offgrid_scene: symbols at
25 ksym/s in capture time), the context with the option off and on against the oracle and the scene's truth."""
import numpy as np

import burst_resample_model as bm
import irdm
import siggen

STAGE_RATIOS = [(25, 24), (40, 41), (8, 7), (7, 8), (400, 401), (4096, 4097)]
STAGE_LENGTHS = [100, 101, 2047, 22480, 65536, 3]
IMPULSE_LEN = 2047
TONE_HZ = 30000.0
CENTER = 1622000000.0
T0 = 1700000000 * 10**9        # the start time irdm.Pipeline and orc.run_stream default to


def stage_rows(L, M):
    """rows of seeded noise plus a tone at 30 kHz (the row's rate is 250000 M / L), every |component| below 0.75 of a full
    scale of 1; behind them three rows of IMPULSE_LEN with one impulse each: at input 0, mid-row and at the last input"""
    rng = np.random.default_rng(1000 * L + M)
    f_in = 250000.0 * M / L
    rows = []
    for n in STAGE_LENGTHS:
        t = np.arange(n) / f_in
        x = 0.5 * np.exp(2j * np.pi * TONE_HZ * t) + 0.05 * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
        rows.append(np.clip(x.real, -0.75, 0.75).astype(np.float32) + 1j * np.clip(x.imag, -0.75, 0.75).astype(np.float32))
    for i in (0, IMPULSE_LEN // 2, IMPULSE_LEN - 1):
        x = np.zeros(IMPULSE_LEN, np.complex64)
        x[i] = 1.0
        rows.append(x)
    return [r.astype(np.complex64) for r in rows], (0, IMPULSE_LEN // 2, IMPULSE_LEN - 1)


def tone_hz(y, rate):
    """the frequency of the largest line of y: Hann window, parabola through the log magnitudes of the three bins"""
    n = len(y)
    sp = np.abs(np.fft.fft(y.astype(np.complex128) * np.hanning(n)))
    k = int(np.argmax(sp))
    a, b, c = np.log(sp[(k - 1) % n]), np.log(sp[k]), np.log(sp[(k + 1) % n])
    d = 0.5 * (a - c) / (a - 2 * b + c)
    f = (k + d) / n
    return (f - 1.0 if f >= 0.5 else f) * rate


_ref_cache = {}


def stage_reference(L, M):
    """(rows, impulse positions, float32 model rows, float64 reference rows), computed once per ratio"""
    if (L, M) not in _ref_cache:
        rows, imp = stage_rows(L, M)
        _ref_cache[(L, M)] = (rows, imp, [bm.resample_f32(r, L, M) for r in rows], [bm.resample_f64(r, L, M) for r in rows])
    return _ref_cache[(L, M)]


def check_stage(L, M, device=0):
    """one launch of burst_resample_kernel over all rows of the ratio; returns the figures it asserted on"""
    rows, imp, want32, want64 = stage_reference(L, M)
    got = irdm.burst_resample_batch(rows, L, M, device=device)
    worst64, worst_hz = 0.0, 0.0
    for r, g, w32, w64 in zip(rows, got, want32, want64):
        assert len(g) == len(r) * L // M == bm.res_len(len(r), L, M), (L, M, len(r), len(g))
        assert g.view(np.uint32).tobytes() == w32.view(np.uint32).tobytes(), \
            (L, M, len(r), int(np.sum(g.view(np.uint32) != w32.view(np.uint32))))
        if len(g):
            worst64 = max(worst64, float(np.max(np.maximum(np.abs(g.real - w64.real), np.abs(g.imag - w64.imag)))))
    print("%d/%d: largest |float32 - float64| %.3e of full scale" % (L, M, worst64))
    assert worst64 <= 2e-6, (L, M, worst64)
    for r, g in zip(rows[:len(STAGE_LENGTHS)], got):
        if len(r) >= 22480:
            f = tone_hz(g, 250000.0)
            print("%d/%d: %d samples, tone at %.3f Hz" % (L, M, len(r), f))
            worst_hz = max(worst_hz, abs(f - TONE_HZ))
            assert abs(f - TONE_HZ) <= 1.0, (L, M, len(r), f)
    for i, g in zip(imp, got[len(STAGE_LENGTHS):]):
        c = i * L / M                                       # an impulse at input i is centred at output i L / M
        k = int(np.argmax(np.abs(g)))
        assert abs(k - c) <= 0.5 + 1e-9 or (k == len(g) - 1 and c > k), (L, M, i, k, c)
        assert np.all(g.imag == 0)
        if 0 < i < IMPULSE_LEN - 1:
            m = np.arange(len(g))
            centroid = float(np.sum(m * g.real.astype(np.float64)) / np.sum(g.real.astype(np.float64)))
            print("%d/%d: impulse at %d, centroid %.5f, i L / M %.5f" % (L, M, i, centroid, c))
            assert abs(centroid - c) <= 1e-3, (L, M, i, centroid, c)
    return dict(worst64=worst64, worst_hz=worst_hz, rows=len(rows))


# ---- pipeline level ----
# eight bursts spaced in time, all within 0.40 of the rate of the centre, amp 0.05 (resample_model.offgrid_scene); 10.24 MS/s is
# no multiple of 25 kHz: its bursts come from resample_model.make_burst_fractional
SCENES = {
    2_400_000: dict(secs=1.0, seed=24, channels=(-22, -15, -9, -3, 4, 10, 16, 22)),
    2_050_000: dict(secs=1.0, seed=205, channels=(-19, -13, -8, -3, 4, 9, 14, 19)),
    10_025_000: dict(secs=0.72, seed=1002, channels=(-90, -60, -31, -7, 22, 48, 75, 95)),
    10_240_000: dict(secs=0.72, seed=1024, channels=(-90, -60, -31, -7, 22, 48, 75, 95)),
    2_000_000: dict(secs=1.0, seed=20, channels=(-19, -13, -8, -3, 4, 9, 14, 19)),
}


def scene(fs):
    """(iq at fs, truth: a list of dict(start, freq_hz, bits) in time order)"""
    import resample_model as rm
    s = SCENES[fs]
    n = int(s["secs"] * fs) // 32768 * 32768
    rng = np.random.default_rng(s["seed"])
    bursts, truth = [], []
    k_n = len(s["channels"])
    for k, ch in enumerate(s["channels"]):
        f = siggen.channel_freq(ch)
        assert abs(f) <= 0.40 * fs
        payload = list(rng.integers(0, 4, 150))
        start = int((0.42 + (s["secs"] - 0.47) * k / k_n) * fs)
        bursts.append(dict(start=start, freq_hz=f, payload=payload, amp=0.05))
        truth.append(dict(start=start, freq_hz=f, bits=siggen.quadrants_to_bits(siggen.frame_quadrants(payload)[16:])))
    if fs % siggen.SYMBOL_RATE == 0:
        iq, _ = siggen.make_stream(fs, n, bursts, seed=s["seed"])
        return iq, truth
    nrng = np.random.default_rng(s["seed"])
    iq = (nrng.standard_normal(n, dtype=np.float32) + 1j * nrng.standard_normal(n, dtype=np.float32)).astype(np.complex64)
    iq *= np.float32(0.002)
    for b in bursts:
        sig = rm.make_burst_fractional(fs, siggen.frame_quadrants(b["payload"]), b["freq_hz"], nrng.uniform(0, 2 * np.pi))
        iq[b["start"]:b["start"] + len(sig)] += sig
    return iq, truth


def demod_bits(d):
    return [int(b) for b in d.bits[:d.n_bits]]


def whole(d, truth):
    """the index of the truth burst whose every bit (unique word and payload) the frame carries, or None"""
    bits = demod_bits(d)
    for i, t in enumerate(truth):
        if bits == t["bits"]:
            return i
    return None


def run(iq, fs, on, depth=0, chunks=None, packed=False, options=None):
    import parity
    opts = dict(options or {})
    if on is not None:
        opts["burst_resample"] = 1 if on else 0
    # (the stat and the ratio are read while the context lives: parity.run_gpu closes it)
    seen = {}
    close = irdm.Pipeline.close

    def closing(p):
        if not p.h or seen:
            return close(p)
        seen["stats_br"] = p.stat("burst_resample_launches")
        if on:
            seen["ratio"] = p.burst_resample_ratio()
            seen["taps_shape"] = p.burst_resample_taps().shape
        close(p)
    irdm.Pipeline.close = closing
    try:
        res = parity.run_gpu(iq, fs, depth=depth, chunks=chunks, packed=packed, options=opts)
    finally:
        irdm.Pipeline.close = close
    res.update(seen)
    return res


def key_of(d):
    return (d.id, d.n_bits, bytes(demod_bits(d)), d.timestamp, d.center_frequency, d.confidence, d.level, d.direction)


def check_on(fs, off, on, truth, calib_ns):
    """the option on against the option off and the scene's truth.  calib_ns: what the frame timestamp of a burst placed at
    sample `start` exceeds start / fs by, measured on the on-grid scene's oracle records (the same bursts at 2 MS/s)"""
    assert [(b.id, b.start, b.stop, b.center_bin) for b in on["bursts"]] == [(b.id, b.start, b.stop, b.center_bin) for b in off["bursts"]]
    assert on["tagged"] == off["tagged"]
    ok_off = {d.id for d in off["demods"]}
    by_id = {d.id: d for d in on["demods"]}
    assert ok_off and ok_off <= set(by_id), (sorted(ok_off), sorted(by_id))
    figures = []
    for i in sorted(ok_off):
        d = by_id[i]
        k = whole(d, truth)
        assert k is not None, (fs, i, "not whole")
        t = truth[k]
        df = d.center_frequency - (CENTER + t["freq_hz"])
        dt_us = ((d.timestamp - T0) - (t["start"] / fs * 1e9 + calib_ns)) / 1e3
        figures.append((k, df, dt_us))
        print("%d: frame %d burst %d: frequency %+.1f Hz, time %+.2f us" % (fs, i, k, df, dt_us))
        assert abs(df) <= 50.0 and abs(dt_us) <= 20.0, (fs, i, df, dt_us)
    return figures


def calibrate():
    """median of (frame timestamp - start / fs) over the oracle's frames of the 2 MS/s scene, ns"""
    import orc
    iq, truth = scene(2_000_000)
    ref = orc.run_stream(iq, 2_000_000)
    v = []
    for d in ref.demods:
        k = whole(d, truth)
        if k is not None:
            v.append((d.timestamp - T0) - truth[k]["start"] / 2_000_000 * 1e9)
    assert len(v) >= 6, len(v)
    assert max(v) - min(v) <= 8000.0, v               # (two samples of 250 kHz)
    return float(np.median(v))


def burst_key(b):
    return (b.id, b.start, b.stop, b.center_bin, b.num_samples)


def full_keys(res):
    return [key_of(d) for d in res["demods"]]


def fine_offset(fs, b, t):
    """the burst's fine offset: its carrier against the centre of the detector bin it was found on"""
    n = 1 << int(round(np.log2(fs / 1000.0)))
    return t["freq_hz"] - (b.center_bin - n / 2) / n * fs


def case_stage(L, M):
    return check_stage(L, M)


def case_pipeline(fs):
    """one scene: option off = the oracle (and, at 2.4 and 2.05 MS/s, no frame whole); option on: the same bursts, every
    frame that passed the unique word whole, frequency within 50 Hz and time within 20 us of the scene's truth"""
    import orc
    import parity
    iq, truth = scene(fs)
    calib_ns = calibrate()
    off = run(iq, fs, False)
    summary = parity.compare(off, orc.run_stream(iq, fs))
    assert summary["demods"] >= 6, summary
    whole_off = sum(whole(d, truth) is not None for d in off["demods"])
    if fs in (2_400_000, 2_050_000):
        assert whole_off == 0, whole_off
    on = run(iq, fs, True)
    assert on["stats_br"] > 0
    figures = check_on(fs, off, on, truth, calib_ns)
    res = dict(frames=len(off["demods"]), whole_off=whole_off, whole_on=len(figures),
               worst_hz=max(abs(f[1]) for f in figures), worst_us=max(abs(f[2]) for f in figures))
    if fs == 2_400_000:
        # option off, the centre frequency is center_offset x 250000 where the row runs at 240000: the fine offset comes out
        # 25/24 of what it is -- an error of fine / 24, above 50 Hz from 1.2 kHz on
        by_id = {b.id: b for b in off["bursts"]}
        far = 0
        for d in off["demods"]:
            b = by_id[d.id]
            t = min(truth, key=lambda t: abs(t["start"] - b.start))
            fine = fine_offset(fs, b, t)
            err = d.center_frequency - (CENTER + t["freq_hz"])
            print("2400000 off: frame %d fine offset %+.0f Hz, frequency error %+.1f Hz" % (d.id, fine, err))
            if abs(fine) >= 1200.0:
                far += 1
                assert abs(err) > 50.0, (d.id, fine, err)
        assert far >= 1
        res["far"] = far
    return res


def case_ongrid():
    """2 MS/s, option on: the records of the option off bit for bit, no launch, nothing designed"""
    fs = 2_000_000
    iq, _ = scene(fs)
    off, on = run(iq, fs, None), run(iq, fs, True)
    assert len(off["demods"]) >= 6
    assert [burst_key(b) for b in on["bursts"]] == [burst_key(b) for b in off["bursts"]]
    assert [bytes(i) for i in on["infos"]] == [bytes(i) for i in off["infos"]]
    assert [bytes(d) for d in on["demods"]] == [bytes(d) for d in off["demods"]]
    assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(on["samples"], off["samples"]))
    assert on["stats_br"] == 0 and on["ratio"] == (1, 1, 0) and on["taps_shape"] == (0, 0)
    return dict(frames=len(on["demods"]))


def case_modes():
    """2.4 MS/s, option on: packed, parsed and full records carry the same frames; pipeline_depth 0 and 3 and two chunk sizes
    give the same records"""
    fs = 2_400_000
    iq, _ = scene(fs)
    n = len(iq)
    base = run(iq, fs, True)
    want = full_keys(base)
    assert len(want) >= 6
    for name, kw in (("depth3", dict(depth=3, chunks=[n // 4 // 32768 * 32768] * 3 + [n - 3 * (n // 4 // 32768 * 32768)])),
                     ("chunks", dict(chunks=[32768 * 8] * (n // (32768 * 8)) + ([n % (32768 * 8)] if n % (32768 * 8) else []))),
                     ("chunks_odd", dict(chunks=[32768 * 11] * (n // (32768 * 11)) + ([n % (32768 * 11)] if n % (32768 * 11) else [])))):
        got = run(iq, fs, True, **kw)
        assert full_keys(got) == want, name
        assert [bytes(d) for d in got["demods"]] == [bytes(d) for d in base["demods"]], name
        assert [burst_key(b) for b in got["bursts"]] == [burst_key(b) for b in base["bursts"]], name
    for name, opts in (("packed", {}), ("parsed", {"parsed_records": 1})):
        got = run(iq, fs, True, packed=True, options=opts)
        pk = got["packed"]
        assert [(d.id, d.n_bits, d.timestamp, d.center_frequency, d.confidence, d.direction) for d in pk] == \
               [(k[0], k[1], k[3], k[4], k[5], k[7]) for k in want], name
        for d, k in zip(pk, want):
            bits = np.unpackbits(np.frombuffer(bytes(d.bits), np.uint8))[:d.n_bits]
            assert bytes(bits.tolist()) == k[2], (name, d.id)
    return dict(frames=len(want))


def case_group():
    """two emulated devices: the option set through irdm_group_set_option gives the single context's records"""
    import parity
    import sharding
    fs, nfft = 2_400_000, 2048
    ov = (sharding.required_overlap(fs, nfft) + 15) // 16 * 16
    chunk = (ov + 32768 * 4) // 32768 * 32768
    n = 2 * chunk
    rng = np.random.default_rng(24)
    starts = np.linspace(530 * nfft, n - fs // 10, 8).astype(np.int64)
    starts[3] = chunk - 9000                     # one burst across the chunk boundary
    bursts = [dict(start=int(s), freq_hz=siggen.channel_freq(ch), payload=rng.integers(0, 4, 150).tolist())
              for s, ch in zip(starts, SCENES[fs]["channels"])]
    iq, _ = siggen.make_stream(fs, n, bursts, seed=24)
    single = parity.run_gpu(iq, fs, depth=1, chunks=[chunk, chunk], options={"burst_resample": 1})
    plain = parity.run_gpu(iq, fs, depth=1, chunks=[chunk, chunk])
    grp = parity.run_group(iq, fs, n_gpus=2, chunk=chunk, options={"burst_resample": 1})
    assert len(single["demods"]) >= 6
    assert [bytes(d) for d in grp["demods"]] == [bytes(d) for d in single["demods"]]
    assert [burst_key(b) for b in grp["bursts"]] == [burst_key(b) for b in single["bursts"]]
    assert [bytes(d) for d in plain["demods"]] != [bytes(d) for d in single["demods"]]
    return dict(frames=len(single["demods"]), chunks=grp["stats"]["chunks"])


def case_refused():
    """a rate whose L exceeds 4096 (2 049 877 S/s: a prime): the option is refused, and the context goes on without it"""
    p = irdm.Pipeline(2_049_877, max_chunk_samples=32768 * 8, max_bursts_per_chunk=64)
    try:
        try:
            p.set_option("burst_resample", 1)
            raise AssertionError("not refused")
        except ValueError:
            pass
        try:
            p.burst_resample_ratio()
            raise AssertionError("ratio with the option off")
        except RuntimeError:
            pass
    finally:
        p.close()
    return dict(refused=1)


# the ratios of the taps test and the rate a context has each at (4096/4097 is no rate's: 250000 / 4096 is no integer)
TAPS_RATES = {(25, 24): 2_400_000, (40, 41): 2_050_000, (30, 29): 725_000, (225, 224): 11_200_000, (400, 401): 10_025_000,
              (1025, 1024): 10_240_000, (1525, 1536): 15_360_000, (4096, 4097): None}


def case_taps():
    """every ratio's table: the context's (irdm_burst_resample_taps) and the stage call's (irdm_burst_resample_design) equal
    the model's bit for bit; the prototype's response; a constant row; L beyond 4096 refused"""
    res = {}
    for (L, M), fs in TAPS_RATES.items():
        want = bm.design(L, M)
        got = irdm.burst_resample_design(L, M)
        assert got.shape == want.shape == (L, bm.T) and got.view(np.uint32).tobytes() == want.view(np.uint32).tobytes(), (L, M)
        if fs is not None:
            assert bm.ratio(fs) == (L, M), (fs, bm.ratio(fs))
            p = irdm.Pipeline(fs, max_chunk_samples=32768 * 8, max_bursts_per_chunk=64)
            try:
                p.set_option("burst_resample", 1)
                assert p.burst_resample_ratio() == (L, M, bm.T)
                assert p.burst_resample_taps().view(np.uint32).tobytes() == want.view(np.uint32).tobytes(), (L, M)
            finally:
                p.close()
        # the table read as the prototype at rate L f_in, f_in = 250000 M / L, gain L taken out
        proto = bm.prototype_of(got)
        rate = 250000.0 * M
        nfft = 1 << int(np.ceil(np.log2(len(proto) * 16)))
        h = np.abs(np.fft.rfft(proto.astype(np.float64), nfft)) / L
        f = np.arange(len(h)) * rate / nfft
        db = 20 * np.log10(np.maximum(h, 1e-300))
        ripple, stop = float(np.max(np.abs(db[f <= 50000.0]))), float(np.max(db[f >= 165000.0]))
        print("%d/%d: within %.5f dB to 50 kHz, %.2f dB from 165 kHz on" % (L, M, ripple, stop))
        assert ripple <= 0.01 and stop <= -80.0, (L, M, ripple, stop)
        y = irdm.burst_resample_batch([np.full(600, 0.5 + 0.25j, np.complex64)], L, M)[0]
        mid = y[bm.T:len(y) - bm.T]
        dev = float(np.max(np.abs(mid - (0.5 + 0.25j))))
        assert len(mid) > 500 and dev <= 1e-4, (L, M, dev)
        res["%d/%d" % (L, M)] = dict(ripple=ripple, stop=stop, const=dev)
    for L, M in ((4099, 4100), (4097, 4096)):
        try:
            irdm.burst_resample_batch([np.zeros(100, np.complex64)], L, M)
            raise AssertionError("L = %d not refused" % L)
        except RuntimeError:
            pass
    return res


CASES = {"taps": case_taps, "stage": case_stage, "pipeline": case_pipeline, "ongrid": case_ongrid, "modes": case_modes, "group": case_group,
         "refused": case_refused}
