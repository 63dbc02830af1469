"""-m gpu: the pipeline against the oracle at every class of sample rate irdm_create accepts (tests/rates.py), not only at
1 / 2 / 4 / 10 / 12 MHz.  The other rates select code that runs nowhere else: from 16 MHz the band scan declines (128 bands
of 128 bins at 16384 points) and the wave walk of scan_fast.hip is the DEFAULT scan, at 16384 points and max_bursts 320-452;
the any-M decimator runs at odd M, at M that does not divide 16, and at M = 50 .. 90 with a dynamic LDS tile of 64-104 KB,
which depends on hipFuncSetAttribute; K1 and the scans meet burst widths of 28-56 bins.

Everything goes through the C-ABI under tests/parity.py's rules as they are: indices, downmixed samples and hard bits exact,
soft outputs within 1e-4.  No case compares empty lists: each asserts its minimum counts and the scan that ran.
Correctness only: nothing here times the pipeline at these rates."""
import ctypes as C
import functools

import numpy as np
import pytest

import frontend_model as fm
import irdm
import orc
import parity
import rates
import scenes
import siggen

pytestmark = pytest.mark.gpu


def _counts(summary):
    return {k: summary[k] for k in ("bursts", "frames", "demods")}


@functools.lru_cache(maxsize=1)
def _stream(fs):
    """(the rate's stream, the oracle's records on it): the tests of one rate follow each other"""
    iq = rates.stream(fs)
    return iq, orc.run_stream(iq, fs)


@pytest.mark.parametrize("fs", rates.GPU_RATES)
def test_every_rate_whole_and_chunked(fs):
    """six bursts behind the priming frames: the stream whole at pipeline_depth 0 and in four chunks at depth 1"""
    d = rates.describe(fs)
    assert d["supported"]
    iq, ref = _stream(fs)
    got = parity.run_gpu(iq, fs)
    s = parity.compare(got, ref)
    rates.check_counts(s)
    rates.check_scan(got["stats"], fs)
    got = parity.run_gpu(iq, fs, chunks=rates.chunks_of(len(iq), 4), depth=1)
    assert _counts(parity.compare(got, ref)) == _counts(s)
    rates.check_scan(got["stats"], fs)


@pytest.mark.parametrize("fs,fmt", [(fs, fmt) for fs in (6_250_000, 12_500_000, 16_000_000) for fmt in (irdm.FMT_CI8, irdm.FMT_CI16)])
def test_integer_formats(fs, fmt):
    """ci8 and ci16 (the any-M decimator's tile fill converts in its load stage) in four chunks at depth 1"""
    iq, _ = _stream(fs)
    x = siggen.to_ci8(iq) if fmt == irdm.FMT_CI8 else siggen.to_ci16(iq)
    ref = orc.run_stream(x, fs, fmt=fmt)
    got = parity.run_gpu(x, fs, fmt=fmt, chunks=rates.chunks_of(len(iq), 4), depth=1)
    rates.check_counts(parity.compare(got, ref))
    rates.check_scan(got["stats"], fs)


@pytest.mark.parametrize("fs", (6_250_000, 15_360_000, 20_000_000))
def test_any_m_decimator_scalar_order_where_it_is_the_default(fs):
    """fir_order 0 (one accumulator per output, every product and sum rounded: simd_generic.c:86-96) at M = 25, 61 and 80
    against the oracle in that order; the two orders differ in rounding on this scene, so the right one was compared"""
    assert rates.describe(fs)["decimator"] == "any-M" and rates.describe(fs)["decim"] in (25, 61, 80)
    iq, ref = _stream(fs)
    try:
        orc.set_fir_order(0)
        ref0 = orc.run_stream(iq, fs)
    finally:
        orc.set_fir_order(1)
    assert any(a.center_offset != b.center_offset for a, b in zip(ref.frames, ref0.frames)), "the two orders should differ in rounding"
    got = parity.run_gpu(iq, fs, options={"fir_order": 0})
    rates.check_counts(parity.compare(got, ref0))
    rates.check_scan(got["stats"], fs)


# ---- the scan forms at 16384 points ----
def _peak_active(bursts):
    ev = sorted([(b.start, 1) for b in bursts] + [(b.stop, -1) for b in bursts])
    cur = peak = 0
    for _, d in ev:
        cur += d
        peak = max(peak, cur)
    return peak


def test_more_active_bursts_than_the_wave_walk_holds_16mhz():
    """70 carriers at once at 16 MHz (the rate-aware many_active scene): below max_bursts (320), above the wave walk's 64
    lane slots -- the default scan there must give the chunk up (scan_fallbacks) and the records stay exact"""
    fs, iq = scenes.many_active_10m(fs=16_000_000)
    ref = orc.run_stream(iq, fs)
    assert _peak_active(ref.bursts) >= 70 and len(ref.demods) >= 70
    got = parity.run_gpu(iq, fs)
    rates.check_counts(parity.compare(got, ref), min_bursts=70, min_demods=70)
    assert got["stats"]["band_chunks"] == 0 and got["stats"]["scan_fallbacks"] >= 1, got["stats"]
    got = parity.run_gpu(iq, fs, chunks=rates.chunks_of(len(iq), 4), depth=1)
    parity.compare(got, ref)
    assert got["stats"]["band_chunks"] == 0 and got["stats"]["scan_fallbacks"] >= 1, got["stats"]


@pytest.mark.parametrize("fs", (12_500_000, 16_000_000))
@pytest.mark.parametrize("name", ("too_long", "strong_simultaneous"))
def test_scene_zoo_at_16384_points(name, fs):
    """forced burst ends / bursts born and deleted in the same frames, laid out for the rate (scenes._Layout): the band scan
    with 256-bin bands at 12.5 MHz, the wave walk at 16 MHz, whole and in five chunks at depth 1"""
    fs, iq = scenes.ALL[name](fs=fs)
    ref = orc.run_stream(iq, fs)
    got = parity.run_gpu(iq, fs)
    s = parity.compare(got, ref)
    rates.check_counts(s, min_bursts=8, min_demods=3)
    if name == "too_long":
        assert sum(1 for b in ref.bursts if b.stop - b.start > int(0.09 * fs)) >= 2
    rates.check_scan(got["stats"], fs)
    got = parity.run_gpu(iq, fs, chunks=rates.chunks_of(len(iq), 5), depth=1)
    assert _counts(parity.compare(got, ref)) == _counts(s)
    rates.check_scan(got["stats"], fs)


@functools.lru_cache(maxsize=1)
def _random16():
    fs, iq = scenes.random_scene(160, fs=16_000_000, secs=1.0)
    return fs, iq, orc.run_stream(iq, fs)


def test_scan_forms_16mhz_random_scene_and_final_baseline():
    """the dense scan (scan_mode 1) and the wave walk on one workgroup (2) and with updater workgroups (3) at 16 MHz on one
    random scene: each equal to the oracle, and the carried noise-floor sums after the stream bit-identical"""
    fs, iq, ref = _random16()
    assert len(ref.bursts) >= 10 and len(ref.demods) >= 4
    cs = rates.chunks_of(len(iq), 3)
    sums = []
    for mode in (1, 2, 3):
        p = irdm.Pipeline(fs, max_chunk_samples=max(cs), max_bursts_per_chunk=1024, pipeline_depth=1)
        p.set_option("keep_frame_samples", 1)
        p.set_option("scan_mode", mode)
        try:
            off = 0
            for c in cs:
                p.feed_host(iq[off:off + c])
                off += c
            p.flush()
            sums.append(p.baseline_sum().copy())
            infos, samples = p.poll_frames()
            got = dict(bursts=p.poll_bursts(), infos=infos, samples=samples, demods=p.poll_demods(), tagged=p.tagged)
            stats = {k: p.stat(k) for k in ("band_chunks", "scan_fast_chunks", "scan_fallbacks")}
        finally:
            p.close()
        rates.check_counts(parity.compare(got, ref), min_bursts=10)
        rates.check_scan(stats, fs, scan="dense" if mode == 1 else "wave")
    assert sums[0].shape == (16384,) and np.isfinite(sums[0]).all() and (sums[0] > 0).all()
    assert np.array_equal(sums[0].view(np.uint32), sums[1].view(np.uint32))
    assert np.array_equal(sums[0].view(np.uint32), sums[2].view(np.uint32))


def test_wave_walk_where_the_band_scan_is_the_default_12m5():
    """scan_mode 2 at 12.5 MHz (burst width 52 bins)"""
    fs = 12_500_000
    iq, ref = _stream(fs)
    got = parity.run_gpu(iq, fs, chunks=rates.chunks_of(len(iq), 4), depth=1, scan_mode=2)
    rates.check_counts(parity.compare(got, ref))
    rates.check_scan(got["stats"], fs, scan="wave")


# ---- the edges of acceptance ----
SMALL = 4 * 32768


@pytest.mark.parametrize("fs", (725_000, 22_600_000))
def test_create_accepts_the_lowest_and_the_highest_rate(fs):
    p = irdm.Pipeline(fs, max_chunk_samples=SMALL, max_bursts_per_chunk=64)
    try:
        assert p.fft_size == rates.describe(fs)["n"] == (1024 if fs < 1_000_000 else 16384)
    finally:
        p.close()


@pytest.mark.parametrize("fs", (700_000, 23_000_000, 46_000_000))
def test_create_refuses_a_rate_outside_with_the_message(fs, capfd):
    assert not rates.describe(fs)["supported"]
    with pytest.raises(RuntimeError):
        irdm.Pipeline(fs, max_chunk_samples=SMALL, max_bursts_per_chunk=64)
    err = capfd.readouterr().err
    assert "irdm_hip: unsupported sample rate %d (fft_size %d)" % (fs, rates.fft_size(fs)) in err, err


@pytest.mark.parametrize("n", (1024, 2048, 4096, 8192))
def test_fft_size_on_both_sides_of_each_boundary(n):
    """the detector's FFT size changes where fs / 1000 crosses sqrt(2) n: the last rate below and the first above, against
    the oracle's detector"""
    edge = int(np.floor(np.sqrt(2.0) * n * 1000.0))
    L = orc.lib()
    sizes = []
    for fs in (edge, edge + 1):
        det = L.orc_detector_create(1.622e9, fs, 0.0, 0)
        want = L.orc_detector_fft_size(det)
        L.orc_detector_destroy(det)
        p = irdm.Pipeline(fs, max_chunk_samples=SMALL, max_bursts_per_chunk=64)
        try:
            assert p.fft_size == want == rates.fft_size(fs), (fs, p.fft_size, want)
        finally:
            p.close()
        sizes.append(want)
    assert sizes == [n, 2 * n]


# ---- a front end composed with a pipeline whose rate is not 10 MHz ----
@functools.lru_cache(maxsize=1)
def _wideband(which):
    s = {"61.44/6": fm.SCENE_61M44_D6, "50/4": fm.SCENE_50M_D4}[which]
    x, expect, q = fm.wideband_scene(s)
    fe = irdm.Frontend(s["fs_in"], s["fmt"], s["D"], s["shift_hz"])
    taps = fe.taps()
    applied = fe.applied_shift_hz
    out_rate = fe.out_rate
    fe.close()
    assert applied == q * s["fs_in"] / 65536.0 and out_rate == s["fs_in"] // s["D"]
    y = fm.run(x, s["fmt"], s["D"], q, taps)
    ref = orc.run_stream(y, out_rate, center_frequency=1622000000.0 + applied)
    return s, x, expect, y, ref, applied


@pytest.mark.parametrize("which,out_rate", [("61.44/6", 10_240_000), ("50/4", 12_500_000)])
def test_front_end_composed_at_another_output_rate(which, out_rate):
    """61.44 MS/s ci16 by 6 -> 10.24 MHz and 50 MS/s ci8 by 4 -> 12.5 MHz: irdm_frontend_feed_host + flush in front of a cf32
    context at pipeline_depth 3 against the oracle on the model's output (tests/frontend_model.c).  12.5 MHz is a multiple of
    250 kHz: every in-band payload whole, nothing else.  At 10.24 MHz (decimation by 40.96 rounded to 41, -0.098 %: a margin
    nobody has measured) only parity and at least 5 frames"""
    s, x, expect, y, ref, applied = _wideband(which)
    assert s["fs_in"] // s["D"] == out_rate
    chunk = 1 << 20
    n = fm.n_samples(x, s["fmt"])
    got, app = fm.run_composed(x, s["fs_in"], s["fmt"], s["D"], s["shift_hz"], fm.block_feeds(n, s["D"] * chunk), 3, chunk, feed="host")
    assert app == applied
    assert got["n_samples"] == len(y)
    summary = parity.compare(got, ref)
    assert summary["frames"] >= 5 and summary["demods"] >= 5 and summary["bursts"] >= 5, summary
    if out_rate % 250_000 == 0:
        assert summary["demods"] == s["n_inband"], summary
        fm.check_scene_demods(got["demods"], expect)
