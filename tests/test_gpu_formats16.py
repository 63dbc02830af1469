"""Full-precision 16-bit IQ input: IRDM_FMT_CI16_FULL (SoapySDR CS16, v / 32768) and IRDM_FMT_SC16Q11 (bladeRF, v / 2048).

The contract (include/irdm_hip.h): a context in either format produces exactly the records of a cf32 context fed
v.astype(np.float32) * scale -- bursts, frames with their samples, demods with their LLRs, the packed, parsed and frame
records -- bit for bit.  Every K1 family and both decimators, every feed path, the time-shard hand-off, the CLI; and what
the formats are for: a bladeRF-range recording that the ci16 narrowing (main.c:245-246) damages decodes in full."""
import os
import subprocess

import numpy as np
import pytest

import formats16 as f16
import irdm
import orc
import parity
import sharding
import siggen

pytestmark = pytest.mark.gpu

# rate -> (seconds, bursts): 2 MHz generic K1 + any-M decimator; 4 MHz r16 K1 + any-M decimator; 10 MHz p32<13> + M = 40;
# 12 MHz p32<14> + M = 48
SCENES = {2_000_000: (1.2, 6), 4_000_000: (1.0, 6), 10_000_000: (0.9, 6), 12_000_000: (0.95, 4)}
_cache = {}


def scene(fs):
    if fs not in _cache:
        secs, nb = SCENES[fs]
        _cache[fs] = f16.int16_scene(fs, secs, nb, seed=fs // 1_000_000 + 160)
    return _cache[fs]


def oracle(y, fs, order):
    try:
        orc.set_fir_order(order)
        return orc.run_stream(y, fs)
    finally:
        orc.set_fir_order(1)


@pytest.mark.parametrize("fmt", f16.FORMATS, ids=lambda f: f16.NAMES[f])
@pytest.mark.parametrize("fs,order", [(2_000_000, 1), (4_000_000, 1), (10_000_000, 0), (10_000_000, 1), (12_000_000, 1)])
def test_every_kernel_variant(fs, order, fmt):
    """the int16 context equals the cf32 context on the converted samples bit for bit, and the oracle on them"""
    x = scene(fs)
    y = f16.converted(x, fmt)
    opts = {"fir_order": order}
    got = f16.run(x, fs, fmt, options=opts)
    assert f16.same_records(got, f16.run(y, fs, irdm.FMT_CF32, options=opts)) > 0
    s = parity.compare(got, oracle(y, fs, order))
    assert s["demods"] >= 3, s


def _boundary_scene():
    """2 MHz, 1.6 s, a burst across every chunk boundary of chunks_of(n, 5), the stream ending 777 samples past a block"""
    fs, nfft = 2_000_000, 2048
    n = int(1.6 * fs) // 32768 * 32768 - 32768 + 777
    sizes = f16.chunks_of(n, 5)
    rng = np.random.default_rng(61)
    bursts = [dict(start=int(s), freq_hz=siggen.channel_freq(int(rng.integers(-20, 21)) or 1),
                   payload=rng.integers(0, 4, int(rng.integers(119, 180))).tolist())
              for s in np.sort(rng.integers(520 * nfft, n - int(0.05 * fs), 6))]
    for b in np.cumsum(sizes)[:-1]:
        bursts.append(dict(start=int(b) - 9000, freq_hz=siggen.channel_freq(int(rng.integers(-20, 21)) or 2),
                           payload=rng.integers(0, 4, 170).tolist()))
    iq, _ = siggen.make_stream(fs, n, bursts, seed=61)
    return fs, siggen.to_ci16(iq), sizes


@pytest.mark.parametrize("fmt", f16.FORMATS, ids=lambda f: f16.NAMES[f])
def test_feed_paths(fmt):
    """pinned host memory, device-resident chunks, in place (irdm_ingest_ptr) with look-ahead at pipeline_depth 3, and the
    packed / parsed / frame records: a ragged last chunk, bursts across the chunk boundaries"""
    fs, x, sizes = _boundary_scene()
    y = f16.converted(x, fmt)
    ref = orc.run_stream(y, fs)
    cuts = np.cumsum(sizes)[:-1]
    assert sum(any(b.start < c < b.start + b.num_samples for b in ref.bursts) for c in cuts) >= 3
    for feed, depth in (("pinned", 0), ("device", 1), ("ingest_lookahead", 3)):
        got = f16.run(x, fs, fmt, chunks=sizes, depth=depth, feed=feed)
        assert f16.same_records(got, f16.run(y, fs, irdm.FMT_CF32, chunks=sizes, depth=depth, feed=feed)) > 0, feed
        s = parity.compare(got, ref)
        assert s["demods"] >= 8, (feed, s)
    got = f16.run(x, fs, fmt, chunks=sizes, depth=3, feed="ingest_lookahead", packed=True)
    want = f16.run(y, fs, irdm.FMT_CF32, chunks=sizes, depth=3, feed="ingest_lookahead", packed=True)
    assert f16.same_records(got, want) > 0
    assert len(got["packed"]) == len(ref.demods) and len(got["ida"]) == len(got["frame"]) == len(got["packed"])


@pytest.mark.parametrize("fmt", f16.FORMATS, ids=lambda f: f16.NAMES[f])
def test_ring_wrap_10mhz_in_place(fmt):
    """10 MHz in 4 Mi-sample chunks written in place at pipeline_depth 3: the history ring wraps, the register-resident
    decimator reads across chunk and ring edges, the stream ends 1234 samples past a feed block"""
    fs = 10_000_000
    n = int(2.6 * fs) // 32768 * 32768 + 1234
    iq, _ = siggen.standard_scene(fs, n, 18, seed=78)
    x = siggen.to_ci16(iq)
    chunk = 4 * 1024 * 1024
    sizes = [chunk] * (n // chunk) + ([n % chunk] if n % chunk else [])
    got = f16.run(x, fs, fmt, chunks=sizes, depth=3, feed="ingest_lookahead")
    assert f16.same_records(got, f16.run(f16.converted(x, fmt), fs, irdm.FMT_CF32, chunks=sizes, depth=3,
                                         feed="ingest_lookahead")) > 0
    assert len(got["demods"]) >= 10


@pytest.mark.parametrize("fmt", f16.FORMATS, ids=lambda f: f16.NAMES[f])
def test_time_shard_handoff(fmt):
    """export_state / import_state with the history seeded from an int16 host buffer (irdm_seed_history, 4 bytes per
    sample) gives the single context's records"""
    fs, nfft = 2_000_000, 2048
    x = scene(fs)
    n = len(x) // 2
    whole = f16.run(x, fs, fmt)
    cut = None
    for b in whole["bursts"]:
        c = (b.start + b.num_samples // 2) // 32768 * 32768
        if b.start < c < b.start + b.num_samples and c > 600 * nfft:
            cut = int(c)
            break
    assert cut is not None
    a = irdm.Pipeline(fs, fmt=fmt, max_chunk_samples=n, max_bursts_per_chunk=1024)
    b = irdm.Pipeline(fs, fmt=fmt, max_chunk_samples=n, max_bursts_per_chunk=1024)
    try:
        assert a.L.irdm_bytes_per_sample(a.h) == 4
        for p in (a, b):
            p.set_option("keep_frame_samples", 1)
        a.feed_host(x[:2 * cut])
        blob = a.export_state()
        ov = min(cut, sharding.required_overlap(fs, nfft))
        b.seed_history(x[2 * (cut - ov):2 * cut], cut)
        b.import_state(blob)
        b.feed_host(x[2 * cut:])
        got = dict(tagged=b.tagged, n_samples=b.sample_count, bursts=a.poll_bursts() + b.poll_bursts())
        ia, sa = a.poll_frames()
        ib, sb = b.poll_frames()
        got["infos"], got["samples"] = ia + ib, sa + sb
        got["demods"] = a.poll_demods() + b.poll_demods()
    finally:
        a.close()
        b.close()
    assert any(bb.start < cut < bb.start + bb.num_samples for bb in got["bursts"])
    assert f16.same_records(got, whole) > 0


def bladerf_scene(seed=1, nb=10, amp=0.006, sigma_lsb=3.0):
    """2 MHz SC16Q11-range recording: noise of 3 LSB rms per component, bursts of ~12 LSB -- a few dB above the detection
    threshold, where the ci16 narrowing (v >> 8 leaves the noise at 0 / -1 and the bursts at a bit or two) costs frames"""
    fs, nfft = 2_000_000, 2048
    first = 520 * nfft + 5000
    slot = int(0.1 * fs)
    n = (first + nb * slot + int(0.05 * fs)) // 32768 * 32768 + 32768
    rng = np.random.default_rng(seed)
    bursts = [dict(start=first + k * slot + int(rng.integers(0, 20000)),
                   freq_hz=siggen.channel_freq(int(rng.integers(-20, 21)) or 1),
                   payload=rng.integers(0, 4, int(rng.integers(119, 180))).tolist(), amp=amp) for k in range(nb)]
    iq, _ = siggen.make_stream(fs, n, bursts, noise_sigma=sigma_lsb / 2048.0, seed=seed)
    v = np.empty(2 * n, np.float32)
    v[0::2], v[1::2] = iq.real, iq.imag
    return fs, np.clip(np.round(v * 2048.0), -2048, 2047).astype(np.int16)


def test_sc16q11_decodes_what_the_narrowing_loses():
    fs, x = bladerf_scene()
    assert np.abs(x).max() <= 2048
    y = f16.converted(x, irdm.FMT_SC16Q11)
    ref = orc.run_stream(y, fs)
    got = f16.run(x, fs, irdm.FMT_SC16Q11)
    s = parity.compare(got, ref)
    assert s["demods"] >= 5, s
    narrowed = f16.run(x, fs, irdm.FMT_CI16)
    assert len(narrowed["demods"]) < len(got["demods"]), (len(narrowed["demods"]), len(got["demods"]))


def test_create_refuses_unknown_formats():
    for fmt in (5, -1):
        with pytest.raises(RuntimeError):
            irdm.Pipeline(2_000_000, fmt=fmt)
    for fmt in f16.FORMATS:
        p = irdm.Pipeline(2_000_000, fmt=fmt)
        try:
            assert p.L.irdm_bytes_per_sample(p.h) == 4
        finally:
            p.close()


def _cli(exe, path, fs, extra=()):
    r = subprocess.run([exe, "-f", str(path), "-r", str(fs), "--file-info", "golden", "--chunk", str(32768 * 16)] + list(extra),
                       capture_output=True, text=True, timeout=180)
    assert r.returncode == 0, r.stderr[-2000:]
    tagged = [l for l in r.stderr.splitlines() if "tagged" in l and "bursts total" in l]
    return r.stdout.splitlines(), tagged


def _same_lines(a, b):
    """equal but for the run's time base: the timestamps follow the run's start time, so they are compared relative to the
    first RAW line, to within 1 ms (and --parsed names the run p-<t0>)"""
    assert len(a) == len(b) >= 3
    t0 = None
    for la, lb in zip(a, b):
        ta, tb = la.split(" "), lb.split(" ")
        assert ta[:1] + ta[3:] == tb[:1] + tb[3:], (la, lb)
        if ta[0] == "RAW:":
            assert ta[1] == tb[1], (la, lb)
            if t0 is None:
                t0 = (float(ta[2]), float(tb[2]))
            assert abs((float(ta[2]) - t0[0]) - (float(tb[2]) - t0[1])) <= 1, (la, lb)


def test_cli_formats(tmp_path):
    """--format ci16-full / sc16q11 on an int16 file print what the binary prints for the converted .cf32 file"""
    exe = os.path.join(os.path.dirname(irdm.LIB_PATH), "iridium-sniffer-hip")
    if not os.path.exists(exe):
        irdm.build(force=True)
    fs = 2_000_000
    x = scene(fs)
    path16 = tmp_path / "scene.raw16"
    x.tofile(path16)
    for fmt in f16.FORMATS:
        path32 = tmp_path / ("scene_%d.cf32" % fmt)
        f16.converted(x, fmt).tofile(path32)
        want, want_tag = _cli(exe, path32, fs)
        got, got_tag = _cli(exe, path16, fs, ["--format", f16.NAMES[fmt]])
        assert got_tag == want_tag and len(want_tag) == 1
        assert all(l.startswith("RAW: ") for l in got)
        _same_lines(got, want)
    want, _ = _cli(exe, tmp_path / ("scene_%d.cf32" % irdm.FMT_SC16Q11), fs, ["--parsed"])
    got, _ = _cli(exe, path16, fs, ["--format", "sc16q11", "--parsed"])
    _same_lines(got, want)
