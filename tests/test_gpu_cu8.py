"""rtl_sdr's unsigned 8-bit I/Q on the GPU: IRDM_FMT_CU8, (u - 127.5) / 128.

The contract (include/irdm_hip.h): a cu8 context produces exactly the records of a cf32 context fed the converted samples --
bursts, frames with their samples, demods with their LLRs, the packed, parsed and frame records -- bit for bit.  Every K1
family and both decimators, every feed path, the ring wrap, the time-shard hand-off, both front ends, the command line."""
import os
import subprocess

import numpy as np
import pytest

import cu8
import formats16 as f16
import frontend_model as fm
import irdm
import orc
import parity
import resample_model as rm
import sharding
import siggen

pytestmark = pytest.mark.gpu

FMT = irdm.FMT_CU8
EXE = os.path.join(os.path.dirname(irdm.LIB_PATH), "iridium-sniffer-hip")
# rate -> (seconds, bursts): the scene sizes of tests/test_gpu_formats16.py
SCENES = {2_000_000: (1.2, 6), 4_000_000: (1.0, 6), 10_000_000: (0.9, 6), 12_000_000: (0.95, 4)}
_cache = {}


def scene(fs):
    if fs not in _cache:
        secs, nb = SCENES[fs]
        _cache[fs] = cu8.cu8_scene(fs, secs, nb, seed=fs // 1_000_000 + 160)
    return _cache[fs]


def oracle(y, fs, order):
    try:
        orc.set_fir_order(order)
        return orc.run_stream(y, fs)
    finally:
        orc.set_fir_order(1)


@pytest.mark.parametrize("fs,order", [(2_000_000, 1), (4_000_000, 1), (10_000_000, 0), (10_000_000, 1), (12_000_000, 1)])
def test_every_kernel_variant(fs, order):
    """generic K1 + any-M decimator, r16 K1, p32<13> + M = 40 in both orders, p32<14> + M = 48: the cu8 context equals the
    cf32 context on the converted samples bit for bit, and the oracle on them"""
    u = scene(fs)
    y = cu8.converted(u)
    opts = {"fir_order": order}
    got = f16.run(u, fs, FMT, options=opts)
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
    return fs, cu8.to_cu8(iq), sizes


def test_feed_paths():
    """pinned host memory, device-resident chunks, in place (irdm_ingest_ptr) with look-ahead at pipeline_depth 3, and the
    packed / parsed / frame records: a ragged last chunk, bursts across the chunk boundaries"""
    fs, u, sizes = _boundary_scene()
    y = cu8.converted(u)
    ref = orc.run_stream(y, fs)
    cuts = np.cumsum(sizes)[:-1]
    assert sum(any(b.start < c < b.start + b.num_samples for b in ref.bursts) for c in cuts) >= 3
    for feed, depth in (("pinned", 0), ("device", 1), ("ingest_lookahead", 3)):
        got = f16.run(u, fs, FMT, chunks=sizes, depth=depth, feed=feed)
        assert f16.same_records(got, f16.run(y, fs, irdm.FMT_CF32, chunks=sizes, depth=depth, feed=feed)) > 0, feed
        s = parity.compare(got, ref)
        assert s["demods"] >= 8, (feed, s)
    got = f16.run(u, fs, FMT, chunks=sizes, depth=3, feed="ingest_lookahead", packed=True)
    want = f16.run(y, fs, irdm.FMT_CF32, chunks=sizes, depth=3, feed="ingest_lookahead", packed=True)
    assert f16.same_records(got, want) > 0
    assert len(got["packed"]) == len(ref.demods) and len(got["ida"]) == len(got["frame"]) == len(got["packed"])


def test_ring_wrap_10mhz_in_place():
    """10 MHz in 4 Mi-sample chunks written in place at pipeline_depth 3: the history ring wraps, the register-resident
    decimator reads across chunk and ring edges, the stream ends 1234 samples past a feed block"""
    fs = 10_000_000
    n = int(2.6 * fs) // 32768 * 32768 + 1234
    iq, _ = siggen.standard_scene(fs, n, 18, seed=78)
    u = cu8.to_cu8(iq)
    chunk = 4 * 1024 * 1024
    sizes = [chunk] * (n // chunk) + ([n % chunk] if n % chunk else [])
    got = f16.run(u, fs, FMT, chunks=sizes, depth=3, feed="ingest_lookahead")
    assert f16.same_records(got, f16.run(cu8.converted(u), fs, irdm.FMT_CF32, chunks=sizes, depth=3,
                                         feed="ingest_lookahead")) > 0
    assert len(got["demods"]) >= 10


def test_time_shard_handoff():
    """export_state / import_state with the history seeded from a cu8 host buffer (irdm_seed_history, 2 bytes per sample)
    gives the single context's records"""
    fs, nfft = 2_000_000, 2048
    u = scene(fs)
    n = len(u) // 2
    whole = f16.run(u, fs, FMT)
    cut = None
    for b in whole["bursts"]:
        c = (b.start + b.num_samples // 2) // 32768 * 32768
        if b.start < c < b.start + b.num_samples and c > 600 * nfft:
            cut = int(c)
            break
    assert cut is not None
    a = irdm.Pipeline(fs, fmt=FMT, max_chunk_samples=n, max_bursts_per_chunk=1024)
    b = irdm.Pipeline(fs, fmt=FMT, max_chunk_samples=n, max_bursts_per_chunk=1024)
    try:
        assert a.L.irdm_bytes_per_sample(a.h) == 2
        for p in (a, b):
            p.set_option("keep_frame_samples", 1)
        a.feed_host(u[:2 * cut])
        blob = a.export_state()
        ov = min(cut, sharding.required_overlap(fs, nfft))
        b.seed_history(u[2 * (cut - ov):2 * cut], cut)
        b.import_state(blob)
        b.feed_host(u[2 * cut:])
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


@pytest.mark.parametrize("kind", ["k0", "k0r"])
def test_front_ends(kind):
    """2^22 + 12345 cu8 samples through K0 (10 MS/s, D = 5) and K0r (2.4 -> 2.5 MS/s, 25/24), whole and in ragged feeds:
    the band of the cf32 capture of the converted samples, bit for bit"""
    n = (1 << 22) + 12345
    u = np.random.default_rng(6).integers(0, 256, 2 * n, dtype=np.uint8)
    y = cu8.converted(u)
    if kind == "k0":
        make = lambda fmt: fm.Stage(10_000_000, fmt, 5, 14418 * 10_000_000 / 65536.0)      # noqa: E731
        ragged = lambda nt: fm.ragged_feeds(n, nt, (999983, 65537))                          # noqa: E731
    else:
        make = lambda fmt: rm.Stage(2_400_000, fmt, 2_500_000, -9000 * 2_400_000 / 65536.0)  # noqa: E731
        ragged = lambda nt: rm.ragged_feeds(n, nt, 25, (999983, 65537))                      # noqa: E731
    st = make(irdm.FMT_CF32)
    want = st.run(y, [n])
    st.close()
    st = make(FMT)
    nt = st.fe.ntaps
    whole = st.run(u, [n])
    st.close()
    assert len(want) > 0 and fm.same_bits(whole, want)
    st = make(FMT)
    got = st.run(u, ragged(nt))
    st.close()
    assert fm.same_bits(got, want)


def test_create_refuses_5_and_7():
    for fmt in (5, 7, -1):
        with pytest.raises(RuntimeError):
            irdm.Pipeline(2_000_000, fmt=fmt)
        with pytest.raises(RuntimeError):
            irdm.Frontend(10_000_000, fmt, 5)
    p = irdm.Pipeline(2_000_000, fmt=FMT)
    try:
        assert p.L.irdm_bytes_per_sample(p.h) == 2
    finally:
        p.close()


def _cli(path, fs, extra=()):
    r = subprocess.run([EXE, "-f", str(path), "-r", str(fs), "--file-info", "golden", "--chunk", str(32768 * 16)] + list(extra),
                       capture_output=True, text=True, timeout=180)
    assert r.returncode == 0, r.stderr[-2000:]
    tagged = [l for l in r.stderr.splitlines() if "tagged" in l and "bursts total" in l]
    return r.stdout.splitlines(), tagged


def _same_lines(a, b):
    """equal but for the run's time base (tests/test_gpu_formats16.py): timestamps relative to the first line, within 1 ms"""
    assert len(a) == len(b) >= 3
    t0 = None
    for la, lb in zip(a, b):
        ta, tb = la.split(" "), lb.split(" ")
        assert ta[:1] + ta[3:] == tb[:1] + tb[3:], (la, lb)
        assert ta[1] == tb[1], (la, lb)
        if t0 is None:
            t0 = (float(ta[2]), float(tb[2]))
        assert abs((float(ta[2]) - t0[0]) - (float(tb[2]) - t0[1])) <= 1, (la, lb)


def test_cli_cu8(tmp_path):
    """--format cu8 on a file of any name, and a bare .cu8 / .u8 file, print what the converted .cf32 file prints; a .cu8
    file beside a .ci8 file in one batch is refused"""
    fs = 2_000_000
    u = scene(fs)
    path32 = tmp_path / "scene.cf32"
    cu8.converted(u).tofile(path32)
    want, want_tag = _cli(path32, fs)
    assert len(want_tag) == 1 and all(l.startswith("RAW: ") for l in want)
    for name, extra in (("scene.raw", ["--format", "cu8"]), ("scene.cu8", []), ("scene.u8", [])):
        path = tmp_path / name
        u.tofile(path)
        got, got_tag = _cli(path, fs, extra)
        assert got_tag == want_tag, name
        _same_lines(got, want)
    other = tmp_path / "other.ci8"
    u.tofile(other)
    r = subprocess.run([EXE, "-f", str(tmp_path / "scene.cu8"), "-f", str(other), "-r", str(fs)], capture_output=True, timeout=120)
    assert r.returncode == 2 and r.stdout == b"" and b"different sample formats" in r.stderr


def test_cli_rtl_sdr_recording(tmp_path):
    """rtl_sdr -s 2400000 -f 1625500000 x.cu8, then -f x.cu8 -r 2400000 -c 1625500000 --resample-to 2500000 --input-stats:
    the eight payloads of the 2.4 -> 2.5 MS/s scene (tests/resample_model.py), every one whole as the leading bits of a
    frame, as tests/test_resample_emul.py asks of the 8-bit rendering of that scene; and the input line.  (Quantised to 8
    bits at scale 512 the scene's noise is one LSB rms; on the MI355X this run tagged 16 bursts and printed 16 frames for
    the eight transmissions, so the count of frames is printed, not pinned.  The cu8 context equals the cf32 context on the
    converted samples bit for bit -- test_every_kernel_variant --, so whatever the detector makes of this scene is a
    property of the quantised samples, not of the format.)"""
    s = rm.SCENES["2.4->2.5"]
    iq, expect = rm.offgrid_scene("2.4->2.5")
    u = cu8.to_cu8(iq)
    path = tmp_path / "x.cu8"
    u.tofile(path)
    r = subprocess.run([EXE, "-f", str(path), "-r", str(s["in_rate"]), "-c", "1625500000", "--resample-to", str(s["out_rate"]),
                        "--input-stats"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    bits = [l.split(" ")[-1] for l in r.stdout.splitlines() if l.startswith("RAW: ")]
    print("rtl_sdr scene: %d frames; frames per payload %s" % (len(bits), [sum(b.startswith("".join(str(v) for v in e)) for b in bits)
                                                                       for e in expect]))
    assert len(expect) == 8 and len(bits) >= 8, (len(bits), r.stderr[-1000:])
    for e in expect:
        assert sum(b.startswith("".join(str(v) for v in e)) for b in bits) >= 1
    line = [l for l in r.stderr.splitlines() if l.startswith("input: ")]
    assert len(line) == 1 and line[0].startswith("input: %d samples cu8; I dc " % (len(u) // 2)), r.stderr[-1000:]
