"""The input statistics on the GPU (csrc/input_stats.hpp): irdm_input_stats_device against the integer / fsum model of
tests/inputstats_model.py; the context option at pipeline_depth 0 and 3 with in-place look-ahead, records untouched by it,
irdm_reset; the front end's getter; the result rings of input_stats, iq_moments and scrub (csrc/pass_ring.hpp) taken round
more than twice without a read; --input-stats and --diagnostic."""
import os
import re
import subprocess

import numpy as np
import pytest

import balance_checks as bc
import balance_model as bm
import cu8
import formats16 as f16
import input_stats_checks as ic
import inputstats_model as im
import irdm
import scrub_checks as sc
import scrub_model as sm
import siggen

pytestmark = pytest.mark.gpu

EXE = os.path.join(os.path.dirname(irdm.LIB_PATH), "iridium-sniffer-hip")


def test_stage_level_equals_the_model():
    """every format, n in {0, 1, 3, 63, 64, 65, 255, 4101, 2^20 + 7}, bases 0 / 1 / 3 samples past a 16-byte boundary, rails
    at the first and last sample, all-rail buffers (int16: the sum of squares 2^50), cf32 with NaN, Inf, +-1.0, subnormals"""
    assert ic.stage_cases()["cases"] >= 6 * 9 * 3 + 6 + 10


@pytest.fixture(scope="module")
def scene():
    fs, u = ic.context_scene()
    return fs, u, im.model(u, irdm.FMT_CU8)


@pytest.mark.parametrize("depth,feed", [(0, "host"), (3, "ingest_lookahead")])
def test_context_option(scene, depth, feed):
    """the option over the 2 MHz cu8 scene in five chunks: the model's struct; the records with the option on equal the
    records with it off, bit for bit; irdm_reset starts the statistics over"""
    fs, u, want = scene
    sizes = f16.chunks_of(len(u) // 2, 5)
    st, on = ic.context_run(u, fs, irdm.FMT_CU8, sizes, depth, feed, reset_first=True)
    im.check(st, want, irdm.FMT_CU8, "depth %d" % depth)
    _, off = ic.context_run(u, fs, irdm.FMT_CU8, sizes, depth, feed, stats=False)
    assert f16.same_records(on, off) > 0 and len(on["demods"]) >= 3


def test_context_cuts_and_cf32(scene):
    """whole, four chunks, ragged pieces: byte-identical structs; a cf32 context on the converted samples: the cf32 model"""
    ic.context_cuts()
    fs, u, _ = scene
    y = cu8.converted(u)
    st, _ = ic.context_run(y, fs, irdm.FMT_CF32, f16.chunks_of(len(y), 4), 1)
    im.check(st, im.model(y, irdm.FMT_CF32), irdm.FMT_CF32, "cf32 context")


def test_frontend_getter():
    ic.frontend_cuts((1 << 20) + 4321)


# ---------------------------------------------------------------- the result ring, more than two turns ----
RING_CHUNKS, RING_CHUNK = 11, 4099          # four slots: the eleventh launch takes slot 2 for the third time


def ring_cf32(sizes):
    """noise in the given cuts with a handful of bad samples in chunks 0, 5 and 10 -- in the vector part and, where the cut
    has one, on its tail sample --, as interleaved floats; with it what option scrub leaves of it and the figures"""
    n = sum(sizes)
    x = (0.3 * np.random.default_rng(411).standard_normal(2 * n)).astype(np.float32)
    starts = np.concatenate(([0], np.cumsum(sizes)))
    for c in (0, 5, 10):
        s, last = int(starts[c]), int(starts[c + 1]) - 1
        x[2 * s] = np.float32("nan")                                   # I of the chunk's first sample
        x[2 * (s + 7) + 1] = np.float32("inf")                         # Q inside a piece
        x[2 * (s + 1026)], x[2 * (s + 1026) + 1] = np.float32("-inf"), np.float32("nan")
        x[2 * last] = np.float32(1e30)                                 # finite, over the limit: the chunk's last sample
    y, fig = sm.scrub(x, 40)
    assert (fig["n_zeroed"], fig["n_nonfinite"], fig["n_over"], fig["first"], fig["last"]) == (12, 12, 3, 0, n - 1)
    return x, y, fig


def check_ring_records(scrub_st, stats_st, moments_st, y, fig, where):
    """the three records, read once, against the models over what the passes behind the scrub saw"""
    n = len(y) // 2
    assert (int(scrub_st.n_samples), scrub_st.limit_log2, scrub_st.active) == (n, 40, 1), where
    assert sc.stat_tuple(scrub_st) == tuple(fig[f] for f in sc.FIGURES), (where, sc.stat_tuple(scrub_st), fig)
    im.check(stats_st, im.model(y.view(np.complex64), irdm.FMT_CF32), irdm.FMT_CF32, where)
    assert list(stats_st.n_nonfinite) == [0, 0], where
    bc.check_moments(moments_st, bm.moments(y), where)
    assert int(moments_st.n_used) == n, where


def test_ring_reuse_context():
    """one cf32 context with scrub, input_stats and iq_moments on, eleven chunks through irdm_feed_host, no figure read in
    between: every slot of the three rings is taken again while its previous launch may still be in flight, and the
    records read at the end are the models'.  (A context's stream takes whole feed blocks until its last chunk: ten chunks
    of two 2048-sample blocks, then one of 4099 samples with a tail behind its last 16-byte piece.)"""
    sizes = [4096] * (RING_CHUNKS - 1) + [RING_CHUNK]
    x, y, fig = ring_cf32(sizes)
    p = irdm.Pipeline(2_000_000, fmt=irdm.FMT_CF32, feed_block=2048, max_chunk_samples=3 * 2048, max_bursts_per_chunk=256)
    try:
        for opt in ("scrub", "input_stats", "iq_moments"):
            p.set_option(opt, 1)
        c, off = x.view(np.complex64), 0
        for s in sizes:
            p.feed_host(np.ascontiguousarray(c[off:off + s]))
            off += s
        check_ring_records(p.scrub_stats(), p.input_stats(), p.iq_moments(), y, fig, "context")
    finally:
        p.close()


def ring_front_end(fmt, scrub):
    fe = irdm.Frontend(10_000_000, fmt, 5, 1_000_000.0)
    p = irdm.Pipeline(fe.out_rate, fmt=irdm.FMT_CF32, max_chunk_samples=1 << 18, max_bursts_per_chunk=256)
    fe.input_stats_enable(True)
    fe.iq_moments_enable(True)
    if scrub:
        fe.scrub(True)
    return fe, p


def test_ring_reuse_front_end_cf32():
    """the same through a cf32 front end, which takes any cut: eleven chunks of 4099 samples through
    irdm_frontend_feed_host, every launch of the three passes with a vector part and a tail"""
    sizes = [RING_CHUNK] * RING_CHUNKS
    x, y, fig = ring_cf32(sizes)
    fe, p = ring_front_end(irdm.FMT_CF32, True)
    try:
        c = x.view(np.complex64)
        for k in range(RING_CHUNKS):
            fe.feed_host(p, c[k * RING_CHUNK:(k + 1) * RING_CHUNK])
        check_ring_records(fe.scrub_stats(), fe.input_stats(), fe.iq_moments(), y, fig, "cf32 front end")
    finally:
        p.close()
        fe.close()


def test_ring_reuse_front_end_ci16():
    """the two statistics over a ci16 capture in eleven chunks of 4099 samples (1024 pieces and three samples behind them):
    the integer record exactly the model's, the moments within the bound of any order of addition"""
    n = RING_CHUNKS * RING_CHUNK
    v = im.with_rails_at_the_ends(im.random_input(irdm.FMT_CI16, n, seed=412), irdm.FMT_CI16)
    fe, p = ring_front_end(irdm.FMT_CI16, False)
    try:
        for k in range(RING_CHUNKS):
            fe.feed_host(p, v[2 * k * RING_CHUNK:2 * (k + 1) * RING_CHUNK])
        stats_st, moments_st = fe.input_stats(), fe.iq_moments()
    finally:
        p.close()
        fe.close()
    im.check(stats_st, im.model(v, irdm.FMT_CI16), irdm.FMT_CI16, "ci16 front end")
    bc.check_moments(moments_st, bm.moments(bm.convert(v, irdm.FMT_CI16)), "ci16 front end")
    assert int(moments_st.n_used) == n


def clipped_scene():
    """the 2 MHz scene quantised with a scale at which the bursts clip: their components reach 0.018, 295 LSB at scale
    16384 against the converter's 127.5 (the noise is 33 LSB rms); the oracle still decodes 6 of 6 frames"""
    fs = 2_000_000
    n = int(1.2 * fs) // 32768 * 32768
    iq, _ = siggen.standard_scene(fs, n, 6, seed=162)
    return fs, cu8.to_cu8(iq, 16384.0)


INPUT_RE = re.compile(r"^input: (\d+) samples (\S+); I dc ([-+][\d.]+) rms (\S+) dBFS peak (\S+) dBFS rails (\d+) \(([\d.]+)%\); "
                      r"Q dc ([-+][\d.]+) rms (\S+) dBFS peak (\S+) dBFS rails (\d+) \(([\d.]+)%\); nonfinite (\d+)$")
RUNTIME_RE = re.compile(r"^Runtime: (\d\d):(\d\d):(\d\d)  \|  Bursts: (\d+) detected \(([\d.]+)/min\)  \|  Decoded: (\d+) \(ok_avg: (\d+)%\)  \|  "
                        r"Noise: (-?[\d.]+) dBFS/Hz  \|  Peak: (-?[\d.]+) dB  (\| .*)?$")


def check_input_line(line, m, name):
    g = INPUT_RE.match(line)
    assert g, line
    n = m["n_samples"]
    assert int(g.group(1)) == n and g.group(2) == name and int(g.group(13)) == sum(m["n_nonfinite"])
    for k in range(2):
        dc, rms, peak, rails, pct = g.groups()[2 + 5 * k:7 + 5 * k]
        assert dc == "%+.5f" % (m["sum"][k] / n)
        assert rms == "%.2f" % (10.0 * np.log10(m["sum_sq"][k] / n))
        assert peak == "%.2f" % (20.0 * np.log10(float(m["abs_max"][k])))
        assert int(rails) == m["n_rail_lo"][k] + m["n_rail_hi"][k]
        assert pct == "%.4f" % (100.0 * int(rails) / n)


def test_cli_lines(tmp_path):
    """--input-stats: stdout and the rest of stderr those of the run without it, the input line the model's numbers -- on a
    scene whose bursts clip, the model's rail counts exactly.  --diagnostic: stdout empty, the input line, the Runtime line
    over the stream time with the bursts tagged and the frames the plain run printed"""
    fs, u = clipped_scene()
    m = im.model(u, irdm.FMT_CU8)
    assert m["n_rail_lo"][0] + m["n_rail_hi"][0] > 100 and m["n_rail_lo"][1] + m["n_rail_hi"][1] > 100
    path = tmp_path / "clip.cu8"
    u.tofile(path)
    common = [EXE, "-f", str(path), "-r", str(fs), "--start-time", "1700000000", "--file-info", "is"]
    plain = subprocess.run(common, capture_output=True, text=True, timeout=180)
    stats = subprocess.run(common + ["--input-stats"], capture_output=True, text=True, timeout=180)
    diag = subprocess.run(common + ["--diagnostic"], capture_output=True, text=True, timeout=180)
    assert plain.returncode == stats.returncode == diag.returncode == 0, (plain.stderr, stats.stderr, diag.stderr)
    assert stats.stdout == plain.stdout and plain.stdout.count("RAW: ") >= 3
    pl, sl, dl = (r.stderr.splitlines() for r in (plain, stats, diag))
    assert sl[:-1] == pl and pl[-1].startswith("burst_detect: tagged ")
    check_input_line(sl[-1], m, "cu8")
    assert diag.stdout == "" and dl[:-2] == pl and dl[-2] == sl[-1]
    g = RUNTIME_RE.match(dl[-1])
    assert g, dl[-1]
    secs = int(len(u) // 2 / fs)
    tagged = int(pl[-1].split()[2])
    frames = plain.stdout.count("RAW: ")
    assert (int(g.group(1)), int(g.group(2)), int(g.group(3))) == (0, 0, secs)
    assert int(g.group(4)) == tagged and int(g.group(6)) == frames
    assert g.group(5) == "%.1f" % (tagged * 60.0 / (len(u) // 2 / fs)) and g.group(7) == "%.0f" % (100.0 * frames / tagged)
    assert -200.0 < float(g.group(8)) < 0.0 and float(g.group(9)) > 0.0


def test_cli_behind_a_front_end_and_save_only(tmp_path):
    """behind --resample-to the line describes the capture; --save-only gives the same line without a context; --gpus 2
    is refused (exit 2)"""
    fs, u = clipped_scene()
    u = u[:2 * 700_000]
    m = im.model(u, irdm.FMT_CU8)
    path = tmp_path / "cap.cu8"
    u.tofile(path)
    common = [EXE, "-f", str(path), "-r", "2400000", "--resample-to", "2500000", "--input-stats"]
    a = subprocess.run(common, capture_output=True, text=True, timeout=180)
    b = subprocess.run(common + ["--save-band", str(tmp_path / "band.ci8"), "--save-only"], capture_output=True, text=True, timeout=180)
    assert a.returncode == 0 and b.returncode == 0, (a.stderr, b.stderr)
    for r in (a, b):
        line = [l for l in r.stderr.splitlines() if l.startswith("input: ")]
        assert len(line) == 1
        check_input_line(line[0], m, "cu8")
    assert b.stdout == ""
    for flag in ("--input-stats", "--diagnostic"):
        r = subprocess.run([EXE, "-f", str(path), "-r", "2000000", flag, "--gpus", "2"], capture_output=True, timeout=60)
        assert r.returncode == 2 and r.stdout == b""
