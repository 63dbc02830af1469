"""A receiver's DC offset on the GPU: the kernels of csrc/dc_block.hpp against the numpy model of tests/dc_model.py through
irdm_dc_block_device, and irdm_dc_block through irdm_feed_host on a stream with a DC of 0.03 (1 + 0.6j) planted, at
pipeline_depth 0 and 3; irdm_frontend_dc_block in front of a decimating front end that saves its band; and the binary's
--dc-block."""
import functools
import os
import subprocess

import numpy as np
import pytest

import balance_model as bm
import dc_checks as dc
import dc_model as dm
import irdm
import siggen

pytestmark = pytest.mark.gpu

EXE = os.path.join(os.path.dirname(irdm.LIB_PATH), "iridium-sniffer-hip")

# (the grid is capped at 2048 workgroups of 256 lanes: with this many 16-byte pieces some lanes take a second one)
BIG = 2048 * 256


def test_dc_kernels_equal_the_model():
    """all eight formats, n in 0 .. 5, 255 .. 257, 4095 .. 4097, 65536 + 3 and 2048 x 256 pieces + 777 samples, src and dst 0 and
    1 sample behind a 16-byte boundary, blocks of 4096 with an edge at sample 1, inside a 16-byte piece, at a wavefront's and
    at a workgroup's edge, a seed and the sums of a block under way; cf32 with quiet and signalling NaN, +-Inf, +-1e30, +-64
    and the floats beside them, -0.0 and subnormals: output bytes, guard bytes and state_io exact; a second call gives the
    same bytes; the 8-byte formats in place"""
    res = dc.kernel_cases(extra_pieces=(BIG,))
    assert res["cases"] == 8 * 13 * 4 + 8 and res["again"] == 8 * 4 * 4 + 8 and res["in_place"] == 3 * (13 * 4 + 1), res


def test_dc_refusals_and_host_mean():
    """an unknown format, a block length outside 12 .. 24, misaligned pointers, overlapping buffers, a mean that is not finite
    or beyond +-64: -1, nothing written; irdm_dc_mean_host equals the model for every format"""
    assert dc.refusal_cases() == 8


def test_dc_carry():
    """one stream cut into calls of 1, 4095, 4097 and 100 003 samples gives the bytes and the final state of a single call"""
    assert dc.carry_case()["streams"] == 4


@pytest.mark.parametrize("depth", (0, 3))
def test_pipeline_with_dc_block_equals_the_corrected_stream(depth):
    """a context with irdm_dc_block (blocks of 2^16) fed the impaired stream in chunks of 262 144 and again of 98 304 samples
    yields the records of a plain context fed dc_model(stream), bit for bit and alike for both chunkings, and agrees with
    the oracle on that stream; irdm_dc_stats equals the model's figures; irdm_reset clears the stream state and keeps the
    setting; the refusals"""
    res = dc.pipeline_case(depth)
    assert res["demods"] >= 12, res


@pytest.mark.parametrize("depth", (0, 3))
def test_pipeline_with_dc_block_from_ci16_full(depth):
    """the ci16-full rendering of the impaired stream as wire format, against a plain cf32 context fed the model's correction
    of its conversion: every record queue bit for bit, the figures the model's"""
    assert dc.wire_case(depth)["demods"] >= 12


@pytest.mark.parametrize("depth", (0, 3))
def test_composition_with_swap_and_balance(depth):
    """swap_iq, irdm_dc_block and irdm_iq_balance on one context: the records of balance(dc_model(swap(x)))"""
    assert dc.composition_case(depth)["bursts"] >= 12


# ---------------------------------------------------------------- the front end ----
FE = dict(fs_in=10_000_000, D=5, shift_hz=1_500_000.0)
FE_CHUNK = 1 << 18
FE_LOG2 = 16


@functools.lru_cache(maxsize=None)
def capture():
    """a 10 MS/s cf32 capture of about 0.1 s with a DC of 0.03 (1 + 0.6j), the band 1.5 MHz above its centre selected at
    D = 5: what the decimator leaves of the tone is aliased to 0.5 MHz above the band's centre, and one of the two bursts sits on
    that channel (12 x 41.667 kHz; the capture is shorter than the detector's 512-frame history, so the band is what is judged).  As interleaved floats, its ci16-full rendering, and the model's corrections of both, seeded
    from their own heads, with the model's figures"""
    fs = FE["fs_in"]
    fe = irdm.Frontend(fs, irdm.FMT_CF32, FE["D"], FE["shift_hz"])
    applied = fe.applied_shift_hz
    fe.close()
    bursts = [dict(start=int((0.03 + 0.03 * k) * fs), freq_hz=applied + siggen.channel_freq(12 - 19 * k), payload=[k, 1, 2, 3] * 40, amp=0.05)
              for k in range(2)]
    n = 4 * FE_CHUNK - 32768 + 4321
    x = dc.as_floats(siggen.make_stream(fs, n, bursts, seed=57)[0]).copy()
    x[0::2] += np.float32(dc.D)
    x[1::2] += np.float32(0.6 * dc.D)
    x16 = np.clip(np.round(x * np.float32(32768.0)), -32768, 32767).astype(np.int16)
    c16 = bm.convert(x16, irdm.FMT_CI16_FULL)
    seed, seed16 = dm.head_mean(x, 1 << FE_LOG2), dm.head_mean(c16, 1 << FE_LOG2)
    return x, dm.dc_model(x, FE_LOG2, seed), x16, dm.dc_model(c16, FE_LOG2, seed16), n, seed, seed16


def front_end_run(x, wire, seed, depth, after=None):
    """a capture (interleaved floats, or int16 codes with wire = ci16-full) through a cf32 front end, feed_host in chunks of
    262 144 capture samples, the band saved as cf32"""
    fe = irdm.Frontend(FE["fs_in"], irdm.FMT_CF32, FE["D"], FE["shift_hz"])
    p = irdm.Pipeline(fe.out_rate, fmt=irdm.FMT_CF32, center_frequency=1622000000.0 + fe.applied_shift_hz,
                      max_chunk_samples=1 << 18, max_bursts_per_chunk=256, pipeline_depth=depth)
    try:
        fe.save(irdm.FMT_CF32)
        if wire is not None:
            fe.dc_block(wire, FE_LOG2, seed)
        for off in range(0, len(x), 2 * FE_CHUNK):
            piece = x[off:off + 2 * FE_CHUNK]
            fe.feed_host(p, piece.view(np.complex64) if piece.dtype == np.float32 else piece)
        st = dc.stats_tuple(fe.dc_stats()) if wire is not None else None
        if after:
            after(fe, p)
        fe.flush(p)
        return dict(band=b"".join(fe.saved), n_out=p.sample_count, st=st)
    finally:
        p.close()
        fe.close()


@pytest.mark.parametrize("depth", (0, 3))
def test_front_end_dc_block(depth):
    """irdm_frontend_dc_block on the capture with DC, cf32 and ci16-full wire formats: the band irdm_frontend_save writes is
    byte for byte the band of the model-corrected capture and differs from the uncorrected one; irdm_frontend_dc_stats
    equals the model's figures on the capture; a device feed and a change in mid-capture are refused"""
    x, (y, fig), x16, (y16, fig16), n, seed, seed16 = capture()
    seen = {}

    def refusals(fe, p):
        L = irdm.lib()
        d = irdm.device_buffer(np.zeros(2 * 4096, np.float32))
        try:
            assert L.irdm_frontend_feed_device(fe.h, p.h, d, 4096, None) == -1
            assert L.irdm_frontend_dc_block(fe.h, irdm.FMT_CF32, FE_LOG2, 0.0, 0.0) == -1
            assert L.irdm_frontend_dc_block(fe.h, irdm.FMT_CF32, -1, 0.0, 0.0) == -1
        finally:
            irdm.device_free(d)
        seen["refusals"] = True

    on = front_end_run(x, irdm.FMT_CF32, seed, depth, after=refusals)
    off = front_end_run(y, None, None, depth)
    assert seen == dict(refusals=True)
    assert len(on["band"]) == 8 * on["n_out"] and on["n_out"] >= n // FE["D"] - 1
    assert on["band"] == off["band"]
    assert on["st"] == dc.fig_tuple(fig), (on["st"], dc.fig_tuple(fig))
    print("front end depth %d: figures %r" % (depth, on["st"]))
    on16 = front_end_run(x16, irdm.FMT_CI16_FULL, seed16, depth)
    off16 = front_end_run(y16, None, None, depth)
    assert on16["band"] == off16["band"] and len(on16["band"]) == len(on["band"])
    assert on16["st"] == dc.fig_tuple(fig16)
    raw = front_end_run(x, None, None, depth)
    assert raw["band"] != on["band"] and len(raw["band"]) == len(on["band"])


def test_front_end_reset_seek_and_other_formats():
    """irdm_frontend_reset starts the stream state over and keeps the setting; behind irdm_frontend_seek blocks count from
    the first sample fed; the refusals; a ci8 front end refuses the pass; no figures with the pass off"""
    x, (y, fig), x16, (y16, fig16), n, seed, seed16 = capture()
    fe = irdm.Frontend(FE["fs_in"], irdm.FMT_CF32, FE["D"], FE["shift_hz"])
    p = irdm.Pipeline(fe.out_rate, fmt=irdm.FMT_CF32, max_chunk_samples=1 << 18, max_bursts_per_chunk=256, pipeline_depth=0)
    try:
        L = irdm.lib()
        assert L.irdm_frontend_dc_stats(fe.h, irdm.DcStats()) == -1
        for log2 in (11, 25):
            assert L.irdm_frontend_dc_block(fe.h, irdm.FMT_CF32, log2, 0.0, 0.0) == -1
        assert L.irdm_frontend_dc_block(fe.h, 5, FE_LOG2, 0.0, 0.0) == -1
        assert L.irdm_frontend_dc_block(fe.h, irdm.FMT_CF32, FE_LOG2, float("nan"), 0.0) == -1
        assert L.irdm_frontend_dc_block(fe.h, irdm.FMT_CF32, FE_LOG2, 0.0, 64.5) == -1
        fe.dc_block(irdm.FMT_CF32, FE_LOG2, seed)
        want = dc.fig_tuple(dm.dc_model(x[:2 * FE_CHUNK], FE_LOG2, seed)[1])
        fe.feed_host(p, x.view(np.complex64)[:FE_CHUNK])
        assert dc.stats_tuple(fe.dc_stats()) == want
        fe.reset()
        p.reset()
        st = dc.stats_tuple(fe.dc_stats())
        assert st[:4] == (0, 0, FE_LOG2, (seed[0], seed[1])) and all(float(v) == 0.0 for pair in st[4:] for v in pair), st
        fe.feed_host(p, x.view(np.complex64)[:FE_CHUNK])
        assert dc.stats_tuple(fe.dc_stats()) == want
        fe.reset()
        p.reset()
        fe.seek(5 * 12345)
        fe.feed_host(p, x.view(np.complex64)[:FE_CHUNK])
        assert dc.stats_tuple(fe.dc_stats()) == want
    finally:
        p.close()
        fe.close()
    fe = irdm.Frontend(FE["fs_in"], irdm.FMT_CI8, FE["D"], FE["shift_hz"])
    try:
        assert irdm.lib().irdm_frontend_dc_block(fe.h, irdm.FMT_CI8, FE_LOG2, 0.0, 0.0) == -1
    finally:
        fe.close()


# ---------------------------------------------------------------- the binary ----
COMMON = ["-r", dc.FS, "--file-info", "dc", "--start-time", "1700000000"]
CLI_LOG2 = 16


def run_cli(args, stdin=None):
    return subprocess.run([EXE] + [str(a) for a in args], capture_output=True, text=True, stdin=stdin, timeout=180)


def dc_lines(stderr):
    return [l for l in stderr.splitlines() if l.startswith("dc:")]


def model_line(fig, fmt_name="cf32"):
    """the line the binary owes for the model's figures"""
    head = "dc: %d samples %s, %d whole block%s of 2^%d; seed I %+.5f Q %+.5f" % (
        fig["n_samples"], fmt_name, fig["n_blocks"], "" if fig["n_blocks"] == 1 else "s", fig["block_log2"], fig["seed"][0], fig["seed"][1])
    if not fig["n_blocks"]:
        return head + " (the only correction)"
    return head + "; block means I %+.5f .. %+.5f, Q %+.5f .. %+.5f, last I %+.5f Q %+.5f" % (
        fig["min"][0], fig["max"][0], fig["min"][1], fig["max"][1], fig["last"][0], fig["last"][1])


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("dc")
    s, x = dc.streams()
    y, fig = dc.corrected(CLI_LOG2, own_head=True)
    x2 = x[:2 * 1_500_000].copy()
    x2[0::2] += np.float32(0.01)
    short = x[:2 * 50_000]
    out = {"dir": d, "fig": fig}
    for name, a in (("clean.cf32", s), ("dc.cf32", x), ("corrected.cf32", y), ("dc2.cf32", x2), ("short.cf32", short)):
        out[name] = d / name
        a.tofile(out[name])
    return out


def test_cli_dc_block_equals_a_plain_run_over_the_corrected_file(files):
    """-f dc.cf32 --dc-block=16 prints byte for byte the stdout of a plain run over the model-corrected file (13 lines where
    the run without the flag prints 3), and the dc: line is the model's; two --chunk values and standard input give the same
    stdout and line; -v names the option once"""
    ref = run_cli(["-f", files["corrected.cf32"]] + COMMON)
    plain = run_cli(["-f", files["dc.cf32"]] + COMMON)
    on = run_cli(["-f", files["dc.cf32"], "--dc-block=%d" % CLI_LOG2, "-v"] + COMMON)
    assert ref.returncode == plain.returncode == on.returncode == 0, (ref.stderr, plain.stderr, on.stderr)
    assert ref.stdout.count("RAW: ") == 13 and plain.stdout.count("RAW: ") == 3 and on.stdout == ref.stdout
    print(dc_lines(on.stderr))
    assert dc_lines(on.stderr) == [model_line(files["fig"])] and dc_lines(ref.stderr) == []
    assert on.stderr.count("--dc-block: the DC offset is tracked over blocks of 2^16 samples") == 1 and "--dc-block" not in ref.stderr
    for chunk in (98304, 1 << 20):
        r = run_cli(["-f", files["dc.cf32"], "--dc-block=%d" % CLI_LOG2, "--chunk", chunk] + COMMON)
        assert r.returncode == 0 and r.stdout == ref.stdout and dc_lines(r.stderr) == dc_lines(on.stderr), (chunk, r.stderr)
    with open(files["dc.cf32"], "rb") as f:
        r = run_cli(["-f", "-", "--format", "cf32", "--dc-block=%d" % CLI_LOG2] + COMMON, stdin=f)
    assert r.returncode == 0 and r.stdout == ref.stdout and dc_lines(r.stderr) == dc_lines(on.stderr), r.stderr


def test_cli_dc_line_and_its_place(files):
    """a file the model leaves unchanged (all zeros): stdout and the rest of stderr are those of the run without the flag; the
    line stands behind clock:, iq: and image: and in front of scrub: and input:, which describe the stream as processed; a
    two-file batch prints one line each with independent seeds; a file under one block long gets the seed alone"""
    zero = files["dir"] / "zero.cf32"
    np.zeros(2 * 300_000, np.float32).tofile(zero)
    base = run_cli(["-f", zero] + COMMON)
    check = run_cli(["-f", zero, "--dc-block=%d" % CLI_LOG2] + COMMON)
    assert base.returncode == check.returncode == 0, (base.stderr, check.stderr)
    bl, cl = base.stderr.splitlines(), check.stderr.splitlines()
    assert check.stdout == base.stdout and cl[:-1] == bl and cl[-1] == model_line(dm.dc_model(np.zeros(600_000, np.float32), CLI_LOG2)[1]), cl
    full = run_cli(["-f", files["dc.cf32"], "--dc-block=%d" % CLI_LOG2, "--image-check", "--scrub", "--iq-check", "--clock-check",
                    "--input-stats"] + COMMON).stderr.splitlines()
    assert [l.split(":")[0] for l in full[-6:]] == ["clock", "iq", "image", "dc", "scrub", "input"], full[-7:]
    assert full[-2].startswith("scrub: 3000000 samples cf32, ") and full[-1].startswith("input: 3000000 samples cf32"), full[-2:]
    s, x = dc.streams()
    x2 = np.fromfile(files["dc2.cf32"], np.float32)
    fig2 = dm.dc_model(x2, CLI_LOG2, dm.head_mean(x2, 1 << CLI_LOG2))[1]
    batch = run_cli(["-f", files["dc.cf32"], "-f", files["dc2.cf32"], "--dc-block=%d" % CLI_LOG2] + COMMON)
    assert batch.returncode == 0 and dc_lines(batch.stderr) == [model_line(files["fig"]), model_line(fig2)], batch.stderr
    assert abs(float(fig2["seed"][0]) - 0.04) < 1e-3 and abs(float(files["fig"]["seed"][0]) - 0.03) < 1e-3
    short = np.fromfile(files["short.cf32"], np.float32)
    fig_s = dm.dc_model(short, 20, dm.head_mean(short, 50_000))[1]
    r = run_cli(["-f", files["short.cf32"], "--dc-block"] + COMMON)
    assert r.returncode == 0 and dc_lines(r.stderr) == [model_line(fig_s)] and dc_lines(r.stderr)[0].endswith("(the only correction)"), r.stderr
    assert "0 whole blocks of 2^20; seed I +0.03" in dc_lines(r.stderr)[0]


def test_cli_prime_with_dc_block_equals_the_model_over_the_prefixed_stream(files):
    """--prime --dc-block: the lines formatted from the oracle's records over dc_model(P || x), seeded from x's head, with the
    rule of tests/test_gpu_parity.py (every field equal but the frequency, within 1 Hz, and the level, within 1e-4)"""
    import orc
    import parity
    import prime_checks as pc
    s, x = dc.streams()
    P = dc.as_floats(pc.prefix(x.view(np.complex64), dc.FS)[0])
    z = dm.dc_model(np.concatenate([P, x]), CLI_LOG2, dm.head_mean(x, 1 << CLI_LOG2))[0]
    ref = orc.run_stream(z.view(np.complex64), dc.FS, start_time_ns=pc.shifted_origin(dc.FS))
    r = run_cli(["-f", files["dc.cf32"], "--prime", "--dc-block=%d" % CLI_LOG2] + COMMON)
    assert r.returncode == 0, r.stderr
    lines, want = r.stdout.splitlines(), [l.strip() for l in ref.raw_lines("dc")]
    assert len(lines) == len(want) >= 13, (len(lines), len(want))
    for a, b in zip(lines, want):
        fa, fb = parity.raw_fields(a), parity.raw_fields(b)
        assert fa[:2] == fb[:2] and fa[3:6] == fb[3:6] and fa[7:] == fb[7:], (a, b)
        assert abs(fa[2] - fb[2]) <= 1 and abs(fa[6] - fb[6]) <= 1e-4, (a, b)
    assert dc_lines(r.stderr)[0].startswith("dc: %d samples cf32, " % (len(P) // 2 + dc.N))


def test_cli_save_only_writes_the_corrected_band(files):
    """--dc-block with --save-only: the band file of the recording with DC is the model-corrected recording's, byte for byte"""
    args = ["-r", "2400000", "--resample-to", "2000000", "--save-only", "--save-band"]      # (read as a 2.4 MS/s capture: 5/6)
    a, b, c = (files["dir"] / n for n in ("corrected.band.cf32", "dc.band.cf32", "plain.band.cf32"))
    ra = run_cli(["-f", files["corrected.cf32"]] + args + [a])
    rb = run_cli(["-f", files["dc.cf32"], "--dc-block=%d" % CLI_LOG2] + args + [b])
    rc = run_cli(["-f", files["dc.cf32"]] + args + [c])
    assert ra.returncode == rb.returncode == rc.returncode == 0, (ra.stderr, rb.stderr, rc.stderr)
    assert a.stat().st_size > 8 * 2_000_000 and a.read_bytes() == b.read_bytes() and c.read_bytes() != b.read_bytes()
    fig = files["fig"]
    assert dc_lines(rb.stderr) == ["dc: 3000000 samples cf32, 45 whole blocks of 2^16; seed I %+.5f Q %+.5f; last I %+.5f Q %+.5f" % (
        fig["seed"][0], fig["seed"][1], fig["last"][0], fig["last"][1])], rb.stderr


def test_cli_refusals(files):
    """--dc-block=11, =25, =x and --gpus 2 exit with 2 and an empty stdout"""
    for extra in (["--dc-block=11"], ["--dc-block=25"], ["--dc-block=x"], ["--dc-block="], ["--dc-block=16.5"], ["--dc-block", "--gpus", "2"]):
        r = run_cli(["-f", files["clean.cf32"]] + extra + COMMON)
        assert r.returncode == 2 and r.stdout == "" and "--dc-block" in r.stderr, (extra, r.stderr)
