"""Exchanged I and Q on the GPU: the exchange kernel (csrc/iq_swap.hpp) exact against numpy through irdm_swap_iq_device; the
sense kernel (iq_sense_kernel, csrc/bitlayer.hip) against the model of tests/iq_sense_model.py through
irdm_iq_sense_batch; options iq_sense and swap_iq on a scene of IRA, IBC and IDA frames fed as it is and exchanged, at
pipeline_depth 0 and 3 and in five input formats; irdm_frontend_swap_iq in front of a decimating front end; and the
binary's --iq-check and --swap-iq."""
import functools
import os
import subprocess

import numpy as np
import pytest

import containers as ct
import iq_checks as ic
import iq_sense_model as im
import irdm
import siggen

pytestmark = pytest.mark.gpu

EXE = os.path.join(os.path.dirname(irdm.LIB_PATH), "iridium-sniffer-hip")


def test_exchange_kernel_equals_numpy():
    """all eight formats, n in 0 .. 4097 and 65536 + 3 (more than one workgroup's worth of 16-byte pieces, a ragged tail),
    the buffer 0 .. 3 samples behind a 16-byte boundary, and 2048 x 256 + 777 pieces (the grid is capped at 2048 workgroups
    of 256: some lanes take a second piece, most do not): exact, guard bytes untouched, the identity applied twice, -1 for
    an unknown format and a pointer that is not sample-aligned"""
    assert ic.swap_cases(extra_n=(65536 + 3,), extra_pieces=(2048 * 256 + 777,)) == 8 * (12 * 4 + 1)


def test_votes_equal_the_model():
    """irdm_iq_sense_batch on frame_corpus and ida_corpus of two seeds, as they are and exchanged (the cases without LLRs
    and the cut frames among them), over a context of 64 bursts per launch: every field the model's"""
    p = irdm.Pipeline(2_000_000, max_chunk_samples=32768 * 8, max_bursts_per_chunk=64, pipeline_depth=0)
    try:
        res = ic.check_votes(p)
    finally:
        p.close()
    assert min(res["kinds"]) >= 20 and res["odd"] > 0 and res["no_llr"] > 0, res


@pytest.mark.parametrize("depth,fmt", ((0, irdm.FMT_CF32), (3, irdm.FMT_CF32), (0, irdm.FMT_CI8), (3, irdm.FMT_CI16),
                                       (3, irdm.FMT_CU8), (0, irdm.FMT_CI32)))
def test_pipeline_votes_and_swap_iq(depth, fmt):
    """(a) the scene: 12 recorded votes, verdict 1; (b, cf32) its exchange: 12 exchanged votes, verdict 2, every RAW
    frequency mirrored; (c) the exchange with swap_iq: (a)'s burst, frame and demod records bit for bit -- through the
    staging buffer (depth 0) and the ring slot (depth 3); the refusals; irdm_reset clears the counts"""
    assert ic.pipeline_case(depth, fmt)["frames"] == 12


def test_random_payloads_do_not_vote():
    assert ic.random_payloads_case(3)["frames"] >= 5


# ---------------------------------------------------------------- the front end ----
FE = dict(fs_in=10_000_000, D=5, shift_hz=1_500_000.0)


@functools.lru_cache(maxsize=None)
def capture():
    """a 10 MS/s capture whose band 1.5 MHz above the centre holds the 12 frames of ic.scene's kind, as cf32"""
    fs = FE["fs_in"]
    fe = irdm.Frontend(fs, irdm.FMT_CI8, FE["D"], FE["shift_hz"])
    applied = fe.applied_shift_hz
    fe.close()
    rng = np.random.default_rng(54)
    bursts = []
    for k, quads in enumerate(frame_quads()):
        bursts.append(dict(start=int((0.56 + 0.02 * k) * fs), freq_hz=applied + siggen.channel_freq(int(rng.integers(-18, 19)) or 3),
                           quads=quads, amp=0.05))
    n = int(0.83 * fs) // 32768 * 32768 + 4321
    return siggen.make_stream(fs, n, bursts, seed=54)[0]


def frame_quads():
    import bitlayer as bl
    rng = np.random.default_rng(55)
    out = []
    for k in range(12):
        if k % 3 == 0:
            st = bl.ira_stream(int(rng.integers(0, 128)), int(rng.integers(0, 64)), int(rng.integers(-2047, 2048)),
                               int(rng.integers(-2047, 2048)), int(rng.integers(-2047, 2048)),
                               [(int(rng.integers(0, 2**32)), int(rng.integers(0, 32))) for _ in range(3)], rng)
            bits = bl.ira_frame(st[:63 + 4 * 42])
        elif k % 3 == 1:
            bits = bl.ibc_frame(int(rng.integers(0, 4)), bl.ibc_stream(int(rng.integers(0, 128)), int(rng.integers(0, 64)), 1, 0,
                                                                        int(rng.integers(0, 2**32)), rng, n_blocks=4))
        else:
            st = bl.ida_stream(int(rng.integers(0, 8)), int(rng.integers(1, 21)), 0, [int(b) for b in rng.integers(0, 256, 20)], rng)
            bits = bl.ida_frame(bl.lcw_bits(2, int(rng.integers(0, 32)), int(rng.integers(0, 1 << 21))), st, rng)
        bits = bits + [0] * (len(bits) % 2)
        out.append([0] * 16 + siggen.bits_to_quadrants("".join(str(b) for b in bits)))
    return out


def front_end_run(x, swap, depth):
    """the ci8 capture x through the front end (feed_host in chunks of 1 Mi capture samples, saving the band as cf32)
    and a context with iq_sense"""
    fe = irdm.Frontend(FE["fs_in"], irdm.FMT_CI8, FE["D"], FE["shift_hz"])
    p = irdm.Pipeline(fe.out_rate, fmt=irdm.FMT_CF32, center_frequency=1622000000.0 + fe.applied_shift_hz,
                      max_chunk_samples=1 << 18, max_bursts_per_chunk=256, pipeline_depth=depth)
    try:
        p.set_option("iq_sense", 1)
        fe.save(irdm.FMT_CF32)
        if swap:
            fe.swap_iq(True)
        n = len(x) // 2
        for off in range(0, n, 1 << 20):
            fe.feed_host(p, x[2 * off:2 * min(n, off + (1 << 20))])
        if swap:
            # a device feed takes the caller's buffer as it is: refused while the switch is on, and the switch stays
            d = irdm.device_buffer(np.zeros(2 * 4096, np.int8))
            try:
                L = irdm.lib()
                assert L.irdm_frontend_feed_device(fe.h, p.h, d, 4096, None) == -1
                assert L.irdm_frontend_swap_iq(fe.h, 0) == -1
            finally:
                irdm.device_free(d)
        fe.flush(p)
        infos, _ = p.poll_frames()
        demods = p.poll_demods()
        st = p.iq_sense()
        return dict(bursts=p.poll_bursts_raw().tobytes(), frames=b"".join(bytes(f) for f in infos),
                    demods=b"".join(bytes(d) for d in demods), n=len(demods), band=b"".join(fe.saved), n_out=p.sample_count,
                    counts=(st.frames, st.votes_recorded, st.votes_exchanged, st.votes_both, st.verdict))
    finally:
        p.close()
        fe.close()


@pytest.mark.parametrize("depth", (0, 3))
def test_front_end_swap_iq(depth):
    """irdm_frontend_swap_iq on the exchanged capture: the records of the plain capture bit for bit, and the band
    irdm_frontend_save writes (cf32) byte for byte; without the switch the exchanged capture shows another band"""
    x = capture()
    plain = front_end_run(siggen.to_ci8(x), False, depth)
    fixed = front_end_run(siggen.to_ci8(im.swap_complex(x)), True, depth)
    assert plain["n"] == 12 and plain["counts"] == (12, 12, 0, 0, irdm.IQ_AS_RECORDED), plain["counts"]
    for k in ("bursts", "frames", "demods", "band", "counts"):
        assert fixed[k] == plain[k], k
    assert len(plain["band"]) == 8 * plain["n_out"] and plain["n_out"] >= len(x) // FE["D"] - 1
    wrong = front_end_run(siggen.to_ci8(im.swap_complex(x)), False, depth)
    assert wrong["band"] != plain["band"] and wrong["counts"][2] + wrong["counts"][1] < 12      # (the band 1.5 MHz BELOW the centre: noise)


# ---------------------------------------------------------------- the binary ----
START = ["--start-time", "1700000000"]


def run_cli(args):
    return subprocess.run([EXE] + [str(a) for a in args], capture_output=True, text=True, timeout=180)


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("iq")
    x = ic.scene()
    out = {}
    for name, iq in (("plain", x), ("swapped", im.swap_complex(x)), ("random", siggen.standard_scene(ic.FS, ic.FS, 12, 3)[0])):
        out[name] = d / (name + ".cf32")
        iq.tofile(out[name])
    for name, iq in (("plain", x), ("swapped", im.swap_complex(x))):
        out[name + ".wav"] = d / (name + ".wav")
        out[name + ".wav"].write_bytes(ct.wav(ct.quantise(iq, 65536.0, -32768, 32767, np.int16).tobytes(), rate=ic.FS, bits=16))
    out["dir"] = d
    return out


AS_RECORDED = "iq: 12 frames decide (4 IDA, 4 IRA, 4 IBC): 12 as recorded, 0 with I and Q exchanged"
EXCHANGED = ("iq: 12 frames decide (4 IDA, 4 IRA, 4 IBC): 0 as recorded, 12 with I and Q exchanged -- the recording is I/Q-swapped "
             "(spectrum inverted): every payload is wrong and every frequency mirrored about -c; run with --swap-iq")
IN_EFFECT = ("iq: 12 frames decide (4 IDA, 4 IRA, 4 IBC): 0 as recorded, 12 with I and Q exchanged -- the samples are I/Q-swapped "
             "with --swap-iq in effect: remove it")
TOO_FEW = "iq: 0 frames decide; too few to judge"


def test_cli_swap_iq_prints_the_plain_files_lines(files):
    """-f swapped.cf32 --swap-iq prints the stdout of -f plain.cf32 byte for byte; so does a Q/I WAV against the I/Q one;
    -v names the exchange once; --gpus 2 is refused"""
    common = ["-r", ic.FS, "--file-info", "iq"] + START
    plain = run_cli(["-f", files["plain"]] + common)
    fixed = run_cli(["-f", files["swapped"], "--swap-iq", "-v"] + common)
    wrong = run_cli(["-f", files["swapped"]] + common)
    assert plain.returncode == fixed.returncode == wrong.returncode == 0, (plain.stderr, fixed.stderr)
    assert plain.stdout.count("RAW: ") == 12 and fixed.stdout == plain.stdout and wrong.stdout != plain.stdout
    assert wrong.stdout.count("RAW: ") == 12                   # (the swapped file runs through: nothing points at the cause)
    assert fixed.stderr.count("--swap-iq: I and Q of every sample are exchanged") == 1 and "--swap-iq" not in plain.stderr
    a, b = run_cli(["-f", files["plain.wav"]] + START), run_cli(["-f", files["swapped.wav"], "--swap-iq"] + START)
    assert a.returncode == b.returncode == 0 and a.stdout.count("RAW: ") == 12 and a.stdout == b.stdout, (a.stderr, b.stderr)
    r = run_cli(["-f", files["plain"], "--swap-iq", "--gpus", "2"] + common)
    assert r.returncode == 2 and r.stdout == "" and "--swap-iq" in r.stderr


def test_cli_iq_check_lines(files):
    """--iq-check on the three scenes: as recorded, exchanged with the remedy, too few; with --swap-iq the verdicts change
    places; stdout and the other stderr lines are those of the run without the flag; behind a clock: line, in front of the
    input: line; a two-file batch prints one line each; --gpus 2 and --save-only are refused"""
    common = ["-r", ic.FS, "--file-info", "iq"] + START
    for name, extra, line in (("plain", [], AS_RECORDED), ("swapped", [], EXCHANGED), ("random", [], TOO_FEW),
                              ("swapped", ["--swap-iq"], AS_RECORDED), ("plain", ["--swap-iq"], IN_EFFECT)):
        base = run_cli(["-f", files[name]] + extra + common)
        check = run_cli(["-f", files[name], "--iq-check"] + extra + common)
        assert base.returncode == check.returncode == 0, (base.stderr, check.stderr)
        bl, cl = base.stderr.splitlines(), check.stderr.splitlines()
        print(cl[-1])
        assert check.stdout == base.stdout and not any(l.startswith("iq:") for l in bl)
        assert bl[-1].startswith("burst_detect: tagged ") and cl[:-1] == bl and cl[-1] == line, cl[-1]
    full = run_cli(["-f", files["swapped"], "--iq-check", "--clock-check", "--input-stats"] + common).stderr.splitlines()
    assert full[-3].startswith("clock: ") and full[-2] == EXCHANGED and full[-1].startswith("input: "), full[-4:]
    diag = run_cli(["-f", files["swapped"], "--diagnostic"] + common)
    assert diag.returncode == 0 and "iq:" not in diag.stderr
    batch = run_cli(["-f", files["plain"], "-f", files["swapped"], "--iq-check"] + common)
    assert batch.returncode == 0 and [l for l in batch.stderr.splitlines() if l.startswith("iq:")] == [AS_RECORDED, EXCHANGED]
    r = run_cli(["-f", files["plain"], "--iq-check", "--gpus", "2"] + common)
    assert r.returncode == 2 and r.stdout == "" and "--iq-check" in r.stderr
    band = files["dir"] / "b.ci8"
    r = run_cli(["-f", files["plain"], "-r", "2400000", "--resample-to", "2000000", "--iq-check", "--save-band", band, "--save-only"])
    assert r.returncode == 2 and r.stdout == "" and "--iq-check" in r.stderr and not band.exists()


def test_cli_save_only_writes_the_corrected_band(files):
    """--swap-iq with --save-only: the band file of the exchanged recording is the plain recording's, byte for byte"""
    a, b = files["dir"] / "plain.band.cf32", files["dir"] / "fixed.band.cf32"
    args = ["-r", "2400000", "--resample-to", "2000000", "--save-only", "--save-band"]      # (read as a 2.4 MS/s capture: 5/6)
    ra = run_cli(["-f", files["plain"]] + args + [a])
    rb = run_cli(["-f", files["swapped"], "--swap-iq"] + args + [b])
    assert ra.returncode == rb.returncode == 0, (ra.stderr, rb.stderr)
    assert a.stat().st_size > 8 * 1_000_000 and a.read_bytes() == b.read_bytes()
