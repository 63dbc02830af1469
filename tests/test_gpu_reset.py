"""irdm_reset / irdm_frontend_reset on the card, and the binary's several recordings per run: a context that has carried a
stream (one chosen to leave it dirty: squelch and re-priming, a burst still active at the end, a ragged last chunk) and is
reset yields for the next stream -- queue by queue, byte for byte -- what a fresh context yields; the binary's batch run prints
the concatenation of the single-file runs.  The checks are tests/reset_checks.py's (shared with tests/test_reset_emul.py,
which runs them at 2 MHz on the CPU emulation); here 10 MHz -- 8192-point frames, decimation by 40 -- and one 12 MHz case."""
import os

import numpy as np
import pytest
import torch

import irdm
import reset_checks as rc

pytestmark = pytest.mark.gpu
FS = 10_000_000
EXE = os.path.join(os.path.dirname(irdm.LIB_PATH), "iridium-sniffer-hip")


@pytest.fixture(scope="module")
def streams():
    return rc.dirty_scene(FS), rc.plain_scene(FS)


@pytest.mark.parametrize("opts", [rc.FULL, rc.PACKED], ids=["full", "packed"])
@pytest.mark.parametrize("fmt", [irdm.FMT_CF32, irdm.FMT_CI8], ids=["cf32", "ci8"])
@pytest.mark.parametrize("depth,parts_a,parts_b", [(0, 2, 1), (1, 3, 4), (3, 5, 4)])
def test_reset_then_b_equals_fresh_b(streams, depth, parts_a, parts_b, fmt, opts):
    """1. create; feed A; flush; poll; reset; feed B; flush == create; feed B; flush (pipeline_depth >= 1: fed in place with
    look-ahead)"""
    a, b = (rc.as_format(x, fmt) for x in streams)
    s = rc.check_reuse(FS, fmt, depth, opts, a, b, parts_a, parts_b)
    assert s["a_tagged"] >= 3 and s["b"]["tagged"] >= 3 and s["resets"] == 1, s
    assert s["b"]["packed" if opts is rc.PACKED else "demods"] > 0, s


@pytest.mark.parametrize("opts", [rc.FULL, rc.PACKED], ids=["full", "packed"])
@pytest.mark.parametrize("depth,parts_a", [(0, 2), (1, 2), (3, 2), (3, 5)])
def test_reset_mid_stream_discards_the_old_stream(streams, depth, parts_a, opts):
    """2. the reset after A's first chunk (with two parts: the one that holds the squelch wave), the scan and the chain in
    flight, nothing polled: the queues hold B's records only"""
    s = rc.check_reuse(FS, irdm.FMT_CF32, depth, opts, streams[0], streams[1], parts_a, 4, mid_stream=True)
    assert s["b"]["tagged"] >= 3 and s["b"]["bursts"] > 0, s


@pytest.mark.parametrize("depth,parts_a,parts_b", [(0, 2, 2), (1, 3, 3), (3, 5, 4)])
def test_state_after_reset_and_three_streams_in_a_row(streams, depth, parts_a, parts_b):
    """3. irdm_export_state right after the reset equals a fresh context's with the same start time, and after B the fresh
    context's after B; 5. A, B, A: the second A's records equal the first's"""
    s = rc.check_reuse(FS, irdm.FMT_CF32, depth, rc.FULL, streams[0], streams[1], parts_a, parts_b, states=True, thrice=True)
    assert s["dirty_state"][5] >= 1 and s["resets"] == 2 and s["a_again"]["tagged"] == s["a_tagged"], s


@pytest.mark.parametrize("depth,parts_b", [(0, 1), (3, 4)])
def test_b_behind_a_reset_against_the_oracle(streams, depth, parts_b):
    """4. B's records behind the reset pass tests/parity.py's comparison with the oracle's for B"""
    s = rc.check_oracle(FS, depth, streams[1], parts_b, streams[0])
    assert s["bursts"] >= 4 and s["demods"] >= 3, s


def test_reset_refused_inside_a_feed(streams):
    """6. (as on the emulation) irdm_reset between irdm_feed_begin and irdm_feed_end: -1, the stream goes on unharmed"""
    s = rc.check_reuse(FS, irdm.FMT_CF32, 1, rc.PACKED, streams[0], streams[1], 3, 4, refused=True)
    assert s["b"]["tagged"] >= 3, s


def test_12mhz():
    """16384-point frames, decimation by 48: A, reset, B at pipeline_depth 1, with the exported states and A once more"""
    fs = 12_000_000
    s = rc.check_reuse(fs, irdm.FMT_CF32, 1, rc.PACKED, rc.dirty_scene(fs), rc.plain_scene(fs), 3, 2, states=True, thrice=True)
    assert s["b"]["tagged"] >= 3 and s["a_again"]["tagged"] == s["a_tagged"], s


def test_frontend_reset():
    """7. front end: run A (ending on a partial block); finish; reset; run B == a fresh front end's B == the plain C model's"""
    for D, fmt in ((5, irdm.FMT_CI8), (4, irdm.FMT_CF32)):
        s = rc.check_frontend(10_000_000 * D, D, fmt)
        assert s["b"] > 0, s


def test_a_reset_allocates_nothing(streams):
    """10. device memory in use after the third stream equals that after the first (torch.cuda.mem_get_info after a
    synchronize, as tests/test_gpu_footprint.py measures it).  The streams are A, B, A: the third is the first again, so it
    needs no more decimated scratch, strip lists or rotator-checkpoint blocks than the context has grown to by then, and B
    (six bursts of ordinary length, on rows the prebuild made) needs less than A; whatever is allocated between the two
    measurements would be the reset's."""
    def used():
        torch.cuda.synchronize()
        free, total = torch.cuda.mem_get_info()
        return total - free

    a, b = streams
    ca, cb = rc.chunks_of(len(a), 3), rc.chunks_of(len(b), 3)
    p = rc.make(FS, irdm.FMT_CF32, 1, max(ca + cb), rc.PACKED)
    try:
        rc.feed(p, a, irdm.FMT_CF32, ca)
        first = rc.queues(p)
        grown = (p.stat("scratch_grows"), p.stat("rot_grows"), p.stat("tiles_grows"))
        after_first = used()
        p.reset(rc.CF_B, rc.T0_B)
        rc.feed(p, b, irdm.FMT_CF32, cb)
        rc.queues(p)
        p.reset(rc.CF_A, rc.T0_A)
        rc.feed(p, a, irdm.FMT_CF32, ca)
        assert rc.queues(p) == first
        assert (p.stat("scratch_grows"), p.stat("rot_grows"), p.stat("tiles_grows")) == grown
        assert used() == after_first, (used(), after_first)
    finally:
        p.close()


# ---- the binary ----
@pytest.fixture(scope="module")
def recordings(tmp_path_factory):
    """three scene files at 10 MHz: IRA frames for --position (with IDA frames between them), a short one (shorter than the
    chunk the runs use), the IDA / ACARS scene"""
    import test_gpu_acars as ta
    import test_gpu_position as tp
    tmp = tmp_path_factory.mktemp("batch")
    scenes = [("position.cf32", tp.position_scene(FS, 1.3)),
              ("short.cf32", rc.plain_scene(FS, seed=9, secs=(520 * 8192 + 0.15 * FS) / FS, n_bursts=3)),
              ("acars.cf32", ta.ida_scene(FS, 12))]
    files = []
    for name, x in scenes:
        path = str(tmp / name)
        np.ascontiguousarray(x).tofile(path)
        files.append(path)
    chunk = 1 << 23
    assert len(scenes[1][1]) < chunk < len(scenes[0][1])
    common = ["-r", FS, "-c", int(tp.CENTER), "--chunk", chunk, "--file-info", "golden"]
    return str(tmp), files, common


TIMES = ["1700000000", "1700003600.25", "1700007200.000000007"]


def test_cli_batch_prints_the_concatenation_of_the_single_runs(recordings):
    """8. --files-from with start times == the three single-file runs with --start-time, stdout and the per-file stderr lines;
    plain, --parsed, --acars-json, --position; --out-dir; the --timing / -v lines"""
    tmp, files, common = recordings
    res = rc.check_cli_batch(EXE, tmp, files, TIMES, common,
                             [[], ["--parsed"], ["--acars-json", "--acars-origin", "1700000000"], ["--position"]])
    assert res["--acars-json --acars-origin 1700000000"][2] > 0, res          # (the ACARS scene printed its messages)


def test_cli_batch_behind_the_front_end(tmp_path):
    """8. --band-center / --decimate: a wideband rendering of the scene (tests/test_gpu_frontend.py's) whole, cut at a ragged
    length behind its fifth burst, and cut behind its third: one front end and one context for the three"""
    import frontend_model as fm
    s = fm.SCENE
    x, _, _ = fm.wideband_scene()
    n = len(x) // 2
    cuts = [n, int(0.66 * s["fs_in"]) + 12345, int(0.58 * s["fs_in"]) // (32768 * s["D"]) * (32768 * s["D"])]
    files = []
    for i, c in enumerate(cuts):
        path = str(tmp_path / ("wide%d.ci8" % i))
        x[:2 * c].tofile(path)
        files.append(path)
    cc = 1615000000.0
    common = ["-r", s["fs_in"], "-c", "%.3f" % cc, "--band-center", "%.3f" % (cc + s["shift_hz"]), "--decimate", s["D"],
              "--file-info", "fe", "--chunk", 1 << 20]
    res = rc.check_cli_batch(EXE, str(tmp_path), files, TIMES, common, [[]])
    assert all(v > 0 for v in res["raw"]), res


def test_cli_refusals_and_a_missing_file(recordings):
    """9. mixed formats, --gpus 2 with two files, -f - with a second file: exit 2, nothing on stdout; a missing middle file: the
    other two outputs intact, exit 1"""
    tmp, files, common = recordings
    rc.check_cli_refusals(EXE, tmp, files, common)
