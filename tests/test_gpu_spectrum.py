"""Option "spectrum_frames" on the card, and the binary's --spectrum: the mean and peak-hold rows reduced from K1's plane
against the oracle's plane -- peak exactly, mean within the bound tests/spectrum_checks.py derives --, the same bytes however
the stream is cut and at every pipeline_depth, polled mid-stream or at the end, behind a reset, and nothing else a context
returns changed.  The checks are tests/spectrum_checks.py's (shared with tests/test_spectrum_emul.py, which runs them at 2
and 1 MHz on the CPU emulation); here 10 MHz -- 8192-point frames --, one case at 12 MHz (16384) and one at 1 MHz (1024)."""
import os

import pytest
import torch

import irdm
import reset_checks as rc
import spectrum_checks as sc

pytestmark = pytest.mark.gpu
FS = 10_000_000
EXE = os.path.join(os.path.dirname(irdm.LIB_PATH), "iridium-sniffer-hip")
FMTS = [irdm.FMT_CF32, irdm.FMT_CI8]


@pytest.fixture(scope="module")
def stream():
    return sc.scene(FS)


@pytest.mark.parametrize("fmt", FMTS, ids=["cf32", "ci8"])
def test_rows_against_the_oracle_plane(stream, fmt):
    """1. R = 1, 7, 64 and more frames than the stream has: row count, headers (first frame, n_frames, timestamp) and values"""
    s = sc.check_values(FS, fmt, rc.as_format(stream, fmt), depth=1 if fmt == irdm.FMT_CF32 else 0)
    assert s["1048576"]["rows"] == 1 and s["1"]["worst"] == 0.0 and s["7"]["last_frames"] == s["1"]["rows"] % 7, s


@pytest.mark.parametrize("fs,depth", [(12_000_000, 3), (1_000_000, 1)], ids=["12mhz", "1mhz"])
def test_rows_at_other_frame_sizes(fs, depth):
    """1. 16384-point frames, and 1024-point frames (the dense scan's rate)"""
    s = sc.check_values(fs, irdm.FMT_CF32, sc.scene(fs), depth=depth)
    assert s["1048576"]["rows"] == 1 and s["1"]["worst"] == 0.0, s


@pytest.mark.parametrize("fmt", FMTS, ids=["cf32", "ci8"])
@pytest.mark.parametrize("depth", [0, 1, 3])
def test_the_same_bytes_however_the_stream_is_cut(stream, depth, fmt):
    """2. one chunk, five parts, single feed blocks: identical bytes"""
    s = sc.check_cuts(FS, fmt, rc.as_format(stream, fmt), depth)
    assert s["rows"] > 1 and s["chunks"]["blocks"] > 200, s


@pytest.mark.parametrize("R,options", [(7, {"detect_only": 1}), (150, None)], ids=["detect_only", "R150"])
def test_the_same_bytes_with_detect_only_and_in_rows_of_several_groups(stream, R, options):
    """2. with detect_only; and rows of 64 + 64 + 22 frames whose summation groups the chunk boundaries cut"""
    s = sc.check_cuts(FS, irdm.FMT_CF32, stream, 3, R=R, options=options)
    assert s["rows"] > 1, s


@pytest.mark.parametrize("depth", [0, 3])
def test_rows_polled_mid_stream(stream, depth):
    """3. the rows polled after every feed, with those after the flush, are the rows of a single poll at the end"""
    s = sc.check_mid_stream_polls(FS, irdm.FMT_CF32, stream, depth)
    assert 0 < s["before_flush"] < s["rows"], s


@pytest.mark.parametrize("depth,opts", [(0, rc.FULL), (3, rc.PACKED)], ids=["depth0_full", "depth3_packed"])
def test_the_records_do_not_change(stream, depth, opts):
    """4. the record queues of a run with the option on equal those of a run with it off, byte for byte"""
    s = sc.check_records_unchanged(FS, irdm.FMT_CF32, stream, depth, opts)
    assert s["packed" if opts is rc.PACKED else "demods"] > 0, s


@pytest.mark.parametrize("depth", [0, 3])
def test_reset_starts_at_row_zero_and_allocates_nothing(stream, depth):
    """5. A with its rows left unpolled, reset, B: B's rows are a fresh context's; the option is refused from the first feed
    until the reset; device memory after the third stream equals that after the first (tests/test_gpu_reset.py's method)"""
    def used():
        torch.cuda.synchronize()
        free, total = torch.cuda.mem_get_info()
        return total - free

    s = sc.check_reset(FS, irdm.FMT_CF32, stream, sc.scene(FS, seed=9, n_bursts=4), depth, used=used)
    assert s["rows_b"] > 1, s


def test_option_range():
    """6. R < 0 and R > 2^20 are refused (the group member's refusal runs on the emulation: a group needs no second GPU there)"""
    assert sc.check_option_range(FS) == [-1, -1, 0, 0]


def test_cli_spectrum_file(stream, tmp_path):
    """7. --spectrum: header fields and rows; stdout and stderr of the run without the flag; the --spectrum-frames default;
    two recordings with --out-dir and auto; the exit-2 cases"""
    s = sc.check_cli(EXE, str(tmp_path), FS, stream)
    assert s["default"]["rows"] == 1 and s["explicit"]["rows"] > 100, s


def test_cli_spectrum_behind_the_front_end(tmp_path):
    """8. --band-center / --decimate with --spectrum: the rows of the selected band, header rate and centre the band's"""
    s = sc.check_cli_frontend(EXE, str(tmp_path))
    assert s["rows"] > 1, s
