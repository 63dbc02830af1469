"""Option "spectrum_frames" without a GPU: the whole product on the HIP emulation (tests/emul_build.py,
tests/frontend_emul_build.py), 2 MHz and 1 MHz, driven through irdm.py by tests/spectrum_emul_run.py.  The mean and
peak-hold rows reduced from K1's plane against the oracle's plane (tests/spectrum_checks.py says how: peak exactly, mean
within the derived bound), the same bytes however the stream is cut, polled mid-stream or at the end, behind a reset; and
nothing else a context returns changes.  Test infrastructure: the product never loads the emulated build."""
import json
import os
import subprocess
import sys

import pytest

import frontend_emul_build

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def emul_lib():
    return frontend_emul_build.build()


def run_case(lib, case, timeout=900):
    env = dict(os.environ, IRDM_LIB=lib)
    p = subprocess.run([sys.executable, os.path.join(HERE, "spectrum_emul_run.py"), case], env=env, capture_output=True, text=True,
                       timeout=timeout)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    line = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")][-1]
    return json.loads(line[7:])


def test_rows_against_the_oracle_plane(emul_lib):
    """1. R = 1, 7, 64 and more frames than the stream has: row count, headers (first frame, n_frames, timestamp) and values;
    2 MHz cf32 and ci8, 1 MHz"""
    res = run_case(emul_lib, "values")
    assert set(res) == {"2mhz_cf32", "2mhz_ci8", "1mhz_cf32"}
    for name, s in res.items():
        assert set(s) == {"1", "7", "64", "1048576"}, (name, s)
        assert s["1048576"]["rows"] == 1 and s["1"]["worst"] == 0.0 and s["7"]["last_frames"] == s["1"]["rows"] % 7, (name, s)


def test_the_same_bytes_however_the_stream_is_cut(emul_lib):
    """2. one chunk, five parts, single feed blocks: identical bytes at pipeline_depth 0, 1 and 3, cf32 and ci8, with
    detect_only, and for rows of several summation groups"""
    res = run_case(emul_lib, "cuts")
    assert len(res) == 9
    for name, s in res.items():
        assert s["rows"] > 1 and s["chunks"]["one"] == 1 and s["chunks"]["five"] == 5 and s["chunks"]["blocks"] > 30, (name, s)


def test_rows_polled_mid_stream(emul_lib):
    """3. the rows polled after every feed, with those after the flush, are the rows of a single poll at the end"""
    res = run_case(emul_lib, "polls")
    for name in ("depth0", "depth3"):
        assert 0 < res[name]["before_flush"] < res[name]["rows"], res


def test_the_records_do_not_change(emul_lib):
    """4. the record queues of a run with the option on equal those of a run with it off, byte for byte"""
    res = run_case(emul_lib, "records")
    assert res["depth0_full"]["demods"] > 0 and res["depth3_packed"]["packed"] > 0, res


def test_reset_starts_at_row_zero(emul_lib):
    """5. A with its rows left unpolled, reset, B: B's rows are a fresh context's; the option is refused from the first feed
    until the reset"""
    res = run_case(emul_lib, "reset")
    assert res["depth0"]["rows_b"] > 1 and res["depth3"]["rows_b"] > 1, res


def test_option_errors(emul_lib):
    """6. R < 0 and R > 2^20 are refused; so is a member of a group, directly and through irdm_group_set_option"""
    res = run_case(emul_lib, "errors")
    assert res["range"] == [-1, -1, 0, 0] and res["group_member"] == -1 and res["group"] == -1, res
