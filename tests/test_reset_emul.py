"""irdm_reset and irdm_frontend_reset without a GPU: the whole product on the HIP emulation (tests/emul_build.py,
tests/frontend_emul_build.py), 2 MHz, driven through irdm.py by tests/reset_emul_run.py.  A context that has carried a
stream -- one chosen to leave it dirty: squelch and re-priming, a burst still active at the end, a ragged last chunk -- and
is reset yields for the next stream, queue by queue and byte for byte, what a fresh context yields.  Test infrastructure: the
product never loads the emulated build."""
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


def run_case(lib, case, timeout=1500):
    env = dict(os.environ, IRDM_LIB=lib)
    p = subprocess.run([sys.executable, os.path.join(HERE, "reset_emul_run.py"), case], env=env, capture_output=True, text=True,
                       timeout=timeout)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    line = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")][-1]
    return json.loads(line[7:])


def test_reset_then_b_equals_fresh_b(emul_lib):
    """1. create; feed A; flush; poll; reset; feed B; flush == create; feed B; flush, at pipeline_depth 0, 1 and 2 (fed in
    place with look-ahead), cf32 and ci8, full records and packed + parsed + frame records"""
    res = run_case(emul_lib, "matrix")
    assert len(res) == 12
    for name, s in res.items():
        assert s["a_tagged"] >= 3 and s["b"]["tagged"] >= 3 and s["resets"] == 1, (name, s)
        if name.endswith("packed"):
            assert s["b"]["packed"] > 0 and s["b"]["ida_packed"] > 0 and s["b"]["frame_packed"] > 0 and s["b"]["demods"] == 0, (name, s)
        else:
            assert s["b"]["demods"] > 0 and s["b"]["samples"] > 0 and s["b"]["packed"] == 0, (name, s)


def test_reset_mid_stream_discards_the_old_stream(emul_lib):
    """2. the reset after A's first chunk, nothing flushed or polled: the queues hold B's records only"""
    res = run_case(emul_lib, "mid_stream")
    assert len(res) == 6
    for name, s in res.items():
        assert s["b"]["tagged"] >= 3 and s["b"]["bursts"] > 0, (name, s)


def test_state_after_reset_and_three_streams_in_a_row(emul_lib):
    """3. irdm_export_state right after the reset equals a fresh context's, and after B the fresh context's after B;
    5. A, B, A: the second A's records equal the first's"""
    res = run_case(emul_lib, "states")
    for name in ("depth0", "depth2"):
        s = res[name]
        assert s["dirty_state"][5] >= 1 and s["resets"] == 2 and s["a_again"]["tagged"] == s["a_tagged"], (name, s)


def test_b_behind_a_reset_against_the_oracle(emul_lib):
    """4. B's records behind the reset pass tests/parity.py's comparison with the oracle's for B"""
    res = run_case(emul_lib, "oracle")
    for name in ("depth0", "depth2"):
        assert res[name]["bursts"] >= 4 and res[name]["demods"] >= 3, res


def test_reset_is_refused_inside_a_feed_and_for_group_members(emul_lib):
    """6. irdm_reset between irdm_feed_begin and irdm_feed_end returns -1 and the stream goes on to the fresh-context
    result; a member of a group is refused as well"""
    res = run_case(emul_lib, "refused")
    assert res["group_member"] == -1
    assert res["depth0"]["b"]["tagged"] >= 3 and res["depth1"]["b"]["tagged"] >= 3, res


def test_frontend_reset(emul_lib):
    """7. front end: run A (ending on a partial block); finish; reset; run B == a fresh front end's B == the plain C model's"""
    res = run_case(emul_lib, "frontend")
    assert res["D2"]["b"] > 0 and res["D5"]["b"] > 0, res
