"""The band scan's decline and redo paths in mid-stream, without a GPU: the whole product on the HIP emulation
(tests/emul_build.py), driven through irdm.py by tests/decline_emul_run.py in a process of its own; the cases, the runners and
every assertion are tests/decline_checks.py's, shared with tests/test_gpu_decline.py.  The 2 MHz cases (5 s a run here) take
three or four configurations that between them cover every depth, both feeds and both record forms; the 10 MHz ones
(8192-point frames: K1's candidate lists, chained scans, speculation passes; 8 to 25 s a run) one each.  The card runs every
case in every configuration.  Test infrastructure: the product never loads the emulated build."""
import json
import os
import subprocess
import sys

import pytest

import decline_checks as dc
import emul_build

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def emul_lib():
    return emul_build.build()


def run_case(lib, name, configs, timeout=900):
    env = dict(os.environ, IRDM_LIB=lib)
    p = subprocess.run([sys.executable, os.path.join(HERE, "decline_emul_run.py"), name] + list(configs), env=env, capture_output=True,
                       text=True, timeout=timeout)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-4000:]
    line = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")][-1]
    res = json.loads(line[7:])
    assert set(res) == set(configs)
    return res


@pytest.mark.parametrize("key", sorted(dc.PINS))
def test_new_scenes_are_the_bytes_they_were_and_hold_what_they_claim(key):
    """the stream's digest, the oracle's burst and frame counts, and the condition on the input each case rests on: the
    click's frame gives birth to more bursts than the sparse scan has lanes and fewer than max_bursts, the late wave is dumped
    behind seven finished bursts, bursts lie on both sides of the drop"""
    dc.check_pin(key)


def test_no_new_scene_joined_the_scene_zoo():
    import scenes
    assert not {"click", "squelch_late", "noise_drop", "crowded"} & set(scenes.ALL)


def test_records_leave_in_stream_order_whatever_max_bursts_per_chunk(emul_lib):
    """2 MHz, 24 bursts, a context made for 2 per chunk: BAND_F_GONECAP at the commit, the record buffer grown once, later
    crowded chunks batch by batch -- every record in the oracle's order at every depth (at depth >= 2 the batches' records
    used to overtake those of the chains in flight)"""
    res = run_case(emul_lib, "cap_2m", ["depth0", "depth1:packed", "depth2", "depth4"])
    for s in res.values():
        assert s["flags"] & dc.F_GONECAP and s["scan_fallbacks"] == 2 and s["bursts"] == 24, res


def test_squelch_wave_in_mid_stream(emul_lib):
    res = run_case(emul_lib, "squelch_late", ["depth1", "depth2", "depth3:packed"])
    for s in res.values():
        assert s["flags"] & dc.F_SQUELCH and s["band_aborts"] >= 1 and s["bursts"] == 46, res


def test_noise_floor_drops_in_mid_stream_2mhz(emul_lib):
    res = run_case(emul_lib, "drop_2m", ["depth0", "depth2", "depth3:packed"])
    for s in res.values():
        assert s["band_retries"] >= 1 and s["band_aborts"] == 0, res


@pytest.mark.parametrize("name", ["rot_random3", "rot_random7"])
def test_scan_form_changed_before_every_chunk_2mhz(emul_lib, name):
    res = run_case(emul_lib, name, ["depth0", "depth1", "depth2_lookahead"])
    for s in res.values():
        assert s["band_chunks"] >= 1 and s["bursts"] >= 20, res


def test_click_overflows_a_candidate_list_10mhz(emul_lib):
    """amplitude 0.5 (161 bursts from one frame, all of them records) at depth 2, amplitude 2.0 (squelch) at depth 3 with
    the packed records: fed in place with look-ahead, the scan chained behind the decline undone"""
    a = run_case(emul_lib, "click_0.5", ["depth2"])["depth2"]
    b = run_case(emul_lib, "click_2.0", ["depth3:packed"])["depth3:packed"]
    assert a["bursts"] == 171 and b["bursts"] == 10
    for s in (a, b):
        assert s["flags"] & dc.F_LIST and s["scan_chain_undone"] >= 1 and s["scan_chained"] >= 3, (a, b)


def test_noise_floor_drops_and_capacity_10mhz(emul_lib):
    res = run_case(emul_lib, "drop_10m", ["depth2"])
    assert res["depth2"]["scan_chain_undone"] >= 1, res
    res = run_case(emul_lib, "cap_10m", ["depth2"])
    assert res["depth2"]["flags"] & dc.F_GONECAP and res["depth2"]["scan_chain_undone"] >= 1, res


def test_scan_form_changed_before_every_chunk_10mhz(emul_lib):
    """scenes.many_active_10m in 14 chunks fed with look-ahead, each sequential form asked for twice in a row so that it runs
    although scans are chained (decline_checks.ROT_PAIRS); the cycle without repeats (ROT8), at every depth, is the card's"""
    res = run_case(emul_lib, "rot_many_10m_pairs", ["depth2_lookahead"])
    assert res["depth2_lookahead"]["bursts"] == 76 and res["depth2_lookahead"]["scan_chained"] >= 1, res
