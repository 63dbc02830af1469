"""Stream positions around 2^31, 2^32, 2^44 and 2^52 without a GPU: the 2 MHz cases of tests/test_gpu_farpos.py (band scan,
any-M decimator), one at 10 MHz (resident decimator) and two front-end cases on the CPU emulation of the product, each in a
process of its own (tests/farpos_emul_run.py), and the layout that tests/farpos.py's shift_state relies on."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import emul_build
import farpos
import resample_emul_build

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def emul_lib():
    return emul_build.build()


def run_case(lib, case, timeout=1200):
    p = subprocess.run([sys.executable, os.path.join(HERE, "farpos_emul_run.py"), case], env=dict(os.environ, IRDM_LIB=lib),
                       capture_output=True, text=True, timeout=timeout)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    line = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")][-1]
    return json.loads(line[7:])


def test_shift_state_offsets_match_the_structures():
    """the byte offsets shift_state patches are those of StateHeader (csrc/state.cpp), DetState and ActiveBurst
    (csrc/types.hpp) written out as ctypes structures; sizes as the sources' comments and static layout give them"""
    H, D, A = farpos.StateHeader, farpos.DetState, farpos.ActiveBurst
    assert C.sizeof(H) == 56 and C.sizeof(A) == farpos.ACT_SIZE == 40 and C.sizeof(D) == 40 + 40 * farpos.K_MAX_ACTIVE
    assert H.total_samples.offset == farpos.OFF_TOTAL == 24
    assert C.sizeof(H) + D.index.offset == farpos.OFF_INDEX == 56
    assert C.sizeof(H) + D.n_act.offset == farpos.OFF_N_ACT == 84
    assert C.sizeof(H) + D.act.offset == farpos.OFF_ACT == 96
    assert A.start.offset == farpos.ACT_START == 8 and A.last_active.offset == farpos.ACT_LAST == 16
    assert C.sizeof(H) + C.sizeof(D) == farpos.HEAD_BYTES
    # the structures are the sources': field names and order as csrc/state.cpp and csrc/types.hpp declare them
    root = os.path.dirname(HERE)
    state = open(os.path.join(root, "iridium-sniffer_amd", "csrc", "state.cpp")).read()
    types = open(os.path.join(root, "iridium-sniffer_amd", "csrc", "types.hpp")).read()
    assert "uint64_t magic, n, hist, total_samples, tagged, start_time_ns;\n    int32_t host_primed, host_hist_idx;" in state
    assert ("struct ActiveBurst {\n    uint64_t id, start, last_active;\n    int32_t center_bin;\n    float peak_rel, base_sum;\n"
            "    int32_t pad;\n};") in types
    det = types[types.index("struct DetState {"):]
    det = det[:det.index("};")]
    names = [l.split("//")[0].strip() for l in det.splitlines()[1:]]
    assert names == ["uint64_t index;", "uint64_t burst_id;", "int32_t hist_idx, primed, squelch, n_act;", "uint32_t n_gone;",
                     "uint32_t overflow;", "ActiveBurst act[kMaxActive];"], names
    assert "constexpr int kMaxActive = %d;" % farpos.K_MAX_ACTIVE in types
    # shift_state on a blob made from the structures: the positions move, nothing else does
    blob = np.zeros(farpos.HEAD_BYTES + 64, np.uint8)
    h, d = H.from_buffer(blob), D.from_buffer(blob, C.sizeof(H))
    h.total_samples, h.tagged, h.start_time_ns = 1000, 7, 1700000000 * 10**9
    d.index, d.burst_id, d.n_act = 1024, 30, 2
    for i in range(3):
        d.act[i].id, d.act[i].start, d.act[i].last_active = 10 * i, 100 + i, 200 + i
    K = (1 << 44) + 5 * 32768
    out = farpos.shift_state(blob, K)
    h2, d2 = H.from_buffer(out), D.from_buffer(out, C.sizeof(H))
    assert (h2.total_samples, h2.tagged, h2.start_time_ns) == (1000 + K, 7, 1700000000 * 10**9)
    assert (d2.index, d2.burst_id, d2.n_act) == (1024 + K, 30, 2)
    assert [(a.id, a.start, a.last_active) for a in d2.act[:3]] == [(0, 100 + K, 200 + K), (10, 101 + K, 201 + K), (20, 102, 202)]
    assert np.array_equal(farpos.shift_state(out, -K), blob)


@pytest.mark.parametrize("where", [31, 32, 44, 52])
def test_pipeline_2mhz_far_out(emul_lib, where):
    """K just under 2^31 and 2^32 (a burst of B across it), 2^44 + 12345 * 32768 and 2^52 + 7 * 32768: depth 0 whole and
    depth 3 fed in place with look-ahead"""
    res = run_case(emul_lib, str(where))
    for form in ("whole", "lookahead"):
        assert res[form]["bursts"] == 12 and res[form]["demods"] == 8, res


def test_resident_decimator_10mhz_across_2_to_32(emul_lib):
    """fir_reg.hip's <40> kernel is the only reader of FirGeom.ring_pos / stale_pos (downmix.hip): the any-M decimator of
    the 2 MHz cases indexes the ring itself (burst_src.hpp), so one case runs at 10 MHz"""
    res = run_case(emul_lib, "10mhz")
    assert res["10mhz"]["bursts"] == 6 and res["10mhz"]["demods"] == 6, res


def test_packed_records_far_out(emul_lib):
    res = run_case(emul_lib, "packed")
    assert res["packed"]["bursts"] == 12 and res["packed"]["demods"] == 8, res


def test_third_context_imports_the_second_ones_state_unpatched(emul_lib):
    res = run_case(emul_lib, "two_hops")
    assert res["two_hops"]["bursts"] == 12 and res["two_hops"]["demods"] == 8, res


def test_state_after_the_run_far_out(emul_lib):
    run_case(emul_lib, "state")


def test_positions_from_2_to_53_on_are_refused(emul_lib):
    res = run_case(emul_lib, "limit")
    assert res["limit"]["bursts"] == 12, res


def test_front_ends_behind_a_seek():
    """K0 at D = 5 and K0r at 25/24 sought to just under 2^32 (crossed inside the run) and above 2^40, and the seek's refusals"""
    res = run_case(resample_emul_build.build(), "frontend")
    assert len(res) == 4 and all(v > 20000 for v in res.values()), res
