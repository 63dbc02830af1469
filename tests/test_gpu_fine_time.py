"""The symbol timing estimator on the GPU (option fine_time, csrc/fine_time.hpp): the kernel against the float64 model of
tests/fine_time_model.py and the records of tests/golden/fine_time_records.json through irdm_fine_time_batch; the context
option off and on against the truth of the scenes, on the full and the packed record path, in one feed and in three;
irdm_reset; the 10 MHz scene with its simplex frame."""
import pytest

import fine_time_checks as fc
import irdm

pytestmark = pytest.mark.gpu


def test_kernel_equals_the_model():
    """irdm_fine_time_batch on the frames of fine_time_checks.kernel_frames (the oracle's frames of the 2 MHz seed-3 scene; cuts
    to 63 / 64 / 65 / 799 / 800 / 801 / 1309 / 1310 / 1311 / 4440 samples, simplex flag both ways; all zero, NaN, Inf, noise;
    synthetic frames with tau at -4.9, 0, +4.9) and in batches of 1, 63 and 65 frames over a context of 64 bursts per launch:
    flags and n equal the model's, |tau - tau_model| <= 1e-9 samples, quality within 1e-6, and Re, Im and the floor of every
    record bit for bit those the CPU emulation gave"""
    p = irdm.Pipeline(2_000_000, max_chunk_samples=32768 * 8, max_bursts_per_chunk=64, pipeline_depth=0)
    try:
        res = fc.stage_cases(p)
    finally:
        p.close()
    print(res)
    assert res["frames"] == res["golden"] >= 16 + 2 * len(fc.CUTS) + 5 + 3
    assert res["worst"] <= fc.TAU_TOL and res["worst_quality"] <= fc.QUALITY_RTOL


def test_context_2mhz():
    """the 2 MHz seed-3 scene with the option off and on, full and packed records: every field but timestamp bit for bit;
    the timestamp is time_ns of the frame's polled record, the model's host rule on the frame record's fields, and within
    0.52 us of truth (the unrefined one wanders by 7 us); fine_time_launches 0 with the option off; one feed at depth 0 and
    three at depth 1 give the same records; irdm_reset restarts the summary; the bit layer's records inherit the time; a
    group refuses the option"""
    seen = fc.context_checks((2_000_000, 3, 0.05), 14)
    print(seen)
    assert seen["full"] == seen["packed"] >= 14 and seen["unrefined_spread_ns"] > 5000.0
    fc.group_refuses()


def test_context_10mhz():
    """the 10 MHz seed-3 scene, 10 M samples, one of whose frames is a simplex one (the 800-sample window): the same with the
    option off and on, both paths, within 1.02 us of truth"""
    seen = fc.context_checks((10_000_000, 3, 0.05), 14, thorough=False)
    print(seen)
    assert seen["full"] == seen["packed"] >= 14
