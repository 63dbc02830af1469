"""The carrier frequency estimator on the GPU (option fine_freq, csrc/fine_freq.hpp): the kernel against the float64 model
of tests/fine_freq_model.py through irdm_fine_freq_batch; the context option off and on against the truth of the scenes, on
the full and the packed record path, in one feed and in three; irdm_reset; the 4440-sample frames of a 10 MHz scene."""
import pytest

import fine_freq_checks as fc
import irdm

pytestmark = pytest.mark.gpu


def test_kernel_equals_the_model():
    """irdm_fine_freq_batch on the frames of fine_freq_checks.kernel_frames (the oracle's frames of the 10 MHz scene; lengths
    63 / 64 / 65 / 255 / 1910 / 4439 / 4440; all zero, NaN, Inf, noise; the line on either edge of the grid and 120 Hz beyond
    it) and in batches of 1, 63 and 65 frames over a context of 64 bursts per launch: flags and n equal the model's,
    |df - df_model| <= 1e-3 Hz, quality within 1e-6"""
    p = irdm.Pipeline(2_000_000, max_chunk_samples=32768 * 8, max_bursts_per_chunk=64, pipeline_depth=0)
    try:
        res = fc.stage_cases(p)
    finally:
        p.close()
    print(res)
    assert res["frames"] >= 7 + 16 + 7 and res["worst"] <= fc.DF_TOL and res["worst_quality"] <= fc.QUALITY_RTOL


def test_context_2mhz():
    """the 2 MHz seed-3 scene with the option off and on, full and packed records: every field but center_frequency bit
    for bit; center_frequency of applied frames is freq_hz of their record and within 4 Hz of truth (the PLL's is up to 33 Hz
    off); fine_freq_launches 0 with the option off; one feed at depth 0 and three at depth 1 give the same records;
    irdm_reset restarts the summary; the bit layer's records inherit the frequency; a group refuses the option"""
    seen = fc.context_checks("standard", (2_000_000, 3, 0.05), 14)
    print(seen)
    assert seen["full"] == seen["packed"] >= 14 and seen["pll_worst"] > 15.0
    fc.group_refuses()


def test_context_10mhz_long_frames():
    """the 10 MHz scene, whose frames are 1910 and 4440 samples long: the same with the option off and on, both paths"""
    seen = fc.context_checks("standard", (10_000_000, 3, 0.05), 14, lengths=(1910, 4440), thorough=False)
    print(seen)
    assert seen["full"] == seen["packed"] >= 14
