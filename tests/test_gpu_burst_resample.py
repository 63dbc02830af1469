"""-m gpu: option "burst_resample" on the device -- the checks of tests/test_burst_resample_emul.py (tests/burst_resample_checks.py)
with burst_resample_kernel running on the GPU: the stage call against the float32 model bit for bit, one launch per ratio; the
off-grid scenes at 2.4, 2.05, 10.025 and 10.24 MS/s (the any-M decimator at M = 10, 8 and 41, the register-resident <40>, FFT
sizes 2048 and 8192) with the option off and on; a rate on the grid; the record modes, depths and chunk sizes."""
import pytest

import burst_resample_checks as bc

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("L,M", bc.STAGE_RATIOS)
def test_kernel_equals_the_model(L, M):
    res = bc.check_stage(L, M)
    assert res["rows"] == len(bc.STAGE_LENGTHS) + 3


@pytest.mark.parametrize("fs", [2_400_000, 2_050_000, 10_025_000, 10_240_000])
def test_off_grid_frames_come_out_whole(fs):
    res = bc.case_pipeline(fs)
    assert res["whole_on"] == res["frames"] >= 6, res


def test_on_the_grid_nothing_changes_and_nothing_is_launched():
    assert bc.case_ongrid()["frames"] >= 6


def test_record_modes_depths_and_chunk_sizes_agree():
    assert bc.case_modes()["frames"] >= 6


def test_tables_and_refusals():
    assert set(bc.case_taps()) == {"%d/%d" % k for k in bc.TAPS_RATES}
    assert bc.case_refused() == {"refused": 1}
