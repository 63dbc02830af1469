"""The records of the two frame line estimators on the GPU (csrc/frame_line.hpp: symbol_clock_kernel, fine_freq_kernel)
against the bytes of tests/golden/line_records.json, which the CPU emulation gives too (tests/test_line_records_emul.py)."""
import pytest

import line_records

pytestmark = pytest.mark.gpu


def test_records_are_the_pinned_bytes():
    """irdm_symbol_clock_batch and irdm_fine_freq_batch over the kernel frames of clock_checks and fine_freq_checks (lengths
    63 / 64 / 65 / 255 / 1910 / 4439 / 4440; zero, NaN, Inf, noise; the line on either edge of the grid and beyond it) and their
    batches of 65 over launches of 64: every record byte for byte, 87 + 95 of them"""
    assert line_records.check(line_records.records()) == 87 + 95
