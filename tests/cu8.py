"""Helpers of the cu8 tests (tests/test_gpu_cu8.py, tests/cu8_emul_run.py): rtl_sdr's unsigned 8-bit I/Q.

The contract (include/irdm_hip.h, IRDM_FMT_CU8): a cu8 context produces exactly the records of a cf32 context fed
(u - 127.5) / 128.  run / same_records / chunks_of are those of tests/formats16.py, which take any integer format."""
import numpy as np

import irdm
import siggen


def to_cu8(iq, scale=512.0):
    """u = clip(round(x * scale + 127.5), 0, 255): mid-scale 127.5, as an offset-binary converter has it"""
    x = np.empty(2 * len(iq), dtype=np.float32)
    x[0::2] = iq.real
    x[1::2] = iq.imag
    return np.clip(np.round(x * np.float32(scale) + np.float32(127.5)), 0, 255).astype(np.uint8)


def converted(u):
    """interleaved uint8 -> the cf32 stream a cu8 context sees"""
    return irdm.convert_cu8(u)


def cu8_scene(fs, secs, nb, seed, scale=512.0):
    n = int(secs * fs) // 32768 * 32768
    iq, _ = siggen.standard_scene(fs, n, nb, seed=seed)
    return to_cu8(iq, scale)
