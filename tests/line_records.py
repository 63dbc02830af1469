"""TEST INFRASTRUCTURE: the pinned records of the two frame line estimators (csrc/frame_line.hpp: symbol_clock_kernel and
fine_freq_kernel).  tests/golden/line_records.json holds, per estimator and named frame, the bytes of the public record
that irdm_symbol_clock_batch / irdm_fine_freq_batch give, as hex, beside a hash of the frame's samples; the GPU test
(tests/test_gpu_line_records.py) and the CPU-emulation test (tests/line_records_emul_run.py) ask for the same bytes.  The
MI355X and the CPU emulation give the same bytes for every frame, so the file has one section."""
import hashlib
import json
import os

import numpy as np

import clock_checks as cc
import fine_freq_checks as fc
import irdm

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "line_records.json")
BATCH = 65          # one launch of 64 bursts and one of 1


def named_frames(checks):
    """name -> frame: the kernel frames of a checks module, then its batch of 65 (which begins with the kernel frames again,
    at other rows of other launches, and goes on with cuts at lengths and offsets of their own)"""
    out = {"kernel/" + k: x for k, x in checks.kernel_frames().items()}
    out.update(("batch%d/%02d" % (BATCH, i), x) for i, x in enumerate(checks.batch_frames(BATCH)))
    return out


def records():
    """{"clock" / "fine": {name: {"frame": hash of the samples, "rec": hex of the record}}} from the library irdm loads, over a
    context of 64 bursts per launch: each set of frames in one call of its own, as the stage checks make them"""
    p = irdm.Pipeline(2_000_000, max_chunk_samples=32768 * 8, max_bursts_per_chunk=64, pipeline_depth=0)
    try:
        out = {}
        for est, checks, call in (("clock", cc, p.symbol_clock_batch), ("fine", fc, p.fine_freq_batch)):
            fr = named_frames(checks)
            names = list(fr)
            nk = len(checks.kernel_frames())
            got = call([fr[k] for k in names[:nk]]) + call([fr[k] for k in names[nk:]])
            assert len(got) == len(names)
            out[est] = {k: dict(frame=hashlib.sha256(np.ascontiguousarray(fr[k], np.complex64).tobytes()).hexdigest()[:16],
                                rec=bytes(g).hex()) for k, g in zip(names, got)}
        return out
    finally:
        p.close()


def check(got):
    """`got` of records() against the file: the same frames, and of every frame the same bytes; returns the number compared"""
    want = json.load(open(GOLDEN))["records"]
    assert sorted(got) == sorted(want)
    n = 0
    for est in want:
        assert list(got[est]) == list(want[est]), (est, "the frames' names")
        for k, w in want[est].items():
            g = got[est][k]
            assert g["frame"] == w["frame"], (est, k, "the frame's samples differ: the test's input, not the kernel")
            assert g["rec"] == w["rec"], (est, k, g["rec"], w["rec"])
            n += 1
    return n
