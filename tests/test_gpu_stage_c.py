"""-m gpu: stage C alone (irdm_qpsk_demod_batch, irdm_qpsk_demod_packed_batch: demod_seq_kernel, demod_par_kernel,
demod_export of csrc/demod.hip) on the designed frames of tests/stage_c_cases.py, on the card, with either decimator:
lengths on either side of every decision, the end-of-frame rule, the unique word on either side of the hard and the soft
check under every input direction, the timing loop at its limits (the LDS sample ring read at its edges: 441 and 447
symbols), exact zeros under the PLL, noise.  Every record is compared with the oracle's orc_qpsk_demod: verdict,
direction, confidence, symbol counts and hard bits exactly, LLRs and level within parity.SOFT_TOL (level relative above 1),
total_phase within the project's 0.05 Hz on the refined frequency.  GPU against GPU, bit for bit over the whole record: the
batch reversed (lane 0 against lane 31, first workgroup against last, first launch against second: the corpus is larger than
the context's 64 bursts per launch), the rows padded with 1e30 instead of zeros, batches of 1, 32 and 33; and the packed
export against the full records.  One context per decimator, the Gardner one closed before the simple one opens;
tests/test_stage_c_emul.py runs the same corpus on the CPU emulation."""
import time

import numpy as np
import pytest

import irdm
import stage_c_cases as sc

pytestmark = pytest.mark.gpu


class Ctx:
    def __init__(self, gardner):
        self.gardner = gardner
        self.cases = sc.cases()
        self.frames = [c.iq for c in self.cases]
        self.dirs = [c.direction for c in self.cases]
        sc.reference(gardner)                # (the oracle's records, computed once, are not part of the times printed)
        self.p = irdm.Pipeline(2_000_000, max_chunk_samples=32768 * 4, max_bursts_per_chunk=64, use_gardner=gardner)
        self._full = None

    @property
    def full(self):
        """irdm_qpsk_demod_batch's records of the corpus in order: what the GPU-against-GPU tests compare with"""
        if self._full is None:
            self._full = self.p.qpsk_demod_batch(self.frames, self.dirs)
        return self._full


@pytest.fixture(scope="module", params=(1, 0), ids=("gardner", "simple"))
def ctx(request):
    c = Ctx(request.param)
    yield c
    c.p.close()


def test_designed_frames_match_the_oracle(ctx):
    assert len(ctx.cases) > 64               # (two launches on reused rows)
    t = time.time()
    res = sc.run(ctx.p, ctx.gardner)
    w = res["worst"]
    print("stage C corpus, use_gardner %d: %d cases (%d accepted) in %.2f s; largest differences from the oracle: level %.3g "
          "(relative above 1), LLR %.3g, total_phase %.3g rad (%.4f Hz of the refined frequency)"
          % (ctx.gardner, res["cases"], res["accepted"], time.time() - t, w["level"], w["llr"], w["total_phase"],
             w["total_phase_hz"]))
    assert res["accepted"] >= 0.7 * res["cases"]


def test_a_record_does_not_depend_on_the_position_in_the_batch(ctx):
    rev = ctx.p.qpsk_demod_batch(ctx.frames[::-1], ctx.dirs[::-1])[::-1]
    bad = [c.name for c, a, b in zip(ctx.cases, ctx.full, rev) if bytes(a) != bytes(b)]
    assert not bad, bad


def test_a_record_does_not_depend_on_what_lies_behind_num_samples(ctx):
    """the kernel stages the samples behind a frame's end into its LDS ring and must never interpolate them"""
    pad = ctx.p.qpsk_demod_batch(ctx.frames, ctx.dirs, pad=1e30)
    bad = [c.name for c, a, b in zip(ctx.cases, ctx.full, pad) if bytes(a) != bytes(b)]
    assert not bad, bad


@pytest.mark.parametrize("n", (1, 32, 33))
def test_batch_sizes(ctx, n):
    i = [c.name for c in ctx.cases].index("len_4440")
    assert ctx.full[i].ok and ctx.full[i].n_symbols == 444
    out = ctx.p.qpsk_demod_batch([ctx.frames[i]] * n, [ctx.dirs[i]] * n)
    assert len(out) == n and all(bytes(d) == bytes(ctx.full[i]) for d in out)


@pytest.mark.parametrize("keep_bits", (1, 0))
def test_packed_export_is_the_full_record(ctx, keep_bits):
    """irdm_qpsk_demod_packed_batch: demod_export's record in pinned memory -- the six scalars bit for bit those of the full
    record, the bits np.packbits of its bits, zero behind n_bits and for a rejected frame; with keep_bits the full record
    beside it, bits and LLRs bit for bit -- at 12, 13, 14, 15 symbols (a last byte of 1, 2, 3 symbols), 100 (a word of one
    byte), 441, 444 and 447 (the last word)"""
    seen = sc.run_packed(ctx.p, keep_bits, ctx.full)
    want = {12, 13, 14, 15, 100, 441, 444, 447} if ctx.gardner else {12, 13, 14, 15, 100, 444}
    assert want <= seen, sorted(want - seen)
    rejected = [f for f in ctx.full if not f.ok]
    assert len(rejected) >= 8
