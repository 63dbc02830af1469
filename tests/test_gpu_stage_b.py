"""-m gpu: stage B alone (irdm_downmix_burst) on the designed burst windows of tests/stage_b_cases.py, on the card: every early
return of burst_downmix.c, the length thresholds, silence, frames shorter than the CFO estimator's input and longer than the
demodulator takes, the simplex rules -- at every class of stream position (start % 8 = 0: the register-resident decimators
fir_decimate_kernel_f / _r at 10 and 12 MHz; start % 8 = 3: the LDS decimator at M = 40 / 48 / 80; windows that end where
the detector's feed block had not delivered them; a start past 2^33), in both FIR orders and in the generic kernel forms.
Every call is compared with the oracle's orc_downmix_process the way parity.compare compares a frame, frame samples bit
for bit.  One context per rate; tests/test_stage_b_emul.py runs the same corpus on the CPU emulation."""
import time

import pytest

import irdm
import stage_b_cases as sb

pytestmark = pytest.mark.gpu

RATES = (2_000_000, 4_000_000, 10_000_000, 12_000_000, 20_000_000)


@pytest.fixture(scope="module")
def context():
    """the context of the rate asked for; the previous rate's is closed first (2 s of history ring each)"""
    held = {}

    def get(fs):
        if fs not in held:
            for p in held.values():
                p.close()
            held.clear()
            held[fs] = irdm.Pipeline(fs, max_chunk_samples=32768 * 8, max_bursts_per_chunk=64)
        return held[fs]

    yield get
    for p in held.values():
        p.close()


def _run(p, fs, fir_order, **options):
    sb.windows(fs)                           # (the corpus, built once per rate, is not part of the time reported)
    p.set_option("fir_order", fir_order)
    for k, v in options.items():
        p.set_option(k, v)
    try:
        t = time.time()
        res = sb.run(p, fs, fir_order)
        print("stage B corpus at %d Hz, fir_order %d %s: %d calls in %.2f s (oracle included), drop reasons %s"
              % (fs, fir_order, options, res["calls"], time.time() - t, res["hist"]))
    finally:
        p.set_option("fir_order", 1)
        for k in options:
            p.set_option(k, 0)
    assert res["calls"] >= 36 * 6
    return res


@pytest.mark.parametrize("fir_order", (1, 0))
@pytest.mark.parametrize("fs", RATES)
def test_designed_windows_match_the_oracle(context, fs, fir_order):
    _run(context(fs), fs, fir_order)


@pytest.mark.parametrize("option", ("post_generic", "fir_generic"))
@pytest.mark.parametrize("fs", (2_000_000, 10_000_000))
def test_designed_windows_generic_kernel_forms(context, fs, option):
    """test hooks post_generic (the runtime-tap-count instances of post_tiles / post_cfo / post2) and fir_generic (always the
    any-M decimator)"""
    _run(context(fs), fs, 1, **{option: 1})
