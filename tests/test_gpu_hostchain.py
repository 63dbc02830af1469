"""swap_iq, irdm_dc_block, irdm_iq_balance and scrub together on the GPU: what the host feeds of a context leave in the history
ring, and the band a front end saves behind its twins of the four, against the numpy models composed in the documented order
-- exchange, DC, balance, scrub; DC's wire format in effect when both DC and balance are on -- byte for byte
(tests/hostchain_checks.py)."""
import pytest

import hostchain_checks as hc

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("wire", (hc.CF32, hc.CI16F), ids=("cf32", "ci16-full"))
def test_context_ring_equals_the_composed_models(wire):
    """a cf32 context at 2 MS/s, pipeline_depth 3, chunks of 65 536 and a ragged one of 4 321, dc_block_log2 12: every subset the
    wire format applies to (16 from cf32, the 12 with DC or balance on from ci16-full; with cf32 also all four from ci8) -- the
    history ring bit for bit, irdm_dc_stats and irdm_scrub_stats the models' figures.  The models tell the orders apart."""
    told = hc.order_facts(wire)
    assert told == ((16, 1) if wire == hc.CF32 else (10, 7))
    done = [hc.context_case(on, w) for on, w in hc.cases() if w == wire]
    assert done == [hc.N] * (16 if wire == hc.CF32 else 12)
    if wire == hc.CF32:
        assert hc.context_case(hc.ALL, hc.CI8) == hc.N


def test_context_primed_with_all_four_on():
    """irdm_prime_host: the ring is the model's of P || x, the recording's part the unprimed run's from its second DC block on;
    the scrub's figures are the recording's alone"""
    assert hc.context_prime_case() == 512 * 2048


def test_front_end_band_equals_the_band_of_the_modelled_stream():
    """a cf32 front end at 10 MS/s, D = 5, feed_host in chunks of 65 536, the band saved as cf32: 16 subsets from cf32 and 12
    from ci16-full, byte for byte the band of a plain front end fed the modelled stream; the figures the models'"""
    assert hc.front_end_cases() == 16 + 12


def test_front_end_primed_with_all_four_on():
    """irdm_frontend_prime_host: the band and the figures of the unprimed run"""
    assert hc.front_end_prime_case() >= hc.N // 5 - 1


def test_refusals_keep_their_sentences():
    """a device feed with a correction on: -1 and the sentence that names the remedy, byte for byte; ci8 objects refuse DC and
    balance and take the exchange alone"""
    assert hc.refusal_cases() == 5 * 4
