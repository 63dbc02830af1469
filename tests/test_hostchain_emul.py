"""swap_iq, irdm_dc_block, irdm_iq_balance and scrub together without a GPU: the host feeds of a context and of a front end on
the HIP emulation (tests/frontend_emul_build.py) against the numpy models composed in the documented order, byte for byte
(tests/hostchain_checks.py); each case in a process of its own.  And the models alone: the input tells the orders apart."""
import json
import os
import subprocess
import sys

import pytest

import frontend_emul_build
import hostchain_checks as hc

HERE = os.path.dirname(os.path.abspath(__file__))


def run_case(case, timeout=1500):
    env = dict(os.environ, IRDM_LIB=frontend_emul_build.build())
    p = subprocess.run([sys.executable, os.path.join(HERE, "hostchain_emul_run.py"), case], env=env, capture_output=True, text=True,
                       timeout=timeout)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    line = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")][-1]
    return json.loads(line[7:])


@pytest.mark.parametrize("fmt", (hc.CF32, hc.CI16F), ids=("cf32", "ci16-full"))
def test_the_input_tells_the_orders_apart(fmt):
    """CPU only, the models alone.  Over the 16 subsets there are 17 exchanges of two adjacent switched-on stages.  From cf32
    16 of them change the expected bytes and one -- exchange <-> scrub with nothing between them, which commute for every
    input -- leaves them; from ci16-full, which holds nothing for the scrub to take, the 10 without the scrub change them"""
    assert hc.order_facts(fmt) == ((16, 1) if fmt == hc.CF32 else (10, 7))


def test_context_ring_equals_the_composed_models():
    """a cf32 context at 2 MS/s, pipeline_depth 3, chunks of 65 536 and a ragged one of 4 321, dc_block_log2 12: all 16 subsets from
    cf32, the 12 with DC or balance on from ci16-full, all four from ci8 -- the history ring bit for bit, irdm_dc_stats and
    irdm_scrub_stats the models' figures"""
    assert run_case("context") == 16 + 12 + 1


def test_context_primed_with_all_four_on():
    """irdm_prime_host: the ring is the model's of P || x, the recording's part the unprimed run's from its second DC block on;
    the scrub's figures are the recording's alone"""
    assert run_case("context_prime") == 512 * 2048


def test_front_end_band_equals_the_band_of_the_modelled_stream():
    """a cf32 front end at 10 MS/s, D = 5, feed_host in chunks of 65 536, the band saved as cf32: 16 subsets from cf32 and 12
    from ci16-full, byte for byte the band of a plain front end fed the modelled stream; the figures the models'"""
    assert run_case("front_end") == 16 + 12


def test_front_end_primed_with_all_four_on():
    """irdm_frontend_prime_host: the band and the figures of the unprimed run"""
    assert run_case("front_end_prime") >= hc.N // 5 - 1


def test_refusals_keep_their_sentences():
    """a device feed with a correction on: -1 and the sentence that names the remedy, byte for byte; ci8 objects refuse DC and
    balance and take the exchange alone"""
    assert run_case("refusals") == 5 * 4
