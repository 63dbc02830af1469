"""The per-burst resampler's prototype (option "burst_resample", csrc/host_design.cpp design_resample_taps) without a GPU.
For 25/24, 40/41, 30/29, 225/224, 400/401, 1025/1024, 1525/1536 and 4096/4097: the library's phase-major table -- the
context's where a sample rate has the ratio, the stage call's everywhere -- equals tests/burst_resample_model.py's bit for
bit; read back as the prototype at rate L f_in it is flat within 0.01 dB to 50 kHz and at least 80 dB down from 165 kHz on; a
constant row comes out constant within 1e-4 away from the edges; L = 4099 is refused."""
import burst_resample_checks as bc
from test_burst_resample_emul import run_case


def test_tables_equal_the_model_and_meet_the_response():
    res = run_case("taps")
    assert set(res) == {"%d/%d" % k for k in bc.TAPS_RATES}
    for name, r in res.items():
        assert r["ripple"] <= 0.01 and r["stop"] <= -80.0 and r["const"] <= 1e-4, (name, r)


def test_a_rate_whose_l_exceeds_4096_is_refused():
    assert run_case("refused") == {"refused": 1}
