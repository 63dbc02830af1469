"""irdm_prime_host / irdm_prime_device / irdm_frontend_prime_host on the GPU: a context primed from the recording's own head
against the CPU oracle run over P || x with start time T0' (P: the 512-frame prefix tiled from the head, built in numpy by
tests/prime_checks.py), at one rate per detector scan -- 1 MHz dense, 2 MHz band scan, 16 MHz wave walk --, with the
options that change what the detector sees, with the side passes, from a resident buffer, and behind the front end."""
import functools

import numpy as np
import pytest

import frontend_model as fm
import irdm
import orc
import parity
import prime_checks as pc
import rates
import resample_model as rm

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("depth", (0, 3))
@pytest.mark.parametrize("name", ("full", "excerpt"))
def test_scenes_of_the_readme_table(name, depth):
    """the 3 000 000-sample scene with 6 bursts inside the first 512 frames: 16 bursts / 16 frames primed, 10 / 10 after
    irdm_reset without priming; its 700 000-sample excerpt, primed from itself tiled: 6 / 6 against 0 / 0; every record
    equal to the oracle's over P || x; irdm_prime_host behind a feed returns -1"""
    res = pc.scene_case(name, depth)
    want = dict(full=((16, 16), (10, 10)), excerpt=((6, 6), (0, 0)))[name]
    assert (res["primed"]["bursts"], res["primed"]["demods"]) == want[0]
    assert (res["plain"]["bursts"], res["plain"]["demods"]) == want[1]


def check_scan_ran(stats, fs):
    """the scan the rate is dispatched to did the work.  (Not tests/rates.py's check_scan: that one also wants no fallback,
    and in 16-frame chunks the wave walk gives up the one chunk in which the history fills -- a plain context fed P || x in
    the same chunks counts the same single fallback, the same 63 fast chunks and 528 dense frames.)"""
    scan = rates.describe(fs)["scan"]
    if scan == "band":
        assert stats["band_chunks"] >= 1 and stats["scan_fallbacks"] == 0, (fs, stats)
    elif scan == "wave":
        assert stats["band_chunks"] == 0 and stats["scan_fast_chunks"] >= 1 and stats["scan_fallbacks"] <= 1, (fs, stats)
    else:
        assert stats["band_chunks"] == 0 and stats["scan_fast_chunks"] == 0, (fs, stats)


@pytest.mark.parametrize("max_chunk", (pc.CHUNK, 0), ids=("256Ki", "default"))
@pytest.mark.parametrize("depth", (0, 3))
@pytest.mark.parametrize("fmt", (irdm.FMT_CF32, irdm.FMT_CI8), ids=("cf32", "ci8"))
@pytest.mark.parametrize("fs", (1_000_000, 2_000_000, 16_000_000))
def test_every_scan_equals_the_oracle_over_the_prefixed_stream(fs, fmt, depth, max_chunk):
    """the smallest scene of tests/rates.py at the rate (16 MHz: its last 500 frames, so the prefix is tiled); max_chunk
    262 144 (the prefix spans 2, 4 and 32 feeds) and the library's default (one feed); the scan the rate is dispatched to
    did the work"""
    x, ref = pc.rate_stream(fs, fmt)
    stats = {}

    def after(p, out):
        stats.update({k: p.stat(k) for k in parity.STAT_KEYS})

    got = pc.run_primed(x, fs, fmt=fmt, depth=depth, max_chunk=max_chunk, after=after)
    rates.check_counts(parity.compare(got, ref))
    check_scan_ran(stats, fs)


@pytest.mark.parametrize("fs", (2_000_000, 16_000_000))
def test_prime_device_gives_prime_hosts_records(fs):
    """irdm_prime_device from a resident buffer: byte for byte the record queues of irdm_prime_host, and the oracle's"""
    x, ref = pc.rate_stream(fs, irdm.FMT_CF32)
    host = pc.run_primed(x, fs, depth=3, how="host")
    dev = pc.run_primed(x, fs, depth=3, how="device")
    assert pc.records_bytes(host) == pc.records_bytes(dev) and host["tagged"] == dev["tagged"]
    rates.check_counts(parity.compare(dev, ref))


def test_packed_records_of_a_primed_stream():
    """option packed_records: the compact records equal the oracle's over P || x (tests/parity.py compare_packed)"""
    x, ref, _ = pc.scene("full")
    got = pc.run_primed(x, pc.FS, depth=3, packed=True)
    assert parity.compare_packed(got, ref)["demods"] == 16


@pytest.mark.parametrize("depth", (0, 3))
def test_swap_balance_and_scrub_apply_to_the_prefix(depth):
    """swap_iq, irdm_iq_balance and scrub on together: byte for byte the records of a plain context with the three on, start
    time T0', fed P || x; the scrub's figures count the recording alone"""
    assert pc.options_case(depth) == dict(demods=6)


@pytest.mark.parametrize("depth", (0, 3))
def test_side_passes_describe_the_recording_alone(depth):
    """input_stats, iq_moments, scrub and spectrum_frames: exactly the results of a plain context fed x alone with start time
    T0, positions and row times included"""
    assert pc.side_case(depth) == dict(rows=4)


def test_refused_for_a_member_of_a_group():
    g = irdm.Group(pc.FS, 1, max_chunk_samples=pc.CHUNK, pipeline_depth=1)
    try:
        x = np.zeros(4096, np.complex64)
        assert irdm.lib().irdm_prime_host(g.member(0), x.ctypes.data, len(x)) == -1
    finally:
        g.close()


# ---------------------------------------------------------------- behind the front end ----
def front_end_case(make_fe, x, y, out_rate, applied, depth, chunk_in):
    """the capture x (ci8) through a front end that saves its band as cf32 and counts its input, unprimed and primed: the
    saved band and the input figures are the same bytes; the unprimed band is the model's y; the primed context's records
    equal the oracle's over P(y) || y"""
    ref = orc.run_stream(np.concatenate([pc.prefix(y, out_rate)[0], y]), out_rate, center_frequency=1622000000.0 + applied,
                         start_time_ns=pc.shifted_origin(out_rate))
    assert len(ref.demods) >= 6
    out = {}
    for primed in (False, True):
        fe = make_fe()
        p = irdm.Pipeline(out_rate, fmt=irdm.FMT_CF32, center_frequency=1622000000.0 + applied, max_chunk_samples=1 << 20,
                          max_bursts_per_chunk=1024, pipeline_depth=depth, start_time_ns=pc.T0)
        try:
            p.set_option("keep_frame_samples", 1)
            fe.save(irdm.FMT_CF32)
            fe.input_stats_enable()
            if primed:
                assert fe.prime_host(p, x) == pc.HISTORY
                H = pc.HISTORY * p.fft_size
                assert (p.primed_samples, p.start_time_ns, p.sample_count) == (H, pc.shifted_origin(out_rate), H)
                assert fe.saved == []
            for off in range(0, len(x) // 2, chunk_in):
                fe.feed_host(p, x[2 * off:2 * (off + chunk_in)])
            fe.flush(p)
            bursts = p.poll_bursts()
            infos, samples = p.poll_frames()
            out[primed] = dict(band=b"".join(fe.saved), stats=bytes(fe.input_stats()), bursts=bursts, infos=infos, samples=samples,
                               demods=p.poll_demods(), tagged=p.tagged, n_samples=p.sample_count)
        finally:
            p.close()
            fe.close()
    assert out[False]["band"] == y.tobytes()
    assert out[True]["band"] == out[False]["band"] and out[True]["stats"] == out[False]["stats"]
    assert out[True]["n_samples"] == len(y) + pc.HISTORY * pc.fft_size(out_rate)
    return parity.compare(out[True], ref)


@pytest.mark.parametrize("depth", (0, 3))
def test_front_end_prime(depth):
    """irdm_frontend_prime_host in front of K0: the wideband scene of tests/test_gpu_frontend.py (50 MS/s ci8, decimated by 5)"""
    x, expect, q = fm.wideband_scene()
    s = fm.SCENE
    fe = irdm.Frontend(s["fs_in"], irdm.FMT_CI8, s["D"], s["shift_hz"])
    taps, applied = fe.taps(), fe.applied_shift_hz
    fe.close()
    y = fm.run(x, irdm.FMT_CI8, s["D"], q, taps)
    summary = front_end_case(lambda: irdm.Frontend(s["fs_in"], irdm.FMT_CI8, s["D"], s["shift_hz"]), x, y, s["fs_in"] // s["D"], applied,
                             depth, s["D"] << 20)
    assert summary["demods"] >= s["n_inband"], summary


@pytest.mark.parametrize("depth", (0, 3))
def test_rational_front_end_prime(depth):
    """... and in front of K0r: the 11.2 -> 10 MS/s scene of tests/test_gpu_resample.py (ratio 25 / 28)"""
    s = rm.SCENES["11.2->10"]
    x, expect = rm.offgrid_scene("11.2->10", irdm.FMT_CI8)
    shift = 150_000.0
    make = functools.partial(irdm.Frontend.rational, s["in_rate"], irdm.FMT_CI8, s["out_rate"], shift)
    fe = make()
    taps, applied = fe.taps(), fe.applied_shift_hz
    fe.close()
    y = rm.run(x, irdm.FMT_CI8, 25, 28, fm.quantise(shift, s["in_rate"]), taps)
    summary = front_end_case(make, x, y, s["out_rate"], applied, depth, (1 << 20) * 28 // 25)
    assert summary["demods"] >= len(expect), summary
