"""-m gpu: the pipeline and both front ends at stream positions around 2^31, 2^32, 2^44 and 2^52 samples, and the refusal
of positions from 2^53 on.

No stream of that length is fed: the position is a number the C-ABI lets a caller set (tests/farpos.py).  Context A takes
[0, cut) of a scene of at most 2.7 s; its exported state, every position in it moved up by K, goes to a context B whose
history ring is seeded at cut + K; B takes the rest.  B's records, moved down by K again, go through tests/parity.py's
compare / compare_packed against the oracle on the unshifted scene, unchanged: integers, dB fields and frame samples bit for
bit, hard bits and confidence exact, soft outputs within SOFT_TOL.  A front end is sought to its position
(irdm_frontend_seek) and compared with the C models bit for bit.

Every pipeline case asserts, besides parity:
(a) a burst that B emitted has start < 2^k <= start + num_samples at its shifted position, 2^k the power of two the case
    is about.  (The cases at K = 2^44 + 12345 * 32768 and 2^52 + 7 * 32768 lie wholly ABOVE their power of two -- that is
    what they are about: every position's high word is non-zero -- so they assert that every burst of B starts above it.)
(b) B emitted at least 5 bursts and 4 demodulated frames;
(c) B's scan_fallbacks is what the same split of the same scene gives at K = 0 (that run, compared with the oracle too, is
    made once per configuration and shared).

tests/test_farpos_emul.py runs the 2 MHz cases of this module, and one at 10 MHz, on the CPU emulation of the product."""
import functools

import numpy as np
import pytest

import farpos
import irdm
import orc
import parity
import rates
import siggen

pytestmark = pytest.mark.gpu

K44 = (1 << 44) + 12345 * 32768
K52 = (1 << 52) + 7 * 32768
FMT_NAMES = {irdm.FMT_CF32: "cf32", irdm.FMT_CI8: "ci8", irdm.FMT_CI16: "ci16", irdm.FMT_CI16_FULL: "ci16-full",
             irdm.FMT_CU8: "cu8", irdm.FMT_CI32: "ci32"}


@functools.lru_cache(maxsize=None)
def _cf32(fs):
    """2 MHz: the scene of test_time_chunk_handoff_equals_single_context (12 bursts); else tests/rates.py's six bursts"""
    if fs == 2_000_000:
        iq = siggen.standard_scene(fs, int(2.6 * fs), 10, seed=18, uplink_every=4)[0]
    else:
        iq = rates.stream(fs)
    iq.setflags(write=False)
    return iq


@functools.lru_cache(maxsize=None)
def scene(fs, fmt=irdm.FMT_CF32, fir_order=1):
    """(samples in the format's own codes, the oracle's records, the cut): generated once and shared, never written to"""
    iq = _cf32(fs)
    if fmt == irdm.FMT_CF32:
        x, seen, ofmt = iq, iq, 2
    elif fmt == irdm.FMT_CI8:
        x = siggen.to_ci8(iq)
        seen, ofmt = x, 0
    elif fmt == irdm.FMT_CI16:
        x = siggen.to_ci16(iq)
        seen, ofmt = x, 1
    elif fmt == irdm.FMT_CI16_FULL:          # (records equal a cf32 context's on the converted stream: include/irdm_hip.h)
        import formats16
        x = siggen.to_ci16(iq)
        seen, ofmt = formats16.converted(x, fmt), 2
    elif fmt == irdm.FMT_CU8:
        import cu8
        x = cu8.to_cu8(iq)
        seen, ofmt = cu8.converted(x), 2
    elif fmt == irdm.FMT_CI32:
        import ci32
        x = ci32.to_ci32(iq, fmt)
        seen, ofmt = ci32.converted(x, fmt), 2
    else:
        raise ValueError(fmt)
    orc.set_fir_order(fir_order)
    try:
        ref = orc.run_stream(seen, fs, fmt=ofmt)
    finally:
        orc.set_fir_order(1)
    x.setflags(write=False)
    return x, ref, farpos.cut_inside_a_burst(ref, rates.fft_size(fs))


def _form(form, n_rest, parts):
    """depth 0 whole, or pipeline_depth 3 fed in place with look-ahead in `parts` chunks"""
    if form == "whole":
        return dict(depth=0, chunks=None, feed="host")
    assert form == "lookahead"
    return dict(depth=3, chunks=rates.chunks_of(n_rest, parts), feed="ingest_lookahead")


def _freeze(d):
    return tuple(sorted((d or {}).items()))


@functools.lru_cache(maxsize=None)
def _at_zero(fs, fmt, form, parts, packed, scan_mode, options, cut2):
    """the same split at K = 0: its scan_fallbacks (and it equals the oracle too)"""
    opts = dict(options)
    x, ref, cut = scene(fs, fmt, opts.get("fir_order", 1))
    n = len(x) // (1 if fmt == irdm.FMT_CF32 else 2)
    res = farpos.run_shifted(x, fs, cut, 0, fmt=fmt, packed=packed, scan_mode=scan_mode, options=opts, cut2=cut2,
                             **_form(form, n - (cut2 or cut), parts))
    (parity.compare_packed if packed else parity.compare)(res, ref)
    return res["stats"]["scan_fallbacks"]


def check_scan_kind(stats, fs, scan_mode):
    """the scan tests/rates.py's restatement of the dispatch rules names ran in B"""
    kind = {0: rates.describe(fs)["scan"], 1: "sequential", 2: "wave"}[scan_mode]
    if kind == "band":
        assert stats["band_chunks"] >= 1, (fs, stats)
    elif kind == "wave":
        assert stats["band_chunks"] == 0 and stats["scan_fast_chunks"] >= 1, (fs, stats)
    else:
        assert stats["band_chunks"] == 0 and stats["scan_fast_chunks"] == 0, (fs, stats)


def run_case(fs, where, form, fmt=irdm.FMT_CF32, parts=4, packed=False, scan_mode=0, options=None, K=None, two_hops=False,
             want_state=False):
    """where: 31 / 32 -- K puts 2^where inside a burst of B; 44 / 52 -- K44 / K52.  Returns (the unshifted result, K, the
    summary of the comparison)."""
    opts = dict(options or {})
    x, ref, cut = scene(fs, fmt, opts.get("fir_order", 1))
    n = len(x) // (1 if fmt == irdm.FMT_CF32 else 2)
    cut2 = farpos.cut_inside_a_burst(ref, rates.fft_size(fs), which=2) if two_hops else None
    if K is None:
        K = {31: None, 32: None, 44: K44, 52: K52}[where] or farpos.k_straddling(ref, cut2 or cut, where)
    res = farpos.run_shifted(x, fs, cut, K, fmt=fmt, packed=packed, scan_mode=scan_mode, options=opts, cut2=cut2,
                             want_state=want_state, **_form(form, n - (cut2 or cut), parts))
    K = res["K"]
    far = res["far"]
    print("fs %d %s %s K 0x%x: B emitted %d bursts, %d frames; scan_fallbacks %d" %
          (fs, FMT_NAMES[fmt], form, K, len(far["bursts"]), len(far["packed"] if packed else far["demods"]), res["stats"]["scan_fallbacks"]))
    # (a)
    if where in (31, 32):
        assert farpos.straddles(far["bursts"], where), [(b.start, b.num_samples) for b in far["bursts"]]
    else:
        assert far["bursts"] and all(b.start > 1 << where for b in far["bursts"])
    # (b)
    assert len(far["bursts"]) >= 5 and len(far["packed"] if packed else far["demods"]) >= 4
    # (c)
    assert res["stats"]["scan_fallbacks"] == _at_zero(fs, fmt, form, parts, packed, scan_mode, _freeze(opts), cut2), res["stats"]
    check_scan_kind(res["stats"], fs, scan_mode)
    assert res["n_samples"] == n + K
    farpos.unshift(res, K, fs)
    summary = (parity.compare_packed if packed else parity.compare)(res, ref)
    return res, K, summary


# rate -> what it is there for (tests/rates.py: describe)
RATES = {1_000_000: "dense scan", 2_000_000: "band scan, any-M decimator", 6_250_000: "any-M decimator, M = 25",
         10_000_000: "resident decimator <40>", 12_000_000: "resident decimator <48>", 16_000_000: "wave walk as the default scan"}


@pytest.mark.parametrize("form", ["whole", "lookahead"])
@pytest.mark.parametrize("where", [32, 44])
@pytest.mark.parametrize("fs", sorted(RATES))
def test_every_decimator_and_scan_form(fs, where, form):
    """each rate's scan and decimator with a burst across 2^32 and wholly above 2^44, at pipeline_depth 0 whole and at
    depth 3 fed in place with look-ahead in 4-5 chunks"""
    d = rates.describe(fs)
    assert d["supported"] and d["scan"] == {1_000_000: "dense", 16_000_000: "wave"}.get(fs, "band")
    assert d["decimator"] == ("register" if fs in (10_000_000, 12_000_000) else "any-M")
    run_case(fs, where, form, parts=4 + (fs // 1_000_000) % 2)


@pytest.mark.parametrize("form", ["whole", "lookahead"])
@pytest.mark.parametrize("where", [32, 44])
def test_resident_decimator_in_the_scalar_order_10mhz(where, form):
    """fir_order 0: fir_decimate_kernel_r, against the oracle in that order"""
    run_case(10_000_000, where, form, options={"fir_order": 0})


@pytest.mark.parametrize("scan_mode", [1, 2], ids=["sequential", "single_cu_wave_walk"])
@pytest.mark.parametrize("where", [32, 44])
def test_other_scans_2mhz(where, scan_mode):
    run_case(2_000_000, where, "lookahead", scan_mode=scan_mode)


def test_burst_across_2_to_31_10mhz():
    run_case(10_000_000, 31, "lookahead")


def test_above_2_to_52_2mhz():
    """(double)start is still exact there"""
    run_case(2_000_000, 52, "whole")
    run_case(2_000_000, 52, "lookahead")


def test_ring_wrap_inside_a_burst_far_out_10mhz_ci8():
    """test_ring_wrap_chunks_and_ragged_end_10mhz_ci8's situation with the high word non-zero: the window of one of B's
    bursts wraps round the end of the history ring"""
    fs, fmt = 10_000_000, irdm.FMT_CI8
    x, ref, cut = scene(fs, fmt)
    later = [b for b in ref.bursts if b.start > cut]
    rb = later[len(later) // 2]

    def wraps(start, num, ring_len):
        return start % ring_len > ring_len - num

    def pick(ring_len):
        # the first K from 2^32 on, on the feed grid, that puts the end of the ring into the middle half of the window
        for j in range(4 * ring_len // farpos.GRID + 4):
            K = (1 << 32) + j * farpos.GRID
            if rb.num_samples // 4 < ring_len - (rb.start + K) % ring_len < 3 * rb.num_samples // 4:
                return K
        raise AssertionError("no K wraps the ring inside the burst")

    n = len(x) // 2
    res = farpos.run_shifted(x, fs, cut, pick, fmt=fmt, **_form("lookahead", n - cut, 5))
    K = res["K"]
    assert K >= 1 << 32
    assert any(wraps(b.start, b.num_samples, res["ring_len"]) for b in res["far"]["bursts"]), (K, res["ring_len"])
    assert len(res["far"]["bursts"]) >= 5 and len(res["far"]["demods"]) >= 4
    assert res["stats"]["scan_fallbacks"] == _at_zero(fs, fmt, "lookahead", 5, False, 0, (), None)
    farpos.unshift(res, K, fs)
    parity.compare(res, ref)


@pytest.mark.parametrize("fmt", [irdm.FMT_CI8, irdm.FMT_CI16, irdm.FMT_CI16_FULL, irdm.FMT_CU8, irdm.FMT_CI32],
                         ids=lambda f: FMT_NAMES[f])
def test_formats_10mhz(fmt):
    """the integer load stages; irdm_seed_history takes each format's own bytes"""
    run_case(10_000_000, 32, "lookahead", fmt=fmt)


@pytest.mark.parametrize("fs", [2_000_000, 10_000_000])
def test_packed_records(fs):
    run_case(fs, 32, "lookahead", packed=True)


def test_both_ends_of_a_hand_off_far_out_2mhz():
    """the time-shard protocol above 2^32 with no shift_state in it: B, at cut + K, exports; C imports B's blob unpatched
    with its history seeded at cut2 + K; 2^32 lies in a burst that C emits"""
    run_case(2_000_000, 32, "lookahead", two_hops=True)
    run_case(2_000_000, 44, "whole", two_hops=True)


@pytest.mark.parametrize("fs", [2_000_000, 10_000_000])
def test_state_after_the_run(fs):
    """B's irdm_export_state, its positions moved down by K, is byte for byte the export of the K = 0 run at that point
    (but for the dead entries of DetState.act behind n_act, which keep the records of bursts that have gone)"""
    x, ref, cut = scene(fs)
    form = _form("lookahead", len(x) - cut, 4)
    zero = farpos.run_shifted(x, fs, cut, 0, want_state=True, **form)
    res, K, _ = run_case(fs, 32, "lookahead", want_state=True)
    back, want = farpos.live_bytes(farpos.shift_state(res["state"], -K)), farpos.live_bytes(zero["state"])
    assert len(back) == len(want)
    assert np.array_equal(back, want), np.flatnonzero(back != want)[:16]


# ---- the limit ----

def check_limit(fs=2_000_000):
    """2^53 - 32768 is accepted, 2^53 is refused, by irdm_seed_history and irdm_import_state (the blob's sample count, and an
    active burst alone); a refused import leaves the context as it was: it goes on to equal the oracle"""
    import ctypes as C
    x, ref, cut = scene(fs)
    n = len(x)
    p = irdm.Pipeline(fs, max_chunk_samples=n, max_bursts_per_chunk=1024)
    p.set_option("keep_frame_samples", 1)
    p.feed_host(x[:cut])
    blob = p.export_state()
    offs = farpos.position_offsets(blob)
    assert len(offs) > 2, "the cut lies inside a burst: the blob carries an active burst"
    top = max(farpos._u64(blob, o) for o in offs)
    assert top == cut
    ok = farpos.shift_state(blob, farpos.MAX_POSITION - farpos.GRID - cut)
    bad = farpos.shift_state(blob, farpos.MAX_POSITION - cut)
    bad_burst = np.array(blob, copy=True)                  # only one active burst's last_active is out of range
    farpos._add(bad_burst, offs[-1], farpos.MAX_POSITION - farpos._u64(blob, offs[-1]))
    q = irdm.Pipeline(fs, max_chunk_samples=n, max_bursts_per_chunk=1024)
    tail = x[cut - 4096:cut]
    assert q.L.irdm_seed_history(q.h, tail.ctypes.data_as(C.c_void_p), len(tail), farpos.MAX_POSITION) == -1
    assert q.sample_count == 0
    assert q.L.irdm_seed_history(q.h, tail.ctypes.data_as(C.c_void_p), len(tail), farpos.MAX_POSITION - farpos.GRID) == 0
    assert q.sample_count == farpos.MAX_POSITION - farpos.GRID
    for b in (bad, bad_burst):
        assert q.L.irdm_import_state(q.h, b.ctypes.data_as(C.c_void_p), len(b)) == -1
    assert q.sample_count == farpos.MAX_POSITION - farpos.GRID
    q.import_state(ok)
    # the device forms: the seeded position, and the blob's sample count (the detector state is not brought back for it)
    d_tail, d_bad, d_ok = irdm.device_buffer(tail), irdm.device_buffer(bad), irdm.device_buffer(ok)
    try:
        assert q.L.irdm_seed_history_device(q.h, C.c_void_p(d_tail), len(tail), farpos.MAX_POSITION) == -1
        assert q.L.irdm_import_state_device(q.h, C.c_void_p(d_bad), len(bad)) == -1
        assert q.L.irdm_import_state_head_device(q.h, C.c_void_p(d_bad), q.state_head_bytes()) == -1
        assert q.sample_count == farpos.MAX_POSITION - farpos.GRID
        q.seed_history_device(d_tail, len(tail), farpos.MAX_POSITION - farpos.GRID)
        q.import_state_device(d_ok, len(ok))
    finally:
        for ptr in (d_tail, d_bad, d_ok):
            irdm.device_free(ptr)
    q.close()
    # the refused calls on the context in mid-stream: it goes on as if they had not been made
    for b in (bad, bad_burst):
        assert p.L.irdm_import_state(p.h, b.ctypes.data_as(C.c_void_p), len(b)) == -1
    assert p.L.irdm_seed_history(p.h, tail.ctypes.data_as(C.c_void_p), len(tail), farpos.MAX_POSITION) == -1
    assert p.sample_count == cut
    p.feed_host(x[cut:])
    infos, samples = p.poll_frames()
    got = dict(bursts=p.poll_bursts(), infos=infos, samples=samples, demods=p.poll_demods(), tagged=p.tagged,
               n_samples=p.sample_count)
    p.close()
    s = parity.compare(got, ref)
    assert s["bursts"] >= 10 and s["demods"] >= 8, s
    return s


def test_positions_from_2_to_53_on_are_refused():
    check_limit()


# ---- the front ends ----

FE_N = (1 << 20) + 12345
FE_CASES = {"K0_D5": (1, 5, 50_000_000, 10_000_000), "K0r_5_28": (5, 28, 56_000_000, 10_000_000),
            "K0r_25_24": (25, 24, 2_400_000, 2_500_000), "K0r_125_768": (125, 768, 61_440_000, 10_000_000)}


def check_frontend(name, fmt, power, r, n=FE_N):
    """the front end sought to P = r modulo 65536 M (farpos.fe_seek_position: 2^32 is crossed inside the run, or P lies
    above 2^40) and run on n samples in ragged feeds: every output bit of the C model run on zeros(r) ++ x, from the
    output on that those r samples leave incomplete (positions that agree modulo farpos.fe_period(M) give the same
    outputs: the model never sees the high bits)"""
    import frontend_model as fm
    import resample_model as rm
    L, M, fi, fo = FE_CASES[name]
    q = {irdm.FMT_CF32: 14418, irdm.FMT_CI8: -9000}[fmt]
    shift = q * fi / 65536.0
    x = fm.random_capture(fmt, n, seed=7000 + 10 * M + fmt)
    if L == 1:
        st = fm.Stage(fi, fmt, M, shift)
        feeds = fm.ragged_feeds(n, st.fe.ntaps, (99991, 65537, 200003, 7 * 32768))
    else:
        st = rm.Stage(fi, fmt, fo, shift)
        assert st.fe.ratio == (L, M)
        feeds = rm.ragged_feeds(n, st.fe.ntaps, L, (99991, 65537, 200003, 7 * 32768))
    try:
        taps = st.fe.taps()
        P = farpos.fe_seek_position(power, M, n, r)
        assert P % farpos.fe_period(M) == r
        st.fe.seek(P)
        got = st.run(x, feeds)
    finally:
        st.close()
    # (the first outputs behind the seek still read the zeros in front of P: with fewer than half a filter of lead-in the
    # model would have to begin before its output 0, so the lead-in is then one period longer)
    lead_n = r if r * L > len(taps) else r + farpos.fe_period(M)
    lead = farpos.lead_in(x, fmt, lead_n)
    want = fm.run(lead, fmt, M, q, taps) if L == 1 else rm.run(lead, fmt, L, M, q, taps)
    want = want[farpos.fe_outputs(lead_n, L, M, len(taps)):]
    assert len(got) > n * L // M - len(taps)
    assert fm.same_bits(got, want), (name, FMT_NAMES[fmt], P, int((got.view(np.uint64) != want.view(np.uint64)).sum())
                                     if len(got) == len(want) else (len(got), len(want)))
    return len(got)


@pytest.mark.parametrize("power,r", [(32, 0), (32, 12345), (40, 0), (40, 12345)])
@pytest.mark.parametrize("fmt", [irdm.FMT_CF32, irdm.FMT_CI8], ids=lambda f: FMT_NAMES[f])
@pytest.mark.parametrize("name", sorted(FE_CASES))
def test_front_end_behind_a_seek(name, fmt, power, r):
    check_frontend(name, fmt, power, r)


def check_seek_refusals():
    """valid only directly after create or reset, and below 2^53; a refused seek leaves the object as it was"""
    import frontend_model as fm
    st = fm.Stage(50_000_000, irdm.FMT_CI8, 5, 0.0)
    try:
        L = st.fe.L
        assert L.irdm_frontend_seek(st.fe.h, farpos.MAX_POSITION) == -1
        x = fm.random_capture(irdm.FMT_CI8, 40000, seed=3)
        want = fm.run(x, irdm.FMT_CI8, 5, 0, st.fe.taps())
        assert fm.same_bits(st.run(x, [40000]), want)
        assert L.irdm_frontend_seek(st.fe.h, 1 << 20) == -1          # (finished)
        st.fe.reset()
        assert L.irdm_frontend_seek(st.fe.h, farpos.MAX_POSITION - 1) == 0
        assert L.irdm_frontend_seek(st.fe.h, 0) == -1                # (a position has been set)
        st.fe.reset()
        assert fm.same_bits(st.run(x, [12345, 27655]), want)
    finally:
        st.close()


def test_seek_refusals():
    check_seek_refusals()
