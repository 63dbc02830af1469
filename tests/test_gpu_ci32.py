"""32-bit integer I/Q on the GPU: IRDM_FMT_CI32 (v / 2^31: SigMF ci32_le, 32-bit PCM WAV) and IRDM_FMT_CI32_24 (24-bit samples
held in int32, v / 2^23: SDRangel's .sdriq).

The contract (include/irdm_hip.h): a context in either format produces exactly the records of a cf32 context fed
v.astype(np.float32) * np.float32(scale) -- bursts, frames with their samples, demods with their LLRs, the packed, parsed
and frame records -- bit for bit.  Every K1 family and both decimators, every feed path, both front ends, the input
statistics against the integer model.  The scenes and sizes are those of tests/test_gpu_cu8.py; format 8's scene is scaled
so that most values need more than 24 bits ((float)v rounds) and carries INT32_MIN and INT32_MAX."""
import numpy as np
import pytest

import ci32
import ci32_stats_checks as cs
import formats16 as f16
import frontend_model as fm
import irdm
import orc
import parity
import resample_model as rm
import siggen

pytestmark = pytest.mark.gpu

F8, F9 = irdm.FMT_CI32, irdm.FMT_CI32_24
# rate -> (seconds, bursts): the scene sizes of tests/test_gpu_cu8.py
SCENES = {2_000_000: (1.2, 6), 4_000_000: (1.0, 6), 10_000_000: (0.9, 6), 12_000_000: (0.95, 4)}
_iq = {}


def scene(fs, fmt):
    if fs not in _iq:
        secs, nb = SCENES[fs]
        n = int(secs * fs) // 32768 * 32768
        _iq[fs] = siggen.standard_scene(fs, n, nb, seed=fs // 1_000_000 + 160)[0]
    v = ci32.to_ci32(_iq[fs], fmt)
    return ci32.with_extremes(v) if fmt == F8 else v


def oracle(y, fs, order):
    try:
        orc.set_fir_order(order)
        return orc.run_stream(y, fs)
    finally:
        orc.set_fir_order(1)


@pytest.mark.parametrize("fmt,fs,order", [(F8, 2_000_000, 1), (F8, 4_000_000, 1), (F8, 10_000_000, 0), (F8, 10_000_000, 1),
                                          (F8, 12_000_000, 1), (F9, 2_000_000, 1), (F9, 10_000_000, 1)])
def test_every_kernel_variant(fmt, fs, order):
    """generic K1 + any-M decimator, r16 K1, p32<13> + M = 40 in both orders, p32<14> + M = 48: the int32 context equals the
    cf32 context on the converted samples bit for bit, and the oracle on them"""
    v = scene(fs, fmt)
    y = ci32.converted(v, fmt)
    if fmt == F8:
        assert np.mean(np.abs(v.astype(np.int64)) >= 2 ** 24) > 0.5
        assert y.view(np.float32)[10:14].tolist() == [-1.0, 1.0, 1.0, -1.0]
    else:
        assert int(np.abs(v.astype(np.int64)).max()) < 2 ** 23
    opts = {"fir_order": order}
    got = f16.run(v, fs, fmt, options=opts)
    assert f16.same_records(got, f16.run(y, fs, irdm.FMT_CF32, options=opts)) > 0
    s = parity.compare(got, oracle(y, fs, order))
    assert s["demods"] >= 3, s


def _boundary_scene():
    """2 MHz, 1.6 s, a burst across every chunk boundary of chunks_of(n, 5), the stream ending 777 samples past a block
    (tests/test_gpu_cu8.py)"""
    fs, nfft = 2_000_000, 2048
    n = int(1.6 * fs) // 32768 * 32768 - 32768 + 777
    sizes = f16.chunks_of(n, 5)
    rng = np.random.default_rng(61)
    bursts = [dict(start=int(s), freq_hz=siggen.channel_freq(int(rng.integers(-20, 21)) or 1),
                   payload=rng.integers(0, 4, int(rng.integers(119, 180))).tolist())
              for s in np.sort(rng.integers(520 * nfft, n - int(0.05 * fs), 6))]
    for b in np.cumsum(sizes)[:-1]:
        bursts.append(dict(start=int(b) - 9000, freq_hz=siggen.channel_freq(int(rng.integers(-20, 21)) or 2),
                           payload=rng.integers(0, 4, 170).tolist()))
    iq, _ = siggen.make_stream(fs, n, bursts, seed=61)
    return fs, iq, sizes


def test_feed_paths():
    """pinned host memory, device-resident chunks, in place from the ring (irdm_ingest_ptr) with look-ahead at pipeline_depth
    3, and the packed / parsed / frame records: a ragged last chunk, bursts across the chunk boundaries; format 8, and the
    in-place path for format 9"""
    fs, iq, sizes = _boundary_scene()
    v = ci32.to_ci32(iq, F8)
    y = ci32.converted(v, F8)
    ref = orc.run_stream(y, fs)
    cuts = np.cumsum(sizes)[:-1]
    assert sum(any(b.start < c < b.start + b.num_samples for b in ref.bursts) for c in cuts) >= 3
    for feed, depth in (("pinned", 0), ("device", 1), ("ingest_lookahead", 3)):
        got = f16.run(v, fs, F8, chunks=sizes, depth=depth, feed=feed)
        assert f16.same_records(got, f16.run(y, fs, irdm.FMT_CF32, chunks=sizes, depth=depth, feed=feed)) > 0, feed
        s = parity.compare(got, ref)
        assert s["demods"] >= 8, (feed, s)
    got = f16.run(v, fs, F8, chunks=sizes, depth=3, feed="ingest_lookahead", packed=True)
    want = f16.run(y, fs, irdm.FMT_CF32, chunks=sizes, depth=3, feed="ingest_lookahead", packed=True)
    assert f16.same_records(got, want) > 0
    assert len(got["packed"]) == len(ref.demods) and len(got["ida"]) == len(got["frame"]) == len(got["packed"])
    v9 = ci32.to_ci32(iq, F9)
    got = f16.run(v9, fs, F9, chunks=sizes, depth=3, feed="ingest_lookahead")
    assert f16.same_records(got, f16.run(ci32.converted(v9, F9), fs, irdm.FMT_CF32, chunks=sizes, depth=3, feed="ingest_lookahead")) > 0


@pytest.mark.parametrize("fmt", [F8, F9])
@pytest.mark.parametrize("kind", ["k0", "k0r"])
def test_front_ends(kind, fmt):
    """2^22 + 12345 int32 samples over the format's whole range through K0 (10 MS/s, D = 5) and K0r (2.4 -> 2.5 MS/s, 25/24),
    whole and in ragged feeds: the band of the cf32 capture of the converted samples, bit for bit"""
    n = (1 << 22) + 12345
    v = ci32.stats_input(fmt, n, seed=6 + fmt)
    y = ci32.converted(v, fmt)
    if kind == "k0":
        make = lambda f: fm.Stage(10_000_000, f, 5, 14418 * 10_000_000 / 65536.0)          # noqa: E731
        ragged = lambda nt: fm.ragged_feeds(n, nt, (999983, 65537))                          # noqa: E731
    else:
        make = lambda f: rm.Stage(2_400_000, f, 2_500_000, -9000 * 2_400_000 / 65536.0)      # noqa: E731
        ragged = lambda nt: rm.ragged_feeds(n, nt, 25, (999983, 65537))                      # noqa: E731
    st = make(irdm.FMT_CF32)
    want = st.run(y, [n])
    st.close()
    st = make(fmt)
    nt = st.fe.ntaps
    whole = st.run(v, [n])
    st.close()
    assert len(want) > 0 and fm.same_bits(whole, want)
    st = make(fmt)
    got = st.run(v, ragged(nt))
    st.close()
    assert fm.same_bits(got, want)


def test_input_stats_equal_the_integer_model():
    """irdm_input_stats_device: both formats, every size and two alignments, rails at both ends, all-rail buffers whose sum of
    squares passes 64 bits; option input_stats over one stream cut three ways gives one struct, the model's"""
    assert cs.stage_cases()["cases"] >= 2 * 10 * 2 + 2 + 6
    assert set(cs.context_cuts()) == {"ci32", "ci32-24"}


def test_input_stats_at_2_pow_30_squares():
    """2^22 + 5 samples, every component INT32_MIN: the sum of squares is (2^22 + 5) 2^62, far past one 64-bit word"""
    n = (1 << 22) + 5
    st = cs.stage_one(np.full(2 * n, ci32.I32_MIN, np.int32), F8, 1, "all INT32_MIN")
    assert list(st.sum_sq) == [float(n), float(n)] and list(st.sum) == [-float(n), -float(n)]
    assert list(st.n_rail_lo) == [n, n]


def test_create_refuses_5_7_and_10():
    for fmt in (5, 7, 10, 11, -1):
        with pytest.raises(RuntimeError):
            irdm.Pipeline(2_000_000, fmt=fmt)
        with pytest.raises(RuntimeError):
            irdm.Frontend(10_000_000, fmt, 5)
        with pytest.raises(RuntimeError):
            irdm.Frontend.rational(2_400_000, fmt, 2_500_000, 0.0)
    for fmt in (F8, F9):
        p = irdm.Pipeline(2_000_000, fmt=fmt)
        try:
            assert p.L.irdm_bytes_per_sample(p.h) == 8
        finally:
            p.close()
