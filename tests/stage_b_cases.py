"""TEST INFRASTRUCTURE: stage B alone (irdm_downmix_burst, burst_downmix.c:643-797) on DESIGNED burst windows -- windows the
detector would never cut from a scene: every early return of the reference (drop_reason 1..5, both sides of reason 4),
the length thresholds to the sample, silence, frames shorter than the CFO estimator's input and longer than the
demodulator can take, carriers off the bin centre and at the band edges, the simplex frame-length rules and their 1626 MHz
threshold -- each presented at stream positions of every class the stage-level entry point tells apart: `start % 8` (the
register-resident decimator or the LDS one), where the window ends within the reader's 32768-sample feed blocks (a
stage-level call owns its whole window wherever it lies), and a position past 2^33.

The reference is the oracle's orc_downmix_process on the same samples; the comparison is what parity.compare asserts per
frame.  Shared by tests/stage_b_emul_run.py (the CPU emulation) and tests/test_gpu_stage_b.py (the card); neither the GPU
nor the product is touched at import."""
import ctypes as C
import functools

import numpy as np

import orc
import rates
import siggen

FC = 1622000000.0                # the capture's centre frequency unless a window says otherwise
T0 = 1700000000 * 10**9          # wall-clock time of sample 0 (burst_data_t.start_time_ns)
BLOCK = 32768                    # the reader's feed block (main.c)
TAPS = 801                       # the input low-pass of burst_downmix.c:417-437: outputs = (n - 801 + 1) / M
SIMPLEX = 1626000000.0           # iridium.h: frames above it follow the simplex length rules
SIGMA = 0.002


def decim(fs):
    return int(round(fs / 250000.0))


def bin_freq(fs, center_bin):
    n = rates.fft_size(fs)
    return (center_bin - n // 2) * (fs / n)


def default_bin(fs):
    n = rates.fft_size(fs)
    return n // 2 + n // 5 + 3


def _payload(k, seed):
    return np.random.default_rng(1000 + seed).integers(0, 4, k).tolist()


def _window(fs, outs, bursts=(), sigma=SIGMA, off_hz=0.0, center_bin=None, seed=0, extra=0, zeros=False):
    """800 + outs M + extra samples (`outs` decimated outputs) of noise with `bursts` on the carrier of center_bin + off_hz;
    a burst dict: at (the output it begins at; sample = 400 + at M, or `sample`), payload (symbols) | quads, uplink, amp"""
    m = decim(fs)
    n = (TAPS - 1) + outs * m + extra
    if zeros:
        return np.zeros(n, np.complex64)
    # Stage B takes its output for 250 kHz whatever fs / M is (burst_downmix.c:423, :633-634: 10 samples per symbol): the
    # window is synthesised at 250 kHz x M -- fs itself at every rate on the 250 kHz grid, 750 kHz for 725 kHz -- so that the
    # unique words lie where the correlator looks for them and every return is reached at every rate.
    fs = 250000 * m
    cb = default_bin(fs) if center_bin is None else center_bin
    f0 = bin_freq(fs, cb) + off_hz
    bl = []
    for i, b in enumerate(bursts):
        d = dict(start=b["sample"] if "sample" in b else (TAPS - 1) // 2 + b["at"] * m, freq_hz=f0, amp=b.get("amp", 0.05),
                 uplink=b.get("uplink", False), phase=0.3 + 1.1 * i)
        if "quads" in b:
            d["quads"] = b["quads"]
        else:
            d["payload"] = _payload(b.get("payload", 150), seed + i)
        bl.append(d)
    iq, _ = siggen.make_stream(fs, n, bl, noise_sigma=sigma, seed=seed)
    return iq


def _refined_minus_fc(fs, iq, center_bin):
    """what stage B adds to the capture's centre frequency for this window (the bin's frequency and the fine CFO,
    burst_downmix.c:672, :720), read off the oracle's frame at FC"""
    L = orc.lib()
    dm = L.orc_downmix_create()
    try:
        rec = orc.BurstRec(id=1, start=0, center_bin=center_bin, num_samples=len(iq))
        want = orc.Frame()
        ok = L.orc_downmix_process(dm, C.byref(rec), orc.fptr(iq.view(np.float32)), FC, fs, rates.fft_size(fs), T0,
                                   C.byref(want))
        assert ok, "the simplex-threshold window gives no frame at %d Hz" % fs
        return want.center_frequency - FC
    finally:
        L.orc_downmix_destroy(dm)


@functools.lru_cache(maxsize=2)
def windows(fs):
    """tuple of (name, iq complex64, center_bin, center_frequency)"""
    m = decim(fs)
    n = rates.fft_size(fs)
    cb = default_bin(fs)
    out = []

    def add(name, iq, center_bin=cb, fc=FC):
        iq = np.ascontiguousarray(iq, np.complex64)
        iq.setflags(write=False)
        out.append((name, iq, center_bin, fc))

    dl = dict(at=40)
    ul = dict(at=40, uplink=True)
    # lengths: burst_downmix.c:645 (fewer than 100 samples), :677 (fewer than 100 outputs), and the first lengths past it
    add("len_99", _window(fs, 0, seed=1)[:99])
    add("len_100", _window(fs, 0, seed=2)[:100])
    add("len_800", _window(fs, 0, seed=3))
    add("outs_99", _window(fs, 99, seed=4))
    add("outs_100", _window(fs, 100, seed=5))
    add("outs_101_less_a_sample", _window(fs, 100, extra=m - 1, seed=6))
    # content
    add("noise_3000", _window(fs, 3000, seed=7))
    add("zeros_2400", _window(fs, 2400, zeros=True))
    add("zeros_100", _window(fs, 100, zeros=True))
    down = _window(fs, 2400, [dl], seed=10)
    up = _window(fs, 2400, [ul], seed=11)
    add("downlink", down)
    # (2300 outputs: the frame's 1910 samples reach into the window's last N samples at every rate)
    add("downlink_2300", down[:(TAPS - 1) + 2300 * m])
    add("uplink", up)
    add("payload_60", _window(fs, 2400, [dict(dl, payload=60)], seed=12))
    add("payload_320_cut", _window(fs, 4000, [dict(dl, payload=320)], seed=13))
    add("frame_560_symbols", _window(fs, 6000, [dict(dl, payload=560 - 28)], seed=14))
    add("begins_60_before_end", _window(fs, 2400, [dict(at=2340)], seed=15))
    add("burst_at_sample_0", _window(fs, 2400, [dict(sample=0)], seed=16))
    add("weak", _window(fs, 2400, [dict(dl, amp=0.004)], seed=17))
    add("amp_3e4", _window(fs, 2400, [dict(dl, amp=3e4)], seed=18))
    add("amp_1e-3_sigma_4e-5", _window(fs, 2400, [dict(dl, amp=1e-3)], sigma=4e-5, seed=19))
    # the carrier off the bin's centre frequency
    for k, off in enumerate((244.1, 11000.0, -30000.0, 62000.0)):
        add("carrier_%+g" % off, _window(fs, 2400, [dl], off_hz=off, seed=20 + k))
    # truncated: frames shorter than the 256 samples the CFO estimator takes; the unique word before / behind the frame
    for k in (130, 160, 200, 250, 290):
        add("downlink_cut_%d" % k, down[:(TAPS - 1) + k * m])
    for k in (300, 312, 340):
        add("uplink_cut_%d" % k, up[:(TAPS - 1) + k * m])
    # The input low-pass is designed once, for 10 MHz (burst_downmix.c:252-258: 100 kHz there, 0.01 cycles per sample at
    # every rate): at 725 kHz it is 7 kHz wide and removes the uplink preamble's +-12.5 kHz tones, no uplink frame is
    # recognised.  A preamble that alternates in pairs (+-6.25 kHz) passes it at every rate: direction 2, and the unique
    # word behind a truncated frame, down to the lowest rate.
    paired = _window(fs, 2400, [dict(at=40, quads=[2, 2, 0, 0] * 4 + siggen.UW_UL)], seed=29)
    add("uplink_paired_preamble", paired)
    add("uplink_paired_preamble_cut_400", paired[:(TAPS - 1) + 400 * m])
    add("two_bursts", _window(fs, 5200, [dl, dict(at=2600, uplink=True, amp=0.1)], seed=30))
    add("unmodulated", _window(fs, 2400, [dict(at=40, quads=[0] * 178)], seed=31))
    # the outermost centre bins, the carrier 2 kHz inside the band
    add("center_bin_0", _window(fs, 2400, [dl], center_bin=0, off_hz=2000.0, seed=32), center_bin=0)
    add("center_bin_last", _window(fs, 2400, [dl], center_bin=n - 1, off_hz=125000.0 * m - 2000.0 - bin_freq(250000 * m, n - 1),
                                       seed=33),
        center_bin=n - 1)
    # simplex (burst_downmix.c:764-767): 4440 samples out, and the threshold itself
    add("simplex_5000", _window(fs, 5000, [dict(dl, payload=400)], seed=34), fc=1626.4e6)
    add("simplex_6000", _window(fs, 6000, [dict(dl, payload=400)], seed=35), fc=1626.4e6)
    d = _refined_minus_fc(fs, down, cb)
    add("refined_50_below_1626", down, fc=SIMPLEX - 50.0 - d)
    add("refined_50_above_1626", down, fc=SIMPLEX + 50.0 - d)
    return tuple(out)


def ref_ring(fs):
    """create.cpp: the reference's ring (2 s of samples at every rate the product accepts), the distance of a stale-slot
    read -- below it such a read gives zeros, past it whatever the context's history ring holds"""
    return 2 * fs


START_CLASSES = ("zero", "inside_block_aligned", "inside_block_plus_3", "ends_on_block", "ends_8_short_of_n_past_block",
                 "past_2^33")


def starts(fs, num):
    """(class, start) for a window of `num` samples.  With r = (start + num - N) % 32768: r in [1, 32768 - N] is where the
    detector's feed block had delivered the whole window; r = 0 and r > 32768 - N are where it had not (a stage-level call
    still owns every sample it is given)."""
    n = rates.fft_size(fs)

    def at(base, r, align=None):
        """the first start >= base with (start + num - N) % BLOCK == r (and start % 8 == align: r moves up to 7 + 3 on)"""
        s = base + (r - (base + num - n)) % BLOCK
        if align is not None:
            s += (align - s) % 8
        return s

    inside = at(3 * BLOCK, 16, align=0)
    assert 1 <= (inside + num - n) % BLOCK and (inside + 3 + num - n) % BLOCK <= BLOCK - n and inside % 8 == 0
    past = ref_ring(fs) + BLOCK
    far = at((1 << 33) + 5 * BLOCK, 16, align=0)
    assert 1 <= (far + num - n) % BLOCK <= BLOCK - n
    return (("zero", 0), ("inside_block_aligned", inside), ("inside_block_plus_3", inside + 3),
            ("ends_on_block", at(past, 0)), ("ends_8_short_of_n_past_block", at(past, BLOCK - n + 8)), ("past_2^33", far))


def check(fi, frame, want, ok):
    """the product's (FrameInfo, frame samples | None) against the oracle's frame: what parity.compare asserts per frame"""
    bits = lambda x: np.float32(x).view(np.uint32)      # noqa: E731
    assert fi.drop_reason == want.drop_reason, ("drop_reason", fi.drop_reason, want.drop_reason)
    assert fi.dec_len == want.dec_len, ("dec_len", fi.dec_len, want.dec_len)
    assert (frame is not None) == bool(ok)
    r = want.drop_reason
    if r in (0, 3, 4, 5):
        assert fi.start == want.start, ("start", fi.start, want.start)
    if r in (0, 4, 5):
        assert bits(fi.center_offset) == bits(want.center_offset), ("center_offset", fi.center_offset, want.center_offset)
        assert fi.uw_start_idx == want.uw_start_idx and fi.direction == want.direction, \
            ("uw_start_idx, direction", fi.uw_start_idx, want.uw_start_idx, fi.direction, want.direction)
        assert bits(fi.corr_re) == bits(want.corr_re) and bits(fi.corr_im) == bits(want.corr_im), \
            ("corr", fi.corr_re, want.corr_re, fi.corr_im, want.corr_im)
    if r == 0:
        assert fi.num_samples == want.num_samples, ("num_samples", fi.num_samples, want.num_samples)
        assert fi.timestamp == want.timestamp, ("timestamp", fi.timestamp, want.timestamp)
        assert fi.center_frequency == want.center_frequency, ("center_frequency", fi.center_frequency, want.center_frequency)
        assert bits(fi.uw_start) == bits(want.uw_start), ("uw_start", fi.uw_start, want.uw_start)
        ws = np.ctypeslib.as_array(want.samples)[:2 * want.num_samples].view(np.uint32)
        gs = frame.view(np.uint32)
        if not np.array_equal(gs, ws):
            bad = np.flatnonzero(gs != ws)
            raise AssertionError("%d of %d frame floats differ from the oracle, from index %d" % (len(bad), len(ws), bad[0]))


def coverage(results):
    """results: dicts(name, cls, reason, dec_len, start, uw_start_idx, direction, num_samples) of one rate's oracle frames"""
    hist = {r: sum(1 for x in results if x["reason"] == r) for r in range(6)}
    assert all(hist[r] >= 1 for r in range(6)), hist
    four = [x for x in results if x["reason"] == 4]
    assert any(x["uw_start_idx"] < 0 for x in four), "no reason 4 with the unique word before the frame"
    assert any(x["uw_start_idx"] >= x["dec_len"] - x["start"] for x in four), "no reason 4 with the unique word behind the frame"
    frames = [x for x in results if x["reason"] == 0]
    assert {x["direction"] for x in frames} == {1, 2}, "not both directions among the frames"
    lens = {x["num_samples"] for x in frames}
    assert 1910 in lens and 4440 in lens, sorted(lens)
    flen = [x["dec_len"] - x["start"] for x in results if x["reason"] in (0, 4, 5)]
    assert min(flen) < 256 and max(flen) > 2832, (min(flen), max(flen))
    return hist


def run(p, fs, fir_order, classes=START_CLASSES):
    """The whole corpus through the context p (an irdm.Pipeline at fs, its options set by the caller to match fir_order)
    at every start of `classes`, each call checked against the oracle in that order; then coverage().  Every mismatch is
    collected: the assertion names the windows and start classes that differ.  Returns dict(calls, hist, failures)."""
    import irdm
    wins = windows(fs)           # (before the order is set: the simplex-threshold windows are placed with the default order)
    L = orc.lib()
    n_fft = rates.fft_size(fs)
    results, failures = [], []
    dm = L.orc_downmix_create()
    orc.set_fir_order(fir_order)
    try:
        for wi, (name, iq, center_bin, fc) in enumerate(wins):
            x = orc.fptr(iq.view(np.float32))
            for cls, start in starts(fs, len(iq)):
                if cls not in classes:
                    continue
                rec = orc.BurstRec(id=100 + wi, start=start, stop=max(start + len(iq) - 2 * n_fft, 0), last_active=start,
                                   center_bin=center_bin, magnitude=-20.0, noise=-110.0, peak_rel=1.0, base_sum=1.0,
                                   num_samples=len(iq), avail_end=start + len(iq))
                want = orc.Frame()
                ok = L.orc_downmix_process(dm, C.byref(rec), x, fc, fs, n_fft, T0, C.byref(want))
                results.append(dict(name=name, cls=cls, reason=want.drop_reason, dec_len=want.dec_len, start=want.start,
                                    uw_start_idx=want.uw_start_idx, direction=want.direction, num_samples=want.num_samples))
                assert p.L.irdm_set_stream_origin(p.h, fc, T0) == 0
                fi, frame = p.downmix_burst(irdm.Burst.from_buffer_copy(bytes(rec)), iq)
                try:
                    check(fi, frame, want, ok)
                except AssertionError as e:
                    failures.append("%s @ %s (start %d, reason %d): %s" % (name, cls, start, want.drop_reason, e))
    finally:
        orc.set_fir_order(1)
        L.orc_downmix_destroy(dm)
    assert not failures, "%d of %d calls differ from the oracle at %d Hz, fir_order %d:\n%s" % (
        len(failures), len(results), fs, fir_order, "\n".join(failures))
    hist = coverage(results) if tuple(classes) == START_CLASSES else None
    return dict(calls=len(results), hist=hist)
