"""TEST INFRASTRUCTURE: the checks of the carrier frequency estimator (option fine_freq, csrc/fine_freq.hpp) that the GPU
test (tests/test_gpu_fine_freq.py) and the CPU-emulation test (tests/fine_freq_emul_run.py) share: the kernel-test frames,
the comparison of irdm_fine_freq_batch with tests/fine_freq_model.py, and context runs with the option off and on."""
import ctypes as C
import functools

import numpy as np

import fine_freq_model as fm
import fine_freq_scenes as sc
import irdm
import line_checks
from line_checks import ragged3

# |df_device - df_model| [Hz].  A wrong grid point is off by 1 Hz and more (a fine step of 4 Hz is 1 Hz of df), so this bound
# cannot hide one.  The largest difference seen is in the docstring of tests/test_fine_freq_emul.py.
DF_TOL = 1e-3
# quality is a ratio of sums the device forms in another order, with other sines and cosines, than numpy
QUALITY_RTOL = 1e-6
# |refined - truth| [Hz] on the 2 MHz seed-3 scene and the 10 MHz scene at amp 0.05: the bound of tests/test_fine_freq_model.py
TRUTH_TOL = 4.0

REC = np.dtype([("id", "<u8"), ("freq_hz", "<f8"), ("df_hz", "<f4"), ("quality", "<f4"), ("flags", "<u4"), ("n", "<u4")])
assert REC.itemsize == C.sizeof(irdm.FineFreq) == 32
CF_OFF = irdm.Demod.center_frequency.offset
assert CF_OFF == irdm.DemodPacked.center_frequency.offset == 16


def shifted(x, hz):
    n = np.arange(len(x), dtype=np.float64)
    return (np.asarray(x, np.complex128) * np.exp(2j * np.pi * hz * n / fm.F_OUT)).astype(np.complex64)


@functools.lru_cache(maxsize=None)
def kernel_frames():
    """name -> frame: the oracle's frames of the 10 MHz scene (1910 and 4440 samples), cuts of them, and the special cases"""
    fr = [f[0] for f in sc.oracle_frames("standard", 10_000_000, 3, 0.05)]
    short = [x for x in fr if len(x) == 1910]
    long_ = [x for x in fr if len(x) == 4440]
    assert len(short) >= 4 and len(long_) >= 1, [len(x) for x in fr]
    out = {"len63": short[0][200:263], "len64": short[0][200:264], "len65": short[1][300:365], "len255": short[2][100:355],
           "len1910": short[3], "len4439": long_[0][:4439], "len4440": long_[0]}
    for i, x in enumerate(fr):
        out["oracle%d" % i] = x
    out["zero"] = np.zeros(700, np.complex64)
    nan = short[3].copy()
    nan[1234] = np.complex64(complex(float("nan"), 0.0))
    out["nan"] = nan
    inf = short[3].copy()
    inf[7] = np.complex64(complex(0.0, float("inf")))
    out["inf"] = inf
    rng = np.random.default_rng(43)
    out["noise"] = (rng.normal(0, 0.01, 1500) + 1j * rng.normal(0, 0.01, 1500)).astype(np.complex64)
    # a frame whose own offset is taken out first, so that its line sits exactly on an edge of the grid, and 120 Hz beyond it
    df0 = fm.estimate(short[2])[0]
    out["edge_plus"] = shifted(short[2], 250.0 - df0)
    out["edge_minus"] = shifted(short[2], -250.0 - df0)
    out["beyond_plus"] = shifted(short[2], 280.0 - df0)
    for k in ("edge_plus", "edge_minus", "beyond_plus"):
        df, _, flags, _ = fm.estimate(out[k])
        assert flags == fm.OUT_OF_RANGE and df == (-250.0 if k == "edge_minus" else 250.0), (k, df, flags)
    return out


def batch_frames(n):
    """n frames for a batch: the kernel frames in turn, then cuts of the oracle's frames at lengths and offsets of their own"""
    kf = kernel_frames()
    fr = [kf[k] for k in kf if k.startswith("oracle")]
    return line_checks.fill_with_cuts(list(kf.values())[:n], fr, n)


def compare(got, frames, what):
    """FineFreq records of irdm_fine_freq_batch against the model; returns the largest |df_device - df_model| and the largest
    relative difference of the qualities"""
    worst, worst_q = 0.0, 0.0
    assert len(got) == len(frames)
    for i, (g, x) in enumerate(zip(got, frames)):
        df, q, flags, n = fm.estimate(x)
        assert (g.flags, g.n, g.id) == (flags, n, i), (what, i, g.flags, g.n, g.id, flags, n)
        assert g.freq_hz == float(g.df_hz)
        d = abs(float(g.df_hz) - df)
        worst = max(worst, d)
        assert d <= DF_TOL, (what, i, float(g.df_hz), df, d)
        dq = abs(float(g.quality) - q) / max(q, 1.0)
        worst_q = max(worst_q, dq)
        assert dq <= QUALITY_RTOL, (what, i, float(g.quality), q)
        if flags & fm.INVALID:
            assert g.df_hz == 0 and g.quality == 0
    return worst, worst_q


def stage_cases(p):
    """the kernel against the model through irdm_fine_freq_batch of context p (any rate: the call takes frames)"""
    kf = kernel_frames()
    names = list(kf)
    got = p.fine_freq_batch([kf[k] for k in names])
    worst, worst_q = compare(got, [kf[k] for k in names], "kernel frames")
    by = dict(zip(names, got))
    assert by["len63"].flags == fm.INVALID and by["len63"].n == 63
    for k in ("len64", "len65", "len255", "len1910", "len4439", "len4440", "noise"):
        assert not by[k].flags & fm.INVALID and by[k].n == len(kf[k]), k
    for k in ("len1910", "len4439", "len4440"):
        assert by[k].flags == 0 and abs(by[k].df_hz) < 30 and by[k].quality > 8, (k, by[k].flags, by[k].df_hz, by[k].quality)
    assert by["noise"].quality < 6
    for k in ("zero", "nan", "inf"):
        assert by[k].flags == fm.INVALID and by[k].df_hz == 0 and by[k].quality == 0, k
    for k, edge in (("edge_plus", 250.0), ("edge_minus", -250.0), ("beyond_plus", 250.0)):
        assert by[k].flags == fm.OUT_OF_RANGE and by[k].df_hz == edge, (k, by[k].flags, by[k].df_hz)
    # batches of 1, 63 and 65 frames: a frame's record does not depend on its place or on its neighbours
    for n in (1, 63, 65):
        fr = batch_frames(n)
        got_n = p.fine_freq_batch(fr)
        w, wq = compare(got_n, fr, "batch of %d" % n)
        worst, worst_q = max(worst, w), max(worst_q, wq)
        for i in range(min(n, len(names))):
            assert bytes(got_n[i]) == bytes(got[i]), (n, i)
    assert p.fine_freq_batch([]) == []
    assert p.stat("fine_freq_launches") == 0          # (the stage call is none of the chain's)
    return dict(frames=len(names), worst=worst, worst_quality=worst_q)


def context_run(iq, fs, sizes, depth, options=(("fine_freq", 1),), packed=False, after=None):
    """iq through a context; returns dict(summary or None, fine = FineFreq records, demods = byte matrix, launches, decoded)"""
    p = irdm.Pipeline(fs, max_chunk_samples=max(sizes), max_bursts_per_chunk=1024, pipeline_depth=depth)
    try:
        if packed:
            p.set_option("packed_records", 1)
        for k, v in options:
            p.set_option(k, v)
        off = 0
        for c in sizes:
            p.feed_host(np.ascontiguousarray(iq[off:off + c]))
            off += c
        assert off == len(iq)
        if depth:
            p.flush()
        try:
            st = p.fine_freq()
        except RuntimeError:
            st = None
        fine = np.frombuffer(p.poll_fine_freq_raw().tobytes(), dtype=REC)
        demods = p.poll_demods_packed_raw() if packed else p.poll_demods_raw()
        out = dict(summary=st, fine=fine, demods=demods, launches=p.stat("fine_freq_launches"), tagged=p.tagged,
                   frames=p.poll_frames()[0] if not packed else None,
                   decoded=p.poll_decoded() if dict(options).get("decode_frames") else None,
                   ida=p.poll_ida() if dict(options).get("decode_ida") else None)
        if after:
            after(p)
        return out
    finally:
        p.close()


def but_frequency(demods):
    """the demodulator records (byte matrix) with center_frequency blanked"""
    d = np.array(demods, copy=True)
    d[:, CF_OFF:CF_OFF + 8] = 0
    return d.tobytes()


def frequencies(demods):
    return np.ascontiguousarray(demods[:, CF_OFF:CF_OFF + 8]).view("<f8").reshape(-1)


def check_summary(st, rec, pll):
    """the summary is the histogram of (refined - PLL) over the applied records; pll: the option-off frequencies of the
    records without NOT_OK"""
    ok = rec[(rec["flags"] & fm.NOT_OK) == 0]
    assert len(ok) == len(pll)
    applied = ok["flags"] == 0
    assert st.frames_seen == len(rec) and st.frames_applied == int(applied.sum()) and st.frames_not_ok == len(rec) - len(ok)
    assert st.frames_out_of_range == int(np.sum(ok["flags"] == fm.OUT_OF_RANGE))
    assert st.frames_invalid == int(np.sum((ok["flags"] & fm.INVALID) != 0))
    counts = np.bincount([fm.bin_of(d) for d in (ok["freq_hz"] - pll)[applied]], minlength=fm.NBINS)
    for q, got in ((0.5, st.median), (0.25, st.q25), (0.75, st.q75)):
        assert got == fm.quantile(counts, q), (q, got, fm.quantile(counts, q))


def context_checks(kind, key, min_frames, lengths=(), thorough=True):
    """A scene through contexts with the option off and on, on the full and the packed record path; thorough: also in three
    feeds at depth 1, with the option set and cleared, through irdm_reset and with the bit layer's records.  Returns what was
    seen, for the caller to print."""
    iq, truth = sc.standard(*key) if kind == "standard" else sc.drifting(*key)
    fs = key[0]
    n = len(iq)
    seen = {}

    def reset_restarts(p):
        p.poll_bursts(), p.poll_frames()
        before = p.fine_freq()
        assert before.frames_applied >= min_frames
        p.reset()
        st = p.fine_freq()
        assert bytes(st) == bytes(irdm.FineFreqSummary()) and p.poll_fine_freq() == []
        # the same stream again: the same summary, not twice its counts
        p.feed_host(np.ascontiguousarray(iq))
        assert bytes(p.fine_freq()) == bytes(before)
        seen["reset"] = True

    worst = 0.0
    for packed in (False, True):
        off = context_run(iq, fs, [n], 0, options=(), packed=packed)
        on = context_run(iq, fs, [n], 0, packed=packed, after=reset_restarts if thorough and not packed else None)
        # off: nothing launched, no records, no summary; set and cleared: the same
        assert off["launches"] == 0 and off["summary"] is None and len(off["fine"]) == 0
        if thorough:
            back = context_run(iq, fs, [n], 0, options=(("fine_freq", 1), ("fine_freq", 0)), packed=packed)
            assert back["launches"] == 0 and len(back["fine"]) == 0 and back["demods"].tobytes() == off["demods"].tobytes()
        assert on["launches"] > 0 and on["tagged"] == off["tagged"]
        # every field but center_frequency bit for bit
        assert len(on["demods"]) == len(off["demods"]) >= min_frames
        assert but_frequency(on["demods"]) == but_frequency(off["demods"])
        if not packed:                                  # (irdm_frame_info_t keeps the downmixer's frequency)
            assert [bytes(f) for f in on["frames"]] == [bytes(f) for f in off["frames"]]
        rec = on["fine"]
        ok = rec[(rec["flags"] & fm.NOT_OK) == 0]
        ids = np.ascontiguousarray(on["demods"][:, :8]).view("<u8").reshape(-1)
        assert list(ok["id"]) == list(ids)
        f_on, f_off = frequencies(on["demods"]), frequencies(off["demods"])
        applied = ok["flags"] == 0
        assert applied.sum() >= min_frames
        # applied: the record's freq_hz; flagged: the PLL's value bit for bit
        assert f_on[applied].tobytes() == ok["freq_hz"][applied].tobytes()
        assert f_on[~applied].tobytes() == f_off[~applied].tobytes()
        if not packed:                                  # freq_hz is the downmixer's value plus df_hz
            cf = {f.id: f.center_frequency for f in on["frames"] if f.drop_reason == 0}
            assert all(r["freq_hz"] == cf[int(r["id"])] + float(r["df_hz"]) for r in rec)
        ts = np.ascontiguousarray(on["demods"][:, 8:16]).view("<u8").reshape(-1)
        e_on, e_off = [], []
        for i in np.flatnonzero(applied):
            t = sc.truth_of(truth, fs, int(ts[i]), int(ok["n"][i]), f_off[i])
            e_on.append(abs(f_on[i] - t))
            e_off.append(abs(f_off[i] - t))
        assert max(e_on) <= TRUTH_TOL, e_on
        worst = max(worst, max(e_on))
        seen["pll_worst"] = max(e_off)
        for m in lengths:
            assert m in set(ok["n"][applied].tolist()), (m, sorted(set(ok["n"].tolist())))
        check_summary(on["summary"], rec, f_off)
        if thorough:
            # one feed at depth 0 and three at depth 1: the same records, the same summary
            on3 = context_run(iq, fs, ragged3(n), 1, packed=packed)
            assert on3["fine"].tobytes() == rec.tobytes() and on3["demods"].tobytes() == on["demods"].tobytes()
            assert bytes(on3["summary"]) == bytes(on["summary"])
        seen["packed" if packed else "full"] = len(ids)
    seen["worst"] = worst
    seen["median"] = on["summary"].median
    if not thorough:
        return seen
    assert seen["reset"]
    # the records derived from a demodulator record inherit its frequency
    dec = context_run(iq, fs, [n], 0, options=(("fine_freq", 1), ("decode_frames", 1), ("decode_ida", 1)))
    f_dec = frequencies(dec["demods"])
    assert len(dec["decoded"]) == len(dec["ida"]) == len(f_dec) >= min_frames
    assert [d.frequency for d in dec["decoded"]] == list(f_dec)
    assert [d.frequency for d in dec["ida"]] == [f if d.ok else 0.0 for d, f in zip(dec["ida"], f_dec)]   # (a failed IDA carries nothing)
    return seen


group_refuses = functools.partial(line_checks.group_refuses, b"fine_freq")
