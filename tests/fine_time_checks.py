"""TEST INFRASTRUCTURE: the checks of the symbol timing estimator (option fine_time, csrc/fine_time.hpp) that the GPU test
(tests/test_gpu_fine_time.py) and the CPU-emulation test (tests/fine_time_emul_run.py) share: the kernel-test frames, the
comparison of irdm_fine_time_batch with tests/fine_time_model.py and with tests/golden/fine_time_records.json, and context
runs with the option off and on."""
import ctypes as C
import functools
import hashlib
import json
import os
import struct

import numpy as np

import fine_freq_scenes as sc
import fine_time_model as tm
import fine_time_scenes as ts
import irdm
import line_checks
import siggen
from line_checks import ragged3

# |tau_device - tau_model| [samples].  The sums are binary64 and the recurrence's error is near 1e-13 of the sum
# (csrc/symbol_clock.hpp): anything larger is a finding.  The largest seen is in the docstring of tests/test_fine_time_emul.py.
TAU_TOL = 1e-9
# quality is a ratio of sums the device forms in another order, with other sines and cosines, than numpy
QUALITY_RTOL = 1e-6
# |applied time - truth| [ns] on the 2 MHz seed-3 scene / the 10 MHz seed-3 scene at amp 0.05: the bounds of
# tests/test_fine_time_model.py
TRUTH_TOL_NS = {2_000_000: 520.0, 10_000_000: 1020.0}

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fine_time_records.json")

REC = np.dtype([("id", "<u8"), ("time_ns", "<u8"), ("tau", "<f8"), ("s_re", "<f8"), ("s_im", "<f8"), ("floor", "<f8"),
                ("corr", "<f4"), ("quality", "<f4"), ("flags", "<u4"), ("n", "<u4")])
assert REC.itemsize == C.sizeof(irdm.FineTime) == 64
TS_OFF = irdm.Demod.timestamp.offset
assert TS_OFF == irdm.DemodPacked.timestamp.offset == 8

CUTS = (63, 64, 65, 799, 800, 801, 1309, 1310, 1311, 4440)


def synthetic(tau, n=1500, seed=7):
    """a clean frame at 10 samples per symbol whose symbol centres lie at tau + 10 k samples: a burst at 100 samples per
    symbol, every tenth sample of it"""
    rng = np.random.default_rng(seed)
    big = siggen.make_burst(2_500_000, rng.integers(0, 4, size=n // 10 + 40).tolist(), 0.0, 0.3, 0.05)
    first = 20 * 100 - int(round(tau * 10))             # symbol 15's centre is sample 2000 of `big`
    return np.ascontiguousarray(big[first:first + 10 * n:10])


@functools.lru_cache(maxsize=None)
def kernel_frames():
    """name -> (frame, simplex): the oracle's 16 frames of the 2 MHz seed-3 scene, cuts of them (a frame repeated, where the cut
    is longer than the frame) with the simplex flag both ways, the special cases and the synthetic frames"""
    fr = [f["x"] for f in ts.oracle_frames(2_000_000, 3, 0.05)]
    assert len(fr) == 16 and all(len(x) >= 1310 for x in fr), [len(x) for x in fr]
    out = {}
    for i, x in enumerate(fr):
        out["oracle%d" % i] = (x, 0)
    for k, m in enumerate(CUTS):
        x = fr[k % len(fr)]
        cut = np.ascontiguousarray(np.tile(x, -(-m // len(x)))[:m])
        out["len%d" % m] = (cut, 0)
        out["len%d_simplex" % m] = (cut, 1)
    out["zero"] = (np.zeros(700, np.complex64), 0)
    nan = fr[3].copy()
    nan[1234] = np.complex64(complex(float("nan"), 0.0))
    out["nan"] = (nan, 0)
    inf = fr[3].copy()
    inf[7] = np.complex64(complex(0.0, float("inf")))
    out["inf"] = (inf, 0)
    late = fr[4].copy()                                 # not finite behind the window: no estimate either
    late[len(late) - 1] = np.complex64(complex(float("nan"), 0.0))
    out["nan_behind_window"] = (late, 1)
    rng = np.random.default_rng(43)
    out["noise"] = ((rng.normal(0, 0.01, 1500) + 1j * rng.normal(0, 0.01, 1500)).astype(np.complex64), 0)
    for tau in (-4.9, 0.0, 4.9):
        out["tau%+.1f" % tau] = (synthetic(tau), 0)
    return out


def batch_frames(n):
    """n (frame, simplex) for a batch: the kernel frames in turn, then cuts of the oracle's frames at lengths and offsets of
    their own, simplex every third"""
    kf = kernel_frames()
    fr = [kf[k][0] for k in kf if k.startswith("oracle")]
    have = list(kf.values())[:n]
    cuts = line_checks.fill_with_cuts([x for x, _ in have], fr, n)
    return have + [(x, int(i % 3 == 0)) for i, x in enumerate(cuts[len(have):])]


def compare(got, frames, what):
    """FineTime records of irdm_fine_time_batch against the model; returns the largest |tau_device - tau_model| and the largest
    relative difference of the qualities"""
    worst, worst_q = 0.0, 0.0
    assert len(got) == len(frames)
    for i, (g, (x, simplex)) in enumerate(zip(got, frames)):
        tau, q, flags, n = tm.estimate(x, bool(simplex))
        assert (g.flags, g.n, g.id) == (flags, n, i), (what, i, g.flags, g.n, g.id, flags, n)
        assert g.time_ns == 0 and g.corr == 0
        if flags & tm.INVALID:
            assert g.tau == 0 and g.quality == 0 and g.s_re == 0 and g.s_im == 0 and g.floor == 0
            continue
        # the record's tau and quality are what the host makes of its sums
        t_rec, q_rec = tm.tau_of_record(g.s_re, g.s_im, g.floor)
        assert g.tau == t_rec and g.quality == np.float32(q_rec), (what, i, g.tau, t_rec, g.quality, q_rec)
        assert -5.0 <= g.tau < 5.0
        d = abs(g.tau - tau)
        d = min(d, 10.0 - d)                            # (a line at the wrap: -5 and +5 are one place)
        worst = max(worst, d)
        assert d <= TAU_TOL, (what, i, g.tau, tau, d)
        dq = abs(float(g.quality) - q) / max(q, 1.0)
        worst_q = max(worst_q, dq)
        assert dq <= QUALITY_RTOL, (what, i, float(g.quality), q)
    return worst, worst_q


def bits(v):
    return "%016x" % struct.unpack("<Q", struct.pack("<d", v))[0]


def golden_records(names, frames, got):
    """{name: {"frame": hash of the samples, "simplex", "re" / "im" / "floor": the bits of the kernel's doubles, "flags", "n"}}"""
    return {k: dict(frame=hashlib.sha256(np.ascontiguousarray(x, np.complex64).tobytes()).hexdigest()[:16], simplex=int(s),
                    re=bits(g.s_re), im=bits(g.s_im), floor=bits(g.floor), flags=int(g.flags), n=int(g.n))
            for k, (x, s), g in zip(names, frames, got)}


def check_golden(got):
    """`got` of golden_records() against tests/golden/fine_time_records.json (the CPU emulation's records: the device gives
    the same bits); returns the number compared"""
    want = json.load(open(GOLDEN))["records"]
    assert list(got) == list(want), "the frames' names"
    for k, w in want.items():
        assert got[k]["frame"] == w["frame"], (k, "the frame's samples differ: the test's input, not the kernel")
        assert got[k] == w, (k, got[k], w)
    return len(want)


def stage_cases(p, write_golden=False):
    """the kernel against the model through irdm_fine_time_batch of context p (any rate: the call takes frames)"""
    kf = kernel_frames()
    names = list(kf)
    frames = [kf[k] for k in names]
    got = p.fine_time_batch([x for x, _ in frames], [s for _, s in frames])
    worst, worst_q = compare(got, frames, "kernel frames")
    by = dict(zip(names, got))
    for m in CUTS:
        for k in ("len%d" % m, "len%d_simplex" % m):
            assert by[k].n == m and by[k].flags == (tm.INVALID if m < 64 else 0), (k, by[k].flags, by[k].n)
    # the window: a cut of 800 samples and less is its own window with the flag either way, a longer one is not
    for m in CUTS:
        same = bits(by["len%d" % m].s_re) == bits(by["len%d_simplex" % m].s_re)
        assert same == (m <= 800), (m, same)
    assert bits(by["len1310"].s_re) != bits(by["len1309"].s_re)
    for k in ("zero", "nan", "inf", "nan_behind_window"):
        assert by[k].flags == tm.INVALID and by[k].tau == 0 and by[k].quality == 0, k
    assert by["noise"].flags == 0 and by["noise"].quality < 8
    # the synthetic frames: the sign and the wrap.  (0.1 samples: the pattern noise of 131 random symbols is near 0.03, and a
    # wrong sign or a wrap at another place is off by 9.8)
    for tau in (-4.9, 0.0, 4.9):
        g = by["tau%+.1f" % tau]
        assert g.flags == 0 and abs(g.tau - tau) < 0.1 and g.quality > 20, (tau, g.tau, g.quality)
    if write_golden:
        json.dump(dict(about="the records of fine_time_kernel (csrc/fine_time.hpp) on the CPU emulation for the frames of "
                             "tests/fine_time_checks.py kernel_frames(): the bits of Re S(f0), Im S(f0) and the floor",
                       records=golden_records(names, frames, got)), open(GOLDEN, "w"), indent=1)
    n_golden = check_golden(golden_records(names, frames, got))
    # batches of 1, 63 and 65 frames: a frame's record does not depend on its place or on its neighbours
    for n in (1, 63, 65):
        fr = batch_frames(n)
        got_n = p.fine_time_batch([x for x, _ in fr], [s for _, s in fr])
        w, wq = compare(got_n, fr, "batch of %d" % n)
        worst, worst_q = max(worst, w), max(worst_q, wq)
        for i in range(min(n, len(names))):
            assert bytes(got_n[i]) == bytes(got[i]), (n, i)
    assert p.fine_time_batch([]) == []
    # simplex = NULL is "none"
    assert bytes(p.fine_time_batch([kf["len1310"][0]])[0])[8:] == bytes(by["len1310"])[8:]
    assert p.stat("fine_time_launches") == 0          # (the stage call is none of the chain's)
    return dict(frames=len(names), golden=n_golden, worst=worst, worst_quality=worst_q)


def context_run(iq, fs, sizes, depth, options=(("fine_time", 1),), packed=False, after=None):
    """iq through a context; returns dict(summary or None, ftime = FineTime records, demods = byte matrix, launches, ...)"""
    p = irdm.Pipeline(fs, max_chunk_samples=max(sizes), max_bursts_per_chunk=1024, pipeline_depth=depth, start_time_ns=sc.START_NS)
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
            st = p.fine_time()
        except RuntimeError:
            st = None
        rec = np.frombuffer(p.poll_fine_time_raw().tobytes(), dtype=REC)
        demods = p.poll_demods_packed_raw() if packed else p.poll_demods_raw()
        out = dict(summary=st, ftime=rec, demods=demods, launches=p.stat("fine_time_launches"), tagged=p.tagged,
                   frames=p.poll_frames()[0] if not packed else None,
                   decoded=p.poll_decoded() if dict(options).get("decode_frames") else None,
                   ida=p.poll_ida() if dict(options).get("decode_ida") else None)
        if after:
            after(p)
        return out
    finally:
        p.close()


def but_time(demods):
    """the demodulator records (byte matrix) with timestamp blanked"""
    d = np.array(demods, copy=True)
    d[:, TS_OFF:TS_OFF + 8] = 0
    return d.tobytes()


def times(demods):
    return np.ascontiguousarray(demods[:, TS_OFF:TS_OFF + 8]).view("<u8").reshape(-1)


def check_summary(st, rec):
    """the summary is the histogram of tau - corr over the applied records"""
    ok = rec[(rec["flags"] & tm.NOT_OK) == 0]
    applied = ok["flags"] == 0
    assert st.frames_seen == len(rec) and st.frames_applied == int(applied.sum()) and st.frames_not_ok == len(rec) - len(ok)
    assert st.frames_invalid == int(np.sum((ok["flags"] & tm.INVALID) != 0))
    assert st.frames_ambiguous == int(np.sum(ok["flags"] == tm.AMBIGUOUS))
    counts = np.bincount([tm.bin_of(d) for d in (ok["tau"] - ok["corr"].astype(np.float64))[applied]], minlength=tm.NBINS)
    for q, got in ((0.5, st.median), (0.25, st.q25), (0.75, st.q75)):
        assert got == tm.quantile(counts, q), (q, got, tm.quantile(counts, q))


def context_checks(key, min_frames, thorough=True):
    """A standard scene through contexts with the option off and on, on the full and the packed record path; thorough: also
    in three feeds at depth 1, with the option set and cleared, through irdm_reset and with the bit layer's records.  Returns
    what was seen, for the caller to print."""
    iq, truth = sc.standard(*key)
    fs = key[0]
    n = len(iq)
    seen = {}

    def reset_restarts(p):
        p.poll_bursts(), p.poll_frames()
        before = p.fine_time()
        assert before.frames_applied >= min_frames
        p.reset()
        st = p.fine_time()
        assert bytes(st) == bytes(irdm.FineTimeSummary()) and p.poll_fine_time() == []
        # the same stream again: the same summary, not twice its counts
        p.feed_host(np.ascontiguousarray(iq))
        assert bytes(p.fine_time()) == bytes(before)
        seen["reset"] = True

    worst, spread = 0.0, 0.0
    for packed in (False, True):
        off = context_run(iq, fs, [n], 0, options=(), packed=packed)
        on = context_run(iq, fs, [n], 0, packed=packed, after=reset_restarts if thorough and not packed else None)
        # off: nothing launched, no records, no summary; set and cleared: the same
        assert off["launches"] == 0 and off["summary"] is None and len(off["ftime"]) == 0
        if thorough:
            back = context_run(iq, fs, [n], 0, options=(("fine_time", 1), ("fine_time", 0)), packed=packed)
            assert back["launches"] == 0 and len(back["ftime"]) == 0 and back["demods"].tobytes() == off["demods"].tobytes()
        assert on["launches"] > 0 and on["tagged"] == off["tagged"]
        # every field but timestamp bit for bit
        assert len(on["demods"]) == len(off["demods"]) >= min_frames
        assert but_time(on["demods"]) == but_time(off["demods"])
        rec = on["ftime"]
        ok = rec[(rec["flags"] & tm.NOT_OK) == 0]
        ids = np.ascontiguousarray(on["demods"][:, :8]).view("<u8").reshape(-1)
        assert list(ok["id"]) == list(ids)                      # the polled records pair with the demodulator's
        t_on, t_off = times(on["demods"]), times(off["demods"])
        assert t_on.tobytes() == ok["time_ns"].tobytes()
        applied = ok["flags"] == 0
        assert applied.sum() >= min_frames
        cf = np.ascontiguousarray(on["demods"][:, 16:24]).view("<f8").reshape(-1)
        if not packed:
            # irdm_frame_info_t keeps the downmixer's timestamp, and the time is the model's host rule on it
            assert [bytes(f) for f in on["frames"]] == [bytes(f) for f in off["frames"]]
            fi = {f.id: f for f in on["frames"] if f.drop_reason == 0}
            for r in rec:
                f = fi[int(r["id"])]
                assert r["corr"] == np.float32(f.uw_start) and r["n"] == f.num_samples
                d, flags = tm.delta(float(r["tau"]), int(r["flags"]) & ~tm.NOT_OK, float(r["corr"]))
                assert flags == int(r["flags"]) & ~tm.NOT_OK
                assert int(r["time_ns"]) == tm.refined_ns(f.timestamp, f.uw_start_idx, d), (r, f.timestamp, f.uw_start_idx)
        e_on, e_off = [], []
        for i in np.flatnonzero(applied):
            t = ts.truth_ns(truth, fs, int(t_off[i]), cf[i])
            e_on.append(float(t_on[i]) - t)
            e_off.append(float(t_off[i]) - (t - (5 + 16) / siggen.SYMBOL_RATE * 1e9))
        e_on, e_off = np.array(e_on), np.array(e_off)
        print("%s %s: %d applied, refined - truth mean %.0f max %.0f ns; unrefined - burst start mean %.0f, deviation from it max %.0f ns"
              % (key, "packed" if packed else "full", len(e_on), e_on.mean(), np.abs(e_on).max(), e_off.mean(),
                 np.abs(e_off - e_off.mean()).max()))
        assert np.abs(e_on).max() <= TRUTH_TOL_NS[fs], e_on
        worst = max(worst, float(np.abs(e_on).max()))
        spread = max(spread, float(np.abs(e_off - e_off.mean()).max()))
        check_summary(on["summary"], rec)
        if thorough:
            # one feed at depth 0 and three at depth 1: the same records, the same summary
            on3 = context_run(iq, fs, ragged3(n), 1, packed=packed)
            assert on3["ftime"].tobytes() == rec.tobytes() and on3["demods"].tobytes() == on["demods"].tobytes()
            assert bytes(on3["summary"]) == bytes(on["summary"])
        seen["packed" if packed else "full"] = len(ids)
    seen["worst_ns"] = worst
    seen["unrefined_spread_ns"] = spread
    seen["median"] = on["summary"].median
    if not thorough:
        return seen
    assert seen["reset"]
    # the records derived from a demodulator record inherit its time; fine_freq beside it changes the frequency alone
    dec = context_run(iq, fs, [n], 0, options=(("fine_time", 1), ("decode_frames", 1), ("decode_ida", 1)))
    t_dec = times(dec["demods"])
    assert len(dec["decoded"]) == len(dec["ida"]) == len(t_dec) >= min_frames and t_dec.tobytes() == t_on.tobytes()
    assert [d.timestamp for d in dec["decoded"]] == list(t_dec)
    assert [d.timestamp for d in dec["ida"]] == [t if d.ok else 0 for d, t in zip(dec["ida"], t_dec)]   # (a failed IDA carries nothing)
    both = context_run(iq, fs, [n], 0, options=(("fine_time", 1), ("fine_freq", 1)))
    assert times(both["demods"]).tobytes() == t_on.tobytes() and both["ftime"].tobytes() == rec.tobytes()
    return seen


group_refuses = functools.partial(line_checks.group_refuses, b"fine_time")
