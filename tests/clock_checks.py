"""TEST INFRASTRUCTURE: the checks of the symbol clock estimator (option symbol_clock, csrc/symbol_clock.hpp) that the GPU
test (tests/test_gpu_clock.py) and the CPU-emulation test (tests/clock_emul_run.py) share: the kernel-test frames, the
comparison of irdm_symbol_clock_batch with tests/clock_model.py, and a context run with the option on."""
import functools

import numpy as np

import clock_model as cm
import irdm
import line_checks
from line_checks import ragged3      # noqa: F401 (the tests call it through this module too)
import orc
import resample_model as rm
import siggen

# |eps_device - eps_model| over kernel_frames(), absolute (a fraction): the largest value measured on the CPU emulation of
# the kernel is 1.85e-9 (1.9e-7 %: the record's eps is a float, half an ulp of 0.04 is 1.9e-9).  Four times that is asserted; the bound
# has to stay under 1e-4 (0.01 %, a tenth of the grid step).
EPS_MEASURED = 1.85e-9
EPS_TOL = 4 * EPS_MEASURED
assert EPS_TOL < 1e-4
# quality is a ratio of sums the device forms in another order than numpy: the same relative bound, on a float
QUALITY_RTOL = 1e-6


@functools.lru_cache(maxsize=None)
def oracle_frames(fs):
    """the downmixed frames (drop_reason 0) of standard_scene(fs, fs // 2, 12, 3) as the CPU oracle cuts them"""
    iq, _ = siggen.standard_scene(fs, fs // 2, 12, 3)
    r = orc.run_stream(iq, fs)
    return tuple(np.array(f.samples[:2 * f.num_samples], np.float32).view(np.complex64) for f in r.frames if f.drop_reason == 0)


def long_frame():
    """4440 samples at 10.025 samples per symbol: a 444-symbol burst at the fractional rate (resample_model)"""
    q = np.random.default_rng(41).integers(0, 4, 450)
    x = rm.make_burst_fractional(250_625, q, 300.0, 0.4)
    x = x[40:40 + cm.MAX_SAMPLES]
    noise = np.random.default_rng(42).normal(0, 0.002, (len(x), 2)).astype(np.float32)
    return (x + noise[:, 0] + 1j * noise[:, 1]).astype(np.complex64)


def resampled(x, L, M):
    """x at L / M of its rate (the float model of the front end's rational mode on its own design for that ratio)"""
    taps = rm.design_taps(20_000 * M, 20_000 * L)
    return rm.run(np.ascontiguousarray(x, np.complex64), irdm.FMT_CF32, L, M, 0, taps)[:cm.MAX_SAMPLES]


@functools.lru_cache(maxsize=None)
def kernel_frames():
    """name -> frame: cut from the oracle's frames of the 10.025 MHz scene, and the special cases"""
    fr = oracle_frames(10_025_000)
    assert len(fr) >= 9 and all(len(x) == 1910 for x in fr)
    rng = np.random.default_rng(43)
    out = {"len63": fr[0][:63], "len64": fr[0][:64], "len65": fr[1][300:365], "len1910": fr[2], "len4440": long_frame()}
    for i, x in enumerate(fr):
        out["oracle%d" % i] = x
    out["zero"] = np.zeros(700, np.complex64)
    nan = fr[3].copy()
    nan[1234] = np.complex64(complex(float("nan"), 0.0))
    out["nan"] = nan
    inf = fr[3].copy()
    inf[7] = np.complex64(complex(0.0, float("inf")))
    out["inf"] = inf
    out["noise"] = (rng.normal(0, 0.01, 1500) + 1j * rng.normal(0, 0.01, 1500)).astype(np.complex64)
    out["resampled_0.9"] = resampled(fr[4], 9, 10)          # sps 9.02, eps -9.8 %: the line among the guard points
    out["resampled_111_121"] = resampled(fr[4], 111, 121)   # sps 9.197, eps -8.03 %: the line a third of a grid step beyond it
    return out


def batch_frames(n):
    """n frames for a batch: the kernel frames in turn, then cuts of the oracle's frames at lengths and offsets of their own"""
    fr = oracle_frames(10_025_000)
    return line_checks.fill_with_cuts(list(kernel_frames().values())[:n], fr, n)


def compare(got, frames, what):
    """ClockEst records of irdm_symbol_clock_batch against the model; returns the largest |eps_device - eps_model|"""
    worst = 0.0
    assert len(got) == len(frames)
    for i, (g, x) in enumerate(zip(got, frames)):
        e, q, flags, n = cm.estimate(x)
        assert (g.flags, g.n, g.id) == (flags, n, i), (what, i, g.flags, g.n, g.id, flags, n)
        d = abs(float(g.eps) - e)
        worst = max(worst, d)
        assert d <= EPS_TOL, (what, i, float(g.eps), e, d)
        assert abs(float(g.quality) - q) <= QUALITY_RTOL * max(q, 1.0), (what, i, float(g.quality), q)
        if flags & cm.INVALID:
            assert g.eps == 0 and g.quality == 0
    return worst


def stage_cases(p):
    """the kernel against the model through irdm_symbol_clock_batch of context p (any rate: the call takes frames)"""
    kf = kernel_frames()
    names = list(kf)
    got = p.symbol_clock_batch([kf[k] for k in names])
    worst = compare(got, [kf[k] for k in names], "kernel frames")
    by = dict(zip(names, got))
    assert by["len63"].flags == cm.INVALID and by["len63"].n == 63
    for k in ("len64", "len65", "len1910", "len4440", "noise"):
        assert not by[k].flags & cm.INVALID and by[k].n == len(kf[k]), k
    for k in ("zero", "nan", "inf"):
        assert by[k].flags == cm.INVALID and by[k].eps == 0 and by[k].quality == 0, k
    assert by["len4440"].flags == 0 and abs(by["len4440"].eps - 0.0025) < 5e-4, by["len4440"].eps
    assert by["noise"].quality < 8 < by["len1910"].quality
    # a line just beyond the edge: the maximum is at the edge; one far beyond it: a guard point exceeds the grid's maximum
    for k in ("resampled_111_121", "resampled_0.9"):
        assert by[k].flags == cm.OUT_OF_RANGE and by[k].eps == np.float32(-0.08), (k, by[k].flags, by[k].eps)
    # batches of 1, 63 and 65 frames: a frame's record does not depend on its place or on its neighbours
    for n in (1, 63, 65):
        fr = batch_frames(n)
        got_n = p.symbol_clock_batch(fr)
        worst = max(worst, compare(got_n, fr, "batch of %d" % n))
        for i in range(min(n, len(names))):
            assert bytes(got_n[i]) == bytes(got[i]), (n, i)
    assert p.symbol_clock_batch([]) == []
    return dict(frames=len(names), worst=worst, far_edge_flags=int(by["resampled_0.9"].flags), far_edge_eps=float(by["resampled_0.9"].eps),
                far_edge_quality=float(by["resampled_0.9"].quality))


def context_run(iq, fs, sizes, depth, options=(("symbol_clock", 1),), packed=False, after=None):
    """iq through a context; returns (SymbolClock or None, ClockEst byte matrix, demod byte matrix, stats)"""
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
            st = p.symbol_clock()
        except RuntimeError:
            st = None
        clock = p.poll_symbol_clock_raw()
        demods = p.poll_demods_packed_raw() if packed else p.poll_demods_raw()
        stats = {k: p.stat(k) for k in ("scan_fast_chunks", "scan_fallbacks", "band_chunks", "band_rounds", "band_retries",
                                        "band_aborts", "k1_lists", "rot_rows", "rot_runs", "rot_ckpts", "scratch_peak", "resets")}
        stats["tagged"] = p.tagged
        if after:
            after(p)
        return st, clock, demods, stats
    finally:
        p.close()


group_refuses = functools.partial(line_checks.group_refuses, b"symbol_clock")


def check_summary(st, clock):
    """the summary is the histogram of the records: counts, quartiles as bin centres, the implied rate"""
    rec = np.frombuffer(clock.tobytes(), dtype=np.dtype([("id", "<u8"), ("eps", "<f4"), ("quality", "<f4"), ("flags", "<u4"), ("n", "<u4")]))
    ok = rec[(rec["flags"] & cm.NOT_OK) == 0]
    used = ok[ok["flags"] == 0]
    assert st.frames_used == len(used) and st.frames_not_ok == len(rec) - len(ok)
    assert st.frames_out_of_range == int(np.sum(ok["flags"] == cm.OUT_OF_RANGE))
    counts = np.bincount([cm.bin_of(e) for e in used["eps"]], minlength=cm.NBINS)
    for q, got in ((0.5, st.median), (0.25, st.q25), (0.75, st.q75)):
        assert abs(got - cm.quantile(counts, q)) < 1e-12, (q, got, cm.quantile(counts, q))
    return rec
