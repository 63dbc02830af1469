"""TEST INFRASTRUCTURE: the checks of option scrub / irdm_scrub_device (csrc/scrub.hpp) that the GPU test
(tests/test_gpu_scrub.py) and the CPU-emulation test (tests/scrub_emul_run.py) share: the kernel against the numpy model of
tests/scrub_model.py, and a context with the option on, fed a stream with non-finite and huge samples, against a context
without it fed the model-scrubbed stream and against the oracle."""
import ctypes as C
import functools

import numpy as np

import irdm
import scrub_model as sm
import siggen

GUARD = 64
SIZES = (0, 1, 2, 3, 4, 5, 255, 256, 257, 4095, 4096, 4097, 65536 + 3)
LIMITS = (0, 24, 40, 127)
OTHER_FORMATS = {irdm.FMT_CI8: 2, irdm.FMT_CU8: 2, irdm.FMT_CI16: 4, irdm.FMT_CI16_FULL: 4, irdm.FMT_SC16Q11: 4, irdm.FMT_CI32: 8,
                 irdm.FMT_CI32_24: 8}                       # format -> bytes per sample
FIGURES = ("n_zeroed", "n_nonfinite", "n_over", "first", "last")


def limit_bits(e):
    return np.uint32((e + 127) << 23)


def zeroed_values(e):
    """bit patterns of components that are not good at limit 2^e: a quiet NaN, a signalling one, +-Inf, the float behind
    +-2^e"""
    L = limit_bits(e)
    return [0x7fc00000, 0x7fa00000, 0x7f800000, 0xff800000, int(L) + 1, (int(L) + 1) | 0x80000000]


def kept_values(e):
    """... and of components that are: +-2^e, -0.0, the smallest subnormal of either sign"""
    L = int(limit_bits(e))
    return [L, L | 0x80000000, 0x80000000, 0x00000001, 0x80000001]


def stat_tuple(st):
    return tuple(int(getattr(st, k)) for k in FIGURES)


def patterns(n, head):
    """the sets of bad sample indices of a region of n samples whose first 16-byte piece starts at sample `head`, each with
    the components to spoil (1 I, 2 Q, 3 both; 0 cycles through the three): none, all, about 1 %, and single ones at the
    head and the tail, 63 / 64 / 65 pieces in (the edge of a wavefront) and 255 / 256 pieces in (of a workgroup)"""
    out = [((), 0), (tuple(range(n)), 0), ("random", 0)]
    singles = [0, 1, n - 2, n - 1] + [head + 2 * k + j for k in (63, 64, 65, 255, 256) for j in (0, 1)]
    for s in sorted(set(i for i in singles if 0 <= i < n)):
        for comp in (1, 2, 3):
            out.append(((s,), comp))
    return out


def build_regions(sizes, extra_pieces, rng):
    """[(start byte, n, e, bad indices, components)] and the host image (uint32 words): clean samples within +-0.9 with the
    kept values strewn in, the bad samples written over them"""
    regions, size, k = [], 0, 0
    plan = []
    for n in sizes:
        for behind in (0, 1):
            for bad, comp in patterns(n, behind):
                plan.append((n, behind, bad, comp))
    for pieces in extra_pieces:
        n = 2 * pieces + 3
        for bad, comp in (((), 0), (tuple(range(n)), 0), ("random", 0), ((1 + 2 * 2048 * 256,), 2), ((n - 1,), 1), ((0,), 3)):
            plan.append((n, 1, bad, comp))
    for n, behind, bad, comp in plan:
        e = LIMITS[k % len(LIMITS)]
        k += 1
        start = size + GUARD + behind * 8                   # (size is a multiple of 64: so is the region's origin)
        if isinstance(bad, str):
            bad = tuple(np.flatnonzero(rng.random(n) < 0.01))
        regions.append((start, n, e, np.asarray(bad, np.int64), comp))
        size = (start + n * 8 + GUARD + 63) // 64 * 64
    host = rng.uniform(-0.9, 0.9, size // 4).astype(np.float32).view(np.uint32)
    for start, n, e, bad, comp in regions:
        w = host[start // 4:start // 4 + 2 * n]
        kept = np.asarray(kept_values(e), np.uint32)
        strew = np.flatnonzero(rng.random(2 * n) < 0.03)
        w[strew] = kept[rng.integers(0, len(kept), len(strew))]
        if len(bad):
            zv = np.asarray(zeroed_values(e), np.uint32)
            comps = np.full(len(bad), comp) if comp else 1 + np.arange(len(bad)) % 3
            vals = zv[(np.arange(len(bad)) + start // 8) % len(zv)]
            vals2 = zv[(np.arange(len(bad)) * 5 + 1 + start // 8) % len(zv)]
            w[2 * bad[(comps & 1) != 0]] = vals[(comps & 1) != 0]
            w[2 * bad[(comps & 2) != 0] + 1] = vals2[(comps & 2) != 0]
    return regions, host


def kernel_cases(extra_pieces=()):
    """irdm_scrub_device on every size, alignment and pattern of bad samples, the limits 2^0, 2^24, 2^40 and 2^127 taking
    turns: one device buffer holds every case's region (guard bytes in front and behind, the samples 0 or 1 sample behind a
    16-byte boundary), uploaded once.  The buffer equals the model's, guards included; all six figures are exact; every
    fifth case runs without statistics; a second pass zeroes and counts nothing.  Returns the number of cases."""
    rng = np.random.default_rng(91)
    regions, host = build_regions(SIZES, extra_pieces, rng)
    want = host.copy()
    figures = []
    for start, n, e, bad, comp in regions:
        y, fig = sm.scrub(host[start // 4:start // 4 + 2 * n].view(np.float32), e)
        want[start // 4:start // 4 + 2 * n] = y.view(np.uint32)
        assert fig["n_zeroed"] == len(bad) and (not len(bad) or (fig["first"], fig["last"]) == (bad.min(), bad.max())), (start, n, e)
        figures.append(fig)
    seen = dict(nonfinite=0, over=0, kept=0)
    d = irdm.device_buffer(host)
    try:
        assert d % 16 == 0
        for k, ((start, n, e, bad, comp), fig) in enumerate(zip(regions, figures)):
            rc, st = irdm.scrub_device(d + start, n, irdm.FMT_CF32, e, stats=k % 5 != 4)
            assert rc == 0, (start, n, e)
            if st is not None:
                assert (int(st.n_samples), st.limit_log2, st.active) == (n, e, 1), (start, n, e)
                assert stat_tuple(st) == tuple(fig[f] for f in FIGURES), (start, n, e, stat_tuple(st), fig)
            seen["nonfinite"] += fig["n_nonfinite"]
            seen["over"] += fig["n_over"]
        got = np.empty_like(host)
        irdm.device_download(got, d)
        diff = np.flatnonzero(got != want)
        assert len(diff) == 0, (len(diff), int(diff[0]), [r[:3] for r in regions if r[0] <= 4 * diff[0]][-1])
        # the kept values are still there
        for start, n, e, bad, comp in regions:
            seen["kept"] += int(np.isin(got[start // 4:start // 4 + 2 * n], np.asarray(kept_values(e), np.uint32)).sum())
        for start, n, e, bad, comp in regions:
            rc, st = irdm.scrub_device(d + start, n, irdm.FMT_CF32, e)
            assert rc == 0 and (int(st.n_samples), st.limit_log2, st.active) + stat_tuple(st) == (n, e, 1, 0, 0, 0, 0, 0), (start, n, e)
        irdm.device_download(got, d)
        assert np.array_equal(got, want)
    finally:
        irdm.device_free(d)
    assert min(seen.values()) > 100, seen
    return len(regions)


def refusal_cases():
    """the seven formats that are not cf32 return 0 with the buffer untouched and active 0; an unknown format, a pointer that
    is not aligned to a sample and a limit outside 0 .. 127 return -1"""
    rng = np.random.default_rng(92)
    host = rng.integers(0, 256, 4096, dtype=np.uint8)
    host[64:72] = np.array([float("nan"), float("inf")], np.float32).view(np.uint8)
    d = irdm.device_buffer(host)
    try:
        for fmt, bps in OTHER_FORMATS.items():
            for stats in (True, False):
                rc, st = irdm.scrub_device(d + GUARD, (4096 - 2 * GUARD) // bps, fmt, 40, stats=stats)
                assert rc == 0 and (st is None or ((int(st.n_samples), st.active, st.limit_log2) + stat_tuple(st) == (0, 0, 40, 0, 0, 0, 0, 0))), fmt
            if bps > 1:
                assert irdm.scrub_device(d + GUARD + bps // 2, 4, fmt)[0] == -1
        for bad_fmt in (-1, 5, 7, 10):
            assert irdm.scrub_device(d + GUARD, 4, bad_fmt)[0] == -1
        for off in (1, 2, 4):
            assert irdm.scrub_device(d + GUARD + off, 4, irdm.FMT_CF32)[0] == -1
        for e in (-1, 128, 1000):
            assert irdm.scrub_device(d + GUARD, 4, irdm.FMT_CF32, e)[0] == -1
            assert irdm.scrub_device(d + GUARD, 4, irdm.FMT_CI8, e)[0] == -1
        assert irdm.scrub_device(d + GUARD, 0, irdm.FMT_CF32)[0] == 0
        got = np.empty_like(host)
        irdm.device_download(got, d)
        assert np.array_equal(got, host)
    finally:
        irdm.device_free(d)
    return len(OTHER_FORMATS)


# ---------------------------------------------------------------- through a context ----
FS = 2_000_000
CHUNK = 262_144
MARGIN = 5000
BAD_VALUES = (float("nan"), float("inf"), float("-inf"), 1e30)


def as_floats(iq):
    return np.ascontiguousarray(iq).view(np.float32).reshape(-1)


@functools.lru_cache(maxsize=None)
def streams():
    """S = siggen.standard_scene(2 MHz, 2 M samples, 12 bursts, seed 3) as interleaved floats; S' = S with NaN, +Inf, -Inf
    and 1e30 written into the gaps between its bursts -- sample 0, the last sample, the last sample of the first
    262 144-sample chunk, the first of the second, and the middle of every gap of the scene's truth that is wide enough --;
    S'' = the model's scrub of S'; and the model's figures"""
    iq, truth = siggen.standard_scene(FS, FS, 12, 3)
    s = as_floats(iq).copy()
    n = len(iq)
    spans = sorted((t["start"], t["start"] + t["n"]) for t in truth)
    where = [0, CHUNK - 1, CHUNK, n - 1]
    for (_, a1), (b0, _) in zip(spans[:-1], spans[1:]):
        if b0 - a1 > 4 * MARGIN:
            where.append((a1 + b0) // 2)
    where = sorted(set(where))
    for w in where:
        assert all(w < a - MARGIN or w >= b + MARGIN for a, b in spans), w
    assert len(where) >= 8
    sp = s.copy()
    for k, w in enumerate(where):
        comp = 1 + k % 3
        if comp & 1:
            sp[2 * w] = np.float32(BAD_VALUES[k % 4])
        if comp & 2:
            sp[2 * w + 1] = np.float32(BAD_VALUES[(k + k // 4 + 1) % 4])
    spp, fig = sm.scrub(sp, 40)
    assert fig["n_zeroed"] == len(where) and (fig["first"], fig["last"]) == (0, n - 1) and fig["n_over"] > 0 and fig["n_nonfinite"] > 0
    for a in (s, sp, spp):
        a.setflags(write=False)
    return s, sp, spp, fig, tuple(where)


def run(samples, depth, options, after=None):
    """interleaved floats through a cf32 context in chunks of 262 144 samples; the records as objects (for tests/parity.py)
    and as bytes"""
    p = irdm.Pipeline(FS, fmt=irdm.FMT_CF32, max_chunk_samples=CHUNK, max_bursts_per_chunk=1024, pipeline_depth=depth)
    try:
        p.set_option("keep_frame_samples", 1)
        for k, v in options:
            p.set_option(k, v)
        x = samples.view(np.complex64)
        for off in range(0, len(x), CHUNK):
            p.feed_host(np.ascontiguousarray(x[off:off + CHUNK]))
        if depth:
            p.flush()
        bursts = p.poll_bursts()
        infos, frame_samples = p.poll_frames()
        demods = p.poll_demods()
        out = dict(bursts=bursts, infos=infos, samples=frame_samples, demods=demods, tagged=p.tagged, n_samples=p.sample_count,
                   bytes=(b"".join(bytes(b) for b in bursts), b"".join(bytes(f) for f in infos), b"".join(bytes(d) for d in demods),
                          b"".join(np.ascontiguousarray(s).tobytes() for s in frame_samples)))
        if after:
            after(p)
        return out
    finally:
        p.close()


def oracle_clean():
    """the CPU-only assertion: the oracle on S'' gives S's 12 frames with every unique word ok"""
    import orc
    s, sp, spp, fig, where = streams()
    ref, ref_s = orc.run_stream(spp.view(np.complex64), FS), orc.run_stream(s.view(np.complex64), FS)
    for r in (ref, ref_s):
        assert len(r.demods) == 12 and all(d.ok for d in r.demods), len(r.demods)
    assert [(d.id, bytes(d.bits[:d.n_bits])) for d in ref.demods] == [(d.id, bytes(d.bits[:d.n_bits])) for d in ref_s.demods]
    return ref


def pipeline_case(depth):
    """a context with scrub on, fed S', against a context without it fed S'': the burst, frame and demod records and the
    frames' samples bit for bit; tests/parity.py's comparison with the oracle on S''; irdm_scrub_stats equals the model's
    figures in stream coordinates; irdm_reset clears them; a change of either option in mid-stream and a device feed with the
    option on return -1"""
    import parity
    s, sp, spp, fig, where = streams()
    ref = oracle_clean()
    seen = {}

    def checks(p):
        L = irdm.lib()
        st = p.scrub_stats()
        print("scrub stats depth %d: n %d zeroed %d nonfinite %d over %d first %d last %d" % ((depth, int(st.n_samples)) + stat_tuple(st)))
        assert (int(st.n_samples), st.limit_log2, st.active) == (len(sp) // 2, 40, 1)
        assert stat_tuple(st) == tuple(fig[f] for f in FIGURES), (stat_tuple(st), fig)
        # the stream has begun with scrub 1 at 2^40: the same values are taken, others are not
        assert L.irdm_set_option(p.h, b"scrub", 0) == -1 and L.irdm_set_option(p.h, b"scrub", 1) == 0
        assert L.irdm_set_option(p.h, b"scrub_limit_log2", 24) == -1 and L.irdm_set_option(p.h, b"scrub_limit_log2", 40) == 0
        d = irdm.device_buffer(np.zeros(2 * 32768, np.float32))
        try:
            assert L.irdm_feed_device(p.h, C.c_void_p(d), 32768, None) == -1
            assert L.irdm_feed_begin(p.h, C.c_void_p(d), 32768, None) == -1
        finally:
            irdm.device_free(d)
        p.reset()
        st = p.scrub_stats()
        assert (int(st.n_samples), st.limit_log2, st.active) + stat_tuple(st) == (0, 40, 1, 0, 0, 0, 0, 0)
        # a new stream may choose again, within 0 .. 127
        assert L.irdm_set_option(p.h, b"scrub_limit_log2", 128) == -1 and L.irdm_set_option(p.h, b"scrub_limit_log2", -1) == -1
        p.set_option("scrub_limit_log2", 24)
        p.feed_host(np.ascontiguousarray(sp.view(np.complex64)[:CHUNK]))
        st = p.scrub_stats()
        want = sm.scrub(sp[:2 * CHUNK], 24)[1]
        assert (int(st.n_samples), st.limit_log2) == (CHUNK, 24) and stat_tuple(st) == tuple(want[f] for f in FIGURES)
        p.set_option("scrub", 1)
        seen["checks"] = True

    def off_checks(p):
        # the option off: no figures
        assert irdm.lib().irdm_scrub_stats(p.h, C.byref(irdm.ScrubStats())) == -1
        seen["off"] = True

    on = run(sp, depth, (("scrub", 1),), after=checks)
    off = run(spp, depth, (), after=off_checks)
    assert seen == dict(checks=True, off=True)
    for k, name in enumerate(("bursts", "frames", "demods", "frame samples")):
        assert on["bytes"][k] == off["bytes"][k], (name, depth)
    assert len(on["demods"]) == 12 and on["tagged"] == off["tagged"]
    return parity.compare(on, ref)


def oracle_blind_case():
    """the oracle alone on S': no frame behind the first bad sample (sample 0: none at all)"""
    import orc
    s, sp, spp, fig, where = streams()
    ref = orc.run_stream(sp.view(np.complex64), FS)
    return dict(bursts=len(ref.bursts), demods=len(ref.demods))
