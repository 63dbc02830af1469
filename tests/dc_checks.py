"""TEST INFRASTRUCTURE: the checks of the DC tracker (csrc/dc_block.hpp) that the GPU test (tests/test_gpu_dc.py) and the
CPU-emulation test (tests/dc_emul_run.py) share: the kernels through irdm_dc_block_device against the numpy model of
tests/dc_model.py, and a context with irdm_dc_block against a plain context fed the model-corrected stream and against the
oracle."""
import ctypes as C
import functools

import numpy as np

import balance_model as bm
import dc_model as dm
import irdm
import siggen

GUARD = 64
FILL = 0xA5
SIZES = (0, 1, 2, 3, 4, 5, 255, 256, 257, 4095, 4096, 4097, 65536 + 3)
FMTS = tuple(bm.FORMATS)
LOG2 = 12
SEED = (0.03, -0.018)
# cf32 bit patterns strewn in: quiet and signalling NaN, +-Inf, +-1e30, +-64 and the floats beside them, -0.0, subnormals, and
# the quantiser's smallest steps: 2^-33 (a tie: 0) and the float above it (1), 2^-32 (1), 1.5 and 2.5 times 2^-32 (ties: 2, 2)
SPECIALS = (0x7fc00000, 0x7fa00000, 0xffc00001, 0xffa00123, 0x7f800000, 0xff800000, 0x7149f2ca, 0xf149f2ca, 0x42800000, 0xc2800000,
            0x427fffff, 0x42800001, 0xc27fffff, 0xc2800001, 0x80000000, 0x00000001, 0x80000001, 0x007fffff, 0x807fffff,
            0x2f000000, 0x2f000001, 0xaf000001, 0x2f800000, 0x2fc00000, 0xafc00000, 0x30200000)


def random_bytes(fmt, n, rng):
    """n samples of format fmt as bytes: the whole code range for the integer formats; cf32 +-0.9 with SPECIALS in I, in Q and
    in both of about one sample in twenty"""
    t = bm.FORMATS[fmt][0]
    if fmt == irdm.FMT_CF32:
        w = rng.uniform(-0.9, 0.9, 2 * n).astype(np.float32).view(np.uint32)
        at = np.flatnonzero(rng.random(n) < 0.05)
        comp = 1 + rng.integers(0, 3, len(at))
        sp = np.asarray(SPECIALS, np.uint32)
        vi, vq = sp[rng.integers(0, len(sp), len(at))], sp[rng.integers(0, len(sp), len(at))]
        w[2 * at[(comp & 1) != 0]] = vi[(comp & 1) != 0]
        w[2 * at[(comp & 2) != 0] + 1] = vq[(comp & 2) != 0]
        return w.view(np.uint8)
    if fmt == irdm.FMT_SC16Q11:
        return rng.integers(-2048, 2048, 2 * n).astype(t).view(np.uint8)
    if fmt == irdm.FMT_CI32_24:
        return rng.integers(-(1 << 23), 1 << 23, 2 * n).astype(t).view(np.uint8)
    info = np.iinfo(t)
    return rng.integers(info.min, info.max + 1, 2 * n).astype(t).view(np.uint8)


def edge_first(fmt, sb, which):
    """the stream position of a region's sample 0 such that an edge of the 4096-sample blocks falls at its sample 1, inside
    its fourth 16-byte piece, at the end of its first wavefront's 64 pieces, at the end of its first workgroup's 256"""
    bps = bm.FORMATS[fmt][1]
    spv = 16 // bps
    head = (spv - sb) % spv                     # samples up to the first 16-byte boundary
    e = (1, head + 3 * spv + 1, head + 64 * spv, head + 256 * spv)[which]
    return 7 * 4096 - e


def build_regions(extra_pieces, rng, behinds=(0, 1)):
    """[(fmt, n, src byte offset, dst byte offset, first sample)] for every format x size x alignment (src and dst 0 and 1
    sample behind a 16-byte boundary), the four edge placements taking turns so that the four alignments of a format and
    a size meet all four; the source image and the size of the destination image; GUARD bytes about every region"""
    plan, k = [], 0
    for fmt in FMTS:
        for n in SIZES:
            for sb in behinds:
                for db in behinds:
                    plan.append((fmt, n, sb, db, edge_first(fmt, sb, (k + k // 4) % 4)))
                    k += 1
    for fmt in FMTS:
        for pieces in extra_pieces:
            plan.append((fmt, pieces * (16 // bm.FORMATS[fmt][1]) + 777, 1, 1, edge_first(fmt, 1, 1)))
    regions, s_size, d_size = [], 0, 0
    for fmt, n, sb, db, first in plan:
        bps = bm.FORMATS[fmt][1]
        s0, d0 = s_size + GUARD + sb * bps, d_size + GUARD + db * 8
        regions.append((fmt, n, s0, d0, first))
        s_size, d_size = (s0 + n * bps + GUARD + 63) // 64 * 64, (d0 + n * 8 + GUARD + 63) // 64 * 64
    src = np.full(s_size, FILL, np.uint8)
    for fmt, n, s0, d0, first in regions:
        src[s0:s0 + n * bm.FORMATS[fmt][1]] = random_bytes(fmt, n, rng)
    return regions, src, d_size


def entry_state(first, k):
    """the state a region's call starts from: the seed, and sums for the block under way"""
    st = irdm.DcState()
    st.mean_i, st.mean_q = SEED
    if first % (1 << LOG2):
        st.sum_i, st.sum_q = (1 << 33) * (k % 7 - 3) + k, -(1 << 31) * (k % 5) + 3 * k
    return st


def state_tuple(st):
    return int(st.sum_i), int(st.sum_q), np.float32(st.mean_i), np.float32(st.mean_q)


def same_state(got, want):
    return got[:2] == tuple(want[:2]) and np.float32(got[2]).tobytes() == np.float32(want[2]).tobytes() and \
        np.float32(got[3]).tobytes() == np.float32(want[3]).tobytes()


def kernel_cases(extra_pieces=()):
    """irdm_dc_block_device against dc_model.run(convert(bytes)), every output byte and state_io exact: all eight formats, n in
    0 .. 5, 255 .. 257, 4095 .. 4097, 65536 + 3 (extra_pieces: and that many 16-byte pieces + 777 samples), src and dst 0 and 1
    sample behind a 16-byte boundary, blocks of 4096 with an edge at sample 1, inside a piece, at a wavefront's and at a
    workgroup's edge, a seed and sums of a block under way; guard bytes of dst and all of src untouched; a second call gives
    the same bytes; the 8-byte formats once more in place"""
    rng = np.random.default_rng(20260)
    regions, src, d_size = build_regions(extra_pieces, rng)
    want = np.full(d_size, FILL, np.uint8)
    want_state, seen = [], dict(nan=0, inf=0, clamp=0, negzero=0, subnormal=0, closed=0, carried=0)
    for k, (fmt, n, s0, d0, first) in enumerate(regions):
        x = bm.convert(src[s0:s0 + n * bm.FORMATS[fmt][1]], fmt)
        st = entry_state(first, k)
        y, state, means = dm.run(x, LOG2, SEED, first, (st.sum_i, st.sum_q))
        want[d0:d0 + 8 * n] = y.view(np.uint8)
        want_state.append(state if n else state_tuple(st))
        with np.errstate(all="ignore"):
            seen["nan"] += int(np.isnan(x).sum())
            seen["inf"] += int(np.isinf(x).sum())
            seen["clamp"] += int((np.abs(x) >= 64).sum())
            seen["negzero"] += int((x.view(np.uint32) == 0x80000000).sum())
            seen["subnormal"] += int(((np.abs(x) < np.float32(2.0**-126)) & (x != 0)).sum())
        seen["closed"] += len(means)
        seen["carried"] += 1 if n and first % 4096 and (first + n) % 4096 else 0
    d_src, d_dst = irdm.device_buffer(src), irdm.device_buffer(np.full(d_size, FILL, np.uint8))
    n_again = n_in_place = 0
    try:
        assert d_src % 16 == 0 and d_dst % 16 == 0
        for k, (fmt, n, s0, d0, first) in enumerate(regions):
            st = entry_state(first, k)
            assert irdm.dc_block_device(fmt, d_dst + d0, d_src + s0, n, LOG2, first, st) == 0, (fmt, n, s0, d0)
            assert same_state(state_tuple(st), want_state[k]), (fmt, n, s0 % 16, d0 % 16, first, state_tuple(st), want_state[k])
        got, src_after = np.empty_like(want), np.empty_like(src)
        irdm.device_download(got, d_dst)
        irdm.device_download(src_after, d_src)
        assert np.array_equal(src_after, src)
        for k, (fmt, n, s0, d0, first) in enumerate(regions):
            g, w = got[d0:d0 + 8 * n].view(np.uint32), want[d0:d0 + 8 * n].view(np.uint32)
            bad = np.flatnonzero(g != w)
            assert len(bad) == 0, (fmt, n, s0 % 16, d0 % 16, first, int(bad[0]), hex(g[bad[0]]), hex(w[bad[0]]))
        assert np.array_equal(got, want)            # (guard bytes and what no region covers included)
        # once more from 4095 samples on: the same bytes
        for k, (fmt, n, s0, d0, first) in enumerate(regions):
            if n >= 4095:
                st = entry_state(first, k)
                assert irdm.dc_block_device(fmt, d_dst + d0, d_src + s0, n, LOG2, first, st) == 0
                assert same_state(state_tuple(st), want_state[k])
                n_again += 1
        irdm.device_download(got, d_dst)
        assert np.array_equal(got, want)
        # the 8-byte formats in place: the source buffer's own regions
        mask = np.ones(len(src), bool)
        for k, (fmt, n, s0, d0, first) in enumerate(regions):
            if bm.FORMATS[fmt][1] == 8:
                st = entry_state(first, k)
                assert irdm.dc_block_device(fmt, d_src + s0, d_src + s0, n, LOG2, first, st) == 0, (fmt, n, s0)
                assert same_state(state_tuple(st), want_state[k])
        irdm.device_download(src_after, d_src)
        for k, (fmt, n, s0, d0, first) in enumerate(regions):
            if bm.FORMATS[fmt][1] == 8:
                assert np.array_equal(src_after[s0:s0 + 8 * n], want[d0:d0 + 8 * n]), ("in place", fmt, n, s0 % 16)
                mask[s0:s0 + 8 * n] = False
                n_in_place += 1
        assert np.array_equal(src_after[mask], src[mask])
    finally:
        irdm.device_free(d_src)
        irdm.device_free(d_dst)
    assert min(seen.values()) > 20, seen
    return dict(cases=len(regions), again=n_again, in_place=n_in_place)


def refusal_cases():
    """-1 for an unknown format, a block length outside 12 .. 24, misaligned pointers, overlapping buffers (other than an 8-byte
    format in place), a mean in state_io that is not finite or lies beyond +-64; nothing is written.  irdm_dc_mean_host
    equals the model and refuses an unknown format and more than 2^24 samples."""
    host = np.full(8192, FILL, np.uint8)
    d = irdm.device_buffer(host)
    try:
        src, dst = d + GUARD, d + 4096

        def call(fmt, out, inp, n=4, log2=LOG2, mean=(0.0, 0.0)):
            st = irdm.DcState()
            st.mean_i, st.mean_q = mean
            return irdm.dc_block_device(fmt, out, inp, n, log2, 0, st)
        for bad_fmt in (-1, 5, 7, 10):
            assert call(bad_fmt, dst, src) == -1
        for fmt, (t, bps) in bm.FORMATS.items():
            assert call(fmt, dst + 2048, src) == 0              # (the control: this one is taken)
            assert call(fmt, dst, src + bps // 2) == -1
            assert call(fmt, dst + 4, src) == -1
            if bps != 8:
                assert call(fmt, src, src) == -1
            assert call(fmt, src - 8, src) == -1
            for log2 in (-1, 0, 11, 25, 64):
                assert call(fmt, dst, src, log2=log2) == -1
        for mean in ((float("nan"), 0.0), (0.0, float("inf")), (64.5, 0.0), (0.0, -65.0)):
            assert call(irdm.FMT_CF32, dst, src, mean=mean) == -1
        assert call(irdm.FMT_CF32, dst, src, mean=(64.0, -64.0)) == 0
        got = np.empty_like(host)
        irdm.device_download(got, d)
        assert (got[:4096] == FILL).all()
    finally:
        irdm.device_free(d)
    rng = np.random.default_rng(5)
    for fmt, (t, bps) in bm.FORMATS.items():
        raw = random_bytes(fmt, 5000, rng)
        for n in (0, 1, 4096, 5000):
            got, want = irdm.dc_mean_host(fmt, raw, n), (dm.head_mean(bm.convert(raw, fmt), n) if n else (np.float32(0), np.float32(0)))
            assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes(), (fmt, n, got, want)
    assert irdm.dc_mean_host(5, np.zeros(16, np.uint8), 1) is None
    assert irdm.dc_mean_host(irdm.FMT_CI8, np.zeros(16, np.uint8), (1 << 24) + 1) is None
    return len(bm.FORMATS)


def carry_case():
    """one stream of 250 000 samples, from position 1000, cut into calls of 1, 4095, 4097 and 100 003 samples in turn: the bytes
    and the final state of a single call, which are the model's; cf32 (in place) and ci16-full; blocks of 4096 and of 65536"""
    rng = np.random.default_rng(77)
    n, first, done = 250_000, 1000, 0
    for fmt in (irdm.FMT_CF32, irdm.FMT_CI16_FULL):
        bps = bm.FORMATS[fmt][1]
        raw = random_bytes(fmt, n, rng)
        x = bm.convert(raw, fmt)
        for log2 in (12, 16):
            st0 = irdm.DcState()
            st0.mean_i, st0.mean_q, st0.sum_i, st0.sum_q = SEED[0], SEED[1], 12345678901, -98765432101
            want, want_state, _ = dm.run(x, log2, SEED, first, (st0.sum_i, st0.sum_q))
            outs = []
            for cuts in ((n,), (1, 4095, 4097, 100_003)):
                d_src, d_dst = irdm.device_buffer(raw), irdm.device_buffer(np.full(8 * n, FILL, np.uint8))
                try:
                    st = irdm.DcState()
                    st.mean_i, st.mean_q, st.sum_i, st.sum_q = st0.mean_i, st0.mean_q, st0.sum_i, st0.sum_q
                    at, j = 0, 0
                    while at < n:
                        m = min(cuts[j % len(cuts)], n - at)
                        out = d_src + at * 8 if fmt == irdm.FMT_CF32 else d_dst + at * 8
                        assert irdm.dc_block_device(fmt, out, d_src + at * bps, m, log2, first + at, st) == 0, (fmt, log2, at, m)
                        at, j = at + m, j + 1
                    got = np.empty(8 * n, np.uint8)
                    irdm.device_download(got, d_src if fmt == irdm.FMT_CF32 else d_dst)
                finally:
                    irdm.device_free(d_src)
                    irdm.device_free(d_dst)
                assert same_state(state_tuple(st), want_state), (fmt, log2, cuts, state_tuple(st), want_state)
                bad = np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))
                assert len(bad) == 0, (fmt, log2, cuts, int(bad[0]))
                outs.append(got)
            assert np.array_equal(outs[0], outs[1])
            done += 1
    return dict(streams=done)


# ---------------------------------------------------------------- through a context ----
FS = 2_000_000
N = 3_000_000
CHUNK = 262_144
# the other chunking: the issue names 100 003 samples, which a context cannot take (a chunk that is no multiple of feed_block
# = 32768 ends the stream); 98 304 = 3 x 32768 is the nearest it takes, and like 100 003 no multiple or divisor of the block
# of 65536: chunk edges fall inside blocks and block edges inside chunks.  (irdm_dc_block_device is cut at 100 003 above.)
CHUNK2 = 98_304
PIPE_LOG2 = 16
D = 0.03
OFFSETS_HZ = (1234.0, -3000.0, 6000.0, -9000.0, 12000.0, -15000.0, 18000.0, 41666.7 + 1234, -3 * 41666.7 + 1234, 7 * 41666.7 + 1234,
              1234.0, -500.0)
BALANCE = (0.999, 4.99)


def as_floats(iq):
    return np.ascontiguousarray(iq).view(np.float32).reshape(-1)


@functools.lru_cache(maxsize=None)
def streams(d=D):
    """S: 2 MS/s, 3 000 000 samples of siggen.make_stream(seed 3) with 12 bursts of amplitude 0.05 from sample 520 x 2048 on,
    140 000 apart, nine inside the centre channel and three off it; X = S + d (1 + 0.6j)"""
    rng = np.random.default_rng(7)
    bursts = [dict(start=520 * 2048 + k * 140000, freq_hz=f, payload=list(rng.integers(0, 4, size=150)), amp=0.05)
              for k, f in enumerate(OFFSETS_HZ)]
    iq, _ = siggen.make_stream(FS, N, bursts, seed=3)
    s = as_floats(iq).copy()
    x = s.copy()
    x[0::2] += np.float32(d)
    x[1::2] += np.float32(0.6 * d)
    for a in (s, x):
        a.setflags(write=False)
    return s, x


@functools.lru_cache(maxsize=None)
def corrected(log2=PIPE_LOG2, own_head=False):
    """dc_model(X) with a zero seed, or seeded with the mean of its own first block as the binary does"""
    s, x = streams()
    seed = dm.head_mean(x, min(1 << log2, len(x) // 2)) if own_head else (0.0, 0.0)
    y, fig = dm.dc_model(x, log2, seed)
    y.setflags(write=False)
    return y, fig


@functools.lru_cache(maxsize=None)
def oracle(which):
    import orc
    s, x = streams()
    z = {"s": s, "x": x, "y": corrected()[0], "yh": corrected(own_head=True)[0]}[which]
    return orc.run_stream(z.view(np.complex64), FS)


def frames_of(r):
    return [(d.timestamp, bytes(d.bits[:d.n_bits])) for d in r.demods if d.ok]


def oracle_facts():
    """what the feature is for, from the oracle alone: the clean stream's frames, how many of them X keeps, and how many the
    model-corrected stream seeded from its own head gives back"""
    rs, rx, ry = oracle("s"), oracle("x"), oracle("yh")
    clean = frames_of(rs)
    return dict(clean=len(rs.demods), clean_ok=len(clean), dc=len(rx.demods), dc_same=len(set(frames_of(rx)) & set(clean)),
                fixed=len(ry.demods), fixed_ok=len(frames_of(ry)),
                fixed_bits=sum(1 for a, b in zip(frames_of(ry), clean) if a[1] == b[1]) if len(ry.demods) == len(rs.demods) else -1,
                fixed_same=len(set(frames_of(ry)) & set(clean)))


def stats_tuple(st):
    return (int(st.n_samples), int(st.n_blocks), st.block_log2, (np.float32(st.seed_i), np.float32(st.seed_q)),
            (np.float32(st.first_i), np.float32(st.first_q)), (np.float32(st.last_i), np.float32(st.last_q)),
            (np.float32(st.min_i), np.float32(st.min_q)), (np.float32(st.max_i), np.float32(st.max_q)))


def fig_tuple(fig):
    f32 = lambda p: (np.float32(p[0]), np.float32(p[1]))
    return (fig["n_samples"], fig["n_blocks"], fig["block_log2"], f32(fig["seed"]), f32(fig["first"]), f32(fig["last"]),
            f32(fig["min"]), f32(fig["max"]))


def run(samples, depth, chunk=CHUNK, dc=None, swap=False, balance=False, after=None):
    """a stream (interleaved floats, or a wire format's integers with dc = that format) through a cf32 context in chunks of
    `chunk` samples; the records as objects (for tests/parity.py) and as bytes"""
    p = irdm.Pipeline(FS, fmt=irdm.FMT_CF32, max_chunk_samples=CHUNK, max_bursts_per_chunk=1024, pipeline_depth=depth)
    try:
        p.set_option("keep_frame_samples", 1)
        if swap:
            p.set_option("swap_iq", 1)
        if balance:
            p.iq_balance(irdm.FMT_CF32, *BALANCE)
        if dc is not None:
            p.dc_block(dc, PIPE_LOG2)
        x = samples.view(np.complex64) if samples.dtype == np.float32 else samples.reshape(-1, 2)
        for off in range(0, len(x), chunk):
            p.feed_host(np.ascontiguousarray(x[off:off + chunk]).reshape(-1))
        if depth:
            p.flush()
        bursts = p.poll_bursts()
        infos, frame_samples = p.poll_frames()
        demods = p.poll_demods()
        out = dict(bursts=bursts, infos=infos, samples=frame_samples, demods=demods, tagged=p.tagged, n_samples=p.sample_count,
                   bytes=(b"".join(bytes(b) for b in bursts), b"".join(bytes(f) for f in infos), b"".join(bytes(d) for d in demods),
                          b"".join(np.ascontiguousarray(s).tobytes() for s in frame_samples)))
        if dc is not None:
            out["stats"] = stats_tuple(p.dc_stats())
        if after:
            after(p)
        return out
    finally:
        p.close()


def same_records(on, off, where):
    for k, name in enumerate(("bursts", "frames", "demods", "frame samples")):
        assert on["bytes"][k] == off["bytes"][k], (name, where)
    assert on["tagged"] == off["tagged"] and on["n_samples"] == off["n_samples"], where


def pipeline_case(depth):
    """a context with irdm_dc_block (cf32 wire, blocks of 65536) fed X in chunks of 262 144 and again of 98 304 against a plain
    context fed dc_model(X): every record queue bit for bit, both chunkings alike, tests/parity.py's comparison with the oracle
    on dc_model(X); irdm_dc_stats equals the model's figures; irdm_reset clears the stream state and keeps the setting; the
    refusals"""
    import parity
    s, x = streams()
    y, fig = corrected()
    seen = {}

    def checks(p):
        L = irdm.lib()
        # the stream has begun: no change, not even to the same values
        assert L.irdm_dc_block(p.h, irdm.FMT_CF32, PIPE_LOG2, 0.0, 0.0) == -1 and L.irdm_dc_block(p.h, irdm.FMT_CF32, -1, 0.0, 0.0) == -1
        assert L.irdm_set_option(p.h, b"dc_block", 0) == -1 and L.irdm_set_option(p.h, b"dc_block_log2", 14) == -1
        d = irdm.device_buffer(np.zeros(2 * 32768, np.float32))
        try:
            assert L.irdm_feed_device(p.h, C.c_void_p(d), 32768, None) == -1
            assert L.irdm_feed_begin(p.h, C.c_void_p(d), 32768, None) == -1
        finally:
            irdm.device_free(d)
        p.reset()
        st = stats_tuple(p.dc_stats())
        assert st[:3] == (0, 0, PIPE_LOG2) and all(float(v) == 0.0 for pair in st[3:] for v in pair), st
        # the setting is still in effect: the first chunk of X gives the figures of the model on it
        p.feed_host(np.ascontiguousarray(x.view(np.complex64)[:CHUNK]))
        assert stats_tuple(p.dc_stats()) == fig_tuple(dm.dc_model(x[:2 * CHUNK], PIPE_LOG2)[1])
        # ... and a stream that has not begun may choose again, within the limits
        p.reset()
        for log2 in (11, 25, 0):
            assert L.irdm_dc_block(p.h, irdm.FMT_CF32, log2, 0.0, 0.0) == -1
        for seed in ((float("nan"), 0.0), (0.0, float("inf")), (64.5, 0.0), (0.0, -65.0)):
            assert L.irdm_dc_block(p.h, irdm.FMT_CF32, PIPE_LOG2, *seed) == -1
        assert L.irdm_dc_block(p.h, 5, PIPE_LOG2, 0.0, 0.0) == -1
        assert L.irdm_dc_block(p.h, irdm.FMT_CI8, 12, 0.01, -0.01) == 0
        st = stats_tuple(p.dc_stats())
        assert st[:4] == (0, 0, 12, (np.float32(0.01), np.float32(-0.01))), st
        assert L.irdm_dc_block(p.h, irdm.FMT_CF32, -1, 0.0, 0.0) == 0 and L.irdm_dc_stats(p.h, C.byref(irdm.DcStats())) == -1
        assert L.irdm_set_option(p.h, b"dc_block_log2", 25) == -1 and L.irdm_set_option(p.h, b"dc_block_log2", 13) == 0
        assert L.irdm_set_option(p.h, b"dc_block", 1) == 0 and stats_tuple(p.dc_stats())[:3] == (0, 0, 13)
        p.set_option("group_member", 1)
        assert L.irdm_dc_block(p.h, irdm.FMT_CF32, PIPE_LOG2, 0.0, 0.0) == -1
        p.set_option("group_member", 0)
        seen["checks"] = True

    on = run(x, depth, dc=irdm.FMT_CF32, after=checks)
    on2 = run(x, depth, chunk=CHUNK2, dc=irdm.FMT_CF32)
    off = run(y, depth)
    assert seen == dict(checks=True)
    same_records(on, off, ("cf32", depth))
    same_records(on2, off, ("cf32", depth, CHUNK2))
    print("depth %d stats %r" % (depth, on["stats"]))
    assert on["stats"] == fig_tuple(fig) and on2["stats"] == fig_tuple(fig), (on["stats"], on2["stats"], fig_tuple(fig))
    assert irdm.lib().irdm_dc_stats is not None
    p = irdm.Pipeline(FS, fmt=irdm.FMT_CI8, max_chunk_samples=CHUNK, max_bursts_per_chunk=64, pipeline_depth=depth)
    try:
        assert irdm.lib().irdm_dc_block(p.h, irdm.FMT_CI8, PIPE_LOG2, 0.0, 0.0) == -1
        assert irdm.lib().irdm_dc_stats(p.h, C.byref(irdm.DcStats())) == -1
    finally:
        p.close()
    res = parity.compare(on, oracle("y"))
    res["demods"] = len(on["demods"])
    return res


def wire_case(depth):
    """the same with the ci16-full rendering of X as wire format, in chunks of 98 304: a context with irdm_dc_block fed the
    integers against a plain cf32 context fed the model's correction of their conversion, bit for bit, and the figures"""
    s, x = streams()
    raw = np.clip(np.round(x * np.float32(32768.0)), -32768, 32767).astype(np.int16)
    yc, fig = dm.dc_model(bm.convert(raw, irdm.FMT_CI16_FULL), PIPE_LOG2)
    on = run(raw, depth, chunk=CHUNK2, dc=irdm.FMT_CI16_FULL)
    off = run(yc, depth)
    same_records(on, off, ("ci16-full", depth))
    assert on["stats"] == fig_tuple(fig), (on["stats"], fig_tuple(fig))
    return dict(demods=len(on["demods"]))


def composition_case(depth):
    """swap_iq, irdm_dc_block and irdm_iq_balance together: the records of balance(dc_model(swap(X)))"""
    s, x = streams()
    sw = np.ascontiguousarray(x.reshape(-1, 2)[:, ::-1]).reshape(-1)
    z = bm.balance(dm.dc_model(sw, PIPE_LOG2)[0], *bm.coeffs(*BALANCE))
    on = run(x, depth, dc=irdm.FMT_CF32, swap=True, balance=True)
    off = run(z, depth)
    same_records(on, off, ("composition", depth))
    return dict(demods=len(on["demods"]), bursts=len(on["bursts"]))
