"""TEST INFRASTRUCTURE: the checks of the I/Q imbalance feature (csrc/iq_moments.hpp, csrc/iq_balance.hpp) that the GPU test
(tests/test_gpu_balance.py) and the CPU-emulation test (tests/balance_emul_run.py) share: the two kernels against the numpy
model of tests/balance_model.py, and a context with irdm_iq_balance / option iq_moments against a plain context fed the
model-corrected stream and against the oracle."""
import ctypes as C
import functools

import numpy as np

import balance_model as bm
import irdm
import siggen

GUARD = 64
FILL = 0xA5
SIZES = (0, 1, 2, 3, 4, 5, 255, 256, 257, 4095, 4096, 4097, 65536 + 3)
FMTS = tuple(bm.FORMATS)
# gain in dB, phase in degrees: the identity, the figures of the binary's test, and a pair of the other signs
PAIRS = ((0.0, 0.0), (0.999, 4.99), (-0.5, -3.0))
# cf32 bit patterns strewn in: quiet and signalling NaN, +-Inf, -0.0, subnormals, and the smallest normals (times alpha or
# beta < 1 they give a subnormal product)
SPECIALS = (0x7fc00000, 0x7fa00000, 0xffc00001, 0x7f800000, 0xff800000, 0x80000000, 0x00000001, 0x80000001, 0x007fffff,
            0x00800000, 0x80800000, 0x00c00000)


def random_bytes(fmt, n, rng):
    """n samples of format fmt as bytes: the whole code range for the integer formats, +-0.9 for cf32"""
    t = bm.FORMATS[fmt][0]
    if fmt == irdm.FMT_CF32:
        return rng.uniform(-0.9, 0.9, 2 * n).astype(np.float32).view(np.uint8)
    if fmt == irdm.FMT_SC16Q11:
        return rng.integers(-2048, 2048, 2 * n).astype(t).view(np.uint8)
    if fmt == irdm.FMT_CI32_24:
        return rng.integers(-(1 << 23), 1 << 23, 2 * n).astype(t).view(np.uint8)
    info = np.iinfo(t)
    return rng.integers(info.min, info.max + 1, 2 * n).astype(t).view(np.uint8)


def strew_specials(words, rng, rate=0.05):
    """words: uint32 view of cf32 samples.  SPECIALS in I, in Q and in both of about `rate` of the samples"""
    n = len(words) // 2
    at = np.flatnonzero(rng.random(n) < rate)
    comp = 1 + rng.integers(0, 3, len(at))
    sp = np.asarray(SPECIALS, np.uint32)
    vi, vq = sp[rng.integers(0, len(sp), len(at))], sp[rng.integers(0, len(sp), len(at))]
    words[2 * at[(comp & 1) != 0]] = vi[(comp & 1) != 0]
    words[2 * at[(comp & 2) != 0] + 1] = vq[(comp & 2) != 0]


def build_regions(extra_pieces, rng, src_behinds=(0, 1, 2, 3), dst_behinds=(0, 1)):
    """every format x size x alignment: [(fmt, n, src byte offset, dst byte offset)], the source image (bytes) and the size
    of the destination image.  src lies 0 .. 3 samples behind a 16-byte boundary, dst 0 or 1 cf32 sample behind one; GUARD
    bytes on either side of both."""
    regions, s_size, d_size = [], 0, 0
    plan = [(fmt, n, sb, db) for fmt in FMTS for n in SIZES for sb in src_behinds for db in dst_behinds]
    for fmt in FMTS:
        for pieces in extra_pieces:
            plan.append((fmt, pieces * (16 // bm.FORMATS[fmt][1]) + 3, 1, 1))
    for fmt, n, sb, db in plan:
        bps = bm.FORMATS[fmt][1]
        s0, d0 = s_size + GUARD + sb * bps, d_size + GUARD + db * 8
        regions.append((fmt, n, s0, d0))
        s_size, d_size = (s0 + n * bps + GUARD + 63) // 64 * 64, (d0 + n * 8 + GUARD + 63) // 64 * 64
    src = np.full(s_size, FILL, np.uint8)
    for fmt, n, s0, d0 in regions:
        bps = bm.FORMATS[fmt][1]
        src[s0:s0 + n * bps] = random_bytes(fmt, n, rng)
        if fmt == irdm.FMT_CF32 and n:
            w = src[s0:s0 + n * 8].view(np.uint32)
            strew_specials(w, rng)
    return regions, src, d_size


def same_bits(got, want):
    """float32 arrays compared as bits; where the model has a NaN any NaN will do.  Returns the indices that differ."""
    g, w = got.view(np.uint32), want.view(np.uint32)
    nan_w = np.isnan(want.view(np.float32))
    return np.flatnonzero(np.where(nan_w, ~np.isnan(got.view(np.float32)), g != w))


def balance_kernel_cases(extra_pieces=()):
    """irdm_iq_balance_device against balance_model.balance(convert(bytes)), bit for bit: all eight formats, n in 0 .. 5,
    255 .. 257, 4095 .. 4097 and 65536 + 3, src 0 .. 3 samples behind a 16-byte boundary, dst 0 and 1 sample behind one, the
    three coefficient pairs taking turns (every format meets every pair at every size); guard bytes of dst and all of src
    untouched; cf32 with NaN, Inf, -0.0 and subnormals strewn in; then the cf32 regions once more in place.  With the
    identity every converted sample comes back with its value, and with its bits unless its Q is a zero (alpha i + -0.0 is
    +0.0 for half the signs of i, in float32 arithmetic as in the model).  Returns the number of cases."""
    rng = np.random.default_rng(1234)
    regions, src, d_size = build_regions(extra_pieces, rng)
    want = np.full(d_size, FILL, np.uint8)
    pairs = [bm.coeffs(*p) for p in PAIRS]
    assert pairs[0] == (np.float32(-0.0), np.float32(1.0)) and all(irdm.iq_balance_coeffs(*p) == c for p, c in zip(PAIRS, pairs)), pairs
    conv = []
    for k, (fmt, n, s0, d0) in enumerate(regions):
        x = bm.convert(src[s0:s0 + n * bm.FORMATS[fmt][1]], fmt)
        conv.append(x)
        want[d0:d0 + 8 * n] = bm.balance(x, *pairs[k % 3]).view(np.uint8)
    seen = dict(nan=0, inf=0, negzero=0, subnormal=0, identity=0)
    d_src, d_dst = irdm.device_buffer(src), irdm.device_buffer(np.full(d_size, FILL, np.uint8))
    try:
        assert d_src % 16 == 0 and d_dst % 16 == 0
        for k, (fmt, n, s0, d0) in enumerate(regions):
            a, b = pairs[k % 3]
            assert irdm.iq_balance_device(d_dst + d0, d_src + s0, n, fmt, a, b) == 0, (fmt, n, s0, d0)
        got, src_after = np.empty_like(want), np.empty_like(src)
        irdm.device_download(got, d_dst)
        irdm.device_download(src_after, d_src)
        assert np.array_equal(src_after, src)
        for k, (fmt, n, s0, d0) in enumerate(regions):
            g, w = got[d0:d0 + 8 * n].view(np.float32), want[d0:d0 + 8 * n].view(np.float32)
            bad = same_bits(g, w)
            assert len(bad) == 0, (fmt, n, s0 % 16, d0 % 16, int(bad[0]), hex(g.view(np.uint32)[bad[0]]), hex(w.view(np.uint32)[bad[0]]))
            assert (got[d0 - GUARD:d0] == FILL).all() and (got[d0 + 8 * n:d0 + 8 * n + GUARD] == FILL).all(), (fmt, n, s0, d0)
            if k % 3 == 0 and n:
                x = conv[k]
                fin = np.isfinite(x[0::2]) & np.isfinite(x[1::2])
                assert np.array_equal(g[0::2].view(np.uint32), x[0::2].view(np.uint32))
                assert np.array_equal(g[1::2][fin], x[1::2][fin])
                keep = fin & (x[1::2] != 0)
                assert np.array_equal(g[1::2].view(np.uint32)[keep], x[1::2].view(np.uint32)[keep])
                seen["identity"] += 1
            with np.errstate(all="ignore"):
                seen["nan"] += int(np.isnan(w).sum())
                seen["inf"] += int(np.isinf(w).sum())
                seen["negzero"] += int((w.view(np.uint32) == 0x80000000).sum())
                seen["subnormal"] += int(((np.abs(w[1::2]) < np.float32(2.0**-126)) & (w[1::2] != 0)).sum())
        # what no region covers is still the fill
        mask = np.ones(d_size, bool)
        for fmt, n, s0, d0 in regions:
            mask[d0:d0 + 8 * n] = False
        assert (got[mask] == FILL).all()
        # cf32 in place: the source buffer's own regions
        for k, (fmt, n, s0, d0) in enumerate(regions):
            if fmt == irdm.FMT_CF32:
                a, b = pairs[k % 3]
                assert irdm.iq_balance_device(d_src + s0, d_src + s0, n, fmt, a, b) == 0, (n, s0)
        irdm.device_download(src_after, d_src)
        mask = np.ones(len(src), bool)
        n_in_place = 0
        for k, (fmt, n, s0, d0) in enumerate(regions):
            if fmt == irdm.FMT_CF32:
                w = bm.balance(conv[k], *pairs[k % 3])
                bad = same_bits(src_after[s0:s0 + 8 * n].view(np.float32), w)
                assert len(bad) == 0, ("in place", n, s0 % 16, int(bad[0]))
                mask[s0:s0 + 8 * n] = False
                n_in_place += 1
        assert np.array_equal(src_after[mask], src[mask])
    finally:
        irdm.device_free(d_src)
        irdm.device_free(d_dst)
    assert min(seen.values()) > 20, seen
    return dict(cases=len(regions), in_place=n_in_place)


def balance_refusal_cases():
    """-1 for an unknown format, a source that is not aligned to a sample, a destination that is not aligned to 8 bytes,
    coefficients outside what the limits allow (a NaN among them), and buffers that overlap other than cf32 in place;
    irdm_iq_balance_coeffs refuses gains beyond +-6 dB and phases beyond +-30 degrees; nothing is written"""
    host = np.full(8192, FILL, np.uint8)
    d = irdm.device_buffer(host)
    try:
        src, dst = d + GUARD, d + 4096
        for bad_fmt in (-1, 5, 7, 10):
            assert irdm.iq_balance_device(dst, src, 4, bad_fmt, 0.0, 1.0) == -1
        for fmt, (t, bps) in bm.FORMATS.items():
            assert irdm.iq_balance_device(dst, src, 4, fmt, 0.0, 1.0) == 0          # (the control: this one is taken)
            assert irdm.iq_balance_device(dst, src + bps // 2, 4, fmt, 0.0, 1.0) == -1
            assert irdm.iq_balance_device(dst + 4, src, 4, fmt, 0.0, 1.0) == -1
            if bps != 8:
                assert irdm.iq_balance_device(src, src, 4, fmt, 0.0, 1.0) == -1        # (in place: the 8-byte formats alone)
            assert irdm.iq_balance_device(src - 8, src, 4, fmt, 0.0, 1.0) == -1        # (overlapping)
        for a, b in ((1.0, 1.0), (-0.6, 1.0), (0.0, 3.0), (0.0, 0.4), (0.0, -1.0), (float("nan"), 1.0), (0.0, float("nan")),
                     (float("inf"), 1.0)):
            assert irdm.iq_balance_device(dst, src, 4, irdm.FMT_CF32, a, b) == -1, (a, b)
            assert irdm.iq_balance_device(dst, src, 0, irdm.FMT_CF32, a, b) == -1, (a, b)
        assert irdm.iq_balance_device(dst, src, 0, irdm.FMT_CF32, 0.0, 1.0) == 0
        for g, p in ((6.01, 0.0), (-6.01, 0.0), (0.0, 30.01), (0.0, -30.01), (float("nan"), 0.0), (0.0, float("nan"))):
            assert irdm.iq_balance_coeffs(g, p) is None and bm.coeffs(g, p) is None
        for g, p in ((6.0, 30.0), (-6.0, -30.0), (6.0, -30.0), (-6.0, 30.0)):
            a, b = irdm.iq_balance_coeffs(g, p)
            assert (a, b) == bm.coeffs(g, p) and irdm.iq_balance_device(dst, src, 4, irdm.FMT_CF32, a, b) == 0, (g, p)
        got = np.empty_like(host)
        irdm.device_download(got, d)
        assert (got[:4096] == FILL).all()
    finally:
        irdm.device_free(d)
    return len(bm.FORMATS)


def check_moments(st, m, where, derived=None):
    """an irdm.IqMoments against the model's dict: counts exact, each sum within N 2^-52 sum|term| (the terms are exact
    doubles: this bounds any order of addition), and with `derived` the figures within 1e-6"""
    assert (int(st.n_samples), int(st.n_used), st.valid) == (m["n_samples"], m["n_used"], m["valid"]), \
        (where, int(st.n_samples), int(st.n_used), st.valid, m["n_samples"], m["n_used"], m["valid"])
    got = (st.sum_i, st.sum_q, st.sum_ii, st.sum_qq, st.sum_iq)
    for g, w, a in zip(got, m["sums"], m["abs"]):
        assert abs(g - w) <= m["n_used"] * 2.0**-52 * a, (where, g, w, a)
    if not m["valid"]:
        assert (st.gain_db, st.phase_deg, st.image_db) == (0.0, 0.0, 0.0), where
    elif derived if derived is not None else m["n_used"] >= 4096:
        assert abs(st.gain_db - m["gain_db"]) <= 1e-6 and abs(st.phase_deg - m["phase_deg"]) <= 1e-6, \
            (where, st.gain_db, m["gain_db"], st.phase_deg, m["phase_deg"])
        assert -120.0 <= st.image_db <= 0.0
    if m["valid"]:
        # (the record's own figures follow from the record's own sums)
        v, g, p, i = bm.derive(int(st.n_used), got)
        assert v == 1 and abs(st.gain_db - g) <= 1e-9 and abs(st.phase_deg - p) <= 1e-9 and abs(st.image_db - i) <= 1e-6, where


def moments_kernel_cases(extra_pieces=()):
    """irdm_iq_moments_device against the float64 model on the regions of the balance cases (all eight formats, the same
    sizes and source alignments; the cf32 ones hold NaN and Inf, which are left out and counted): counts exact, sums within
    the bound, gain and phase within 1e-6 from 4096 samples on; two launches of one buffer give identical bytes.  Then cf32
    buffers with single non-finite samples at the head, the tail, the edge of a wavefront and of a workgroup; valid = 0 for
    n = 0, n = 1, an all-zero and an all-NaN buffer; the refusals."""
    rng = np.random.default_rng(4321)
    regions, src, _ = build_regions(extra_pieces, rng, dst_behinds=(0,))
    d = irdm.device_buffer(src)
    n_valid = n_left_out = 0
    try:
        for fmt, n, s0, d0 in regions:
            bps = bm.FORMATS[fmt][1]
            m = bm.moments(bm.convert(src[s0:s0 + n * bps], fmt))
            rc, st = irdm.iq_moments_device(d + s0, n, fmt)
            assert rc == 0, (fmt, n, s0)
            check_moments(st, m, (fmt, n, s0 % 16))
            rc, again = irdm.iq_moments_device(d + s0, n, fmt)
            assert rc == 0 and bytes(again) == bytes(st), (fmt, n, s0)
            n_valid += m["valid"]
            n_left_out += m["n_samples"] - m["n_used"]
            if n >= 255:
                assert m["valid"] == 1, (fmt, n)
        for bad_fmt in (-1, 5, 7, 10):
            assert irdm.iq_moments_device(d + GUARD, 4, bad_fmt)[0] == -1
        for fmt, (t, bps) in bm.FORMATS.items():
            assert irdm.iq_moments_device(d + GUARD + bps // 2, 4, fmt)[0] == -1
    finally:
        irdm.device_free(d)
    assert n_left_out > 100 and n_valid > len(regions) // 2, (n_left_out, n_valid)
    # single non-finite samples: the head, the tail, 63 / 64 / 65 pieces in, 255 / 256 pieces in (a piece: two cf32 samples)
    n = 2 * 300 + 3
    for behind in (0, 1):
        base = rng.uniform(-0.9, 0.9, 2 * (n + 9)).astype(np.float32)   # (a multiple of 16 bytes)
        singles = sorted(set([0, 1, n - 2, n - 1] + [behind + 2 * k + j for k in (63, 64, 65, 255, 256) for j in (0, 1)]))
        cases = [((s,), c) for s in singles for c in (1, 2, 3)] + [(tuple(singles), 3), (tuple(range(n)), 1)]
        host = np.concatenate([base] * len(cases)).view(np.uint32)
        for k, (bad, comp) in enumerate(cases):
            w = host[k * len(base):(k + 1) * len(base)]
            for j, s in enumerate(bad):
                v = (0x7fc00000, 0x7f800000, 0xff800000, 0x7fa00000)[(j + k) % 4]
                if comp & 1:
                    w[2 * (4 - behind + s)] = v
                if comp & 2:
                    w[2 * (4 - behind + s) + 1] = v
        d = irdm.device_buffer(host)
        try:
            for k, (bad, comp) in enumerate(cases):
                off = 4 * (k * len(base) + 2 * (4 - behind))
                assert (d + off) % 16 == 8 * behind
                m = bm.moments(host[off // 4:off // 4 + 2 * n].view(np.float32))
                assert m["n_used"] == n - len(bad)
                rc, st = irdm.iq_moments_device(d + off, n, irdm.FMT_CF32)
                assert rc == 0
                check_moments(st, m, ("single", behind, bad[:3], comp))
                assert st.valid == (0 if len(bad) == n else 1)
        finally:
            irdm.device_free(d)
    # nothing to judge
    rc, st = irdm.iq_moments_device(0, 0, irdm.FMT_CF32)
    assert rc == 0 and (int(st.n_samples), int(st.n_used), st.valid) == (0, 0, 0)
    for fmt, (t, bps) in bm.FORMATS.items():
        zero = np.zeros(4096 * bps, np.uint8)
        if fmt == irdm.FMT_CU8:
            zero[:] = 128                                   # (cu8 has no zero: a constant)
        d = irdm.device_buffer(zero)
        try:
            for n in (1, 4096):
                rc, st = irdm.iq_moments_device(d, n, fmt)
                assert rc == 0 and (int(st.n_samples), int(st.n_used), st.valid, st.gain_db, st.image_db) == (n, n, 0, 0.0, 0.0), (fmt, n)
        finally:
            irdm.device_free(d)
    return dict(cases=len(regions), left_out=n_left_out)


# ---------------------------------------------------------------- through a context ----
FS = 2_000_000
CHUNK = 262_144
PLANTED = (1.0, 5.0)                # gain in dB, phase in degrees
REMEDY = (0.999, 4.99)              # what the binary's line prints for it


def as_floats(iq):
    return np.ascontiguousarray(iq).view(np.float32).reshape(-1)


@functools.lru_cache(maxsize=None)
def streams():
    """S = siggen.standard_scene(2 MHz, 2 M samples, 12 bursts, seed 3, amp 0.2) as interleaved floats; Y = S with 1 dB and 5
    degrees of imbalance and a DC offset planted; Z = the model's correction of Y with the coefficients of 0.999 dB, 4.99
    degrees"""
    iq, truth = siggen.standard_scene(FS, FS, 12, 3, amp=0.2)
    s = as_floats(iq).copy()
    y = bm.impair(s, *PLANTED)
    z = bm.balance(y, *bm.coeffs(*REMEDY))
    for a in (s, y, z):
        a.setflags(write=False)
    return s, y, z


@functools.lru_cache(maxsize=None)
def wire_streams(fmt):
    """Y rendered as ci8 (scale 256) or ci16: the wire bytes (as the format's integers), and the model's correction of their
    conversion"""
    s, y, z = streams()
    raw = siggen.to_ci8(y.view(np.complex64), scale=256) if fmt == irdm.FMT_CI8 else siggen.to_ci16(y.view(np.complex64))
    zc = bm.balance(bm.convert(raw, fmt), *bm.coeffs(*REMEDY))
    raw.setflags(write=False)
    zc.setflags(write=False)
    return raw, zc


@functools.lru_cache(maxsize=None)
def oracle(which):
    import orc
    s, y, z = streams()
    return orc.run_stream({"s": s, "y": y, "z": z}[which].view(np.complex64), FS)


def oracle_facts():
    """the three facts the feature rests on, from the oracle alone: S gives 12 frames and no image; Y gives 24 frames with
    ok, at least 8 of them images by the rule; Z gives 12 frames, no image, and S's payload bits"""
    rs, ry, rz = oracle("s"), oracle("y"), oracle("z")
    c = 1622000000.0
    out = {}
    for name, r in (("s", rs), ("y", ry), ("z", rz)):
        images, n_ok = bm.count_images(bm.frames_of(r.demods), c)
        out[name] = dict(frames=len(r.demods), ok=n_ok, images=images)
    assert out["s"] == dict(frames=12, ok=12, images=0), out
    assert out["y"]["ok"] == 24 and out["y"]["images"] >= 8, out
    assert out["z"] == dict(frames=12, ok=12, images=0), out
    assert [bytes(d.bits[:d.n_bits]) for d in rz.demods] == [bytes(d.bits[:d.n_bits]) for d in rs.demods]
    return out


def run(samples, depth, fmt=irdm.FMT_CF32, balance=None, moments=False, after=None):
    """a stream (interleaved floats, or the wire format's integers with `balance` = that format) through a cf32 context in
    chunks of 262 144 samples; the records as objects (for tests/parity.py) and as bytes"""
    p = irdm.Pipeline(FS, fmt=irdm.FMT_CF32, max_chunk_samples=CHUNK, max_bursts_per_chunk=1024, pipeline_depth=depth)
    try:
        p.set_option("keep_frame_samples", 1)
        if moments:
            p.set_option("iq_moments", 1)
        if balance is not None:
            p.iq_balance(balance, *REMEDY)
        per = 2 * CHUNK if samples.dtype != np.complex64 else CHUNK
        for off in range(0, len(samples), per):
            p.feed_host(np.ascontiguousarray(samples[off:off + per]))
        if depth:
            p.flush()
        bursts = p.poll_bursts()
        infos, frame_samples = p.poll_frames()
        demods = p.poll_demods()
        out = dict(bursts=bursts, infos=infos, samples=frame_samples, demods=demods, tagged=p.tagged, n_samples=p.sample_count,
                   bytes=(b"".join(bytes(b) for b in bursts), b"".join(bytes(f) for f in infos), b"".join(bytes(d) for d in demods),
                          b"".join(np.ascontiguousarray(s).tobytes() for s in frame_samples)))
        if moments:
            out["moments"] = p.iq_moments()
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
    """a context with irdm_iq_balance (cf32 wire) fed Y against a plain context fed Z: every record queue bit for bit, and
    tests/parity.py's comparison with the oracle on Z; option iq_moments on the corrected stream reads below -60 dB and equals
    the model on Z; irdm_reset clears the moments and keeps the balance; a change of the balance after the first feed, a
    device feed with it on and a context of another format return -1"""
    import parity
    s, y, z = streams()
    seen = {}

    def checks(p):
        L = irdm.lib()
        assert L.irdm_iq_balance(p.h, irdm.FMT_CF32, 0.5, 1.0) == -1 and L.irdm_iq_balance(p.h, irdm.FMT_CF32, *REMEDY) == -1
        d = irdm.device_buffer(np.zeros(2 * 32768, np.float32))
        try:
            assert L.irdm_feed_device(p.h, C.c_void_p(d), 32768, None) == -1
            assert L.irdm_feed_begin(p.h, C.c_void_p(d), 32768, None) == -1
        finally:
            irdm.device_free(d)
        p.reset()
        st = p.iq_moments()
        assert (int(st.n_samples), int(st.n_used), st.valid, st.sum_ii) == (0, 0, 0, 0.0)
        # the balance is still in effect: the first chunk of Y gives the moments of the first chunk of Z
        p.feed_host(np.ascontiguousarray(y.view(np.complex64)[:CHUNK]))
        check_moments(p.iq_moments(), bm.moments(z[:2 * CHUNK]), "after reset")
        # ... and a stream that has not begun may choose again, within the limits
        p.reset()
        assert L.irdm_iq_balance(p.h, irdm.FMT_CF32, 6.5, 0.0) == -1 and L.irdm_iq_balance(p.h, irdm.FMT_CF32, 0.0, 31.0) == -1
        assert L.irdm_iq_balance(p.h, 5, 0.0, 0.0) == -1
        assert L.irdm_iq_balance(p.h, irdm.FMT_CI8, 0.5, 1.0) == 0
        seen["checks"] = True

    on = run(y.view(np.complex64), depth, balance=irdm.FMT_CF32, moments=True, after=checks)
    off = run(z.view(np.complex64), depth)
    assert seen == dict(checks=True)
    same_records(on, off, ("cf32", depth))
    st = on["moments"]
    print("depth %d corrected stream: gain %+.6f dB phase %+.5f deg image %.1f dB" % (depth, st.gain_db, st.phase_deg, st.image_db))
    check_moments(st, bm.moments(z), "corrected", derived=False)
    assert st.valid == 1 and st.image_db < -60.0, st.image_db
    assert len(on["demods"]) == 12
    return parity.compare(on, oracle("z"))


def wire_case(depth, fmt):
    """the same with a ci8 / ci16 wire format: a context with irdm_iq_balance fed the integer rendering of Y against a plain
    cf32 context fed the model's correction of its conversion, bit for bit"""
    raw, zc = wire_streams(fmt)
    on = run(raw, depth, balance=fmt)
    off = run(zc.view(np.complex64), depth)
    same_records(on, off, (fmt, depth))
    assert len(on["demods"]) >= 10, len(on["demods"])
    return dict(demods=len(on["demods"]))


def moments_case(depth):
    """option iq_moments on Y in a plain context: the model's figures, and within 0.01 dB and 0.05 degrees of the planted
    1 dB, 5 degrees (the model itself is 0.0009 dB and 0.008 degrees off); without the option irdm_iq_moments returns -1, as
    does irdm_iq_balance on a context that is not cf32"""
    s, y, z = streams()
    m = bm.moments(y)
    assert abs(m["gain_db"] - PLANTED[0]) < 0.002 and abs(m["phase_deg"] - PLANTED[1]) < 0.02, m
    res = run(y.view(np.complex64), depth, moments=True)
    st = res["moments"]
    print("depth %d stream as recorded: gain %+.6f dB phase %+.5f deg image %.2f dB (model %+.6f %+.5f %.2f)" % (
        depth, st.gain_db, st.phase_deg, st.image_db, m["gain_db"], m["phase_deg"], m["image_db"]))
    check_moments(st, m, "as recorded", derived=True)
    assert abs(st.image_db - m["image_db"]) <= 1e-5
    assert abs(st.gain_db - PLANTED[0]) <= 0.01 and abs(st.phase_deg - PLANTED[1]) <= 0.05
    assert "%.3f,%.2f" % (st.gain_db, st.phase_deg) == "%.3f,%.2f" % REMEDY
    assert len(res["demods"]) == 24
    p = irdm.Pipeline(FS, fmt=irdm.FMT_CI8, max_chunk_samples=CHUNK, max_bursts_per_chunk=64, pipeline_depth=depth)
    try:
        assert irdm.lib().irdm_iq_moments(p.h, C.byref(irdm.IqMoments())) == -1
        assert irdm.lib().irdm_iq_balance(p.h, irdm.FMT_CI8, *REMEDY) == -1
        p.set_option("group_member", 1)
        assert irdm.lib().irdm_set_option(p.h, b"iq_moments", 1) == -1
        p.set_option("group_member", 0)
        p.set_option("iq_moments", 1)
        st = p.iq_moments()
        assert (int(st.n_samples), st.valid) == (0, 0)
    finally:
        p.close()
    p = irdm.Pipeline(FS, fmt=irdm.FMT_CF32, max_chunk_samples=CHUNK, max_bursts_per_chunk=64, pipeline_depth=depth)
    try:
        p.set_option("group_member", 1)
        assert irdm.lib().irdm_iq_balance(p.h, irdm.FMT_CF32, *REMEDY) == -1
    finally:
        p.close()
    return dict(demods=len(res["demods"]), gain_db=res["moments"].gain_db)
