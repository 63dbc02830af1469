"""TEST INFRASTRUCTURE: the checks of exchanged I and Q (option swap_iq / irdm_swap_iq_device, csrc/iq_swap.hpp; option
iq_sense, iq_sense_kernel of csrc/bitlayer.hip) that the GPU test (tests/test_gpu_iq.py) and the CPU-emulation test
(tests/iq_emul_run.py) share: the exchange kernel against numpy, irdm_iq_sense_batch against tests/iq_sense_model.py, and
the pipeline on a scene of IRA, IBC and IDA frames fed as it is and with its components exchanged."""
import ctypes as C
import functools

import numpy as np

import bitlayer as bl
import bitlayer_checks as bc
import iq_sense_model as im
import irdm
import siggen

FORMATS = {irdm.FMT_CI8: 2, irdm.FMT_CU8: 2, irdm.FMT_CI16: 4, irdm.FMT_CI16_FULL: 4, irdm.FMT_SC16Q11: 4, irdm.FMT_CF32: 8,
           irdm.FMT_CI32: 8, irdm.FMT_CI32_24: 8}                        # format -> bytes per sample
SWAP_N = (0, 1, 2, 7, 8, 9, 15, 16, 17, 4095, 4097)
GUARD = 64


# ---------------------------------------------------------------- the exchange kernel ----
def swap_cases(extra_n=(), extra_pieces=()):
    """irdm_swap_iq_device on every format, length and alignment: one device buffer per format holds every case's region
    (guard bytes in front and behind, the samples 0..3 samples behind a 16-byte boundary), uploaded once; exact against
    numpy, the guards untouched, the identity when applied twice; and the refusals.  extra_pieces: lengths given in 16-byte
    pieces (+ 3 samples), one sample behind a boundary -- for the sizes at which a lane takes a second piece.  Returns the
    number of cases."""
    rng = np.random.default_rng(77)
    cases = 0
    for fmt, bps in FORMATS.items():
        regions, size = [], 0
        for n in SWAP_N + tuple(extra_n):
            for behind in range(4):
                start = size + GUARD + behind * bps                      # (size is a multiple of 64: so is the region's origin)
                regions.append((start, n))
                size = (start + n * bps + GUARD + 63) // 64 * 64
        for pieces in extra_pieces:
            n = pieces * (16 // bps) + 3
            regions.append((size + GUARD + bps, n))
            size = (size + GUARD + bps + n * bps + GUARD + 63) // 64 * 64
        host = rng.integers(0, 256, size, dtype=np.uint8)
        if bps == 8:
            # (cf32: a NaN and an Inf among the samples stay what they are)
            host[regions[3][0]:regions[3][0] + 8] = np.array([float("nan"), float("inf")], np.float32).view(np.uint8)
        want = host.copy()
        for start, n in regions:
            want[start:start + n * bps] = im.swap_bytes(host[start:start + n * bps], bps // 2)
        d = irdm.device_buffer(host)
        try:
            assert d % 16 == 0
            for rounds, expect in ((1, want), (2, host)):
                for start, n in regions:
                    assert (d + start) % 16 == (start % 16) and irdm.swap_iq_device(d + start, n, fmt) == 0, (fmt, start, n)
                got = np.empty_like(host)
                irdm.device_download(got, d)
                bad = np.flatnonzero(got != expect)
                assert len(bad) == 0, (fmt, rounds, len(bad), int(bad[0]), [r for r in regions if r[0] <= bad[0]][-1])
            cases += len(regions)
            # a pointer that is not aligned to a sample, and formats that do not exist
            assert irdm.swap_iq_device(d + GUARD + bps // 2, 4, fmt) == -1
            if bps > 2:
                assert irdm.swap_iq_device(d + GUARD + 1, 4, fmt) == -1
            for bad_fmt in (-1, 5, 7, 10):
                assert irdm.swap_iq_device(d + GUARD, 4, bad_fmt) == -1
            assert irdm.swap_iq_device(d + GUARD, 0, fmt) == 0
            got = np.empty_like(host)
            irdm.device_download(got, d)
            assert np.array_equal(got, host), fmt
        finally:
            irdm.device_free(d)
    return cases


# ---------------------------------------------------------------- the votes ----
def to_demod(bits, llr, direction, k):
    d = irdm.Demod()
    d.id = 10 * k
    d.n_bits = len(bits)
    d.n_symbols = len(bits) // 2
    d.ok = 1
    d.direction = direction
    for i, b in enumerate(bits):
        d.bits[i] = int(b)
    if llr is not None:
        for i, v in enumerate(llr):
            d.llr[i] = float(v)
    return d


@functools.lru_cache(maxsize=None)
def vote_corpus():
    """[(bits, llr or None, direction, exchanged?)]: frame_corpus and ida_corpus of seeds 0 and 1 (the cases without LLRs and
    the cut frames among them), every case as it is and with dibits and LLRs exchanged"""
    out = []
    for seed in (0, 1):
        for b, l in bc.frame_corpus(seed):
            out.append((b, l, 1))
        for b, l, d in bc.ida_corpus(seed):
            out.append((b, l, d))
    both = []
    for b, l, d in out:
        both.append((tuple(b), None if l is None else tuple(float(v) for v in l), d, False))
        xb, xl = im.exchange(b, l)
        # (an odd frame keeps its last bit: the kernel looks at whole dibits only)
        xb = list(xb) + list(b[len(xb):])
        xl = None if l is None else list(xl) + list(l[len(xl):])
        both.append((tuple(int(v) for v in xb), None if xl is None else tuple(float(v) for v in xl), d, True))
    return tuple(both)


@functools.lru_cache(maxsize=None)
def model_votes():
    """the model's (recorded, exchanged, n_bits) of every case of vote_corpus, and the two conditions on the corpus checked
    on the model alone: at least 20 recorded votes of each kind among the unexchanged cases, no vote in the wrong sense"""
    votes = [im.vote(b, l, d) for b, l, d, _ in vote_corpus()]
    kinds = [0, 0, 0]
    for (rec, exch, _), (_, _, _, swapped) in zip(votes, vote_corpus()):
        right, wrong = (exch, rec) if swapped else (rec, exch)
        assert wrong == 0, ("the model votes in the wrong sense", rec, exch, swapped)
        if not swapped:
            for j in range(3):
                kinds[j] += right >> j & 1
    assert min(kinds) >= 20, kinds
    return tuple(votes), tuple(kinds)


def check_votes(p):
    """irdm_iq_sense_batch of context p against the model, field for field"""
    want, kinds = model_votes()
    corpus = vote_corpus()
    got = p.iq_sense_batch([to_demod(b, l, d, k) for k, (b, l, d, _) in enumerate(corpus)])
    assert len(got) == len(want)
    for k, (g, w) in enumerate(zip(got, want)):
        assert (g.id, g.recorded, g.exchanged, g.pad, g.n_bits) == (k, w[0], w[1], 0, w[2]), (k, g.recorded, g.exchanged, g.n_bits, w)
    assert p.iq_sense_batch([]) == []
    return dict(cases=len(want), kinds=list(kinds), odd=sum(len(c[0]) % 2 for c in corpus), no_llr=sum(c[1] is None for c in corpus))


# ---------------------------------------------------------------- the pipeline ----
FS = 2_000_000
CHUNK = 262_144


@functools.lru_cache(maxsize=None)
def scene():
    """a 2 MHz stream of 4 IRA, 4 IBC and 4 IDA frames, built as tests/test_gpu_bitlayer.py builds its frame scene; bursts
    2, 5 and 9 straddle an edge of the 262 144-sample chunks it is fed in, and the last chunk is ragged"""
    rng = np.random.default_rng(53)
    first = 530 * 2048
    bursts = []
    for k in range(12):
        if k % 3 == 0:
            pages = [(int(rng.integers(0, 2**32)), int(rng.integers(0, 32))) for _ in range(2 + k % 2)]
            st = bl.ira_stream(int(rng.integers(0, 128)), int(rng.integers(0, 64)), int(rng.integers(-2047, 2048)),
                               int(rng.integers(-2047, 2048)), int(rng.integers(-2047, 2048)), pages, rng)
            bits = bl.ira_frame(st[:63 + 4 * 42])
        elif k % 3 == 1:
            st = bl.ibc_stream(int(rng.integers(0, 128)), int(rng.integers(0, 64)), int(rng.integers(0, 2)),
                               int(rng.integers(0, 2)), int(rng.integers(0, 2**32)), rng, n_blocks=4)
            bits = bl.ibc_frame(int(rng.integers(0, 4)), st)
        else:
            st = bl.ida_stream(int(rng.integers(0, 8)), int(rng.integers(1, 21)), int(rng.integers(0, 2)),
                               [int(b) for b in rng.integers(0, 256, 20)], rng)
            bits = bl.ida_frame(bl.lcw_bits(2, int(rng.integers(0, 32)), int(rng.integers(0, 1 << 21))), st, rng)
        if len(bits) < 290:
            bits = bits + [int(b) for b in rng.integers(0, 2, 290 - len(bits))]
        if len(bits) % 2:
            bits.append(0)
        start = first + 3000 + 100_000 * k
        if k in (2, 5, 9):
            start = (start // CHUNK + 1) * CHUNK - 6000
        bursts.append(dict(start=start, freq_hz=siggen.channel_freq(int(rng.integers(-20, 21)) or 3),
                           quads=[0] * 16 + siggen.bits_to_quadrants("".join(str(b) for b in bits)), amp=0.05))
    n = first + 3000 + 100_000 * 12 + 77_777
    assert n % CHUNK != 0 and n % 32768 != 0
    return siggen.make_stream(FS, n, bursts, seed=53)[0]


def in_format(iq, fmt):
    """the cf32 stream in one of the input formats, as the file would hold it"""
    if fmt == irdm.FMT_CF32:
        return iq
    if fmt == irdm.FMT_CI8:
        return siggen.to_ci8(iq)
    if fmt == irdm.FMT_CI16:
        return siggen.to_ci16(iq)
    if fmt == irdm.FMT_CU8:
        return (siggen.to_ci8(iq).astype(np.int16) + 128).astype(np.uint8)
    if fmt == irdm.FMT_CI32:
        return siggen.to_ci16(iq).astype(np.int32) << 16
    raise ValueError(fmt)


def run(samples, fmt, depth, options, chunk=CHUNK, after=None):
    """samples (as in_format gives them) through a context in chunks of `chunk` samples; returns the records as bytes, the
    votes, the summary and the RAW frequencies"""
    p = irdm.Pipeline(FS, fmt=fmt, max_chunk_samples=chunk, max_bursts_per_chunk=256, pipeline_depth=depth)
    per = 1 if fmt == irdm.FMT_CF32 else 2
    try:
        for k, v in options:
            p.set_option(k, v)
        n = len(samples) // per
        for off in range(0, n, chunk):
            p.feed_host(np.ascontiguousarray(samples[per * off:per * min(n, off + chunk)]))
        if depth:
            p.flush()
        try:
            st = p.iq_sense()
        except RuntimeError:
            st = None
        votes = p.poll_iq_votes()
        infos, _ = p.poll_frames()
        demods = p.poll_demods()
        out = dict(bursts=p.poll_bursts_raw().tobytes(), frames=b"".join(bytes(f) for f in infos),
                   demods=b"".join(bytes(d) for d in demods), n_demods=len(demods), votes=votes, st=st,
                   freqs=[int(l.split()[3]) for l in irdm.format_raw(demods, "iq")], ids=[d.id for d in demods], tagged=p.tagged)
        if after:
            after(p)
        return out
    finally:
        p.close()


def counts(r):
    st = r["st"]
    return (int(st.frames), int(st.votes_recorded), int(st.votes_exchanged), int(st.votes_both), int(st.verdict))


def check_summary(r):
    """the summary is the count of the votes, which pair with the demodulator's records"""
    st, votes = r["st"], r["votes"]
    assert [v.id for v in votes] == r["ids"]
    kinds = {"recorded": [0, 0, 0], "exchanged": [0, 0, 0], "both": [0, 0, 0]}
    n = {"recorded": 0, "exchanged": 0, "both": 0}
    for v in votes:
        w = im.decides(v.recorded, v.exchanged)
        if w:
            n[w] += 1
            for j in range(3):
                kinds[w][j] += (v.recorded | v.exchanged) >> j & 1
    assert (st.frames, st.votes_recorded, st.votes_exchanged, st.votes_both) == (len(votes), n["recorded"], n["exchanged"], n["both"])
    assert (list(st.kind_recorded), list(st.kind_exchanged), list(st.kind_both)) == (kinds["recorded"], kinds["exchanged"], kinds["both"])
    assert st.verdict == im.verdict(n["recorded"], n["exchanged"])


SENSE = (("iq_sense", 1),)


def pipeline_case(depth, fmt):
    """(a) the scene with iq_sense: 12 recorded votes, verdict 1; (b) its exchange: 12 exchanged votes, verdict 2, every RAW
    frequency the mirror of (a)'s; (c) the exchange with swap_iq: the records of (a) bit for bit.  Formats other than cf32
    run (a) and (c) alone."""
    x = scene()
    plain, swapped = in_format(x, fmt), in_format(im.swap_complex(x), fmt)
    seen = {}

    def reset_clears(p):
        p.reset(start_time_ns=1700000000 * 10**9)
        st = p.iq_sense()
        assert (st.frames, st.votes_recorded, st.votes_exchanged, st.votes_both, st.verdict) == (0, 0, 0, 0, 0)
        assert p.poll_iq_votes() == []
        # a new stream may choose its sense again
        p.set_option("swap_iq", 1)
        seen["reset"] = True

    def refusals(p):
        L = irdm.lib()
        # (the stream has begun with swap_iq 1)
        assert L.irdm_set_option(p.h, b"swap_iq", 0) == -1 and L.irdm_set_option(p.h, b"swap_iq", 1) == 0
        d = irdm.device_buffer(np.zeros(2 * 32768, np.float32))
        try:
            assert L.irdm_feed_device(p.h, C.c_void_p(d), 32768, None) == -1
            assert L.irdm_feed_begin(p.h, C.c_void_p(d), 32768, None) == -1
        finally:
            irdm.device_free(d)
        seen["refusals"] = True

    a = run(plain, fmt, depth, SENSE, after=reset_clears)
    check_summary(a)
    assert a["n_demods"] == 12 and counts(a) == (12, 12, 0, 0, irdm.IQ_AS_RECORDED), counts(a)
    assert list(a["st"].kind_recorded) == [4, 4, 4]
    c = run(swapped, fmt, depth, SENSE + (("swap_iq", 1),), after=refusals)
    for k in ("bursts", "frames", "demods", "freqs", "tagged"):
        assert c[k] == a[k], (k, depth, fmt)
    assert counts(c) == counts(a) and [bytes(v) for v in c["votes"]] == [bytes(v) for v in a["votes"]]
    assert seen == dict(reset=True, refusals=True)
    if fmt == irdm.FMT_CF32:
        b = run(swapped, fmt, depth, SENSE)
        check_summary(b)
        assert b["n_demods"] == 12 and counts(b) == (12, 0, 12, 0, irdm.IQ_EXCHANGED), counts(b)
        assert list(b["st"].kind_exchanged) == [4, 4, 4]
        # mirrored about the centre, to the printed Hz
        centre = 1622000000
        assert [f - centre for f in b["freqs"]] == [centre - f for f in a["freqs"]], (a["freqs"], b["freqs"])
        # the packed record path (what the binary runs): the demodulator keeps its bits on the device for the kernel
        pk = run(plain, fmt, depth, SENSE + (("packed_records", 1),))
        assert counts(pk) == counts(a) and [bytes(v) for v in pk["votes"]] == [bytes(v) for v in a["votes"]]
        # the option off: no votes, no summary, the same records
        off = run(plain, fmt, depth, ())
        assert off["st"] is None and off["votes"] == [] and all(off[k] == a[k] for k in ("bursts", "frames", "demods"))
    return dict(frames=a["n_demods"], freqs=a["freqs"])


def random_payloads_case(depth):
    """(d) siggen.standard_scene, random payloads: frames, but no votes"""
    iq, _ = siggen.standard_scene(FS, FS, 12, 3)
    r = run(iq, irdm.FMT_CF32, depth, SENSE)
    check_summary(r)
    assert r["n_demods"] >= 5 and counts(r) == (r["n_demods"], 0, 0, 0, irdm.IQ_TOO_FEW), counts(r)
    return dict(frames=r["n_demods"])
