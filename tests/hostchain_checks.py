"""TEST INFRASTRUCTURE: the corrections of the host feeds together -- swap_iq, irdm_dc_block, irdm_iq_balance and scrub on one
context, and their irdm_frontend_* twins on one front end -- that the GPU test (tests/test_gpu_hostchain.py) and the
CPU-emulation test (tests/hostchain_emul_run.py) share.  Bytes, not records: what the chain leaves in the history ring (or the
band a front end saves of it) against scrub_model(balance(dc_model(swap(convert(x))))) with the switched-off stages left out.

The input can tell the orders apart before any device sees it (order_facts): an asymmetric seed separates exchange and DC,
the planted bad samples DC and scrub, and two samples of 0.8 x 2^40 in one arm pass the exchange and the DC tracker and leave
the scrub's range only through the correction's beta = 1.43.  One pair cannot be told apart by any input: the scrub treats both
arms alike, so it commutes with the exchange; that is asserted as an equality.  The integer wire formats hold no sample the
scrub takes, so there the scrub commutes with everything."""
import ctypes as C
import functools
import itertools
import os
import sys
import tempfile

import numpy as np

import balance_model as bm
import dc_model as dm
import irdm
import prime_checks as pc
import scrub_checks as sc
import scrub_model as sm

FS = 2_000_000
CHUNK = 65_536
N = 3 * CHUNK + 4321
LOG2 = 12
SEED = (0.02, -0.035)
BALANCE = (-3.0, 10.0)              # dB, degrees: alpha = -0.176, beta = 1.434
LIMIT = 40
BIG = np.float32(0.8 * 2.0**40)
STAGES = ("swap", "dc", "balance", "scrub")
SUBSETS = tuple(frozenset(s for s, b in zip(STAGES, bits) if b) for bits in itertools.product((0, 1), repeat=4))
ALL = frozenset(STAGES)
CF32, CI16F, CI8 = irdm.FMT_CF32, irdm.FMT_CI16_FULL, irdm.FMT_CI8
FE = dict(fs_in=10_000_000, D=5, shift_hz=1_500_000.0)


@functools.lru_cache(maxsize=None)
def wire_input(fmt):
    """N samples of noise at unit scale plus a DC of 0.03 (1 + 0.6j).  cf32: interleaved floats with four bad samples -- the
    first, the last and those on either side of the first chunk's edge -- and the two samples that only the correction
    carries past 2^40; ci16-full and ci8: the same noise at 1/8 of full scale as integer codes"""
    rng = np.random.default_rng(2026)
    x = rng.standard_normal(2 * N).astype(np.float32)
    x[0::2] += np.float32(0.03)
    x[1::2] += np.float32(0.018)
    if fmt == CF32:
        x[0] = np.float32("nan")
        x[2 * (CHUNK - 1) + 1] = np.float32("inf")
        x[2 * CHUNK], x[2 * CHUNK + 1] = np.float32("-inf"), np.float32(1e30)
        x[2 * (N - 1)] = np.float32(1e30)
        x[2 * 100_000 + 1] = BIG            # (Q: over the limit behind the correction unless exchanged first)
        x[2 * 150_000] = BIG                # (I: over the limit behind the correction only when exchanged first)
    else:
        t, scale = {CI16F: (np.int16, 4096.0), CI8: (np.int8, 16.0)}[fmt]
        x = np.clip(np.rint(x * np.float32(scale)), np.iinfo(t).min, np.iinfo(t).max).astype(t)
    x.setflags(write=False)
    return x


def swap(y):
    return np.ascontiguousarray(y.reshape(-1, 2)[:, ::-1]).reshape(-1)


def model(raw, fmt, on, order=STAGES, upto=None):
    """(the stream the stages of `on` leave of raw, in `order` and as far as stage `upto` exclusive; the figures of DC and scrub)"""
    y, figs = bm.convert(raw, fmt), {}
    for s in order:
        if s == upto:
            break
        if s not in on:
            continue
        if s == "swap":
            y = swap(y)
        elif s == "dc":
            y, figs["dc"] = dm.dc_model(y, LOG2, SEED)
        elif s == "balance":
            y = bm.balance(y, *bm.coeffs(*BALANCE))
        else:
            y, figs["scrub"] = sm.scrub(y, LIMIT)
    return y, figs


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


def differing(got, want, on):
    """the 32-bit words of two cf32 streams (arrays or bytes) that differ.  Every bit counts, with the one allowance the balance
    kernel's own test makes (tests/balance_checks.py): behind the balance, where the model has a NaN any NaN will do -- the
    correction's contract leaves a NaN's payload open, and the DC tracker's does not"""
    g, w = (np.frombuffer(a, np.uint32) if isinstance(a, bytes) else np.ascontiguousarray(a).view(np.uint32) for a in (got, want))
    if len(g) != len(w):
        return np.arange(1)
    if "balance" not in on:
        return np.flatnonzero(g != w)
    return np.flatnonzero(np.where(np.isnan(w.view(np.float32)), ~np.isnan(g.view(np.float32)), g != w))


def order_facts(fmt):
    """on the models alone: for every subset, every exchange of two adjacent switched-on stages changes the expected bytes --
    but exchange <-> scrub, which commute for every input, and, for an integer wire format, any pair with the scrub"""
    raw, told, commuting = wire_input(fmt), 0, 0
    for on in SUBSETS:
        seq = [s for s in STAGES if s in on]
        want = model(raw, fmt, on)[0]
        for k in range(len(seq) - 1):
            other = seq[:k] + [seq[k + 1], seq[k]] + seq[k + 2:]
            pair = {seq[k], seq[k + 1]}
            commute = pair == {"swap", "scrub"} or (fmt != CF32 and "scrub" in pair)
            assert same_bits(model(raw, fmt, on, other)[0], want) == commute, (fmt, sorted(on), other)
            told, commuting = told + (not commute), commuting + commute
    if fmt == CF32:
        # the sample that meets the scrub through the correction alone
        y = model(raw, fmt, ALL - {"swap"})[0].reshape(-1, 2)
        pre = model(raw, fmt, ALL - {"swap"}, upto="balance")[0].reshape(-1, 2)
        assert np.abs(pre[100_000]).max() <= 2.0**LIMIT and not y[100_000].any() and y[150_000].all()
        y = model(raw, fmt, ALL)[0].reshape(-1, 2)
        assert not y[150_000].any() and y[100_000].all()
    return told, commuting


def cases():
    """(subset, wire format): all 16 subsets with the object's own cf32, those with DC or balance on once more from ci16-full"""
    out = [(on, CF32) for on in SUBSETS]
    out += [(on, CI16F) for on in SUBSETS if on & {"dc", "balance"}]
    return out


def other_wire(wire):
    return CI16F if wire == CF32 else CF32


def configure(obj, on, wire):
    """the corrections of `on` on a Pipeline or a Frontend.  With DC and balance both on, balance is given the other wire
    format: DC's is the one in effect"""
    fe = isinstance(obj, irdm.Frontend)
    if "swap" in on:
        obj.swap_iq(True) if fe else obj.set_option("swap_iq", 1)
    if "scrub" in on:
        obj.scrub(True) if fe else obj.set_option("scrub", 1)
    if "balance" in on:
        obj.iq_balance(other_wire(wire) if "dc" in on else wire, *BALANCE)
    if "dc" in on:
        obj.dc_block(wire, LOG2, SEED)
    assert getattr(obj, "wire_fmt", CF32) == wire or not on & {"dc", "balance"}


def pieces(raw, chunk=CHUNK):
    """the arrays feed_host takes, `chunk` samples each"""
    a = raw.view(np.complex64) if raw.dtype == np.float32 else raw.reshape(-1, 2)
    for off in range(0, len(a), chunk):
        yield np.ascontiguousarray(a[off:off + chunk]).reshape(-1)


def head_of(raw):
    return raw.view(np.complex64) if raw.dtype == np.float32 else raw


def figures(obj, on):
    out = {}
    if "dc" in on:
        out["dc"] = sc_dc_tuple(obj.dc_stats())
    if "scrub" in on:
        st = obj.scrub_stats()
        out["scrub"] = (int(st.n_samples), st.limit_log2, st.active) + sc.stat_tuple(st)
    return out


def sc_dc_tuple(st):
    f = lambda v: np.float32(v).tobytes()
    return (int(st.n_samples), int(st.n_blocks), st.block_log2, st.wire_format, f(st.seed_i), f(st.seed_q), f(st.first_i), f(st.first_q),
            f(st.last_i), f(st.last_q), f(st.min_i), f(st.min_q), f(st.max_i), f(st.max_q))


def model_figures(figs, wire, n=N, active=1):
    out = {}
    if "dc" in figs:
        g, f = figs["dc"], lambda v: np.float32(v).tobytes()
        out["dc"] = (g["n_samples"], g["n_blocks"], LOG2, wire, f(g["seed"][0]), f(g["seed"][1]), f(g["first"][0]), f(g["first"][1]),
                     f(g["last"][0]), f(g["last"][1]), f(g["min"][0]), f(g["min"][1]), f(g["max"][0]), f(g["max"][1]))
    if "scrub" in figs:
        out["scrub"] = (n, LIMIT, active) + tuple(figs["scrub"][k] for k in sc.FIGURES)
    return out


# ---------------------------------------------------------------- a context ----
def context_run(raw, on=frozenset(), wire=CF32, fmt=CF32, prime=False):
    """raw through a context at 2 MS/s, pipeline_depth 3, max_chunk_samples 65 536, in three full chunks and a ragged one:
    (the stream as the history ring holds it, as bytes; the figures)"""
    p = irdm.Pipeline(FS, fmt=fmt, max_chunk_samples=CHUNK, max_bursts_per_chunk=256, pipeline_depth=3)
    try:
        configure(p, on, wire)
        if prime:
            assert p.prime_host(head_of(raw)) == N // 2048
        for piece in pieces(raw):
            p.feed_host(piece)
        p.flush()
        figs = figures(p, on)
        ptr, ring_len = p.ring()
        n = p.sample_count
        assert n == N + (512 * 2048 if prime else 0) and n <= ring_len
        got = np.empty(n * bm.FORMATS[fmt][1], np.uint8)
        irdm.device_download(got, ptr)
        return got, figs
    finally:
        p.close()


def context_case(on, wire):
    raw = wire_input(wire)
    want, figs = model(raw, wire, on)
    got, got_figs = context_run(raw, on, wire)
    bad = differing(got, want, on)
    assert len(bad) == 0, (sorted(on), wire, int(bad[0]) // 2, len(bad))
    assert got_figs == model_figures(figs, wire), (sorted(on), wire, got_figs, model_figures(figs, wire))
    return len(got) // 8


def context_cases():
    """all 16 subsets from cf32, the 12 with DC or balance on from ci16-full, and all four on from ci8"""
    done = sum(1 for on, wire in cases() if context_case(on, wire) == N)
    return done + (context_case(ALL, CI8) == N)


def context_prime_case():
    """irdm_prime_host with all four on, cf32: the ring holds the model of P || x whole, P the 512 frames tiled from x's 98; its
    part for the recording is the unprimed run's from the recording's second DC block on (its first block is corrected by the
    mean of the prefix's last block, where the unprimed run has the seed).  The scrub's figures are the recording's alone; the
    DC tracker's count the prefix, which it has tracked."""
    raw = wire_input(CF32)
    P = pc.cf32_floats(pc.prefix(raw.view(np.complex64), FS)[0])
    H = len(P) // 2
    assert H == 512 * 2048 and H % (1 << LOG2) == 0
    both = np.concatenate([P, raw])
    want, figs = model(both, CF32, ALL)
    alone = model(raw, CF32, ALL)[0]
    B = 1 << LOG2
    assert same_bits(want[2 * (H + B):], alone[2 * B:]) and not same_bits(want[2 * H:2 * (H + B)], alone[:2 * B])
    got, got_figs = context_run(raw, ALL, CF32, prime=True)
    bad = differing(got, want, ALL)
    assert len(bad) == 0, (int(bad[0]) // 2, len(bad))
    assert same_bits(got[8 * (H + B):], alone[2 * B:])
    figs["scrub"] = sm.scrub(model(both, CF32, ALL, upto="scrub")[0][2 * H:], LIMIT)[1]
    assert figs["scrub"]["n_zeroed"] == 5 and got_figs == model_figures(figs, CF32), (got_figs, model_figures(figs, CF32))
    return H


# ---------------------------------------------------------------- a front end ----
def front_end_run(raw, on=frozenset(), wire=CF32, fmt=CF32, prime=False):
    """raw as a 10 MS/s capture through a front end with D = 5, feed_host in chunks of 65 536, the band saved as cf32"""
    fe = irdm.Frontend(FE["fs_in"], fmt, FE["D"], FE["shift_hz"])
    p = irdm.Pipeline(fe.out_rate, fmt=CF32, center_frequency=1622000000.0 + fe.applied_shift_hz, max_chunk_samples=CHUNK,
                      max_bursts_per_chunk=256, pipeline_depth=0)
    try:
        fe.save(CF32)
        configure(fe, on, wire)
        if prime:
            assert fe.prime_host(p, head_of(raw)) >= 1
        for piece in pieces(raw):
            fe.feed_host(p, piece)
        figs = figures(fe, on)
        fe.flush(p)
        band = b"".join(fe.saved)
        assert len(band) >= 8 * (N // FE["D"] - 1)
        return band, figs
    finally:
        p.close()
        fe.close()


def front_end_cases():
    """the 16 subsets from cf32 and the 12 with DC or balance on from ci16-full: the saved band is the band of a plain front end
    fed the modelled stream, the figures the model's"""
    done = 0
    for on, wire in cases():
        raw = wire_input(wire)
        want, figs = model(raw, wire, on)
        got, got_figs = front_end_run(raw, on, wire)
        plain, _ = front_end_run(want)
        assert len(differing(got, plain, on)) == 0, (sorted(on), wire)
        assert got_figs == model_figures(figs, wire), (sorted(on), wire, got_figs)
        done += 1
    return done


def front_end_prime_case():
    """irdm_frontend_prime_host with all four on: the band and the figures of the unprimed run"""
    raw = wire_input(CF32)
    primed, unprimed = front_end_run(raw, ALL, CF32, prime=True), front_end_run(raw, ALL, CF32)
    assert primed[0] == unprimed[0] and primed[1] == unprimed[1] == model_figures(model(raw, CF32, ALL)[1], CF32)
    return len(primed[0]) // 8


# ---------------------------------------------------------------- refusals ----
CONTEXT_LINES = {
    "swap": "irdm_hip: option swap_iq exchanges the chunks of irdm_feed_host only: a device feed takes the caller's buffer as it is -- "
            "exchange it with irdm_swap_iq_device first\n",
    "scrub": "irdm_hip: option scrub cleans the chunks of irdm_feed_host only: a device feed takes the caller's buffer as it is -- "
             "scrub it with irdm_scrub_device first\n",
    "balance": "irdm_hip: irdm_iq_balance corrects the chunks of irdm_feed_host only: a device feed takes the caller's buffer as it is -- "
               "correct it with irdm_iq_balance_device first\n",
    "dc": "irdm_hip: irdm_dc_block corrects the chunks of irdm_feed_host only: a device feed takes the caller's buffer as it is -- "
          "correct it with irdm_dc_block_device first\n",
}
FRONT_END_LINES = {
    "swap": "irdm_hip: front end: irdm_frontend_swap_iq exchanges the chunks of irdm_frontend_feed_host only: a device feed takes the "
            "caller's buffer as it is -- exchange it with irdm_swap_iq_device first\n",
    "scrub": "irdm_hip: front end: irdm_frontend_scrub cleans the chunks of irdm_frontend_feed_host only: a device feed takes the "
             "caller's buffer as it is -- scrub it with irdm_scrub_device first\n",
    "balance": "irdm_hip: front end: irdm_frontend_iq_balance corrects the chunks of irdm_frontend_feed_host only: a device feed takes "
               "the caller's buffer as it is -- correct it with irdm_iq_balance_device first\n",
    "dc": "irdm_hip: front end: irdm_frontend_dc_block corrects the chunks of irdm_frontend_feed_host only: a device feed takes the "
          "caller's buffer as it is -- correct it with irdm_dc_block_device first\n",
}


def stderr_of(call):
    """(what call() returns, what the library wrote to file descriptor 2 meanwhile)"""
    sys.stderr.flush()
    saved = os.dup(2)
    with tempfile.TemporaryFile() as f:
        os.dup2(f.fileno(), 2)
        try:
            rc = call()
        finally:
            os.dup2(saved, 2)
            os.close(saved)
        f.seek(0)
        return rc, f.read().decode()


def refusal_cases():
    """a device feed of an object with one correction on returns -1 with that correction's sentence on stderr, with all four
    on the exchange's; a ci8 object refuses DC and balance and takes the exchange alone"""
    L = irdm.lib()
    d = irdm.device_buffer(np.zeros(2 * 32768, np.float32))
    lines = 0
    try:
        for on in [frozenset([s]) for s in STAGES] + [ALL]:
            first = next(s for s in ("swap", "scrub", "balance", "dc") if s in on)          # (the order they are looked at in)
            p = irdm.Pipeline(FS, fmt=CF32, max_chunk_samples=CHUNK, max_bursts_per_chunk=256, pipeline_depth=3)
            fe = irdm.Frontend(FE["fs_in"], CF32, FE["D"], FE["shift_hz"])
            try:
                configure(p, on, CF32)
                configure(fe, on, CF32)
                for call in (lambda: L.irdm_feed_device(p.h, C.c_void_p(d), 32768, None),
                             lambda: L.irdm_feed_begin(p.h, C.c_void_p(d), 32768, None)):
                    assert stderr_of(call) == (-1, CONTEXT_LINES[first]), (sorted(on), stderr_of(call))
                    lines += 1
                q = irdm.Pipeline(fe.out_rate, fmt=CF32, max_chunk_samples=CHUNK, max_bursts_per_chunk=256, pipeline_depth=0)
                try:
                    for call in (lambda: L.irdm_frontend_feed_device(fe.h, q.h, C.c_void_p(d), 4096, None),
                                 lambda: L.irdm_frontend_run_device(fe.h, C.c_void_p(d), 4096, C.c_void_p(d + 8 * 16384), 4096, None)):
                        assert stderr_of(call) == (-1, FRONT_END_LINES[first]), (sorted(on), stderr_of(call))
                        lines += 1
                finally:
                    q.close()
            finally:
                p.close()
                fe.close()
    finally:
        irdm.device_free(d)
    # ci8 objects
    raw = wire_input(CI8)
    want = swap(raw)
    p = irdm.Pipeline(FS, fmt=CI8, max_chunk_samples=CHUNK, max_bursts_per_chunk=256, pipeline_depth=3)
    fe = irdm.Frontend(FE["fs_in"], CI8, FE["D"], FE["shift_hz"])
    try:
        assert L.irdm_iq_balance(p.h, CI8, *BALANCE) == -1 and L.irdm_dc_block(p.h, CI8, LOG2, 0.0, 0.0) == -1
        assert L.irdm_frontend_iq_balance(fe.h, CI8, *BALANCE) == -1 and L.irdm_frontend_dc_block(fe.h, CI8, LOG2, 0.0, 0.0) == -1
    finally:
        p.close()
        fe.close()
    got, _ = context_run(raw, frozenset(["swap"]), CI8, fmt=CI8)
    assert same_bits(got, want) and not same_bits(got, raw)
    band, _ = front_end_run(raw, frozenset(["swap"]), CI8, fmt=CI8)
    assert band == front_end_run(want, fmt=CI8)[0] and band != front_end_run(raw, fmt=CI8)[0]
    return lines
