"""TEST INFRASTRUCTURE: stage C alone (irdm_qpsk_demod_batch: demod_seq_kernel, demod_par_kernel, demod_export of
csrc/demod.hip; qpsk_demod.c:393-535) on DESIGNED frames -- frames stage B would never hand over from a scene: every length
at which a decision changes, the end-of-frame rule on either side of each of its thresholds, the unique word with every
number and kind of error on either side of the hard and the soft check, under every input direction, the timing loop held
at its limit for a whole frame (the LDS sample ring read at its edges, 441 and 447 symbols instead of 444), exact zeros
under the PLL, noise -- with both decimators.

The reference is the oracle's orc_qpsk_demod with samples_per_symbol = 10 on the same samples.  The builder designs with
the oracle (orc_qpsk_demod_trace tells what the call decided on the way) and ASSERTS what each case is for; coverage()
asserts the corpus as a whole.  Shared by tests/stage_c_emul_run.py (the CPU emulation), tests/test_gpu_stage_c.py (the
card) and tests/test_oracle_vs_ref.py (the oracle against the reference's compiled code); neither the GPU nor the product
is touched at import."""
import collections
import ctypes as C
import functools
import math

import numpy as np

import orc
import parity
import scenes

MAX_FRAME = 4440
SPS = 10
AMP = 0.4                        # scenes.stage_c_frames
UW = scenes.UW_QUADS             # {1: downlink, 2: uplink}

# reference_safe: the reference sizes its symbol buffers num_samples / 10 + 1 (qpsk_demod.c:398) and its timing loop has no
# cap: a frame whose loop runs EARLY long enough makes more symbols than that and the reference writes behind its buffers
# (the oracle allocates 8 more, irdm_oracle.c: max_sym + 8).  Such a case is compared with the oracle only and never handed
# to the reference's compiled code.
Case = collections.namedtuple("Case", "name iq direction reference_safe")


def synth(n, quads, amp=AMP, phase=0.0, offsets=None, carrier=0.0, sigma=0.0, seed=0):
    """n samples of the symbols `quads` (quadrant centres, 10 samples apart, straight lines between them: the way
    scenes.stage_c_frames draws them).  amp: one amplitude or one per symbol; phase: added to every symbol; offsets: radians
    added to single symbols {index: offset}; carrier: residual carrier, radians per sample; sigma: noise, seeded."""
    nsym = n // SPS + 3
    q = np.zeros(nsym)
    q[:min(len(quads), nsym)] = np.asarray(quads[:nsym], float)
    a = np.broadcast_to(np.asarray(amp, float), (nsym,)) if np.ndim(amp) == 0 else np.asarray(amp, float)[:nsym]
    ph = np.pi / 4 + q * np.pi / 2 + phase
    for i, off in (offsets or {}).items():
        ph[i] += off
    sym = a * np.exp(1j * ph)
    t = np.arange(n) / SPS
    k = t.astype(int)
    x = sym[k] * (1 - (t - k)) + sym[k + 1] * (t - k)
    if carrier:
        x = x * np.exp(1j * carrier * np.arange(n))
    if sigma:
        r = np.random.default_rng(5000 + seed)
        x = x + (r.standard_normal(n) + 1j * r.standard_normal(n)) * sigma
    return x.astype(np.complex64)


def payload(k, seed):
    return np.random.default_rng(100 + seed).integers(0, 4, k).tolist()


def oracle_frame(iq, direction):
    fr = orc.Frame()
    fr.samples_per_symbol = float(SPS)
    fr.sample_rate = 250000.0
    fr.direction = int(direction)
    fr.num_samples = len(iq)
    np.ctypeslib.as_array(fr.samples)[:2 * len(iq)] = np.ascontiguousarray(iq, np.complex64).view(np.float32)
    return fr


def oracle(iq, direction, gardner):
    """(verdict, orc.Demod, orc.DemodTrace) of the oracle for one frame"""
    fr = oracle_frame(iq, direction)
    d, tr = orc.Demod(), orc.DemodTrace()
    ok = orc.lib().orc_qpsk_demod_trace(C.byref(fr), int(gardner), C.byref(d), C.byref(tr))
    return ok, d, tr


def soft_errors64(tr):
    """soft_check_sync_word (qpsk_demod.c:297-325) restated in float64 on the PLL's output for the unique word: the summed
    phase distance to the downlink and to the uplink word, in quadrants"""
    out = []
    for d in (1, 2):
        total = 0.0
        for i in range(12):
            expect = math.pi / 4 + UW[d][i] * math.pi / 2
            actual = math.atan2(float(tr.uw_im[i]), float(tr.uw_re[i]))
            if actual < 0:
                actual += 2 * math.pi
            df = actual - expect
            if df > math.pi:
                df -= 2 * math.pi
            if df < -math.pi:
                df += 2 * math.pi
            total += abs(df) * 2 / math.pi
        out.append(total)
    return tuple(out)


SOFT_LIMIT = 3.0                 # qpsk_demod.c:441
SOFT_MARGIN = 0.05               # what a designed soft case keeps between its smaller error and the limit: the device's
                                 # atan2f differs from the host's by an ulp or two of 6 rad, 12 of them sum to ~1e-5


@functools.lru_cache(maxsize=1)
def cases():
    """the corpus, a tuple of Case; every case's purpose is asserted on the oracle while it is built"""
    out = []

    def add(name, iq, direction=1, expect=None, gardner=(1, 0), unsafe=False):
        """expect: dict of ok / ns (n_symbols of an accepted frame) / direction / conf100 / dec (symbols decimated) /
        skips (PLL skips > 0), asserted on the oracle for the decimators in `gardner`"""
        iq = np.ascontiguousarray(iq, np.complex64)
        assert len(iq) <= MAX_FRAME and np.all(np.isfinite(iq.view(np.float32))), name
        tiny = np.abs(iq.view(np.float32))
        assert not np.any((tiny > 0) & (tiny < np.finfo(np.float32).tiny)), name
        iq.setflags(write=False)
        safe = True
        for g in (1, 0):
            ok, d, tr = oracle(iq, direction, g)
            safe = safe and tr.n_decimated <= len(iq) // SPS + 1
            if expect and g in gardner:
                got = dict(ok=ok, ns=d.n_symbols if ok else tr.n_sliced, direction=d.direction, conf100=d.confidence == 100,
                           dec=tr.n_decimated, skips=tr.pll_skips > 0)
                for k, v in expect.items():
                    assert got[k] == v, "%s, gardner %d: %s is %r, designed for %r" % (name, g, k, got[k], v)
        assert safe == (not unsafe), "%s: more symbols than the reference's buffers hold: %s" % (name, not safe)
        out.append(Case(name, iq, direction, safe))

    def frame(n, d=1, seed=0, **kw):
        return synth(n, UW[d] + payload(n // SPS + 3, seed), **kw)

    # ---- lengths: nothing, below the interpolator's four samples, either side of 12 symbols for each decimator (Gardner:
    # the loop runs while pos < n - 3; simple: ceil(n / 10) symbols), the normal and the simplex maximum and one off
    long_dl = frame(MAX_FRAME, 1, seed=1, phase=0.1)
    long_ul = frame(MAX_FRAME, 2, seed=2, phase=-0.15)
    for n in (0, 1, 3, 4, 13):
        add("len_%d" % n, long_dl[:n], 1, dict(ok=0))
    g_rej = max(n for n in range(100, 130) if oracle(long_dl[:n], 1, 1)[2].n_decimated < 12)
    s_rej = max(n for n in range(100, 130) if oracle(long_dl[:n], 1, 0)[2].n_decimated < 12)
    assert (g_rej, s_rej) == (113, 110), (g_rej, s_rej)
    add("len_110", long_dl[:110], 1, dict(ok=0, dec=11), gardner=(0,))
    add("len_111", long_dl[:111], 1, dict(ok=1, ns=12, direction=1), gardner=(0,))
    add("len_113", long_dl[:113], 1, dict(ok=0, dec=11), gardner=(1,))
    add("len_114", long_dl[:114], 1, dict(ok=1, ns=12, direction=1), gardner=(1,))
    add("len_1910", long_ul[:1910], 2, dict(ok=1, ns=191, direction=2))
    add("len_1911", long_ul[:1911], 2, dict(ok=1, direction=2))
    add("len_4439", long_dl[:4439], 1, dict(ok=1, ns=444, direction=1))
    add("len_4440", long_dl, 1, dict(ok=1, ns=444, direction=1))
    add("len_4440_uplink", long_ul, 2, dict(ok=1, ns=444, direction=2))
    # symbol counts that are no multiple of 4 (the export's last byte holds 1, 2, 3 symbols) or of 16 (its last word is
    # not full)
    for n, ns in ((124, 13), (134, 14), (144, 15), (154, 16), (164, 17), (1004, 101), (3214, 322)):
        add("len_%d" % n, long_ul[:n], 2, dict(ok=1, ns=ns, direction=2), gardner=(1,))

    # ---- the end-of-frame rule (qpsk_demod.c:210-225): three symbols in a row below an eighth of the running maximum end
    # the frame three symbols back
    def dropped(n, at, k, to, d=1, seed=3):
        a = np.full(n // SPS + 3, AMP)
        a[at:at + k] *= to
        return frame(n, d, seed=seed, amp=a, phase=0.05)

    for k, ns in ((1, 191), (2, 191), (3, 100), (4, 100)):
        add("drop_tenth_%d_symbols_from_100" % k, dropped(1910, 100, k, 0.1), 1, dict(ok=1, ns=ns))
    add("drop_to_1/7.5_3_symbols", dropped(1910, 100, 3, 1 / 7.5), 1, dict(ok=1, ns=191))
    add("drop_to_1/8.5_3_symbols", dropped(1910, 100, 3, 1 / 8.5), 1, dict(ok=1, ns=100))
    add("drop_tenth_from_10", dropped(1910, 10, 3, 0.1), 1, dict(ok=0, ns=10))
    add("drop_tenth_from_11", dropped(1910, 11, 3, 0.1), 1, dict(ok=0, ns=11))
    add("drop_tenth_from_12", dropped(1910, 12, 3, 0.1), 1, dict(ok=1, ns=12))
    add("drop_tenth_from_13", dropped(1910, 13, 3, 0.1, d=2), 2, dict(ok=1, ns=13, direction=2))
    add("drop_tenth_from_440_of_444", dropped(MAX_FRAME, 440, 3, 0.1), 1, dict(ok=1, ns=440))
    add("drop_tenth_last_two_of_444", dropped(MAX_FRAME, 442, 3, 0.1), 1, dict(ok=1, ns=444))
    # a loud beginning: symbol 0 is sample 1 (the interpolator's index is clamped), 0.9 of the word's first symbol and 0.1 of
    # its second, the opposite one: 0.8 of the amplitude.  The running maximum is set there: x9 leaves the symbols behind
    # it at 1 / 7.2 of it and the frame goes on, x12 at 1 / 9.6 and the frame ends at its first symbol.  (x10 is 1 / 8.0,
    # the threshold itself to the last bit of the device's sincosf: not used.)  The simple decimator takes sample 0, the whole
    # first symbol: x7 goes on, x9 and x12 end the frame.
    for factor, ends in ((7.0, (False, False)), (9.0, (True, False)), (12.0, (True, True))):
        x = frame(1910, 1, seed=4).copy()
        x[:5] *= factor
        for g in (0, 1):
            add_expect = dict(ok=0, ns=1) if ends[g] else dict(ok=1, ns=191)
            assert oracle(x, 1, g)[0] == add_expect["ok"], (factor, g)
        add("first_5_samples_x%g" % factor, x, 1, dict(ok=0, ns=1) if ends[1] else dict(ok=1, ns=191), gardner=(1,))
    # exact zeros under on-time positions: the PLL's `continue` (:174) leaves phi and total_phase alone; two such symbols
    # and the frame goes on, three and the rule ends it
    for k, ns in ((2, 191), (3, 60)):
        x = frame(1910, 1, seed=5, phase=0.05).copy()
        x[SPS * 60 - 4:SPS * (60 + k - 1) + 5] = 0
        add("zeros_under_%d_symbols_from_60" % k, x, 1, dict(ok=1, ns=ns, skips=True))

    # ---- the unique word (qpsk_demod.c:277-325, :429-465), each word under input direction 0, 1 and 2
    def uw_frame(d, errors, offset=0.0, seed=6):
        """errors: {position: quadrants off}; the erroneous symbols' phases moved by `offset` radians away from the word's
        own quadrant (negative: towards it)"""
        q = list(UW[d])
        for i, e in errors.items():
            q[i] = (q[i] + e) % 4
        return synth(400, q + payload(45, seed + d), offsets={i: offset * (1 if e == 1 else -1) for i, e in errors.items()})

    hard = (("clean", {}, 1), ("1_adjacent", {3: 1}, 1), ("2_adjacent", {3: 1, 8: 3}, 1), ("1_opposite", {6: 2}, 1),
            ("2_opposite", {1: 2, 7: 2}, 0))
    # three adjacent-quadrant errors fail the hard check by one; the soft check sums the phase distances: 3.0 at exactly
    # 90 degrees each.  Offsets towards the word's own quadrants rescue the frame, offsets away reject it
    soft = (("rescued_-30deg", -30.0, 1), ("rescued_-3deg", -3.0, 1), ("rejected_+2deg", 2.0, 0), ("rejected_+30deg", 30.0, 0))
    for d, word in ((1, "downlink"), (2, "uplink")):
        other = 3 - d
        for name, errors, ok in hard:
            x = uw_frame(d, errors)
            _, _, tr = oracle(x, 0, 1)
            assert (tr.hard_dl, tr.hard_ul) == ((d == 1) * ok, (d == 2) * ok), (name, word)
            if not ok:                   # (two opposite-quadrant errors are 4.0 to the soft check)
                assert min(soft_errors64(tr)) - SOFT_LIMIT >= SOFT_MARGIN, (name, word)
            for given in (0, 1, 2):
                # (the hard check overrides the direction given: also 0, also the other word's)
                add("uw_%s_%s_given_%d" % (word, name, given), x, given, dict(ok=ok, direction=d) if ok else dict(ok=0, ns=40))
        for name, deg, ok in soft:
            x = uw_frame(d, {2: 1, 5: 3, 9: 1}, offset=math.radians(deg))
            _, _, tr = oracle(x, 0, 1)
            e = soft_errors64(tr)
            assert not (tr.hard_dl or tr.hard_ul), (word, name)
            assert e[d - 1] < e[other - 1] and abs(e[d - 1] - SOFT_LIMIT) >= SOFT_MARGIN and (e[d - 1] < SOFT_LIMIT) == bool(ok), \
                (word, name, e)
            assert abs(min(tr.soft_dl, tr.soft_ul) - e[d - 1]) < 1e-4, (word, name, e, tr.soft_dl, tr.soft_ul)
            for given in (0, 1, 2):
                add("uw_%s_soft_%s_given_%d" % (word, name, given), x, given, dict(ok=ok, direction=d) if ok else dict(ok=0, ns=40))

    # ---- the timing loop at its limits: a constant payload quadrant gives the Gardner detector no transitions, a linear
    # amplitude envelope gives it an error of one sign, clamped, for the whole frame: the position runs away from 10 samples
    # per symbol by 0.02 K + 0.0001 K^2 samples over K symbols (+-29 at 4440 samples), to the edges of the kernel's window
    def ramp(n, a0, a1, d, carrier):
        return synth(n, UW[d] + [1] * (n // SPS + 3), amp=np.linspace(a0, a1, n // SPS + 3), carrier=carrier)

    for carrier in (0.0, 0.002):
        c = "_carrier" if carrier else ""
        add("drift_late_60_to_10" + c, ramp(MAX_FRAME, 60, 10, 1, carrier), 1, dict(ok=1, ns=441, dec=441, conf100=True), gardner=(1,))
        add("drift_early_10_to_60" + c, ramp(MAX_FRAME, 10, 60, 2, carrier), 2, dict(ok=1, ns=447, dec=447, conf100=True),
            gardner=(1,), unsafe=True)
        add("drift_early_10_to_60_1910" + c, ramp(1910, 10, 60, 1, carrier), 1, dict(ok=1, ns=192, dec=192, conf100=True), gardner=(1,))
        add("drift_late_60_to_10_3000" + c, ramp(3000, 60, 10, 2, carrier), 2, dict(ok=1, ns=299, dec=299, conf100=True), gardner=(1,))
        add("drift_early_10_to_60_3000" + c, ramp(3000, 10, 60, 1, carrier), 1, dict(ok=1, ns=302, dec=302, conf100=True),
            gardner=(1,), unsafe=True)
    add("random_payload_amplitude_50", synth(MAX_FRAME, UW[1] + payload(450, 7), amp=50.0, phase=0.1), 1, dict(ok=1, direction=1),
        gardner=(1,))
    # the proof that the positions left the window's centre: the symbol count is not the ceil((n - 3) / 10) of a loop that
    # keeps 10 samples per symbol -- off by 2 or more (20 samples or more) at 4440 samples, by 1 or more at 1910 and 3000
    for c in [c for c in out if c.name.startswith("drift_")]:
        n_dec = oracle(c.iq, c.direction, 1)[2].n_decimated
        assert abs(n_dec - math.ceil((len(c.iq) - 3) / SPS)) >= (2 if len(c.iq) == MAX_FRAME else 1), (c.name, n_dec)

    # ---- noise (the three levels of scenes.stage_c_frames), both directions, residual carriers of both signs
    lens = (1910, 1910, 1897, 1903, 2377, 4440, 997, 1910, 1910, 3001, 555, 1910,
            4440, 4431, 1915, 1234, 777, 346, 4101, 2999, 1910, 1906, 131, 4440)
    for i, n in enumerate(lens):
        d = 1 + i % 2
        sigma = AMP * (0.01, 0.05, 0.15)[i % 3]
        carrier = (0.0015, -0.0015, 0.0005, -0.0025)[i % 4]
        add("noise_%02d_%d_sigma_%g_carrier_%+g" % (i, n, sigma / AMP, carrier),
            frame(n, d, seed=20 + i, phase=(-0.15, 0.0, 0.15)[i % 3], sigma=sigma, carrier=carrier), d, dict(ok=1, direction=d))

    # ---- silence
    add("silence_1910", np.zeros(1910, np.complex64), 1, dict(ok=0, skips=True))
    return tuple(out)


@functools.lru_cache(maxsize=2)
def reference(gardner):
    """the oracle's (verdict, Demod, DemodTrace) for every case, computed once per decimator and left alone"""
    return tuple(oracle(c.iq, c.direction, gardner) for c in cases())


def coverage():
    """what the corpus must hold, on the oracle alone; returns a dict of counts"""
    cs = cases()
    res = {g: reference(g) for g in (1, 0)}
    names = lambda pred: [c.name for c, r in zip(cs, res[1]) if pred(c, *r)]            # noqa: E731
    hard = lambda tr: tr.hard_dl or tr.hard_ul                                          # noqa: E731
    cov = dict(
        short=names(lambda c, ok, d, tr: not ok and tr.n_sliced < 12),
        soft_rejected=names(lambda c, ok, d, tr: not ok and tr.n_sliced >= 12 and not hard(tr)),
        soft_rescued_dl=names(lambda c, ok, d, tr: ok and not hard(tr) and d.direction == 1),
        soft_rescued_ul=names(lambda c, ok, d, tr: ok and not hard(tr) and d.direction == 2),
        hard_overrides_to_dl=names(lambda c, ok, d, tr: ok and hard(tr) and c.direction == 2 and d.direction == 1),
        hard_overrides_to_ul=names(lambda c, ok, d, tr: ok and hard(tr) and c.direction == 1 and d.direction == 2),
        hard_sets_direction_0=names(lambda c, ok, d, tr: ok and hard(tr) and c.direction == 0 and d.direction in (1, 2)),
        ns_12=names(lambda c, ok, d, tr: ok and d.n_symbols == 12),
        ended_by_rule=names(lambda c, ok, d, tr: ok and d.n_symbols < tr.n_decimated),
        ns_441=names(lambda c, ok, d, tr: ok and d.n_symbols == 441),
        ns_444=names(lambda c, ok, d, tr: ok and d.n_symbols == 444),
        ns_447=names(lambda c, ok, d, tr: ok and d.n_symbols == 447),
        confidence_below_100=names(lambda c, ok, d, tr: ok and d.confidence < 100),
        pll_skip=names(lambda c, ok, d, tr: ok and tr.pll_skips > 0),
        phase_positive=names(lambda c, ok, d, tr: ok and d.total_phase > 1.0),
        phase_negative=names(lambda c, ok, d, tr: ok and d.total_phase < -1.0),
    )
    for k, v in cov.items():
        assert v, "no case of: " + k
    counts = {k: len(v) for k, v in cov.items()}
    for g in (1, 0):
        acc = sum(1 for ok, _, _ in res[g] if ok)
        assert acc >= 0.7 * len(cs) and len(cs) - acc >= 8, (g, acc, len(cs))
        counts["accepted_gardner%d" % g] = acc
    assert any(not ok and tr.n_sliced < 12 for ok, _, tr in res[0]) and any(ok and d.n_symbols == 12 for ok, d, _ in res[0])
    assert 120 <= len(cs) <= 160, len(cs)
    assert len({c.name for c in cs}) == len(cs)
    counts["cases"] = len(cs)
    counts["reference_unsafe"] = sum(1 for c in cs if not c.reference_safe)
    return counts


def phase_tol(n_symbols):
    """the project's 0.05 Hz on the refined frequency (parity.compare) carried back through qpsk_demod.c:521-524:
    frequency = total_phase / (n_symbols / 25000) / 2 pi"""
    return 0.05 * 2 * math.pi * n_symbols / 25000.0


def u32(x):
    return np.float32(x).view(np.uint32)


def check(name, got, ok, want, exact, worst):
    """one record of irdm_qpsk_demod_batch against the oracle's; worst: the largest soft differences seen so far"""
    assert got.ok == ok, (name, "ok", got.ok, ok)
    if not ok:
        return
    for f in ("direction", "confidence", "n_symbols", "n_payload_symbols", "n_bits"):
        assert getattr(got, f) == getattr(want, f), (name, f, getattr(got, f), getattr(want, f))
    nb = want.n_bits
    assert bytes(got.bits[:nb]) == bytes(want.bits[:nb]), (name, "bits")
    gl, wl = np.array(got.llr[:nb], np.float32), np.array(want.llr[:nb], np.float32)
    dl = float(np.max(np.abs(gl - wl))) if nb else 0.0
    dv = abs(got.level - want.level) / max(1.0, want.level)
    dp = abs(got.total_phase - want.total_phase)
    worst["llr"] = max(worst["llr"], dl)
    worst["level"] = max(worst["level"], dv)
    worst["total_phase"] = max(worst["total_phase"], dp)
    worst["total_phase_hz"] = max(worst["total_phase_hz"], dp / phase_tol(want.n_symbols) * 0.05)
    if exact:
        assert np.array_equal(gl.view(np.uint32), wl.view(np.uint32)), (name, "llr", dl)
        assert u32(got.level) == u32(want.level), (name, "level", got.level, want.level)
        assert u32(got.total_phase) == u32(want.total_phase), (name, "total_phase", got.total_phase, want.total_phase)
    else:
        assert dl <= parity.SOFT_TOL, (name, "llr", dl)
        assert dv <= parity.SOFT_TOL, (name, "level", got.level, want.level)
        assert dp <= phase_tol(want.n_symbols), (name, "total_phase", got.total_phase, want.total_phase)


def run(p, gardner, exact=False):
    """The whole corpus in one call of irdm_qpsk_demod_batch on the context p (an irdm.Pipeline made with use_gardner =
    gardner), each record against the oracle.  exact: the product runs on the host's libm (the emulation): soft outputs bit
    for bit.  Every mismatch is collected.  Returns dict(cases, accepted, worst)."""
    cs = cases()
    ref = reference(gardner)
    got = p.qpsk_demod_batch([c.iq for c in cs], [c.direction for c in cs])
    worst = dict(llr=0.0, level=0.0, total_phase=0.0, total_phase_hz=0.0)
    failures = []
    for c, g, (ok, want, _) in zip(cs, got, ref):
        try:
            check(c.name, g, ok, want, exact, worst)
        except AssertionError as e:
            failures.append(str(e))
    assert not failures, "%d of %d cases differ from the oracle, gardner %d:\n%s" % (len(failures), len(cs), gardner,
                                                                                 "\n".join(failures))
    return dict(cases=len(cs), accepted=sum(1 for ok, _, _ in ref if ok), worst=worst)


def record_bytes(d):
    """the whole record, for the GPU-against-GPU comparisons"""
    return bytes(d)


def run_packed(p, keep_bits, full):
    """the corpus through irdm_qpsk_demod_packed_batch on p; `full`: irdm_qpsk_demod_batch's records of the same frames on
    the same context.  What the packed record path exports is what the full path computes."""
    cs = cases()
    packed, kept = p.qpsk_demod_packed_batch([c.iq for c in cs], [c.direction for c in cs], keep_bits)
    assert len(packed) == len(cs) and (kept is not None) == bool(keep_bits)
    failures = []
    seen = set()
    for i, (c, q, f) in enumerate(zip(cs, packed, full)):
        try:
            assert q.ok == f.ok, "ok"
            for fld in ("direction", "confidence", "n_symbols", "n_payload_symbols", "n_bits"):
                assert getattr(q, fld) == getattr(f, fld), fld
            assert u32(q.level) == u32(f.level) and u32(q.total_phase) == u32(f.total_phase), "level / total_phase"
            bits = np.frombuffer(bytes(q.bits), np.uint8)
            if not f.ok:
                assert not bits.any(), "a rejected frame's bit words are not zero"
            else:
                nb = f.n_bits
                want = np.packbits(np.frombuffer(bytes(f.bits), np.uint8)[:nb])         # (MSB first, zero-filled last byte)
                assert np.array_equal(bits[:len(want)], want), "bits"
                assert not bits[len(want):].any(), "bits behind n_bits"
                seen.add(f.n_symbols)
            if keep_bits:
                k = kept[i]
                assert bytes(k)[:orc.Demod.llr.offset] == bytes(f)[:orc.Demod.llr.offset], "full_out's scalars and bits"
                assert bytes(k.llr) == bytes(f.llr), "full_out's LLRs"
        except AssertionError as e:
            failures.append("%s: %s" % (c.name, e))
    assert not failures, "%d of %d packed records (keep_bits %d) differ from the full records:\n%s" % (
        len(failures), len(cs), keep_bits, "\n".join(failures))
    return seen
