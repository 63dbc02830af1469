"""TEST INFRASTRUCTURE: the band scan's decline and redo paths in MID-STREAM -- scenes, runners and assertions shared by
tests/test_decline_emul.py (through tests/decline_emul_run.py, on the CPU emulation) and tests/test_gpu_decline.py (on the
card).

The band scan speculates: a chunk it cannot carry it declines, leaving the carried state untouched, and the sequential
kernels redo the chunk (scan_finish, csrc/scan_host.cpp).  Every case here puts the event that makes it decline behind
chunks the band scan has committed, and in front of chunks it must take back, and runs the stream at pipeline_depth 0 and 1
(irdm_feed_host per chunk) and at depth 2 and 3 (4 for the capacity cases) fed in place with one chunk of look-ahead -- at
10 MHz with the next chunk's scan chained behind the one that declines and its round 0 taken by a speculation pass --, with
the full records and with packed_records.  Every run is held to

  * the oracle, by tests/parity.py: every burst, frame sample bit for bit, hard bit and LLR, in the oracle's order;
  * the path it claims: the decline's flag in band_last_flags (read after every feed), band_aborts / band_retries, at 10 MHz
    with look-ahead scan_chained >= 3, spec_scans >= 3 and scan_chain_undone >= 1, and band_chunks still rising behind the
    event: the band scan took the stream back;
  * the carried state after the flush -- (index, burst_id, hist_idx, primed, squelch, n_act) of the exported DetState and
    the baseline sums bit for bit -- of a second context that ran the same chunks with the dense kernel (scan_mode 1) at
    depth 0.

Cases (CASES below; bursts / frames are the oracle's, pinned with each stream's digest in PINS):
  click_0.5     10 MHz, 17 chunks of 16 blocks, ONE sample of chunk 11 raised by 0.5: 161 bursts born in one frame -- below
                max_bursts (200), so no squelch; a candidate list overflows (BAND_F_LIST, 4), the sparse scan's 64 lanes
                overflow too and the dense kernel ends up with the chunk
  click_2.0     the same with 2.0: the squelch dumps the wave (10 bursts); the list has overflowed before the scan can tell
  drop_10m      10 MHz, the ten bursts alone, every sample from the click's index on times 0.25: no abort; fed with
                look-ahead the chunk does not settle on its own and the scan chained behind it is undone
  squelch_late  2 MHz, 13 chunks of 16 blocks, scenes.squelch's wave in chunk 4 behind seven committed bursts, one burst
                still active when it starts, six behind the re-priming (BAND_F_SQUELCH, 16)
  drop_2m       2 MHz, 17 chunks of 10 blocks, times 0.25 from the middle of chunk 10 on: band_retries >= 1
  cap_2m        2 MHz, 24 bursts, max_bursts_per_chunk 2, chunks of 10 blocks: chunk 4 ends four bursts -- the commit turns
                the accepted round into a decline (BAND_F_GONECAP, 256), the sequential redo overflows as well, the record
                buffer grows by 4096 and the dense kernel redoes the chunk; burst_cap stays 2, so chunks 7, 9 and 11 are
                worked off batch by batch in deferred_enqueue with no redo.  Records must leave in stream order all the same
                (they did not at pipeline_depth >= 2 before this module was added: 0 1 2 3 5 6 4 7 8 11 12 9 10 ...)
  cap_10m       10 MHz, the ten bursts, max_bursts_per_chunk 2, ten chunks of 16 blocks and then chunks of 32: chunks 10 and
                12 end three bursts each; the first declines at its commit with a chained scan behind it
  rot_*         the scan form changed before every feed (option scan_mode: band, dense, sparse on one workgroup, sparse on
                several) on scenes.random_scene(3), (7) and scenes.many_active_10m(), a burst alive across every chunk boundary:
                the DetState the band commit writes is continued by the dense and sparse kernels and the other way round.
                (At depth 2 with look-ahead a chained band scan may be enqueued already when the mode changes: legal.)

Flags no input of this size reaches, and for which no hook is added to the product: BAND_F_SLOTS (24 simultaneous bursts
in one band), BAND_F_RECS (1024 records in a band), BAND_F_TOTAL (8192 records in a chunk), BAND_F_SNAP, BAND_F_ITER (no
fixed point in five rounds), BAND_F_COOP (the cooperative launch's grid barrier timing out).

What the runs took, as check() prints it: band_last_flags ORed over the stream's declines, band_aborts, band_retries,
band_extra, scan_fallbacks, scan_chained, spec_scans, scan_chain_undone.  On the MI355X, every configuration; the CPU
emulation runs the configurations tests/test_decline_emul.py names and reported the same eight figures in each of them; the
packed runs took the paths of the full ones throughout.
                                   flags aborts retries extra fallbacks chained spec undone
  click_0.5, click_2.0  depth 0        4      1       0     0         2       0    0      0
                        depth 1        4      1       0     0         2       8    0      1
                        depth 2, 3     4      1       0     1         2       7    7      2
  drop_10m              depth 0        0      0       0     0         0       0    0      0
                        depth 1        0      0       0     0         0       8    0      0
                        depth 2, 3     0      0       0     1         0       7    7      1
  squelch_late          every depth   16      1       1     0         2       0    0      0
  drop_2m               every depth    0      0       2     0         0       0    0      0
  cap_2m                every depth  256      1       0     0         2       0    0      0
  cap_10m               depth 0      256      1       0     0         2       0    0      0
                        depth 1      256      1       0     0         2       5    0      1
                        depth 2 .. 4 256      1       0     1         2       4    4      1
  rot_random3, _random7 every config   0      0       0     0         0       0    0      0   band_chunks 2, 2, 1
  rot_many_10m          depth 0        0      0       0     0         1       0    0      0   band_chunks 9 (the sparse scan gave one
                        depth 1        0      0       0     0         1       2    0      0   band_chunks 9  chunk of the wave to the dense)
                        look-ahead     0      0       0     2         0       7    7      0   band_chunks 13 of 14: the chained scans
  rot_many_10m_pairs    look-ahead     0      0       0     1         0       4    4      0   band_chunks 8
At 2 MHz K1 writes no candidate lists (k1_lists 0), so nothing is chained there: the chained paths are the 10 MHz cases'.
drop_10m makes no list stale -- the chunk's scan needs rounds beyond those enqueued up front (band_extra), which is enough to
undo the scan chained behind it; the band retry is drop_2m's.
"""
import collections
import functools
import hashlib

import irdm
import orc
import parity
import reset_checks
import scenes

BLOCK = 32768
F_LIST, F_STALE, F_SQUELCH, F_GONECAP = 4, 8, 16, 256
CONFIGS = {"depth0": (0, "host"), "depth1": (1, "host"), "depth2": (2, "ingest_lookahead"), "depth3": (3, "ingest_lookahead"),
           "depth4": (4, "ingest_lookahead"), "depth2_lookahead": (2, "lookahead")}
STANDARD = ("depth0", "depth1", "depth2", "depth3")
SNAP_KEYS = ("band_chunks", "band_aborts", "band_retries", "band_last_flags", "scan_fallbacks", "scan_chain_undone")
ROT6 = (0, 1, 2, 0, 3, 1)
ROT8 = (0, 0, 1, 0, 2, 0, 0, 3)
ROT_PAIRS = (0, 0, 1, 1, 0, 2, 2, 0, 3, 3, 0, 0, 2, 1)


def uniform(n, blocks):
    """n samples (whole feed blocks) in chunks of `blocks` feed blocks, the rest a shorter last chunk"""
    assert n % BLOCK == 0
    c = blocks * BLOCK
    return [c] * (n // c) + ([n % c] if n % c else [])


def _cap_10m_sizes(n):
    return [16 * BLOCK] * 10 + uniform(n - 160 * BLOCK, 32)


def _blocks(*sizes):
    return lambda n: [s * BLOCK for s in sizes]


Case = collections.namedtuple("Case", "stream sizes event flag abort retries cap modes configs")


def _case(stream, sizes, event=None, flag=0, abort=False, retries=False, cap=1024, modes=None, configs=STANDARD):
    return Case(stream, sizes, event, flag, abort, retries, cap, modes, configs)


# stream: a key of STREAMS; sizes: stream length -> chunk sizes; event: the sample that makes the scan decline (None: taken
# from the oracle -- the first chunk that ends more bursts than `cap` -- or, for the rotation, none)
CASES = {
    "click_0.5": _case("click_0.5", lambda n: uniform(n, 16), event=scenes.click_index(), flag=F_LIST, abort=True),
    "click_2.0": _case("click_2.0", lambda n: uniform(n, 16), event=scenes.click_index(), flag=F_LIST, abort=True),
    "drop_10m": _case("drop_10m", lambda n: uniform(n, 16), event=scenes.noise_drop_cut(10_000_000)),
    "squelch_late": _case("squelch_late", lambda n: uniform(n, 16), event=530 * 2048 + 1_200_000, flag=F_SQUELCH, abort=True),
    "drop_2m": _case("drop_2m", lambda n: uniform(n, 10), event=scenes.noise_drop_cut(2_000_000), retries=True),
    "cap_2m": _case("crowded", lambda n: uniform(n, 10), flag=F_GONECAP, abort=True, cap=2, configs=STANDARD + ("depth4",)),
    "cap_10m": _case("ten_10m", _cap_10m_sizes, flag=F_GONECAP, abort=True, cap=2, configs=STANDARD + ("depth4",)),
    "rot_random3": _case("random3", _blocks(35, 13, 7, 17, 11, 14), modes=ROT6, configs=("depth0", "depth1", "depth2_lookahead")),
    "rot_random7": _case("random7", _blocks(37, 6, 10, 8, 12, 24), modes=ROT6, configs=("depth0", "depth1", "depth2_lookahead")),
    "rot_many_10m": _case("many_10m", _blocks(133, 2, 2, 2, 40, 4, 2, 4, 4, 4, 2, 4, 4, 21), modes=ROT8,
                          configs=("depth0", "depth1", "depth2_lookahead")),
    "rot_many_10m_pairs": _case("many_10m", _blocks(133, 2, 2, 2, 40, 4, 2, 4, 4, 4, 2, 4, 4, 21), modes=ROT_PAIRS,
                                configs=("depth2_lookahead",)),
}

STREAMS = {
    "click_0.5": lambda: scenes.click(amp=0.5),
    "click_2.0": lambda: scenes.click(amp=2.0),
    "ten_10m": lambda: scenes.click(amp=0),
    "drop_10m": lambda: scenes.noise_drop(10_000_000),
    "squelch_late": scenes.squelch_late,
    "drop_2m": lambda: scenes.noise_drop(2_000_000),
    "crowded": scenes.crowded,
    "random3": lambda: scenes.random_scene(3),
    "random7": lambda: scenes.random_scene(7),
    "many_10m": scenes.many_active_10m,
}

# (rate, samples, sha256 of the samples, the oracle's bursts, its frames that reach the demodulator): the new scenes' bytes
# and what the reference makes of them -- conditions on the INPUT, checked on the CPU (tests/test_decline_emul.py)
PINS = {
    "click_0.5": (10_000_000, 8814592, "316015bff09df5b91141f736eb741994c6b26c17a5f50ab037157a5b896ab750", 171, 170),
    "click_2.0": (10_000_000, 8814592, "d2ba32c9b4939c7d6aa5047c39be1f13a8d94f653fe41816f90ad58c0304efcf", 10, 10),
    "ten_10m": (10_000_000, 8814592, "4828c0bfd206841ed63c3a0696d39f5ef6d0093db22aeec5ec273bb1eacd43ff", 10, 10),
    "drop_10m": (10_000_000, 8814592, "2ade6dec37b35c18828484e8745cee8439a1b124e250412fd7354782bb78f316", 10, 10),
    "squelch_late": (2_000_000, 6553600, "e20d4e79547e9be0b11fbd73fc2b9fdb3ec5b09710b8a2518a142aa01c845b75", 46, 14),
    "drop_2m": (2_000_000, 5570560, "3c95c8b85594ad50fb0e8c9045914469831b20ddb50b7d9f9d4b9e17529bfc43", 10, 10),
    "crowded": (2_000_000, 5570560, "4dd840a80e14b3984b328f5b47502e3fc237a57b3358e20959cd0496229d720a", 24, 24),
}


@functools.lru_cache(maxsize=None)
def stream(key):
    """(fs, samples, the oracle's result): made once per process and never modified"""
    fs, iq = STREAMS[key]()
    iq.setflags(write=False)
    return fs, iq, orc.run_stream(iq, fs)


def check_pin(key):
    """the scene is the bytes it was and the reference sees in it what the case is about"""
    fs, iq, ref = stream(key)
    frames = sum(1 for f in ref.frames if f.drop_reason == 0)
    assert (fs, len(iq), hashlib.sha256(iq.tobytes()).hexdigest(), len(ref.bursts), frames) == PINS[key]
    nfft = scenes.nfft_of(fs)
    max_bursts = int(fs / 40000.0 * 0.8)
    frame, born = collections.Counter(b.start // nfft for b in ref.bursts).most_common(1)[0]
    if key == "click_0.5":
        # more births in the click's frame than the sparse scan has lanes, fewer than the squelch needs: each becomes a record
        # (a burst's start lies two frames in front of the frame that detects it)
        assert 64 < born < max_bursts and frame == scenes.click_index(fs) // nfft - 2, (frame, born)
    elif key in ("click_2.0", "ten_10m", "drop_10m", "drop_2m"):
        assert born == 1
        if key.startswith("drop"):
            cut = scenes.noise_drop_cut(fs)
            assert sum(b.stop < cut for b in ref.bursts) >= 3 and sum(b.start > cut for b in ref.bursts) >= 3
    elif key == "squelch_late":
        wave = 530 * nfft + 1_200_000
        dumped = [b for b in ref.bursts if wave - 9000 <= b.start < wave + 40 * nfft]
        assert len(dumped) >= 30 and max(b.stop - b.start for b in dumped) < 30_000        # (a burst of 150 symbols lasts 14_000)
        assert sum(b.stop < wave - 9000 for b in ref.bursts) == 7 and sum(b.start > wave + 1_000_000 for b in ref.bursts) == 6
    return dict(bursts=len(ref.bursts), frames=frames, most_born_in_a_frame=born)


def chunk_ends(sizes):
    out, off = [], 0
    for c in sizes:
        off += c
        out.append(off)
    return out


def chunk_of(sample, sizes):
    return next(k for k, e in enumerate(chunk_ends(sizes)) if sample < e)


def ended_per_chunk(ref, sizes):
    """how many of the oracle's bursts stop inside each chunk"""
    per = [0] * len(sizes)
    for b in ref.bursts:
        per[chunk_of(b.stop, sizes)] += 1
    return per


class _Tap:
    """what parity.feed_chunks calls of a Pipeline, with option scan_mode set before every feed (modes) and a few counters
    read behind every feed (they are plain reads: nothing is waited for)"""

    def __init__(self, p, modes):
        self.p, self.modes, self.begun, self.snaps = p, modes, 0, []

    def _before(self):
        if self.modes:
            self.p.set_option("scan_mode", self.modes[self.begun % len(self.modes)])
        self.begun += 1

    def snap(self):
        self.snaps.append({k: self.p.stat(k) for k in SNAP_KEYS})

    def feed_host(self, x):
        self._before()
        rc = self.p.feed_host(x)
        self.snap()
        return rc

    def ingest_ptr(self, c):
        return self.p.ingest_ptr(c)

    def feed_begin(self, ptr, c):
        self._before()
        self.p.feed_begin(ptr, c)

    def feed_end(self):
        rc = self.p.feed_end()
        self.snap()
        return rc


def drive(iq, fs, sizes, depth, feed, packed=False, cap=1024, modes=None, scan_mode=0, detect_only=False):
    """The stream through a context of its own; every feed raises on an error.  Returns the records as parity.run_gpu does,
    with `snaps` (SNAP_KEYS behind every feed and, last, behind the flush), `flags` (band_last_flags of every decline, ORed),
    `state` and `base` (the carried state after the flush).  detect_only: the detector alone, burst records only."""
    p = irdm.Pipeline(fs, max_chunk_samples=max(sizes), max_bursts_per_chunk=cap, pipeline_depth=depth)
    try:
        p.set_option("packed_records" if packed else "keep_frame_samples", 1)
        p.set_option("scan_mode", scan_mode)
        p.set_option("detect_only", int(detect_only))
        tap = _Tap(p, modes)
        assert parity.feed_chunks(tap, iq, irdm.FMT_CF32, list(sizes), feed, past_ring_end="buffer") == len(iq)
        if depth:
            p.flush()
        tap.snap()
        bursts = p.poll_bursts()
        infos, samples = p.poll_frames()
        got = dict(bursts=bursts, infos=infos, samples=samples, demods=p.poll_demods(),
                   packed=p.poll_demods_packed() if packed else [], tagged=p.tagged, n_samples=p.sample_count,
                   stats={k: p.stat(k) for k in parity.STAT_KEYS}, snaps=tap.snaps)
        flags, aborts = 0, 0
        for s in tap.snaps:
            if s["band_aborts"] > aborts:
                flags |= s["band_last_flags"]
            aborts = s["band_aborts"]
        got["flags"] = flags
        got["state"] = reset_checks.state_fields(p.export_state())
        got["base"] = p.baseline_sum()
        return got
    finally:
        p.close()


@functools.lru_cache(maxsize=None)
def dense_state(key, sizes):
    """the carried state behind the same chunks (a tuple) on a context that ran the dense kernel alone at depth 0, one
    irdm_feed_host per chunk; its records are held to the oracle as well"""
    fs, iq, ref = stream(key)
    got = drive(iq, fs, sizes, 0, "host", scan_mode=1, detect_only=True)
    assert [(b.id, b.start, b.stop) for b in got["bursts"]] == [(b.id, b.start, b.stop) for b in ref.bursts]
    assert got["stats"]["band_chunks"] == 0 and got["stats"]["scan_fast_chunks"] == 0, got["stats"]
    return got["state"], got["base"].tobytes()


def order_of(bursts):
    return [b.id // 10 for b in bursts]


def check(name, config, packed=False):
    """one case in one configuration; returns its counters"""
    c = CASES[name]
    fs, iq, ref = stream(c.stream)
    sizes = tuple(c.sizes(len(iq)))
    assert sum(sizes) == len(iq)
    depth, feed = CONFIGS[config]
    look = feed.endswith("lookahead")
    ends = chunk_ends(sizes)
    if c.modes:
        # a burst alive across every chunk boundary: each form continues what another one left behind
        for cut in ends[:-1]:
            assert any(b.start < cut < b.stop for b in ref.bursts), cut
    per = ended_per_chunk(ref, sizes)
    crowded = [k for k, m in enumerate(per) if m > c.cap]
    if c.cap < 1024:
        # three bursts and more end in a chunk of a context made for two, at least twice: behind the first the record buffer
        # has grown and the batch buffers have not
        assert len(crowded) >= 2 and per[crowded[0]] >= 3 and crowded[1] >= crowded[0] + 2 and crowded[-1] < len(sizes) - 1, per
    event = chunk_of(c.event, sizes) if c.event is not None else (crowded[0] if c.cap < 1024 else None)
    if event is not None:
        # behind at least two chunks the band scan has committed since the priming frames, and not in the last chunk
        primed = chunk_of(512 * scenes.nfft_of(fs) - 1, sizes)
        # (cap_2m: the chunking of the record-order bug, whose first crowded chunk is the first one behind the priming)
        assert primed + (1 if name == "cap_2m" else 3) <= event < len(sizes) - 1, (primed, event, len(sizes))

    got = drive(iq, fs, sizes, depth, feed, packed=packed, cap=c.cap, modes=c.modes)
    st, snaps = got["stats"], got["snaps"]
    counters = dict(flags=got["flags"], **{k: st[k] for k in ("band_aborts", "band_retries", "band_extra", "scan_fallbacks", "scan_chained",
                                                           "spec_scans", "scan_chain_undone", "band_chunks", "k1_lists")})
    print("decline %s %s%s: %s" % (name, config, " packed" if packed else "", counters))
    if c.cap < 1024 and not packed and order_of(got["bursts"]) != order_of(ref.bursts):
        print("record order (burst id / 10):", " ".join(str(i) for i in order_of(got["bursts"])))
    # 1. the oracle's records, in its order
    summary = (parity.compare_packed if packed else parity.compare)(got, ref)
    assert summary["bursts"] == len(ref.bursts) and got["n_samples"] == len(iq)
    # 2. the path
    if c.flag:
        assert got["flags"] & c.flag, counters
    if c.abort:
        assert st["band_aborts"] >= 1, counters
    if c.retries:
        assert st["band_retries"] >= 1, counters
    if fs == 10_000_000 and look and event is not None:
        assert st["scan_chained"] >= 3 and st["spec_scans"] >= 3 and st["scan_chain_undone"] >= 1, counters
    if event is not None:
        # the event's chunk has settled behind the feed of the next one at every depth: band commits after that
        assert st["band_chunks"] - snaps[event + 1]["band_chunks"] >= 1, (counters, event, [s["band_chunks"] for s in snaps])
    if c.modes:
        # the forms ran: band commits, sparse chunks (scan_fast_chunks counts both), dense frames behind the 512 priming ones.
        # Fed with look-ahead at 10 MHz, a chunk whose scan was chained behind a band scan stays a band scan whatever the
        # option says by then: ROT8 (no two sequential forms in a row) then leaves the sequential kernels one chunk, ROT_PAIRS all
        sparse, dense = st["scan_fast_chunks"] > st["band_chunks"], st["scan_dense_frames"] > 512
        assert st["band_chunks"] >= 1 and (sparse or dense), st
        if not look or c.modes is ROT_PAIRS:
            assert sparse and dense, st
        if look and fs == 10_000_000:
            assert st["scan_chained"] >= 1, st
    if c.cap < 1024:
        assert got["tagged"] == len(ref.bursts)
        k0, k1 = crowded[0], crowded[1]
        grown = snaps[k0 + 1]["scan_fallbacks"] - snaps[k0 - 1]["scan_fallbacks"]
        later = snaps[-1]["scan_fallbacks"] - snaps[k0 + 1]["scan_fallbacks"]
        # the first crowded chunk: the decline at the commit and the redo behind the growth; every later one -- the record
        # buffer holds 4096 more by then -- no redo at all: its bursts go through the batches of deferred_enqueue
        assert grown >= 2 and later == 0 and per[k1] > c.cap, (grown, later, per)
    # 3. the carried state
    state, base = dense_state(c.stream, sizes)
    assert got["state"] == state, (got["state"], state)
    assert got["base"].tobytes() == base
    return dict(counters, bursts=summary["bursts"], demods=summary["demods"], state=list(state))
