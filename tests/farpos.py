"""TEST INFRASTRUCTURE: the pipeline "at" a stream position K without a stream of K samples.

The position is a number the C-ABI lets a caller set: irdm_export_state / irdm_import_state carry total_samples,
DetState.index and every active burst's start / last_active, and irdm_seed_history(p, tail, n, abs_start) places the
history ring.  Context A is fed [0, cut) of a scene; its blob, with those fields moved up by K (shift_state), goes to a
context B whose history is seeded at cut + K; B is fed the rest.  B's records, moved down again (unshift), must be the
oracle's for the unshifted scene under tests/parity.py's rules, unchanged.

K is a multiple of 32768: a burst's avail_end is the sample count at its extraction on the reference's 32768-sample feed
grid, and that grid is anchored at absolute 0 -- another K moves every avail_end by 32768 - K mod 32768, correctly.

Layout of the blob (csrc/state.cpp: StateHeader, six u64 and two i32; csrc/types.hpp: DetState, ActiveBurst), restated as
ctypes structures below; tests/test_farpos_emul.py checks the offsets shift_state uses against them."""
import ctypes as C

import numpy as np

import irdm
import parity

GRID = 32768
K_MAX_ACTIVE = 1024          # types.hpp: kMaxActive
MAX_POSITION = 1 << 53       # include/irdm_hip.h: IRDM_MAX_POSITION


class StateHeader(C.Structure):
    _fields_ = [("magic", C.c_uint64), ("n", C.c_uint64), ("hist", C.c_uint64), ("total_samples", C.c_uint64),
                ("tagged", C.c_uint64), ("start_time_ns", C.c_uint64), ("host_primed", C.c_int32), ("host_hist_idx", C.c_int32)]


class ActiveBurst(C.Structure):
    _fields_ = [("id", C.c_uint64), ("start", C.c_uint64), ("last_active", C.c_uint64), ("center_bin", C.c_int32),
                ("peak_rel", C.c_float), ("base_sum", C.c_float), ("pad", C.c_int32)]


class DetState(C.Structure):
    _fields_ = [("index", C.c_uint64), ("burst_id", C.c_uint64), ("hist_idx", C.c_int32), ("primed", C.c_int32),
                ("squelch", C.c_int32), ("n_act", C.c_int32), ("n_gone", C.c_uint32), ("overflow", C.c_uint32),
                ("act", ActiveBurst * K_MAX_ACTIVE)]


# bytes from the start of the blob
OFF_TOTAL, OFF_INDEX, OFF_N_ACT, OFF_ACT, ACT_SIZE, ACT_START, ACT_LAST = 24, 56, 84, 96, 40, 8, 16
HEAD_BYTES = 56 + 40 + ACT_SIZE * K_MAX_ACTIVE          # header + DetState


def _u64(blob, off):
    return int(blob[off:off + 8].view(np.uint64)[0])


def _add(blob, off, K):
    v = _u64(blob, off) + K
    assert 0 <= v < 1 << 64
    blob[off:off + 8] = np.array([v], np.uint64).view(np.uint8)


def position_offsets(blob):
    """byte offsets of every stream position in a state blob"""
    n_act = int(blob[OFF_N_ACT:OFF_N_ACT + 4].view(np.int32)[0])
    assert 0 <= n_act <= K_MAX_ACTIVE
    offs = [OFF_TOTAL, OFF_INDEX]
    for i in range(n_act):
        offs += [OFF_ACT + ACT_SIZE * i + ACT_START, OFF_ACT + ACT_SIZE * i + ACT_LAST]
    return offs


def shift_state(blob, K):
    """a copy of the blob with every stream position moved by K (negative: back); burst ids, sums, history and
    start_time_ns are copied"""
    out = np.array(blob, np.uint8, copy=True)
    for off in position_offsets(out):
        _add(out, off, K)
    return out


def live_bytes(blob):
    """a copy of the blob with the entries of DetState.act behind n_act zeroed: bursts that have gone leave their records
    there, positions included, and nothing reads them"""
    out = np.array(blob, np.uint8, copy=True)
    n_act = int(out[OFF_N_ACT:OFF_N_ACT + 4].view(np.int32)[0])
    out[OFF_ACT + ACT_SIZE * n_act:HEAD_BYTES] = 0
    return out


def _configure(p, packed, scan_mode, options):
    p.set_option("packed_records" if packed else "keep_frame_samples", 1)
    p.set_option("scan_mode", scan_mode)
    for k, v in (options or {}).items():
        p.set_option(k, v)


def _drain(p, packed):
    infos, samples = p.poll_frames()
    return dict(bursts=p.poll_bursts(), infos=infos, samples=samples, demods=p.poll_demods(),
                packed=p.poll_demods_packed() if packed else [])


def _take_over(fs, fmt, iq, at, K, blob, sizes, depth, packed, scan_mode, options):
    """a fresh context that takes the stream over at sample `at`, moved to at + K: history seeded with the format's own
    bytes, the blob imported as it is"""
    per = 1 if fmt == irdm.FMT_CF32 else 2
    p = irdm.Pipeline(fs, fmt=fmt, max_chunk_samples=max(sizes), max_bursts_per_chunk=1024, pipeline_depth=depth)
    _configure(p, packed, scan_mode, options)
    ov = min(at, int(p.L.irdm_required_overlap(p.h)))
    p.seed_history(iq[(at - ov) * per:at * per], at + K)
    p.import_state(blob)
    return p


def run_shifted(iq, fs, cut, K, fmt=irdm.FMT_CF32, depth=0, chunks=None, feed="host", packed=False, options=None, scan_mode=0,
                cut2=None, want_state=False):
    """Context A (pipeline_depth 0) takes [0, cut), as in test_time_chunk_handoff_equals_single_context; B gets
    irdm_seed_history at cut + K and A's blob shifted by K, and the rest in `chunks` (sample counts; default: whole) in
    parity.feed_chunks' feed form.  K may be a function of B's ring length (irdm_ring_ptr).
    cut2: B stops there and exports; a third context C is seeded at cut2 + K, imports B's blob UNPATCHED and takes the rest
    (`chunks` are then C's; B is fed [cut, cut2) whole).
    Returns A's and B's (and C's) records merged -- B's and C's at their shifted positions: see unshift() -- with K, the
    records of B and C alone ("far"), the last context's statistics and ring length, and with want_state its final
    irdm_export_state."""
    per = 1 if fmt == irdm.FMT_CF32 else 2
    n = len(iq) // per
    assert cut % GRID == 0 and 0 < cut < n and (cut2 is None or (cut2 % GRID == 0 and cut < cut2 < n))
    a = irdm.Pipeline(fs, fmt=fmt, max_chunk_samples=cut, max_bursts_per_chunk=1024)
    _configure(a, packed, scan_mode, options)
    a.feed_host(iq[:cut * per])
    parts = [_drain(a, packed)]
    blob = a.export_state()
    assert len(blob) == a.state_bytes()
    a.close()
    last = n if cut2 is None else cut2
    sizes_b = list(chunks) if chunks and cut2 is None else [last - cut]
    assert sum(sizes_b) == last - cut
    b = irdm.Pipeline(fs, fmt=fmt, max_chunk_samples=max(sizes_b), max_bursts_per_chunk=1024, pipeline_depth=depth)
    _configure(b, packed, scan_mode, options)
    if callable(K):
        K = K(b.ring()[1])
    assert K % GRID == 0 and (K == 0 or K > n)
    ov = min(cut, int(b.L.irdm_required_overlap(b.h)))
    b.seed_history(iq[(cut - ov) * per:cut * per], cut + K)
    b.import_state(shift_state(blob, K))
    assert parity.feed_chunks(b, iq, fmt, sizes_b, feed if cut2 is None else "host", off=cut, past_ring_end="buffer") == last
    if depth:
        b.flush()
    parts.append(_drain(b, packed))
    p = b
    if cut2 is not None:
        blob_b = b.export_state()
        b.close()
        sizes_c = list(chunks or [n - cut2])
        assert sum(sizes_c) == n - cut2
        p = _take_over(fs, fmt, iq, cut2, K, blob_b, sizes_c, depth, packed, scan_mode, options)
        assert parity.feed_chunks(p, iq, fmt, sizes_c, feed, off=cut2, past_ring_end="buffer") == n
        if depth:
            p.flush()
        parts.append(_drain(p, packed))
    res = {k: [r for part in parts for r in part[k]] for k in parts[0]}
    res["far"] = {k: [r for part in parts[1:] for r in part[k]] for k in parts[0]}
    res.update(K=K, tagged=p.tagged, n_samples=p.sample_count, ring_len=p.ring()[1],
               stats={k: p.stat(k) for k in parity.STAT_KEYS})
    if want_state:
        res["state"] = p.export_state()
    p.close()
    return res


def timestamp_shift(start, K, fs):
    """what K adds to the timestamp of every frame of the burst that starts at `start` (unshifted): the reference's
    start_time + (uint64_t)((double)start / sample_rate * 1e9) evaluated at start + K and at start, in binary64 as there"""
    return int(float(start + K) / fs * 1e9) - int(float(start) / fs * 1e9)


def unshift(res, K, fs):
    """run_shifted()'s records moved back by K, in place, for parity.compare / compare_packed: start, stop, last_active and
    avail_end of every burst that lies at a shifted position (start >= K; K is larger than the scene), the sample count,
    and the timestamp of each frame / demodulated frame / packed record of such a burst."""
    if not K:
        return res
    assert res["n_samples"] > K
    res["n_samples"] -= K
    dt = {}
    for b in res["bursts"]:
        if b.start >= K:
            for f in ("start", "stop", "last_active", "avail_end"):
                assert getattr(b, f) >= K, (f, b.id)
                setattr(b, f, getattr(b, f) - K)
            dt[b.id] = timestamp_shift(b.start, K, fs)
    for f in res["infos"]:
        if f.drop_reason == 0 and f.id in dt:
            f.timestamp -= dt[f.id]
    for key in ("demods", "packed"):
        for d in res[key]:
            if d.id in dt:
                d.timestamp -= dt[d.id]
    return res


def cut_inside_a_burst(ref, fft_size, which=0):
    """a multiple of 32768 behind the priming frames and inside the window of one of the oracle's bursts: the which-th of
    the bursts whose window holds one"""
    found = []
    for rb in ref.bursts:
        mid = (rb.start + rb.num_samples // 2) // GRID * GRID
        for c in (mid, mid + GRID):
            if rb.start < c < rb.start + rb.num_samples and c > 520 * fft_size:
                if not found or c > found[-1]:
                    found.append(int(c))
                break
    assert len(found) > which, "too few burst windows of the scene hold a multiple of 32768"
    return found[which]


def k_straddling(ref, cut, power):
    """K, a multiple of 32768, so that 2^power falls inside the shifted window of a burst that the context behind `cut`
    emits: start + K < 2^power <= start + num_samples + K.  The burst's window must hold a multiple of 32768; of the bursts
    that begin behind the cut the middle one is taken, so that the position is crossed inside the feed."""
    holds = [(rb, (rb.start + rb.num_samples) // GRID * GRID) for rb in ref.bursts]
    holds = [(rb, m) for rb, m in holds if m > rb.start]
    later = [m for rb, m in holds if rb.start > cut]
    if later:
        return (1 << power) - int(later[len(later) // 2])
    across = [m for rb, m in holds if rb.start + rb.num_samples > cut]
    assert across, "no burst behind the cut holds a multiple of 32768 in its window"
    return (1 << power) - int(across[0])


def straddles(bursts, power):
    """(a): one of the bursts, at its shifted position, has start < 2^power <= start + num_samples"""
    return any(b.start < (1 << power) <= b.start + b.num_samples for b in bursts)


# ---- the front ends: irdm_frontend_seek ----

def fe_outputs(total, L, M, ntaps):
    """csrc/frontend.cpp: outputs complete once `total` input samples are in"""
    c = (ntaps - 1) // 2
    return (total * L - 1 - c) // M + 1 if total * L > c else 0


def fe_period(M):
    """input positions that agree modulo this give the same outputs: the rotator's index has period 65536 samples, the
    polyphase schedule M"""
    import math
    return 65536 * M // math.gcd(65536, M)


def fe_seek_position(power, M, n, r):
    """P = r modulo fe_period(M): near 2^32 so that 2^32 is crossed inside a run of n samples from P on, else the first
    such position from 2^power on"""
    per = fe_period(M)
    if power != 32:
        return -(-(1 << power) // per) * per + r
    base = ((1 << 32) - n // 2) // per * per
    if base + r + n <= 1 << 32:
        base = (1 << 32) // per * per
    assert base + r < 1 << 32 < base + r + n, (M, n, r)
    return base + r


def lead_in(x, fmt, r):
    """zeros(r) ++ x in the format's own codes"""
    x = np.ascontiguousarray(x)
    return np.concatenate([np.zeros(r if fmt == irdm.FMT_CF32 else 2 * r, x.dtype), x])
