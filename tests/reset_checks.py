"""TEST INFRASTRUCTURE: what the irdm_reset tests share (tests/test_reset_emul.py through tests/reset_emul_run.py on the
CPU emulation, tests/test_gpu_reset.py on the card): the two scenes, a feeder for an EXISTING context, the record queues as
bytes, and the checks themselves.  Every comparison is between two runs of the same library on the same device (or against
the oracle through tests/parity.py), so equal means byte for byte."""
import ctypes as C

import numpy as np

import irdm
import siggen

T0_A = 1700000000 * 10**9
T0_B = 1711111111 * 10**9 + 123456789
CF_A = 1622000000.0
CF_B = 1625250000.0          # (below 1626 MHz: the frame-length rules of duplex frames, as for A)
FULL = {"keep_frame_samples": 1}
PACKED = {"packed_records": 1, "parsed_records": 1, "frame_records": 1}


def nfft_of(fs):
    return 1 << int(round(np.log2(fs / 1000.0)))


def dirty_scene(fs, seed=31):
    """Stream A, chosen to leave a context dirty: a wave of more carriers than max_bursts (squelch, squelch_count past
    10: the noise-floor history is reset and the detector primes again, burst_detect.c:594-631), a few bursts after the
    re-priming, and the end of the stream in the middle of the last of them, not on a feed-block boundary: a burst still
    active at the end (never emitted), a ragged last chunk, burst ids and the history index far from their start values."""
    n_f = nfft_of(fs)
    rng = np.random.default_rng(seed)
    first = 530 * n_f
    k = int(fs / 2 / (1e6 / 24.0) * 0.92)
    chans = [c for c in range(-k, k + 1) if c != 0]
    assert len(chans) > int(fs / 40000.0 * 0.8)            # more than max_bursts
    bursts = [dict(start=first + 4000 + 37 * i, freq_hz=siggen.channel_freq(ch), payload=rng.integers(0, 4, 150).tolist(), amp=0.03)
              for i, ch in enumerate(chans)]
    second = first + 4000 + 20 * n_f + 530 * n_f
    for i, ch in enumerate((7, -11, 16, -5)):
        bursts.append(dict(start=second + 20 * n_f * i, freq_hz=siggen.channel_freq(ch), payload=rng.integers(0, 4, 150).tolist()))
    n = second + 60 * n_f + 3 * n_f + 1234             # three frames into the fourth burst
    return siggen.make_stream(fs, n, bursts, seed=seed)[0]


def plain_scene(fs, seed=5, secs=None, n_bursts=6):
    """Stream B: another scene (tests/emul_pipeline_run.py's kind), a whole number of feed blocks"""
    n_f = nfft_of(fs)
    secs = secs if secs is not None else (600 * n_f + 0.45 * fs) / fs
    n = int(secs * fs) // 32768 * 32768
    return siggen.standard_scene(fs, n, n_bursts, seed=seed)[0]


def as_format(iq, fmt):
    return iq if fmt == irdm.FMT_CF32 else siggen.to_ci8(iq)


def n_samples(x, fmt):
    return len(x) if fmt == irdm.FMT_CF32 else len(x) // 2


def chunks_of(n, parts):
    """n samples in `parts` chunks of whole feed blocks, the remainder (a ragged end) on the last"""
    blocks = n // 32768
    cuts = [blocks * (i + 1) // parts for i in range(parts)]
    out, prev = [], 0
    for c in cuts:
        if c > prev:
            out.append((c - prev) * 32768)
            prev = c
    if n % 32768:
        out[-1] += n % 32768
    return out


def make(fs, fmt, depth, max_chunk, options, cf=CF_A, t0=T0_A):
    p = irdm.Pipeline(fs, fmt=fmt, center_frequency=cf, start_time_ns=t0, max_chunk_samples=max_chunk, max_bursts_per_chunk=1024,
                      pipeline_depth=depth)
    for k, v in options.items():
        p.set_option(k, v)
    return p


def feed(p, x, fmt, chunks, between=None, only_first=False):
    """x through the existing context p.  pipeline_depth 0: irdm_feed_begin / _end per chunk from device buffers;
    otherwise every chunk written in place (irdm_ingest_ptr) and fed with one chunk of look-ahead.  between: called once,
    between an irdm_feed_begin and its irdm_feed_end.  only_first: the first chunk alone, no flush."""
    L = irdm.lib()
    per = 1 if fmt == irdm.FMT_CF32 else 2
    depth = p.cfg.pipeline_depth
    held, off, pending = [], 0, 0
    sizes = list(chunks[:1] if only_first else chunks)

    def begin(c):
        nonlocal off
        part = np.ascontiguousarray(x[off * per:(off + c) * per])
        if depth:
            ptr = p.ingest_ptr(c)
            assert ptr, "irdm_ingest_ptr refused a chunk of %d samples" % c
            assert L.irdm_device_upload(C.c_void_p(ptr), part.ctypes.data_as(C.c_void_p), part.nbytes) == 0
            held.append(None)
        else:
            ptr = irdm.device_buffer(part)
            held.append(ptr)
        p.feed_begin(ptr, c)
        off += c

    def end():
        nonlocal between
        if between is not None:
            between()
            between = None
        p.feed_end()
        ptr = held.pop(0)
        if ptr:
            irdm.device_free(ptr)

    ahead = 1 if depth else 0
    for c in sizes:
        begin(c)
        pending += 1
        if pending > ahead:
            end()
            pending -= 1
    while pending:
        end()
        pending -= 1
    if only_first:
        return
    assert off == n_samples(x, fmt)
    if depth:
        p.flush()


def queues(p):
    """every record queue drained, as bytes, with the two counters a stream's end prints"""
    infos, samples = p.poll_frames()
    return dict(bursts=b"".join(bytes(r) for r in p.poll_bursts()),
                infos=b"".join(bytes(r) for r in infos),
                samples=b"".join(np.ascontiguousarray(s).tobytes() for s in samples),
                demods=b"".join(bytes(r) for r in p.poll_demods()),
                packed=b"".join(bytes(r) for r in p.poll_demods_packed()),
                ida_packed=b"".join(bytes(r) for r in p.poll_ida_packed()),
                frame_packed=b"".join(bytes(r) for r in p.poll_frame_packed()),
                tagged=int(p.tagged), n_samples=int(p.sample_count))


def same(got, want, what):
    assert set(got) == set(want)
    for k in want:
        assert got[k] == want[k], "%s: queue %r differs (%s)" % (what, k, (len(got[k]), len(want[k])) if isinstance(want[k], bytes) else (got[k], want[k]))
    return {k: (len(v) if isinstance(v, bytes) else v) for k, v in want.items()}


def state_fields(blob):
    """(index, burst_id, hist_idx, primed, squelch, n_act) of the DetState inside an irdm_export_state blob"""
    head = 6 * 8 + 2 * 4
    idx, bid = np.frombuffer(blob[head:head + 16].tobytes(), np.uint64)
    h, pr, sq, na = np.frombuffer(blob[head + 16:head + 32].tobytes(), np.int32)
    return int(idx), int(bid), int(h), int(pr), int(sq), int(na)


def fresh_run(fs, fmt, depth, options, x, chunks, max_chunk, cf, t0, want_state=False):
    p = make(fs, fmt, depth, max_chunk, options, cf, t0)
    try:
        st0 = p.export_state() if want_state else None
        feed(p, x, fmt, chunks)
        st1 = p.export_state() if want_state else None
        return queues(p), st0, st1
    finally:
        p.close()


def check_reuse(fs, fmt, depth, options, a, b, parts_a, parts_b, mid_stream=False, refused=False, states=False, thrice=False):
    """create; feed A; flush; poll; reset; feed B; flush  ==  create; feed B; flush on a fresh context, queue by queue.
    mid_stream: the reset comes after A's first chunk, nothing flushed or polled.  refused: an irdm_reset between an
    irdm_feed_begin and its irdm_feed_end of B returns -1 and changes nothing.  states: irdm_export_state right after
    the reset and after B against the fresh context's.  thrice: A again behind B equals the first A."""
    na, nb = n_samples(a, fmt), n_samples(b, fmt)
    ca, cb = chunks_of(na, parts_a), chunks_of(nb, parts_b)
    mc = max(ca + cb)              # (the same irdm_config_t for both contexts)
    want_b, st0, st1 = fresh_run(fs, fmt, depth, options, b, cb, mc, CF_B, T0_B, want_state=states)
    res = {}
    p = make(fs, fmt, depth, mc, options, CF_A, T0_A)
    try:
        if mid_stream:
            feed(p, a, fmt, ca, only_first=True)
        else:
            feed(p, a, fmt, ca)
            if states:
                f = state_fields(p.export_state())
                # (the context is dirty: a burst still active at the end, ids and the history index advanced)
                assert f[5] >= 1 and f[1] > 0 and f[0] > 0 and f[3] == 1, f
                res["dirty_state"] = f
            first_a = queues(p)
            assert first_a["n_samples"] == na and first_a["tagged"] >= 3, (first_a["tagged"], first_a["n_samples"])
            res["a_tagged"] = first_a["tagged"]
        p.reset(CF_B, T0_B)
        assert p.tagged == 0 and p.sample_count == 0
        if states:
            assert np.array_equal(p.export_state(), st0), "irdm_export_state after the reset differs from a fresh context's"
        rcs = []
        feed(p, b, fmt, cb, between=(lambda: rcs.append(irdm.lib().irdm_reset(p.h, CF_A, T0_A))) if refused else None)
        if refused:
            assert rcs == [-1], rcs
        if states:
            assert np.array_equal(p.export_state(), st1), "irdm_export_state after B differs from the fresh context's"
        res["b"] = same(queues(p), want_b, "B behind a reset")
        assert res["b"]["tagged"] >= 3
        if thrice:
            p.reset(CF_A, T0_A)
            feed(p, a, fmt, ca)
            res["a_again"] = same(queues(p), first_a, "A behind B behind A")
        res["resets"] = p.stat("resets")
    finally:
        p.close()
    return res


def check_oracle(fs, depth, b, parts_b, a):
    """B's records behind a reset against the oracle's for B, by the rules of tests/parity.py"""
    import orc
    import parity
    ca, cb = chunks_of(len(a), 3), chunks_of(len(b), parts_b)
    p = make(fs, irdm.FMT_CF32, depth, max(ca + cb), FULL)
    try:
        feed(p, a, irdm.FMT_CF32, ca)
        p.reset(CF_B, T0_B)
        feed(p, b, irdm.FMT_CF32, cb)
        bursts = p.poll_bursts()
        infos, samples = p.poll_frames()
        got = dict(bursts=bursts, infos=infos, samples=samples, demods=p.poll_demods(), tagged=p.tagged)
    finally:
        p.close()
    return parity.compare(got, orc.run_stream(b, fs, center_frequency=CF_B, start_time_ns=T0_B))


def check_frontend(fs_in=4_000_000, D=2, fmt=irdm.FMT_CI8):
    """run A; finish; reset; run B == a fresh front end's B (and the plain C model's), A ending on a partial block"""
    import frontend_model as fm
    shift = 0.31 * fs_in / D
    na, nb = 3 * 4096 * D + 777, 2 * 4096 * D + 5
    xa, xb = fm.random_capture(fmt, na, seed=1), fm.random_capture(fmt, nb, seed=2)
    st = fm.Stage(fs_in, fmt, D, shift)
    try:
        taps = st.fe.taps()
        want_b = fm.run(xb, fmt, D, fm.quantise(shift, fs_in), taps)
        got_a = st.run(xa, fm.block_feeds(na, 4096 * D))
        assert irdm.lib().irdm_frontend_run_device(st.fe.h, None, 0, C.c_void_p(1), 0, None) == -1       # finished: refused
        st.fe.reset()
        got_b = st.run(xb, fm.ragged_feeds(nb, st.fe.ntaps, (997,)))
    finally:
        st.close()
    st = fm.Stage(fs_in, fmt, D, shift)
    try:
        fresh_b = st.run(xb, [nb])
    finally:
        st.close()
    assert fm.same_bits(got_a, fm.run(xa, fmt, D, fm.quantise(shift, fs_in), taps))
    assert fm.same_bits(got_b, fresh_b) and fm.same_bits(got_b, want_b)
    return dict(a=len(got_a), b=len(got_b))


# ---- the binary: several recordings per run ----
def run_cli(exe, args, timeout=600):
    import subprocess
    r = subprocess.run([exe] + [str(a) for a in args], capture_output=True, timeout=timeout)
    return r.returncode, r.stdout, r.stderr.decode("latin-1")


def summary(err):
    """a run's own stderr lines (the library's create-time diagnostics, 'irdm_hip: ...', come once per process)"""
    return [l for l in err.splitlines() if not l.startswith("irdm_hip")]


def check_cli_batch(exe, tmp, files, times, common, modes):
    """--files-from with start times against the single-file runs with --start-time: stdout the concatenation, the per-file
    stderr lines likewise; with --out-dir one file each with those contents.  files: paths; common: the options every run
    takes; modes: lists of further options, each checked."""
    import os
    lst = os.path.join(tmp, "list.txt")
    with open(lst, "w") as fh:
        for path, t in zip(files, times):
            fh.write("%s %s\n" % (path, t))
    res = {}
    for mode in modes:
        singles = []
        for path, t in zip(files, times):
            rc, out, err = run_cli(exe, ["-f", path, "--start-time", t] + common + mode)
            assert rc == 0, (mode, path, err[-2000:])
            singles.append((out, summary(err)))
        if mode == modes[0]:
            assert all(len(o) > 0 for o, _ in singles) and len({o for o, _ in singles}) == len(singles)   # (the recordings differ)
        rc, out, err = run_cli(exe, ["--files-from", lst] + common + mode)
        assert rc == 0, (mode, err[-2000:])
        assert out == b"".join(o for o, _ in singles), "stdout of the batch run is not the concatenation (%s)" % mode
        assert summary(err) == sum((e for _, e in singles), []), (mode, summary(err), [e for _, e in singles])
        # the same with -f given three times: the first recording's time by --start-time, the others at the wall clock --
        # their lines differ in the timestamps only, so here the burst counts are compared
        rc, out2, err2 = run_cli(exe, sum((["-f", p] for p in files), []) + ["--start-time", times[0]] + common + mode)
        assert rc == 0 and out2.startswith(singles[0][0]), mode
        assert [l for l in err2.splitlines() if "tagged" in l] == [l for l in err.splitlines() if "tagged" in l], mode
        res[" ".join(mode) or "raw"] = [len(o) for o, _ in singles]
    # --out-dir: one file per recording
    od = os.path.join(tmp, "outs")
    rc, out, err = run_cli(exe, ["--files-from", lst, "--out-dir", od] + common + modes[0])
    assert rc == 0 and out == b"", err[-2000:]
    for path, t in zip(files, times):
        rc, want, _ = run_cli(exe, ["-f", path, "--start-time", t] + common + modes[0])
        assert open(os.path.join(od, os.path.basename(path) + ".out"), "rb").read() == want, path
    # --timing / -v: a line that names the file and its reset time, for every recording behind the first
    rc, out, err = run_cli(exe, ["--files-from", lst, "--timing", "-v"] + common + modes[0])
    assert rc == 0
    for path in files[1:]:
        assert "irdm timing: %s: reset " % path in err and "%s: context reset in " % path in err, err[-3000:]
    assert err.count("irdm timing: startup ") == 1
    return res


def check_cli_refusals(exe, tmp, files, common):
    """what is refused before anything is processed (exit 2, nothing on stdout), and a missing middle file (exit 1, the
    other two outputs intact)"""
    import os
    import shutil
    other = os.path.join(tmp, "other_format.ci16")
    shutil.copy(files[0], other)
    for args in (["-f", files[0], "-f", other], ["-f", files[0], "-f", files[1], "--gpus", "2"], ["-f", "-", "-f", files[1]]):
        rc, out, err = run_cli(exe, args + common)
        assert rc == 2 and out == b"", (args, rc, err[-1000:])
    t = "1700000123.5"
    lst = os.path.join(tmp, "missing.txt")
    with open(lst, "w") as fh:
        fh.write("%s %s\n%s %s\n%s %s\n" % (files[0], t, os.path.join(tmp, "no_such_file.cf32"), t, files[2], t))
    rc, out, err = run_cli(exe, ["--files-from", lst] + common)
    want = b""
    for path in (files[0], files[2]):
        r1, o1, _ = run_cli(exe, ["-f", path, "--start-time", t] + common)
        assert r1 == 0 and len(o1) > 0
        want += o1
    assert rc == 1 and out == want and "no_such_file.cf32" in err, (rc, err[-1000:])
