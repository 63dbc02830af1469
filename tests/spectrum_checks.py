"""TEST INFRASTRUCTURE: what the tests of option "spectrum_frames" share (tests/test_spectrum_emul.py through
tests/spectrum_emul_run.py on the CPU emulation, tests/test_gpu_spectrum.py on the card): the scenes, the oracle's
magnitude plane as the reference (orc_detector_set_mag_sink: the plane K1 writes equals it bit for bit), the expected rows,
and the checks themselves.

Reference and bounds.  peak[r] must equal plane[r R : (r + 1) R].max(0) exactly.  mean[r] is compared with the float64 mean
of the same rows: with u = 2^-24 and k frames in the row, |mean32 - mean64| <= 1.01 (k + 1) u mean64 per bin -- every
summand is non-negative, so k - 1 fp32 additions in ANY order are off by at most (k - 1) u (1 + O(k u)) relative to the
exact sum, and the one division adds u; nothing here is fitted to what the kernel returns.  For R = 1 both equal the plane."""
import ctypes as C
import os
import struct

import numpy as np

import irdm
import orc
import reset_checks as rc
import siggen

U = 2.0 ** -24
R_CASES = (1, 7, 64, 1 << 20)       # 7: every chunk boundary inside a row; 2^20: more frames than the stream has
ROW = np.dtype([("row", "<u8"), ("first_frame", "<u8"), ("timestamp_ns", "<u8"), ("n_frames", "<u4"), ("n_bins", "<u4")])
_planes = {}


def scene(fs, seed=5, n_bursts=6):
    """reset_checks.plain_scene's size -- 600 frames + 0.45 s, a few bursts -- with a ragged end: one whole frame and 777
    samples past the last feed block"""
    n_f = rc.nfft_of(fs)
    n = int(600 * n_f + 0.45 * fs) // 32768 * 32768 + n_f + 777
    return siggen.standard_scene(fs, n, n_bursts, seed=seed)[0]


def plane_of(x, fs, fmt, key=None):
    """the oracle's |X|^2 plane of the stream, [frames][n]; computed once per key and never written to"""
    if key is not None and key in _planes:
        return _planes[key]
    L = orc.lib()
    d = L.orc_detector_create(rc.CF_A, int(fs), 0.0, 0)
    n = L.orc_detector_fft_size(d)
    total = rc.n_samples(x, fmt)
    mag = np.zeros((total // n + 1, n), np.float32)
    L.orc_detector_set_mag_sink(d, orc.fptr(mag), mag.shape[0])
    # (two float32 per cf32 sample, two int8 per ci8 sample)
    flat = np.ascontiguousarray(x).view(np.float32) if fmt == irdm.FMT_CF32 else np.ascontiguousarray(x)
    per = 2
    for o in range(0, total, 32768):
        blk = np.ascontiguousarray(flat[per * o:per * min(total, o + 32768)])
        if fmt == irdm.FMT_CF32:
            L.orc_detector_feed_cf32(d, orc.fptr(blk), len(blk) // 2, orc.BURST_CB(0), None)
        else:
            L.orc_detector_feed_i8(d, blk.ctypes.data_as(C.c_void_p), len(blk) // 2, orc.BURST_CB(0), None)
    done = L.orc_detector_frames_done(d)
    L.orc_detector_destroy(d)
    assert done == total // n, (done, total, n)
    out = mag[:done]
    out.setflags(write=False)
    if key is not None:
        _planes[key] = out
    return out


def check_rows(rows, plane, R, fs, t0=rc.T0_A):
    """rows = (headers, mean, peak) of a whole stream against its plane: the row count, every header, every value"""
    hdrs, mean, peak = rows
    F, n = plane.shape
    want = (F + R - 1) // R
    assert len(hdrs) == want == len(mean) == len(peak), (len(hdrs), want)
    worst = 0.0
    for r in range(want):
        seg = plane[r * R:(r + 1) * R]
        k = len(seg)
        h = hdrs[r]
        assert (int(h["row"]), int(h["first_frame"]), int(h["n_frames"]), int(h["n_bins"])) == (r, r * R, k, n), (r, h)
        assert int(h["timestamp_ns"]) == t0 + int((r * R * n) / fs * 1e9), (r, h)
        assert np.array_equal(peak[r].view(np.uint32), seg.max(0).view(np.uint32)), "peak of row %d" % r
        m64 = seg.astype(np.float64).mean(0)
        err = np.abs(mean[r].astype(np.float64) - m64)
        bound = 1.01 * (k + 1) * U * m64
        assert np.all(err <= bound), "mean of row %d: %g over the bound in bin %d" % (r, float((err - bound).max()), int((err - bound).argmax()))
        worst = max(worst, float((err / np.maximum(bound, 1e-300)).max()))
        if R == 1:
            assert np.array_equal(mean[r].view(np.uint32), seg[0].view(np.uint32)), "R = 1: mean of row %d is not the plane" % r
    return dict(rows=want, last_frames=int(hdrs[-1]["n_frames"]), worst=worst)


def headers(hs):
    """a list of irdm.SpectrumRow as the structured array the file reader returns"""
    out = np.zeros(len(hs), ROW)
    for i, h in enumerate(hs):
        out[i] = (h.row, h.first_frame, h.timestamp_ns, h.n_frames, h.n_bins)
    return out


def as_bytes(rows):
    hdrs, mean, peak = rows
    return hdrs.tobytes() + np.ascontiguousarray(mean).tobytes() + np.ascontiguousarray(peak).tobytes()


def poll(p):
    hs, mean, peak = p.poll_spectrum()
    return headers(hs), mean, peak


def join(parts):
    return (np.concatenate([a[0] for a in parts]), np.concatenate([a[1] for a in parts]), np.concatenate([a[2] for a in parts]))


def feed_plain(p, x, fmt, chunks, after=None):
    """x in chunks through irdm_feed_device from a device buffer each, `after` called behind every feed; then irdm_flush"""
    per = 1 if fmt == irdm.FMT_CF32 else 2
    off = 0
    for c in chunks:
        ptr = irdm.device_buffer(np.ascontiguousarray(x[off * per:(off + c) * per]))
        try:
            p.feed_device(ptr, c)
        finally:
            irdm.device_free(ptr)
        off += c
        if after is not None:
            after()
    assert off == rc.n_samples(x, fmt)
    p.flush()


def cuts(n):
    """a stream of n samples three ways: one chunk; five parts (reset_checks.chunks_of: the ragged end on the last); single
    feed blocks with the ragged end as a chunk of its own"""
    return dict(one=[n], five=rc.chunks_of(n, 5), blocks=[32768] * (n // 32768) + ([n % 32768] if n % 32768 else []))


def run(fs, fmt, depth, x, chunks, R, options=None, in_place=True, want_queues=False, t0=rc.T0_A):
    """a fresh context with the option at R (None: never set), x fed in chunks -- in place with look-ahead at
    pipeline_depth >= 1 (reset_checks.feed) or from plain device buffers --, flushed; every row, and the record queues"""
    opts = dict(options or {})
    if R is not None:
        opts["spectrum_frames"] = R
    p = rc.make(fs, fmt, depth, max(chunks), opts, rc.CF_A, t0)
    try:
        if in_place:
            rc.feed(p, x, fmt, chunks)
            p.flush()
        else:
            feed_plain(p, x, fmt, chunks)
        rows = poll(p) if R is not None else None
        return (rows, rc.queues(p)) if want_queues else rows
    finally:
        p.close()


def check_values(fs, fmt, x, depth=1, parts=5, r_cases=R_CASES):
    """1. every R of R_CASES: row count, headers, values against the plane"""
    n = rc.n_samples(x, fmt)
    plane = plane_of(x, fs, fmt, key=(fs, fmt, n))
    res = {}
    for R in r_cases:
        s = check_rows(run(fs, fmt, depth, x, rc.chunks_of(n, parts), R), plane, R, fs)
        if R > plane.shape[0]:
            assert s["rows"] == 1 and s["last_frames"] == plane.shape[0], s
        res[str(R)] = s
    return res


def check_cuts(fs, fmt, x, depth, R=7, options=None, verify=True):
    """2. one stream as one chunk, in five parts and in single feed blocks: the same bytes (and, once, the right ones)"""
    n = rc.n_samples(x, fmt)
    got = {name: run(fs, fmt, depth, x, c, R, options) for name, c in cuts(n).items()}
    if verify:
        check_rows(got["one"], plane_of(x, fs, fmt, key=(fs, fmt, n)), R, fs)
    for name in ("five", "blocks"):
        assert as_bytes(got[name]) == as_bytes(got["one"]), "fed as %r: rows differ from the stream fed as one chunk" % name
    return dict(rows=len(got["one"][0]), chunks={k: len(c) for k, c in cuts(n).items()})


def check_mid_stream_polls(fs, fmt, x, depth, R=7, parts=5):
    """3. rows polled after every feed and after the flush, concatenated == the rows of one poll at the end"""
    n = rc.n_samples(x, fmt)
    chunks = rc.chunks_of(n, parts)
    want = run(fs, fmt, depth, x, chunks, R, in_place=False)
    p = rc.make(fs, fmt, depth, max(chunks), {"spectrum_frames": R})
    try:
        parts_got = []
        feed_plain(p, x, fmt, chunks, after=lambda: parts_got.append(poll(p)))
        early = sum(len(a[0]) for a in parts_got)
        parts_got.append(poll(p))
        assert as_bytes(join(parts_got)) == as_bytes(want)
    finally:
        p.close()
    return dict(rows=len(want[0]), before_flush=early)


def check_records_unchanged(fs, fmt, x, depth, options, R=64, parts=4):
    """4. the record queues of a run with the option on == those with it off, byte for byte"""
    n = rc.n_samples(x, fmt)
    chunks = rc.chunks_of(n, parts)
    _, off = run(fs, fmt, depth, x, chunks, None, options, want_queues=True)
    rows, on = run(fs, fmt, depth, x, chunks, R, options, want_queues=True)
    s = rc.same(on, off, "records with spectrum_frames %d" % R)
    assert s["tagged"] >= 3 and len(rows[0]) > 0, s
    return s


def check_reset(fs, fmt, a, b, depth, R=7, used=None):
    """5. A with its rows left unpolled, reset, B: B's rows == a fresh context's; the option is refused (-1) from the first
    feed until the reset and taken again after it.  used: a callable returning the device memory in use -- then A, B, A
    and the figure after the third stream must equal that after the first."""
    L = irdm.lib()
    na, nb = rc.n_samples(a, fmt), rc.n_samples(b, fmt)
    ca, cb = rc.chunks_of(na, 3), rc.chunks_of(nb, 4)
    mc = max(ca + cb)
    want_b = run(fs, fmt, depth, b, cb, R, t0=rc.T0_B)
    p = rc.make(fs, fmt, depth, mc, {"spectrum_frames": R})
    try:
        assert L.irdm_set_option(p.h, b"spectrum_frames", R + 1) == 0 and L.irdm_set_option(p.h, b"spectrum_frames", R) == 0
        rc.feed(p, a, fmt, ca, only_first=True)
        assert L.irdm_set_option(p.h, b"spectrum_frames", R) == -1, "the option was taken mid-stream"
        p.reset(rc.CF_A, rc.T0_A)
        assert L.irdm_set_option(p.h, b"spectrum_frames", R) == 0, "the option was refused after irdm_reset"
        rc.feed(p, a, fmt, ca)
        p.flush()                                   # (A's rows stay in the queue, unpolled)
        after_first = used() if used else None
        p.reset(rc.CF_B, rc.T0_B)
        rc.feed(p, b, fmt, cb)
        p.flush()
        got_b = poll(p)
        assert as_bytes(got_b) == as_bytes(want_b), "B behind a reset: rows differ from a fresh context's"
        assert int(got_b[0]["row"][0]) == 0 and int(got_b[0]["timestamp_ns"][0]) == rc.T0_B
        if used:
            p.reset(rc.CF_A, rc.T0_A)
            rc.feed(p, a, fmt, ca)
            p.flush()
            poll(p)
            assert used() == after_first, (used(), after_first)
    finally:
        p.close()
    return dict(rows_b=len(want_b[0]))


def check_option_range(fs):
    """6. R < 0 and R > 2^20 are refused, 0 and 2^20 are taken"""
    L = irdm.lib()
    p = rc.make(fs, irdm.FMT_CF32, 0, 32768 * 4, {})
    try:
        got = [L.irdm_set_option(p.h, b"spectrum_frames", v) for v in (-1, (1 << 20) + 1, 1 << 20, 0)]
        assert got == [-1, -1, 0, 0], got
        assert L.irdm_spectrum_bins(p.h) == rc.nfft_of(fs)
    finally:
        p.close()
    return got


# ---- the binary ----
def read_spec(path):
    """a --spectrum file: (header fields, row headers, mean, peak)"""
    b = open(path, "rb").read()
    magic, ver, n, R, rate, cf, t0 = struct.unpack_from("<8sIIIIdQ", b)
    assert magic == b"IRDMSPEC" and ver == 1 and b[40:64] == bytes(24), (magic, ver)
    rec = np.dtype([("h", ROW), ("mean", "<f4", (n,)), ("peak", "<f4", (n,))])
    assert (len(b) - 64) % rec.itemsize == 0, (len(b), rec.itemsize)
    rows = np.frombuffer(b, rec, offset=64)
    return dict(n_bins=n, R=R, rate=rate, center=cf, start_ns=t0), (rows["h"].copy(), rows["mean"].copy(), rows["peak"].copy())


def check_cli(exe, tmp, fs, x, R=7):
    """7. --spectrum: the file parses to the header fields and to the rows of check 1; stdout is that of the run without the
    flag; the default of --spectrum-frames; two recordings with --out-dir and auto; what exits with 2"""
    n_f = rc.nfft_of(fs)
    plane = plane_of(x, fs, irdm.FMT_CF32, key=(fs, irdm.FMT_CF32, len(x)))
    f1 = os.path.join(tmp, "one.cf32")
    np.ascontiguousarray(x).tofile(f1)
    common = ["-r", fs, "-c", int(rc.CF_A), "--chunk", 1 << 22, "--file-info", "golden", "--start-time", "1700000000"]
    rcode, plain_out, plain_err = rc.run_cli(exe, ["-f", f1] + common)
    assert rcode == 0 and len(plain_out) > 0, plain_err[-2000:]
    spec = os.path.join(tmp, "one.spec")
    rcode, out, err = rc.run_cli(exe, ["-f", f1, "--spectrum", spec, "--spectrum-frames", R] + common)
    assert rcode == 0, err[-2000:]
    assert out == plain_out, "stdout changes with --spectrum"
    assert rc.summary(err) == rc.summary(plain_err), (rc.summary(err), rc.summary(plain_err))
    hdr, rows = read_spec(spec)
    assert hdr == dict(n_bins=n_f, R=R, rate=fs, center=rc.CF_A, start_ns=rc.T0_A), hdr
    res = dict(explicit=check_rows(rows, plane, R, fs))
    # the default: round(rate / fft_size) frames, about a second
    rcode, out, err = rc.run_cli(exe, ["-f", f1, "--spectrum", spec] + common)
    assert rcode == 0 and out == plain_out, err[-2000:]
    hdr, rows = read_spec(spec)
    assert hdr["R"] == max(1, int(np.floor(fs / n_f + 0.5))), hdr
    res["default"] = check_rows(rows, plane, hdr["R"], fs)
    # two recordings, --out-dir and auto: each .spec is its single-file run's
    f2 = os.path.join(tmp, "two.cf32")
    np.ascontiguousarray(x[:len(x) // 2 // 32768 * 32768 + 4321]).tofile(f2)
    od = os.path.join(tmp, "specs")
    lst = os.path.join(tmp, "list.txt")
    times = ["1700000000", "1700003600.25"]
    with open(lst, "w") as fh:
        for path, t in zip((f1, f2), times):
            fh.write("%s %s\n" % (path, t))
    batch = ["-r", fs, "-c", int(rc.CF_A), "--chunk", 1 << 22, "--file-info", "golden"]
    rcode, out, err = rc.run_cli(exe, ["--files-from", lst, "--out-dir", od, "--spectrum", "auto", "--spectrum-frames", R] + batch)
    assert rcode == 0 and out == b"", err[-2000:]
    for path, t in zip((f1, f2), times):
        rcode, _, err = rc.run_cli(exe, ["-f", path, "--start-time", t, "--spectrum", spec, "--spectrum-frames", R] + batch)
        assert rcode == 0, err[-2000:]
        got = open(os.path.join(od, os.path.basename(path) + ".spec"), "rb").read()
        assert got == open(spec, "rb").read(), path
        assert len(got) > 64
    # refused before anything is processed
    for args in (["-f", f1, "--spectrum", spec, "--gpus", "2"],
                 ["-f", f1, "-f", f2, "--spectrum", spec, "--out-dir", od],
                 ["-f", f1, "-f", f2, "--spectrum", "auto"]):
        rcode, out, err = rc.run_cli(exe, args + batch)
        assert rcode == 2 and out == b"", (args, rcode, err[-1000:])
    return res


def check_cli_frontend(exe, tmp, R=64):
    """8. behind the front end: the wideband scene with --band-center / --decimate; the .spec rows == the rows of a context
    fed the output of irdm_frontend_run_device for the same capture; header rate = the output rate, header centre = the
    capture's centre + the applied shift"""
    import frontend_model as fm
    s = fm.SCENE
    x, _, _ = fm.wideband_scene()
    path = os.path.join(tmp, "wide.ci8")
    x.tofile(path)
    cc = 1615000000.0
    spec = os.path.join(tmp, "wide.spec")
    rcode, out, err = rc.run_cli(exe, ["-f", path, "-r", s["fs_in"], "-c", "%.3f" % cc, "--band-center", "%.3f" % (cc + s["shift_hz"]),
                                       "--decimate", s["D"], "--file-info", "fe", "--chunk", 1 << 20, "--start-time", "1700000000",
                                       "--spectrum", spec, "--spectrum-frames", R])
    assert rcode == 0 and len(out) > 0, err[-2000:]
    hdr, rows = read_spec(spec)
    st = fm.Stage(s["fs_in"], irdm.FMT_CI8, s["D"], s["shift_hz"])
    try:
        out_rate, applied = st.fe.out_rate, st.fe.applied_shift_hz
        y = st.run(x, [len(x) // 2])
    finally:
        st.close()
    assert hdr["rate"] == out_rate == s["fs_in"] // s["D"] and hdr["center"] == cc + applied and hdr["R"] == R, hdr
    assert hdr["start_ns"] == rc.T0_A and hdr["n_bins"] == rc.nfft_of(out_rate), hdr
    chunks = [1 << 22] * (len(y) // (1 << 22)) + ([len(y) % (1 << 22)] if len(y) % (1 << 22) else [])
    want = run(out_rate, irdm.FMT_CF32, 1, y, chunks, R, in_place=False)
    assert len(want[0]) == (len(y) // hdr["n_bins"] + R - 1) // R > 1
    assert as_bytes(rows) == as_bytes(want), "rows behind the front end differ from those of its output fed directly"
    return dict(rows=len(want[0]), samples=len(y))
