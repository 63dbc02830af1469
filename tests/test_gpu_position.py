"""Option frame_records (frame_decode() on the packed record path: frame_packed_kernel) and the CLI's --position.

Frame records: IRA / IBC scenes (tests/bitlayer.py frames through siggen), some bursts weak enough for Chase decoding.
irdm_frame_unpack of every compact frame record must be the record the decode_frames path returns for the same frame
(lat / lon bit for bit) and what the oracle's frame_decode makes of the oracle's frame; the compact demod records must be
those of a packed_records-only run, with parsed_records as well as without.

--position: a scene of downlink IRA frames from four satellites over a chosen receiver, each burst at its satellite's
Doppler-shifted frequency.  The POSITION lines must be what the library's solver prints for the decode_frames path's records
of the same file, on every decoding path, and stdout must not change."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import bitlayer as bl
import irdm
import orc
import siggen
from test_oracle_bitlayer import decode_with

pytestmark = pytest.mark.gpu

DECODED_FIELDS = ("type", "sat_id", "beam_id", "alt", "n_pages", "timeslot", "sv_blocking", "bc_type", "iri_time",
                  "bch_len", "id", "timestamp")


def frame_scene(fs, seed):
    """IRA and IBC frames on several channels, a quarter of them weak (bit errors for Chase to fix)"""
    rng = np.random.default_rng(seed)
    fft = 1 << int(round(np.log2(fs / 1000.0)))
    first = 520 * fft + 3000
    slot = int(0.042 * fs)
    n_slots = 16
    n = (first + n_slots * slot + int(0.06 * fs)) // 32768 * 32768 + 32768
    bursts = []
    for s in range(n_slots):
        for c, ch in enumerate((-15, -3, 9, 21)):
            k = 4 * s + c
            if k % 3:
                pages = [(int(rng.integers(0, 2**32)), int(rng.integers(0, 32))) for _ in range(k % 5)]
                st = bl.ira_stream(int(rng.integers(1, 128)), int(rng.integers(0, 64)), int(rng.integers(-2047, 2048)),
                                   int(rng.integers(-2047, 2048)), int(rng.integers(-2047, 2048)), pages, rng)
                bits = bl.ira_frame(st[:63 + (k % 5) * 42 + 42])
            else:
                st = bl.ibc_stream(int(rng.integers(0, 128)), int(rng.integers(0, 64)), int(rng.integers(0, 2)),
                                   int(rng.integers(0, 2)), int(rng.integers(0, 2**32)), rng, n_blocks=4)
                bits = bl.ibc_frame(int(rng.integers(0, 4)), st)
            if len(bits) < 290:
                bits = bits + [int(b) for b in rng.integers(0, 2, 290 - len(bits))]
            if len(bits) % 2:
                bits.append(0)
            amp = (0.0075, 0.0065, 0.006)[k % 3] if k % 4 == 3 else 0.05
            bursts.append(dict(start=first + s * slot + c * int(0.0011 * fs), freq_hz=siggen.channel_freq(ch),
                               quads=[0] * 16 + siggen.bits_to_quadrants("".join(str(b) for b in bits)), amp=amp))
    return siggen.make_stream(fs, n, bursts, seed=seed)[0]


_SCENES = {}


def scene(fs):
    if fs not in _SCENES:
        iq = frame_scene(fs, 11 if fs == 2_000_000 else 12)
        _SCENES[fs] = (iq, orc.run_stream(iq, fs))
    return _SCENES[fs]


def run(iq, fs, depth, options, group=False):
    kw = dict(max_chunk_samples=len(iq) // 2 + 32768, max_bursts_per_chunk=1024, pipeline_depth=depth)
    if group:
        chunk = max(len(iq) // 2 // 32768 * 32768 + 32768, 1 << 25)
        p = irdm.Group(fs, 1, max_chunk_samples=chunk, pipeline_depth=depth)
        p.set_option("group_loopback", 1)
    else:
        p = irdm.Pipeline(fs, **kw)
    for k, v in options.items():
        p.set_option(k, v)
    try:
        if group:
            p.feed_host(iq)
        else:
            half = len(iq) // 2 // 32768 * 32768
            p.feed_host(iq[:half])
            p.feed_host(iq[half:])
        p.flush()
        if "decode_frames" in options:
            return p.poll_demods(), p.poll_decoded(), None
        return (p.poll_demods_packed(), p.poll_frame_packed() if "frame_records" in options else None,
                p.poll_ida_packed() if "parsed_records" in options else None)
    finally:
        p.close()


def same_decoded(a, b):
    for f in DECODED_FIELDS:
        assert getattr(a, f) == getattr(b, f), f
    assert list(a.pos_xyz) == list(b.pos_xyz)
    assert list(a.page_tmsi) == list(b.page_tmsi) and list(a.page_msc) == list(b.page_msc)
    assert a.lat.hex() == b.lat.hex() and a.lon.hex() == b.lon.hex()
    assert a.frequency == b.frequency


@pytest.mark.parametrize("fs", (2_000_000, 10_000_000))
@pytest.mark.parametrize("depth", (0, 1))
def test_frame_records_equal_decode_frames_and_the_oracle(fs, depth):
    iq, ref = scene(fs)
    packed, _, _ = run(iq, fs, depth, {"packed_records": 1})
    framed, frp, _ = run(iq, fs, depth, {"frame_records": 1})
    demods, dec, _ = run(iq, fs, depth, {"decode_frames": 1})
    assert len(framed) == len(packed) == len(frp) == len(demods) == len(dec) == len(ref.demods) >= 40
    for a, b in zip(packed, framed):
        assert bytes(a) == bytes(b)
    L = orc.lib()
    L.orc_frame_decode.restype = C.c_int
    types = {0: 0, 1: 0, 2: 0}
    for fp, dp, full, rd in zip(frp, framed, dec, ref.demods):
        u = irdm.frame_unpack(fp, dp)
        same_decoded(u, full)
        _, o = decode_with(L.orc_frame_decode, np.ctypeslib.as_array(rd.bits)[:rd.n_bits],
                           np.ctypeslib.as_array(rd.llr)[:rd.n_bits])
        for f in ("type", "sat_id", "beam_id", "n_pages", "bc_type", "iri_time", "timeslot", "sv_blocking"):
            assert getattr(u, f) == getattr(o, f), f
        assert list(u.pos_xyz) == list(o.pos_xyz)
        types[u.type] += 1
        if u.type == 0:
            assert bytes(fp) == bytes(irdm.FramePacked())
    assert types[1] >= 20 and types[2] >= 10, types


@pytest.mark.parametrize("depth", (0, 1))
def test_frame_and_parsed_records_together(depth):
    fs = 10_000_000
    iq, _ = scene(fs)
    _, frp, _ = run(iq, fs, depth, {"frame_records": 1})
    _, _, idp = run(iq, fs, depth, {"parsed_records": 1})
    both, frp2, idp2 = run(iq, fs, depth, {"frame_records": 1, "parsed_records": 1})
    assert len(both) == len(frp) == len(frp2) == len(idp) == len(idp2)
    assert [bytes(a) for a in frp] == [bytes(b) for b in frp2]
    assert [bytes(a) for a in idp] == [bytes(b) for b in idp2]


def test_group_frame_records():
    fs = 2_000_000
    iq, _ = scene(fs)
    packed, frp, _ = run(iq, fs, 1, {"frame_records": 1})
    gp, gfrp, _ = run(iq, fs, 1, {"frame_records": 1}, group=True)
    assert len(gp) == len(gfrp) == len(frp) >= 40
    for a, b, c, d in zip(packed, gp, frp, gfrp):
        assert (a.id, a.timestamp - packed[0].timestamp) == (b.id, b.timestamp - gp[0].timestamp)
        assert bytes(c) == bytes(d)


# ---------------------------------------------------------------- --position ----
A, F = 6378137.0, 1 / 298.257223563
E2 = 2 * F - F * F
GM, C_LIGHT = 3.986004418e14, 299792458.0
IR_BASE, IR_WIDTH = 1616000000.0, 41666.667
CENTER = 1622000000.0


def ecef(lat, lon, h):
    la, lo = math.radians(lat), math.radians(lon)
    N = A / math.sqrt(1 - E2 * math.sin(la) ** 2)
    return np.array([(N + h) * math.cos(la) * math.cos(lo), (N + h) * math.cos(la) * math.sin(lo),
                     (N * (1 - E2) + h) * math.sin(la)])


def position_scene(fs, secs, seed=5):
    """downlink IRA frames from four satellites passing near a receiver at 47.5 N 8.5 E: pos_xyz along each orbit, every
    burst at its channel plus the Doppler shift the receiver sees (satellite velocity minus Earth rotation); and on a channel
    of its own an IDA frame every tenth burst (--parsed / --acars output)"""
    rng = np.random.default_rng(seed)
    rng_ida = np.random.default_rng(seed + 100)
    rx = ecef(47.5, 8.5, 400.0)
    up = rx / np.linalg.norm(rx)
    east = np.cross([0, 0, 1.0], up)
    east /= np.linalg.norm(east)
    north = np.cross(up, east)
    r = 7158e3
    speed = math.sqrt(GM / r)
    sats = []
    for k, (az, off, ch) in enumerate(((0.3, 900e3, -12), (1.9, -700e3, -2), (3.3, 1200e3, 8), (4.6, -400e3, 17))):
        d = math.cos(az) * north + math.sin(az) * east
        side = np.cross(up, d)
        p0 = up * r + side * off - d * speed * secs / 2
        sats.append(dict(sat=20 + 11 * k, p0=p0, v=d * speed, ch=ch))
    fft = 1 << int(round(np.log2(fs / 1000.0)))
    first = 520 * fft + 3000
    n = int(secs * fs) // 32768 * 32768
    period = 0.09                                         # one IRA burst per satellite every 90 ms, staggered
    bursts = []
    t = first / fs
    k = 0
    while t * fs + 0.04 * fs < n:
        s = sats[k % 4]
        p = s["p0"] + s["v"] * t
        p = p / np.linalg.norm(p) * r                     # back onto the sphere of radius r
        los = p - rx
        rxv = np.array([-7.2921150e-5 * rx[1], 7.2921150e-5 * rx[0], 0.0])
        rr = float(np.dot(los, s["v"] - rxv) / np.linalg.norm(los))
        chan = IR_BASE + round((CENTER + siggen.channel_freq(s["ch"]) - IR_BASE) / IR_WIDTH) * IR_WIDTH
        f_hz = chan - CENTER - rr / (C_LIGHT / chan)
        q = [int(v) for v in np.round(p / 4000.0)]
        st = bl.ira_stream(s["sat"], int(rng.integers(0, 48)), q[0], q[1], q[2], [], rng)
        bits = bl.ira_frame(st[:63 + 42])
        bits = bits + [int(b) for b in rng.integers(0, 2, max(0, 290 - len(bits)))]
        if len(bits) % 2:
            bits.append(0)
        bursts.append(dict(start=int(t * fs), freq_hz=f_hz,
                           quads=[0] * 16 + siggen.bits_to_quadrants("".join(str(b) for b in bits)), amp=0.05))
        if k % 10 == 0:
            st = bl.ida_stream(k % 8, (0, 3, 11, 20)[k // 10 % 4], k // 10 & 1,
                               [int(b) for b in rng_ida.integers(0, 256, 20)], rng_ida)
            bits = bl.ida_frame(bl.lcw_bits(2, int(rng_ida.integers(0, 32)), int(rng_ida.integers(0, 1 << 21))), st, rng_ida)
            bursts.append(dict(start=int(t * fs) + int(0.004 * fs), freq_hz=siggen.channel_freq(-18),
                               quads=[0] * 16 + siggen.bits_to_quadrants("".join(str(b) for b in bits)), amp=0.05))
        t += period / 4 + float(rng.uniform(0, 0.004))
        k += 1
    return siggen.make_stream(fs, n, bursts, seed=seed)[0]


def position_lines(text):
    return [l for l in text.splitlines() if l.startswith("POSITION: ")]


def test_cli_position(tmp_path):
    fs = 2_000_000
    secs = 12.5
    iq = position_scene(fs, secs)
    exe = os.path.join(os.path.dirname(irdm.LIB_PATH), "iridium-sniffer-hip")
    if not os.path.exists(exe):
        irdm.build(force=True)
    path = tmp_path / "pos.cf32"
    np.ascontiguousarray(iq).tofile(path)
    chunk = 1 << 25
    base = [exe, "-f", str(path), "-r", str(fs), "-c", str(int(CENTER)), "--chunk", str(chunk), "--file-info", "golden"]
    runs = {}
    for name, extra in (("packed", ["--position"]), ("save", ["--position", "--save-bursts", str(tmp_path / "b")]),
                        ("group", ["--position", "--gpus", "1", "--group-loopback"]),
                        ("plain", []), ("group_plain", ["--gpus", "1", "--group-loopback"]),
                        ("parsed", ["--position=250", "--parsed"]), ("parsed_plain", ["--parsed"]),
                        ("acars", ["--position", "--acars", "--acars-origin", "1700000000"]),
                        ("acars_plain", ["--acars", "--acars-origin", "1700000000"])):
        r = subprocess.run(base + extra, capture_output=True, timeout=300)
        assert r.returncode == 0, (name, r.stderr.decode()[-2000:])
        runs[name] = (r.stdout.decode("latin-1"), r.stderr.decode())
    # what the library's solver prints for the decode_frames path's records of the same file
    origin = 1700000000 * 10**9
    p = irdm.Pipeline(fs, max_chunk_samples=chunk, max_bursts_per_chunk=4096, pipeline_depth=1, center_frequency=CENTER,
                      start_time_ns=origin)
    p.set_option("decode_frames", 1)
    try:
        for k in range(0, len(iq), chunk):
            p.feed_host(iq[k:k + chunk])
        p.flush()
        demods, dec = p.poll_demods(), p.poll_decoded()
    finally:
        p.close()
    assert len(dec) == len(demods) >= 300 and sum(d.type == 1 for d in dec) >= 300
    dop = irdm.Doppler(0.0, origin)
    want = position_lines(dop.format_batch(dec) + dop.finish(origin + int(len(iq) / fs * 1e9)))
    assert len(want) >= 2 and any("waiting" not in l for l in want), want
    for name in ("packed", "save", "group"):
        out, err = runs[name]
        assert "Doppler positioning: enabled (height aiding: 0 m)" in err
        assert position_lines(err) == want, (name, err[-3000:])
    assert "Doppler positioning: enabled (height aiding: 250 m)" in runs["parsed"][1]
    assert position_lines(runs["plain"][1]) == []
    # stdout does not change (a run's timestamps follow its start time)
    untimed = lambda o: [" ".join(l.split(" ")[:1] + l.split(" ")[3:]) for l in o.splitlines()]
    assert untimed(runs["packed"][0]) == untimed(runs["plain"][0]) == untimed(runs["save"][0])
    assert len(runs["plain"][0].splitlines()) >= 300
    assert untimed(runs["group"][0]) == untimed(runs["group_plain"][0])
    assert len(runs["group"][0].splitlines()) == len(runs["plain"][0].splitlines())
    # --parsed: the same IDA / RAW lines with and without --position; --acars (fixed wall clock): the same bytes
    assert untimed(runs["parsed"][0]) == untimed(runs["parsed_plain"][0])
    assert sum(l.startswith("IDA: ") for l in runs["parsed"][0].splitlines()) >= 20
    assert runs["acars"][0] == runs["acars_plain"][0]
    assert runs["acars"][1].count("ACARS") == runs["acars_plain"][1].count("ACARS") >= 1
    r = subprocess.run(base + ["--position=9001"], capture_output=True, timeout=120)
    assert r.returncode == 1 and b"--position height must be 0-9000 m (got 9001)" in r.stderr
