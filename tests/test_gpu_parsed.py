"""Option parsed_records: ida_decode() on the packed record path (ida_packed_kernel), and the CLI's --parsed.

IDA-rich scenes (tests/bitlayer.py frames through siggen): every burst an IDA frame, some at low amplitude (Chase decoding
on the LLRs), some with a bad CRC, da_len from 0 to 20.  The compact IDA records must turn into exactly the records the
decode_ida path returns for the same frames, and those into what the oracle's ida_decode makes of the oracle's frames;
the compact frame records must be those of a packed_records-only run."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import bitlayer as bl
import irdm
import orc
import siggen
from test_gpu_bitlayer import ida_decode_with, same_ida

pytestmark = pytest.mark.gpu

CHANNELS = (-17, -5, 7, 19)
SLOTS = 20                      # 4 bursts per slot: 80 IDA bursts


def ida_scene(fs, seed):
    rng = np.random.default_rng(seed)
    fft = 1 << int(round(np.log2(fs / 1000.0)))
    first = 520 * fft + 3000
    slot = int(0.042 * fs)
    n = (first + SLOTS * slot + int(0.06 * fs)) // 32768 * 32768 + 32768
    bursts = []
    for s in range(SLOTS):
        for c, ch in enumerate(CHANNELS):
            k = 4 * s + c
            da_len = (0, 1, 3, 11, 20)[k % 5] if k % 7 else int(rng.integers(0, 21))
            st = bl.ida_stream(k % 8, da_len, k & 1, [int(b) for b in rng.integers(0, 256, 20)], rng,
                               good_crc=bool(k % 6 != 5))
            uplink = k % 9 == 4
            bits = bl.ida_frame(bl.lcw_bits(2, int(rng.integers(0, 32)), int(rng.integers(0, 1 << 21))), st, rng,
                                uplink=uplink)
            amp = 0.0065 if k % 4 == 3 else 0.05
            bursts.append(dict(start=first + s * slot + c * int(0.0011 * fs), freq_hz=siggen.channel_freq(ch),
                               quads=[0] * 16 + siggen.bits_to_quadrants("".join(str(b) for b in bits)), amp=amp,
                               uplink=uplink))
    return siggen.make_stream(fs, n, bursts, seed=seed)[0]


_SCENES = {}


def scene(fs):
    if fs not in _SCENES:
        iq = ida_scene(fs, 7 if fs == 2_000_000 else 8)
        _SCENES[fs] = (iq, orc.run_stream(iq, fs))
    return _SCENES[fs]


def run(iq, fs, depth, options):
    p = irdm.Pipeline(fs, max_chunk_samples=len(iq) // 2 + 32768, max_bursts_per_chunk=1024, pipeline_depth=depth)
    for k, v in options.items():
        p.set_option(k, v)
    try:
        half = len(iq) // 2 // 32768 * 32768
        p.feed_host(iq[:half])
        p.feed_host(iq[half:])
        p.flush()
        if "decode_ida" in options:
            return p.poll_demods(), p.poll_ida()
        return p.poll_demods_packed(), (p.poll_ida_packed() if "parsed_records" in options else None)
    finally:
        p.close()


@pytest.mark.parametrize("fs", (2_000_000, 10_000_000))
@pytest.mark.parametrize("depth", (0, 1))
def test_parsed_records_equal_decode_ida_and_the_oracle(fs, depth):
    iq, ref = scene(fs)
    packed, _ = run(iq, fs, depth, {"packed_records": 1})
    parsed, idp = run(iq, fs, depth, {"parsed_records": 1})
    demods, ida = run(iq, fs, depth, {"decode_ida": 1})
    # the compact frame records are those of a packed_records-only run, one IDA record each
    assert len(parsed) == len(packed) == len(idp) == len(demods) == len(ida) == len(ref.demods) >= 50
    for a, b in zip(packed, parsed):
        assert bytes(a) == bytes(b)
    L = orc.lib()
    L.orc_ida_decode.restype = C.c_int
    n_ok = n_bad_crc = n_fixed = n_ul = 0
    for ip, dp, full, dm, rd in zip(idp, parsed, ida, demods, ref.demods):
        u = irdm.ida_unpack(ip, dp)
        same_ida(u, full)                                    # field by field, lcw_header included
        for f in ("id", "timestamp", "frequency", "direction", "magnitude", "noise", "level", "confidence", "n_symbols"):
            assert getattr(u, f) == getattr(full, f), f
        assert u.id == dm.id == dp.id
        bits = np.ctypeslib.as_array(rd.bits)[:rd.n_bits]
        llr = np.ctypeslib.as_array(rd.llr)[:rd.n_bits]
        _, o = ida_decode_with(L.orc_ida_decode, bits, llr, rd.direction)
        same_ida(u, o)
        if u.ok:
            n_ok += 1
            n_bad_crc += u.da_len > 0 and not u.crc_ok
            n_fixed += u.fixederrs > 0
            n_ul += u.direction == 2
        else:
            assert bytes(ip) == bytes(irdm.IdaPacked())
    assert n_ok >= 50 and n_bad_crc >= 5 and n_fixed >= 5, (n_ok, n_bad_crc, n_fixed, n_ul)


def _expected_parsed_lines(ref, file_info):
    """--parsed's lines from the oracle's frames: its ida_decode, the IDA line where it succeeds, its RAW line otherwise"""
    L = orc.lib()
    L.orc_ida_decode.restype = C.c_int
    raw = ref.raw_lines(file_info)
    t0 = ref.demods[0].timestamp // 10**9 * 10**9            # (ensure_initialized: whichever kind of line comes first)
    out = []
    for rd, rl in zip(ref.demods, raw):
        bits = np.ctypeslib.as_array(rd.bits)[:rd.n_bits]
        llr = np.ctypeslib.as_array(rd.llr)[:rd.n_bits]
        _, o = ida_decode_with(L.orc_ida_decode, bits, llr, rd.direction)
        if not o.ok:
            out.append(rl)
            continue
        b = irdm.Ida()
        for f in ("ok", "ft", "lcw_ft", "lcw_code", "ec_lcw", "lcw3_val", "da_ctr", "da_len", "cont", "crc_ok",
                  "stored_crc", "computed_crc", "fixederrs", "payload_len", "bch_len", "lcw_header"):
            setattr(b, f, getattr(o, f))
        b.payload[:] = list(o.payload)
        b.bch_stream[:] = list(o.bch_stream)
        b.direction, b.timestamp, b.frequency = rd.direction, rd.timestamp, rd.center_frequency
        b.magnitude, b.noise, b.level = rd.magnitude, rd.noise, rd.level
        b.confidence, b.n_symbols = rd.confidence, rd.n_payload_symbols
        out.append(irdm.format_ida([b], t0)[0])
    return out


def _same_line(a, b):
    """the same line but for the soft values the device libm may round differently and the timestamp (as the RAW CLI
    tests compare: tests/test_gpu_group.py test_cli_gpus_flag)"""
    ta, tb = a.split(), b.split()
    assert len(ta) == len(tb) and ta[0] == tb[0], (a, b)
    if ta[0] == "RAW:":
        same = [0, 1, 4, 5, 6, 8, 9]
        assert abs(int(ta[3]) - int(tb[3])) <= 1 and abs(float(ta[7]) - float(tb[7])) <= 1e-4, (a, b)
    else:
        same = [0, 4] + list(range(6, len(ta)))       # (p-<t0>: the run's start time, as the timestamp)
        assert abs(int(ta[3]) - int(tb[3])) <= 1, (a, b)
        la, lb = ta[5].split("|"), tb[5].split("|")
        assert la[1:] == lb[1:] and abs(float(la[0]) - float(lb[0])) <= 0.011, (a, b)
    for i in same:
        assert ta[i] == tb[i], (i, a, b)


def test_cli_parsed(tmp_path):
    """iridium-sniffer-hip --parsed on the 10 MHz scene: the packed default and --save-bursts (the decode_ida path) print
    the same lines; those and --gpus 1 --group-loopback's are the oracle's IDA / RAW lines"""
    fs = 10_000_000
    iq, ref = scene(fs)
    exe = os.path.join(os.path.dirname(irdm.LIB_PATH), "iridium-sniffer-hip")
    if not os.path.exists(exe):
        irdm.build(force=True)
    path = tmp_path / "scene.cf32"
    np.ascontiguousarray(iq).tofile(path)
    chunk = 1 << 25                 # (a group chunk holds at least the 10 MHz overlap, 21 M samples)
    outs = []
    for extra in ([], ["--save-bursts", str(tmp_path / "bursts")], ["--gpus", "1", "--group-loopback"]):
        r = subprocess.run([exe, "-f", str(path), "-r", str(fs), "--chunk", str(chunk), "--file-info", "golden",
                            "--parsed"] + extra,
                           capture_output=True, timeout=300)
        assert r.returncode == 0, r.stderr.decode()[-2000:]
        outs.append(r.stdout)
    # (a file-mode run's timestamps follow its start time: two runs agree in every byte but the t0 name and timestamp)
    untimed = [[" ".join(l.split(" ")[:1] + l.split(" ")[3:]) for l in o.decode("latin-1").splitlines()] for o in outs]
    assert untimed[0] == untimed[1]
    want = _expected_parsed_lines(ref, "golden")
    for out in (outs[0], outs[2]):
        lines = out.decode("latin-1").splitlines(keepends=True)
        assert len(lines) == len(want) >= 50
        assert sum(l.startswith("IDA: ") for l in lines) >= 50
        for a, b in zip(lines, want):
            _same_line(a, b)
    # without --parsed: RAW lines only, as before
    r = subprocess.run([exe, "-f", str(path), "-r", str(fs), "--chunk", str(chunk), "--file-info", "golden"],
                       capture_output=True, timeout=300)
    assert r.returncode == 0
    raw = r.stdout.decode().splitlines()
    assert len(raw) == len(lines) and all(l.startswith("RAW: ") for l in raw)
