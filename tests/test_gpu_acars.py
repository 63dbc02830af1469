"""--acars / --acars-json on the GPU's records: IDA reassembly, SBD and ACARS from the packed record path and the CLI.

IQ scenes at 2 and 10 MHz (tests/bitlayer.py IDA frames through siggen) carry on four channels at once: single-burst and
multi-burst IDA messages (up to 8 bursts, 40 ms apart), SBD messages spread over 2-3 IDA messages, a
low-amplitude burst that only Chase decoding recovers, a bad-CRC burst that breaks its message, an ACARS block with a wrong
Kermit CRC and a burst more than 280 ms after the one before it.  tests/acars_model.py computes the expected lines from the
oracle's frames and its ida_decode; the library's lines from the GPU's records must be those, and the scene's known
registrations, labels and texts must appear where the generator put them.

The scenes are downlink only: uplink frames made this way do not pass the demodulator's unique-word check, in the oracle
as on the GPU.  Uplink SBD / ACARS (the SEQ / FNO fields, the 0x50 / 0x51 skip) is covered by tests/test_acars_format.py."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import acars_model as am
import bitlayer as bl
import irdm
import orc
import siggen
from test_oracle_bitlayer import ida_decode_with

pytestmark = pytest.mark.gpu

CHANNELS = (-17, -5, 7, 19)
ORIGIN = (1760000000, 0)
ETX = b"\x03"


def _messages():
    """per channel, the IDA messages in order: dict(payload, ul, kind, expect, [bad_crc_burst], [weak_burst], [gap_burst])"""
    blk = am.acars_block
    ch = [[] for _ in CHANNELS]
    # channel 0: single-burst messages and a multi-burst DL message
    ch[0].append(dict(payload=am.sbd_short_dl(blk(reg=b".N101AA", label=b"Q0", body=ETX)), expect=b"REG:N101AA"))
    ch[0].append(dict(payload=am.sbd_short_dl(blk(reg=b".N202BB", label=b"H1", ack=b"A",
                                                  body=b"\x02MULTI BURST DOWNLINK TEXT WITH SOME LENGTH TO IT" + ETX)),
                      expect=b"[MULTI BURST DOWNLINK TEXT WITH SOME LENGTH TO IT]"))
    ch[0].append(dict(payload=am.sbd_short_dl(blk(reg=b".N303CC", label=b"5Z", body=b"\x02WRONG KERMIT" + ETX,
                                                  crc="bad")), expect=b"[WRONG KERMIT] ERRORS"))
    # channel 1: 8 bursts, then a message whose first burst has a bad CRC
    body = b"\x02M42AUA0123" + b"DOWNLINK POSITION REPORT " * 5 + ETX
    ch[1].append(dict(payload=am.sbd_short_dl(blk(reg=b".N404DD", label=b"H1", bid=b"7", body=body)),
                      expect=b"bID:7 [M42AUA0123DOWNLINK"))
    ch[1].append(dict(payload=am.sbd_short_dl(blk(reg=b".N414DE", body=b"\x02HEAD LOST" + ETX)), bad_crc_burst=0,
                      expect=None))
    # channel 2: one SBD message spread over three IDA messages, then one whose 2nd burst comes 300 ms late
    pkts = am.split_sbd(blk(reg=b".N505EE", label=b"SA", body=b"\x02THREE PACKET SBD MESSAGE ACROSS IDA MESSAGES " * 2
                            + ETX), 3)
    for k, p in enumerate(pkts):
        ch[2].append(dict(payload=p, expect=b"[THREE PACKET SBD" if k == 2 else None))
    ch[2].append(dict(payload=am.sbd_short_dl(blk(reg=b".N606FF", body=b"\x02LATE SECOND BURST TEXT" + ETX)),
                      gap_burst=1, expect=None))
    # channel 3: a weak burst inside a multi-burst message (Chase), a bad-CRC burst that breaks a message, UL 2-packet SBD
    ch[3].append(dict(payload=am.sbd_short_dl(blk(reg=b".N707GG", label=b"B9", body=b"\x02CHASE RECOVERS THE WEAK ONE" + ETX)),
                      weak_burst=1, expect=b"[CHASE RECOVERS THE WEAK ONE]"))
    ch[3].append(dict(payload=am.sbd_short_dl(blk(reg=b".N808HH", body=b"\x02BROKEN BY A BAD CRC BURST" + ETX)),
                      bad_crc_burst=1, expect=None))
    pk = am.split_sbd(blk(reg=b".N909JJ", label=b"B6", body=b"\x02S11AXY9876 TWO PACKETS" + ETX), 2)
    ch[3].append(dict(payload=pk[0], expect=None))
    ch[3].append(dict(payload=pk[1], expect=b"[S11AXY9876 TWO PACKETS]"))
    return ch


def ida_scene(fs, seed):
    rng = np.random.default_rng(seed)
    fft = 1 << int(round(np.log2(fs / 1000.0)))
    first = 520 * fft + 3000
    step = int(0.040 * fs)
    bursts = []
    end = 0
    for c, msgs in enumerate(_messages()):
        t = first + c * int(0.0011 * fs)
        for m in msgs:
            pl = m["payload"]
            n = max(1, -(-len(pl) // 20))
            assert n <= 8 and len(pl) <= 160
            for k in range(n):
                part = list(pl[20 * k:20 * k + 20])
                st = bl.ida_stream(k % 8, len(part), 1 if k < n - 1 else 0, part + [0] * (20 - len(part)), rng,
                                   good_crc=m.get("bad_crc_burst") != k)
                ul = bool(m.get("ul"))
                bits = bl.ida_frame(bl.lcw_bits(2, int(rng.integers(0, 32)), int(rng.integers(0, 1 << 21))), st, rng,
                                    uplink=ul)
                if m.get("gap_burst") == k:
                    t += int(0.300 * fs)
                bursts.append(dict(start=t, freq_hz=siggen.channel_freq(CHANNELS[c]),
                                   quads=([2, 0] * 16 if ul else [0] * 16)            # (UL: a 32-symbol preamble, burst_downmix.c:633-634)
                                   + siggen.bits_to_quadrants("".join(str(b) for b in bits)),
                                   amp=0.0075 if m.get("weak_burst") == k else 0.05, uplink=ul))
                t += step
            t += step
        end = max(end, t)
    n = (end + int(0.06 * fs)) // 32768 * 32768 + 32768
    return siggen.make_stream(fs, n, bursts, seed=seed)[0]


_SCENES = {}


def scene(fs):
    if fs not in _SCENES:
        iq = ida_scene(fs, 11 if fs == 2_000_000 else 12)
        _SCENES[fs] = (iq, orc.run_stream(iq, fs))
    return _SCENES[fs]


def oracle_bursts(ref):
    """(burst dict or None, frame timestamp) per oracle frame: its ida_decode and the demod's fields"""
    L = orc.lib()
    L.orc_ida_decode.restype = C.c_int
    out = []
    for rd in ref.demods:
        bits = np.ctypeslib.as_array(rd.bits)[:rd.n_bits]
        llr = np.ctypeslib.as_array(rd.llr)[:rd.n_bits]
        _, o = ida_decode_with(L.orc_ida_decode, bits, llr, rd.direction)
        b = None
        if o.ok:
            b = dict(ok=1, crc_ok=o.crc_ok, da_ctr=o.da_ctr, da_len=o.da_len, cont=o.cont, payload=list(o.payload),
                     direction=rd.direction, timestamp=rd.timestamp, frequency=rd.center_frequency,
                     magnitude=rd.magnitude, fixederrs=o.fixederrs)
        out.append((b, rd.timestamp))
    return out


def expected(ref, json_mode=False, station=None):
    r = am.IdaReasm()
    a = am.Acars(json=json_mode, station=station, origin=ORIGIN)
    text = ""
    for b, ts in oracle_bursts(ref):
        m = r.push(b, ts)
        if m:
            text += a.feed([m])
    return text.encode("latin-1"), a


def run_pipeline(iq, fs, depth, n_chunks):
    """the packed record path with parsed_records, fed in n_chunks pieces (messages cross the boundaries)"""
    step = -(-len(iq) // n_chunks) // 32768 * 32768 + 32768
    p = irdm.Pipeline(fs, max_chunk_samples=step, max_bursts_per_chunk=1024, pipeline_depth=depth)
    p.set_option("parsed_records", 1)
    try:
        dp, ip = [], []
        for i in range(0, len(iq), step):
            p.feed_host(iq[i:i + step])
            dp += p.poll_demods_packed()
            ip += p.poll_ida_packed()
        p.flush()
        dp += p.poll_demods_packed()
        ip += p.poll_ida_packed()
        return dp, ip
    finally:
        p.close()


def same_json(a, b):
    """the same JSON lines but for the soft values the device may round differently (freq +-1 Hz, sig_level, usec)"""
    la, lb = a.decode("latin-1").splitlines(), b.decode("latin-1").splitlines()
    assert len(la) == len(lb)
    for x, y in zip(la, lb):
        jx, jy = json.loads(x, strict=False), json.loads(y, strict=False)      # (ack and mode are printed raw)
        ix, iy = jx["iridium"], jy["iridium"]
        assert abs(ix["freq"] - iy["freq"]) <= 1 and abs(ix["sig_level"] - iy["sig_level"]) <= 0.011, (x, y)
        assert abs((ix["t"]["sec"] * 10**6 + ix["t"]["usec"]) - (iy["t"]["sec"] * 10**6 + iy["t"]["usec"])) <= 1, (x, y)
        for k in ("freq", "sig_level", "t"):
            del ix[k], iy[k]
        assert jx == jy


def check_known(text):
    """(b) what the generator put into the scene: every message meant to arrive does, the broken ones do not"""
    for msgs in _messages():
        for m in msgs:
            if m["expect"]:
                assert m["expect"] in text, m["expect"]
    for absent in (b"N606FF", b"N808HH", b"N414DE"):
        assert absent not in text


@pytest.mark.parametrize("fs", (2_000_000, 10_000_000))
@pytest.mark.parametrize("depth", (0, 3))
def test_packed_path_acars_equals_the_model(fs, depth):
    iq, ref = scene(fs)
    want, model = expected(ref)
    check_known(want)
    ob = oracle_bursts(ref)
    assert any(b and b["fixederrs"] > 0 for b, _ in ob)                       # Chase / BCH corrections happened
    assert any(b and not b["crc_ok"] for b, _ in ob)                          # and the bad-CRC bursts decoded as such
    dp, ip = run_pipeline(iq, fs, depth, 5)
    assert len(dp) == len(ip) == len(ref.demods)
    # the library, fed in uneven batches
    reasm = irdm.IdaReassembler()
    acars = irdm.AcarsPrinter(origin=ORIGIN)
    got, i, k = b"", 0, 1
    while i < len(dp):
        got += acars.format_packed_batch(reasm, dp[i:i + k], ip[i:i + k])
        i += k
        k = k * 2 % 29 + 1
    assert got == want
    assert acars.stats() == model.st
    assert acars.stats_text().decode() == model.stats_text()
    assert model.st["acars_errors"] >= 1 and model.st["sbd_multi_ok"] >= 2 and model.st["sbd_broken"] == 0
    # --acars-json --station, the same records all at once
    wj, _ = expected(ref, json_mode=True, station="GPU-TEST")
    aj = irdm.AcarsPrinter(json=True, station="GPU-TEST", origin=ORIGIN)
    gj = aj.format_packed_batch(irdm.IdaReassembler(), dp, ip)
    same_json(gj, wj)
    assert b"WRONG KERMIT" not in gj and b'"station":"GPU-TEST"' in gj


def _exe():
    exe = os.path.join(os.path.dirname(irdm.LIB_PATH), "iridium-sniffer-hip")
    if not os.path.exists(exe):
        irdm.build(force=True)
    return exe


def test_cli_acars(tmp_path):
    fs = 10_000_000
    iq, ref = scene(fs)
    path = tmp_path / "scene.cf32"
    np.ascontiguousarray(iq).tofile(path)
    base = [_exe(), "-f", str(path), "-r", str(fs), "--chunk", str(1 << 25), "--acars-origin", "%d" % ORIGIN[0]]
    want, model = expected(ref)
    stats = model.stats_text()

    def run(extra):
        r = subprocess.run(base + extra, capture_output=True, timeout=300)
        assert r.returncode == 0, r.stderr.decode()[-2000:]
        return r.stdout, r.stderr.decode("latin-1")

    for extra in (["--acars"], ["--save-bursts", str(tmp_path / "bursts"), "--acars"],
                  ["--gpus", "1", "--group-loopback", "--acars"]):
        out, err = run(extra)
        assert out == want, extra
        assert "ACARS: enabled (text output)\n" in err and err.endswith(stats), extra
    check_known(want)
    # JSON with a station, both ID forms
    wj, _ = expected(ref, json_mode=True, station="ST1")
    for extra in (["--acars-json", "--station", "ST1"], ["--acars", "--acars-json", "--station=ST1"]):
        out, err = run(extra)
        same_json(out, wj)
        assert "ACARS: enabled (JSON output, station set)\n" in err and err.endswith(stats)
    # --parsed --acars: the IDA lines where the burst decodes, no RAW line, each frame's ACARS lines behind its IDA line
    out, err = run(["--parsed", "--acars"])
    lines = out.split(b"\n")[:-1]
    n_ok = sum(1 for b, _ in oracle_bursts(ref) if b)
    assert sum(l.startswith(b"IDA: ") for l in lines) == n_ok
    assert not any(l.startswith(b"RAW: ") for l in lines)
    ac = [l for l in lines if l.startswith(b"ACARS: ")]
    assert b"\n".join(ac) + b"\n" == want
    for i, l in enumerate(lines):
        if l.startswith(b"ACARS: "):
            assert i > 0 and (lines[i - 1].startswith(b"IDA: ") or lines[i - 1].startswith(b"ACARS: "))
    # the IDA printer's t0 comes from the first IDA line (suppressed RAW lines do not set it)
    assert lines[0].startswith(b"IDA: p-")


@pytest.mark.parametrize("flag", ["--acars-udp=127.0.0.1:5555", "--feed", "--feed=udp://127.0.0.1:5558", "--gsmtap",
                                  "--web=8888", "--acars-udp"])
def test_cli_refuses_network_outputs(flag):
    r = subprocess.run([_exe(), "-f", "x.cf32", "-r", "2000000", "--acars", flag], capture_output=True, timeout=60)
    assert r.returncode == 2
    err = r.stderr.decode()
    assert "network output is not built" in err and "unknown option" not in err
