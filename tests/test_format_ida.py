"""irdm_format_ida / irdm_format_parsed_packed_batch (the --parsed lines) against the reference's own printers.

Where oracle/_ref is built, the reference's frame_output_print_ida (frame_output.c:203-361) and frame_output_print (through
ref_frame_output_line) print the same records in a child process -- they write to stdout and keep a static t0 -- and the
text must be ours byte for byte; its SHA-256 must also be the one recorded in tests/golden/ida_lines.json
(IRDM_WRITE_GOLDEN=1 records it).  Where oracle/_ref is not built, our text is checked against that recorded digest.
The records go through irdm_ida_unpack first, so the LCW header text is format_lcw_header's."""
import ctypes as C
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import irdm
import orc

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "ida_lines.json")

_CHILD = r'''
import ctypes as C, json, os, sys
R = C.CDLL(sys.argv[1])
libc = C.CDLL(None)
spec = json.loads(sys.stdin.read())

class Lcw(C.Structure):
    _fields_ = [("ft", C.c_int), ("lcw_ok", C.c_int), ("lcw_ft", C.c_int), ("lcw_code", C.c_int), ("lcw3_val", C.c_uint32),
                ("ec_lcw", C.c_int)]

class IdaBurst(C.Structure):             # ida_burst_t, ida_decode.h:31-54
    _fields_ = [("timestamp", C.c_uint64), ("frequency", C.c_double), ("direction", C.c_int), ("magnitude", C.c_float),
                ("noise", C.c_float), ("level", C.c_float), ("confidence", C.c_int), ("n_symbols", C.c_int),
                ("da_ctr", C.c_int), ("da_len", C.c_int), ("cont", C.c_int), ("payload", C.c_uint8 * 32),
                ("payload_len", C.c_int), ("crc_ok", C.c_int), ("stored_crc", C.c_uint16), ("computed_crc", C.c_uint16),
                ("fixederrs", C.c_int), ("bch_stream", C.c_uint8 * 256), ("bch_len", C.c_int), ("lcw", Lcw),
                ("lcw_header", C.c_char * 128)]

R.ref_frame_output_line.argtypes = [C.c_uint64, C.c_uint64, C.c_double, C.c_float, C.c_float, C.c_int, C.c_float,
                                    C.c_int, C.c_int, C.POINTER(C.c_uint8), C.c_char_p, C.c_int]
fi_keep = C.create_string_buffer(spec["file_info"].encode())       # frame_output_init keeps the pointer
R.ref_frame_output_init(fi_keep if spec["file_info"] else None)
for it in spec["items"]:
    if it["kind"] == "ida":
        b = IdaBurst()
        for k, v in it.items():
            if k in ("kind", "payload", "bch_stream", "lcw_header"):
                continue
            setattr(b, k, v)
        b.payload[:] = it["payload"]
        b.bch_stream[:] = it["bch_stream"]
        b.lcw_header = it["lcw_header"].encode()
        R.frame_output_print_ida(C.byref(b))
        libc.fflush(None)
    else:
        bits = (C.c_uint8 * max(1, len(it["bits"])))(*it["bits"])
        buf = C.create_string_buffer(4096)
        n = R.ref_frame_output_line(it["id"], it["timestamp"], it["center_frequency"], it["magnitude"], it["noise"],
                                    it["confidence"], it["level"], it["n_payload_symbols"], it["n_bits"], bits, buf, 4096)
        assert n > 0
        os.write(1, buf.raw[:n])
'''


def _ref_text(items, file_info):
    ref = orc.ref()
    spec = json.dumps(dict(file_info=file_info, items=items)).encode()
    r = subprocess.run([sys.executable, "-c", _CHILD, ref._name], input=spec,
                       capture_output=True, text=False, timeout=120)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    return r.stdout


_want = json.load(open(GOLDEN)) if os.path.exists(GOLDEN) else {}
_recorded = {}


@pytest.fixture(scope="module", autouse=True)
def _record():
    yield
    if _recorded:
        want = json.load(open(GOLDEN)) if os.path.exists(GOLDEN) else {}
        want.update(_recorded)
        with open(GOLDEN, "w") as f:
            json.dump(want, f, indent=1, sort_keys=True)
            f.write("\n")


def pin(key, ours, items, file_info):
    """ours (bytes) is the reference's text for items, live where oracle/_ref is built, by its recorded digest elsewhere"""
    if orc.ref() is not None:
        ref = _ref_text(items, file_info)
        assert ours == ref, key
        if os.environ.get("IRDM_WRITE_GOLDEN") == "1":
            _recorded[key] = hashlib.sha256(ref).hexdigest()
            return
    assert key in _want, "%s: no recorded reference output (IRDM_WRITE_GOLDEN=1 where oracle/_ref is built)" % key
    assert hashlib.sha256(ours).hexdigest() == _want[key], "%s differs from the reference's recorded output" % key


def pack_bits(bits, n_bytes):
    out = [0] * n_bytes
    for i, b in enumerate(bits):
        out[i >> 3] |= int(b) << (7 - (i & 7))
    return out


def make_pairs(seed, n):
    """(IdaPacked, DemodPacked) pairs over the printer's cases: da_len 0 / 1 / 20 / other, zero and non-zero payload tails,
    bch_len < 20, 180..196 and up to 256, any SBD byte, CRC ok / not, level 0 and below, negative n_symbols, UL / DL,
    frequencies ending in .5"""
    rng = np.random.default_rng(seed)
    t = 1700000000 * 10**9 + int(rng.integers(0, 10**9))
    out = []
    for k in range(n):
        ip = irdm.IdaPacked()
        ip.ok = 1
        ip.ft = 2
        ip.lcw_ft = int(rng.integers(0, 4))
        ip.lcw_code = int(rng.choice([0, 1, 3, 6, 12, 15, int(rng.integers(0, 16))]))
        ip.lcw3_val = int(rng.integers(0, 1 << 21))
        ip.ec_lcw = int(rng.integers(0, 4))
        ip.da_len = (0, 1, 20, int(rng.integers(2, 20)))[k % 4]
        ip.da_ctr = int(rng.integers(0, 8))
        ip.cont = int(rng.integers(0, 2))
        ip.crc_ok = int(k % 3 == 0)
        ip.stored_crc = int(rng.integers(0, 1 << 16))
        ip.computed_crc = 0 if ip.crc_ok else int(rng.integers(0, 1 << 16))
        ip.fixederrs = int(rng.integers(0, 12))
        ip.payload_len = ip.da_len if ip.da_len > 0 else 20
        pl = [int(b) for b in rng.integers(0, 256, 32)]
        if k % 5 in (1, 2) and ip.da_len > 0:                  # the tail behind da_len all zero (payload[da_len] aside)
            for i in range(ip.da_len + 1, 32):
                pl[i] = 0
        if k % 8 == 6:                                         # printable SBD bytes
            pl[:20] = [int(b) for b in rng.integers(32, 127, 20)]
        ip.payload[:] = pl
        ip.bch_len = int(rng.choice([int(rng.integers(0, 20)), int(rng.integers(180, 197)), 200, 216, 240, 256,
                                     int(rng.integers(197, 257))]))
        ip.bch_stream[:] = pack_bits(rng.integers(0, 2, min(ip.bch_len, 256)), 32)
        dp = irdm.DemodPacked()
        dp.id = int(rng.integers(0, 10**7)) * 10
        t += int(rng.integers(1, 10**9))
        dp.timestamp = t
        f = float(rng.uniform(1.616e9, 1.6265e9))
        dp.center_frequency = float(int(f)) + 0.5 if k % 6 == 1 else f
        dp.direction = 2 if k % 2 else 1
        dp.magnitude = float(np.float32(rng.uniform(-5, 60)))
        dp.noise = float(np.float32(rng.uniform(-140, -80)))
        dp.confidence = int(rng.integers(0, 101))
        dp.level = (0.0, float(np.float32(-rng.uniform(0, 1))), float(np.float32(rng.uniform(1e-4, 2))),
                    float(np.float32(rng.uniform(0.01, 1))))[k % 7 if k % 7 < 4 else 3]
        dp.n_symbols = int(rng.integers(20, 445))
        dp.n_payload_symbols = -int(rng.integers(1, 12)) if k % 9 == 4 else dp.n_symbols - 12
        dp.n_bits = 2 * dp.n_symbols
        dp.ok = 1
        dp.bits[:] = [int(b) for b in rng.integers(0, 256, irdm.MAX_BITS // 8)]
        out.append((ip, dp))
    return out


def ida_item(b):
    return dict(kind="ida", timestamp=b.timestamp, frequency=b.frequency, direction=b.direction, magnitude=b.magnitude,
                noise=b.noise, level=b.level, confidence=b.confidence, n_symbols=b.n_symbols, da_ctr=b.da_ctr,
                da_len=b.da_len, cont=b.cont, payload=list(b.payload), payload_len=b.payload_len, crc_ok=b.crc_ok,
                stored_crc=b.stored_crc, computed_crc=b.computed_crc, fixederrs=b.fixederrs,
                bch_stream=list(b.bch_stream), bch_len=b.bch_len, lcw_header=b.lcw_header.decode())


def raw_item(d):
    bits = [(d.bits[i >> 3] >> (7 - (i & 7))) & 1 for i in range(d.n_bits)]
    return dict(kind="raw", id=d.id, timestamp=d.timestamp, center_frequency=d.center_frequency, magnitude=d.magnitude,
                noise=d.noise, confidence=d.confidence, level=d.level, n_payload_symbols=d.n_payload_symbols,
                n_bits=d.n_bits, bits=bits)


def test_ida_unpack_fields():
    ip, dp = make_pairs(5, 1)[0]
    b = irdm.ida_unpack(ip, dp)
    assert (b.ok, b.ft, b.da_len, b.bch_len, b.id, b.timestamp, b.frequency, b.direction, b.n_symbols) == \
           (1, 2, ip.da_len, ip.bch_len, dp.id, dp.timestamp, dp.center_frequency, dp.direction, dp.n_payload_symbols)
    assert bytes(b.payload) == bytes(ip.payload)
    assert [b.bch_stream[i] for i in range(256)] == [(ip.bch_stream[i >> 3] >> (7 - (i & 7))) & 1 for i in range(256)]
    assert b.lcw_header.startswith(b"LCW(2,T:") and len(b.lcw_header) == 111
    ip.ok = 0
    assert irdm.ida_unpack(ip, dp).ok == 0


@pytest.mark.parametrize("file_info", ("golden", ""))
@pytest.mark.parametrize("seed", (0, 1))
def test_format_ida_matches_the_reference(seed, file_info):
    pairs = make_pairs(seed, 60)
    idas = [irdm.ida_unpack(ip, dp) for ip, dp in pairs]
    lines = irdm.format_ida(idas)
    assert all(l.startswith("IDA: p-17") and l.endswith("\n") for l in lines)
    assert any(" ---   " in l for l in lines) and any("!" in l.split("[")[1] for l in lines if "[" in l)
    assert any("-99.99|" in l for l in lines) and any(" UL " in l for l in lines) and any(" SBD: " in l for l in lines)
    ours = "".join(lines).encode("latin-1")
    pin("ida_lines/%d/%s" % (seed, file_info or "auto"), ours, [ida_item(b) for b in idas], file_info)


@pytest.mark.parametrize("first", ("ida", "raw"))
@pytest.mark.parametrize("file_info", ("golden", ""))
def test_parsed_batch_matches_the_reference(first, file_info):
    pairs = make_pairs(3, 48)
    for k, (ip, dp) in enumerate(pairs):
        if (k % 3 == 1) or (k == 0 and first == "raw"):
            ip.ok = 0
    if first == "ida":
        pairs[0][0].ok = 1
    dps = [dp for _, dp in pairs]
    ips = [ip for ip, _ in pairs]
    text = irdm.format_parsed_packed_batch(dps, ips, file_info or None)
    # the batch is the per-line concatenation, one t0 for both kinds
    L = irdm.lib()
    t0 = C.c_uint64(0)
    buf = C.create_string_buffer(4096)
    per = []
    for ip, dp in pairs:
        if ip.ok:
            n = L.irdm_format_ida(C.byref(irdm.ida_unpack(ip, dp)), C.byref(t0), buf, 4096)
        else:
            n = L.irdm_format_raw_packed(C.byref(dp), file_info.encode() if file_info else None, C.byref(t0), buf, 4096)
        assert n > 0
        per.append(buf.raw[:n].decode("latin-1"))
    assert text == "".join(per)
    assert text.startswith("IDA: " if first == "ida" else "RAW: ")
    items = [ida_item(irdm.ida_unpack(ip, dp)) if ip.ok else raw_item(dp) for ip, dp in pairs]
    pin("parsed_batch/%s/%s" % (first, file_info or "auto"), text.encode("latin-1"), items, file_info)
