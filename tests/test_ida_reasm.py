"""irdm_ida_reasm_push / _push_packed (multi-burst IDA reassembly, ida_decode.c:669-748) on randomised burst sequences.

Where oracle/_ref is built, the reference's own ida_reassemble + ida_reassemble_flush run the same sequence and their
messages must be ours field for field; the SHA-256 of that output must also be the one recorded in
tests/golden/ida_reasm.json (IRDM_WRITE_GOLDEN=1 records it).  Where oracle/_ref is not built, our output is checked
against that recorded digest.  tests/acars_model.py's IdaReasm must agree everywhere.  Runs without a GPU."""
import ctypes as C
import hashlib
import json
import os
import struct

import numpy as np
import pytest

import acars_model as am
import irdm
import orc

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "ida_reasm.json")


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


class IdaSlot(C.Structure):              # ida_reassembly_t, ida_decode.h:58-66
    _fields_ = [("active", C.c_int), ("direction", C.c_int), ("frequency", C.c_double), ("last_timestamp", C.c_uint64),
                ("last_ctr", C.c_int), ("data", C.c_uint8 * 256), ("data_len", C.c_int)]


class IdaContext(C.Structure):           # ida_context_t, ida_decode.h:70-75
    _fields_ = [("slots", IdaSlot * 16)]


MSG_CB = C.CFUNCTYPE(None, C.POINTER(C.c_uint8), C.c_int, C.c_uint64, C.c_double, C.c_int, C.c_float, C.c_void_p)


def scenario(seed, n=1200):
    """frames in stream order: IDA bursts of up to 24 concurrent messages (UL / DL, channel jitter around the 260 Hz edge,
    gaps around 280 ms, ctr wrap, out-of-order timestamps, > 256 bytes), bad CRCs, da_len 0, and frames that only flush"""
    rng = np.random.default_rng(seed)
    t = 10_000_000_000
    frames = []
    streams = []
    for _ in range(n):
        t += int(rng.integers(500_000, 4_000_000)) if rng.random() < 0.97 else 300_000_000
        r = rng.random()
        if r < 0.12:                                                 # not IDA: flush only
            frames.append(dict(ok=0, timestamp=t))
            continue
        if r < 0.2 or not streams:
            streams.append(dict(dir=int(rng.choice([1, 2])), f=1.6215e9 + float(rng.integers(0, 30)) * 41667.0,
                                ctr=int(rng.choice([0, 0, 0, 5])), left=int(rng.integers(1, 20)), t=t))
            if len(streams) > 24:
                streams.pop(0)
        s = streams[int(rng.integers(0, len(streams)))]
        q = rng.random()
        if q < 0.04:
            ts = s["t"] - int(rng.integers(1, 1_000_000))            # earlier than the slot's last burst
        elif q < 0.10:
            ts = s["t"] + int(rng.choice([0, 279_999_999, 280_000_000, 280_000_001]))
        else:
            ts = t
        s["t"] = max(s["t"], ts)
        t = max(t, ts)
        df = float(rng.uniform(-60.0, 60.0)) if rng.random() < 0.85 else \
            float(rng.choice([259.9, 260.0, 260.1, -260.0, -300.0]))
        da_len = 20 if rng.random() < 0.8 else int(rng.choice([0, 1, 5, 31]))
        s["left"] -= 1
        cont = 1 if s["left"] > 0 else 0
        if rng.random() < 0.03:
            cont = 1 - cont
        ctr = s["ctr"] if rng.random() > 0.03 else int(rng.integers(0, 8))
        s["ctr"] = (s["ctr"] + 1) % 8
        payload = [int(x) for x in rng.integers(0, 256, 32)]
        frames.append(dict(ok=1, crc_ok=int(rng.random() > 0.03), da_ctr=ctr, da_len=da_len, cont=cont,
                           payload=payload, direction=s["dir"], timestamp=ts, frequency=s["f"] + df,
                           magnitude=float(np.float32(rng.uniform(0.001, 40.0)))))
        if s["left"] <= 0:
            streams.remove(s)
    return frames


def msg_bytes(msgs):
    out = b""
    for m in msgs:
        out += struct.pack("<iiQdf", len(m["data"]), m["direction"], m["timestamp"], m["frequency"], m["magnitude"])
        out += bytes(m["data"])
    return out


def ours(frames, packed=False, batch=64):
    r = irdm.IdaReassembler()
    out = []
    for i in range(0, len(frames), batch):
        chunk = frames[i:i + batch]
        if packed:
            ds, ps = [], []
            for f in chunk:
                d, p = irdm.DemodPacked(), irdm.IdaPacked()
                d.timestamp = f["timestamp"]
                if f["ok"]:
                    d.direction, d.center_frequency, d.magnitude = f["direction"], f["frequency"], f["magnitude"]
                    p.ok, p.crc_ok, p.da_ctr, p.da_len, p.cont = 1, f["crc_ok"], f["da_ctr"], f["da_len"], f["cont"]
                    p.payload[:] = f["payload"]
                ds.append(d)
                ps.append(p)
            got = r.push_packed(ds, ps)
        else:
            recs = []
            for f in chunk:
                b = irdm.Ida()
                b.timestamp = f["timestamp"]
                if f["ok"]:
                    b.ok, b.crc_ok, b.da_ctr, b.da_len, b.cont = 1, f["crc_ok"], f["da_ctr"], f["da_len"], f["cont"]
                    b.payload[:] = f["payload"]
                    b.direction, b.frequency, b.magnitude = f["direction"], f["frequency"], f["magnitude"]
                recs.append(b)
            got = r.push(recs)
        out += [dict(data=bytes(m.data[:m.len]), direction=m.direction, timestamp=m.timestamp, frequency=m.frequency,
                     magnitude=m.magnitude) for m in got]
    r.close()
    return out


def model(frames):
    r = am.IdaReasm()
    out = []
    for f in frames:
        m = r.push(f if f["ok"] else None, f["timestamp"])
        if m:
            out.append(m)
    return out


def reference(frames):
    R = orc.ref()
    R.ida_reassemble.argtypes = [C.POINTER(IdaContext), C.POINTER(IdaBurst), MSG_CB, C.c_void_p]
    R.ida_reassemble_flush.argtypes = [C.POINTER(IdaContext), C.c_uint64]
    ctx = IdaContext()
    out = []

    def cb(data, n, ts, freq, direction, mag, user):
        out.append(dict(data=bytes(data[:n]), direction=direction, timestamp=ts, frequency=freq, magnitude=mag))

    ccb = MSG_CB(cb)
    for f in frames:
        if f["ok"]:
            b = IdaBurst()
            b.timestamp, b.frequency, b.direction, b.magnitude = f["timestamp"], f["frequency"], f["direction"], f["magnitude"]
            b.da_ctr, b.da_len, b.cont, b.crc_ok = f["da_ctr"], f["da_len"], f["cont"], f["crc_ok"]
            b.payload[:] = f["payload"]
            R.ida_reassemble(C.byref(ctx), C.byref(b), ccb, None)
        R.ida_reassemble_flush(C.byref(ctx), f["timestamp"])
    return out


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


@pytest.mark.parametrize("seed", range(6))
def test_reassembly_matches_the_reference(seed):
    frames = scenario(seed)
    got = ours(frames)
    assert msg_bytes(got) == msg_bytes(model(frames))
    assert msg_bytes(got) == msg_bytes(ours(frames, packed=True, batch=37))
    assert msg_bytes(got) == msg_bytes(ours(frames, batch=1))
    assert len(got) >= 20
    key = "ida_reasm_seed%d" % seed
    if orc.ref() is not None:
        ref = msg_bytes(reference(frames))
        assert msg_bytes(got) == ref
        if os.environ.get("IRDM_WRITE_GOLDEN") == "1":
            _recorded[key] = hashlib.sha256(ref).hexdigest()
            return
    assert key in _want, "%s: no recorded reference output (IRDM_WRITE_GOLDEN=1 where oracle/_ref is built)" % key
    assert hashlib.sha256(msg_bytes(got)).hexdigest() == _want[key]


def test_scenarios_reach_the_edges():
    """the sequences hold multi-burst messages of up to 8+ bursts (ctr wrap: test_edges_by_hand, overflow too); 17+ open
    slots evict the oldest"""
    multi = longest = 0
    for seed in range(6):
        for m in model(scenario(seed)):
            multi += len(m["data"]) > 31
            longest = max(longest, len(m["data"]))
    assert multi >= 20 and longest > 160
    # 17+ concurrent open slots: eviction happens
    r = am.IdaReasm()
    for k in range(18):
        r.push(dict(ok=1, crc_ok=1, da_ctr=0, da_len=20, cont=1, payload=[k] * 32, direction=1, timestamp=1000 + k,
                    frequency=1.62e9 + 1000.0 * k, magnitude=1.0), 1000 + k)
    assert all(s is not None for s in r.slots) and r.slots[0]["frequency"] == 1.62e9 + 16000.0


def test_edges_by_hand():
    """ctr 7 -> 0 continues a slot; 260 Hz and 280 ms are inside, 260.1 Hz / 280 ms + 1 ns are not; past 256 bytes the
    payload is dropped while the slot goes on; a frame that only flushes closes a stale slot"""
    def b(ctr, cont, ts, df=0.0, da_len=20, crc=1, fill=1):
        return dict(ok=1, crc_ok=crc, da_ctr=ctr, da_len=da_len, cont=cont, payload=[fill] * 32, direction=1,
                    timestamp=ts, frequency=1.6e9 + df, magnitude=2.0)
    ms = 1_000_000
    seq = [b(0, 1, 0)] + [b(k % 8, 1, k * 280 * ms, df=260.0 if k % 2 else -260.0) for k in range(1, 13)] + \
        [b(13 % 8, 0, 13 * 280 * ms)]
    frames = seq + [b(0, 1, 10**10), b(1, 0, 10**10 + 280 * ms + 1)]          # gap too long: orphan
    frames += [b(0, 1, 2 * 10**10), b(1, 0, 2 * 10**10 + ms, df=260.1)]        # too far apart in frequency
    frames += [b(0, 1, 3 * 10**10), b(1, 1, 3 * 10**10 + ms, crc=0), b(1, 0, 3 * 10**10 + 2 * ms, da_len=0)]
    frames += [b(0, 1, 4 * 10**10), dict(ok=0, timestamp=4 * 10**10 + 281 * ms), b(1, 0, 4 * 10**10 + 282 * ms)]
    got = ours(frames)
    assert msg_bytes(got) == msg_bytes(model(frames))
    assert len(got) == 1 and len(got[0]["data"]) == 240 and got[0]["frequency"] == 1.6e9     # 14 x 20 B, 12 kept
    if orc.ref() is not None:
        assert msg_bytes(got) == msg_bytes(reference(frames))


def test_push_refuses_a_short_output():
    L = irdm.lib()
    r = irdm.IdaReassembler()
    recs = (irdm.Ida * 2)()
    out = (irdm.IdaMessage * 1)()
    assert L.irdm_ida_reasm_push(r._h, recs, 2, out, 1) == -1
    assert L.irdm_ida_reasm_push(None, recs, 2, out, 2) == -1
    assert L.irdm_ida_reasm_push(r._h, recs, 2, out, 2) == 0
