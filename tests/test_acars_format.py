"""irdm_acars_* (--acars / --acars-json) and tests/acars_model.py against the reference's own output.

tests/golden/acars_fixtures.json holds IDA messages and what the reference's acars_ida_cb / acars_print_stats printed for
them (sbd_acars.c built without libacars, the wall clock pinned; "provenance" says how), in text mode, JSON mode and JSON
mode with a station.  The library and the model must print the same bytes.  Runs without a GPU."""
import ctypes as C
import json
import os
import re
import time

import pytest

import acars_model as am
import irdm

HERE = os.path.dirname(os.path.abspath(__file__))
FIX = json.load(open(os.path.join(HERE, "golden", "acars_fixtures.json")))
ORIGIN = tuple(FIX["origin"])
HEADER = os.path.join(HERE, "..", "include", "irdm_hip.h")


def model_msgs():
    return [dict(m, data=bytes.fromhex(m["data"])) for m in FIX["messages"]]


def lib_msgs():
    out = []
    for m in FIX["messages"]:
        r = irdm.IdaMessage()
        d = bytes.fromhex(m["data"])
        r.data[:len(d)] = list(d)
        r.len, r.direction, r.timestamp = len(d), m["direction"], m["timestamp"]
        r.frequency, r.magnitude = m["frequency"], m["magnitude"]
        out.append(r)
    return out


RUNS = [(r["json"], r["station"]) for r in FIX["runs"]]


def _run(js, station):
    return next(r for r in FIX["runs"] if r["json"] == js and r["station"] == station)


def test_fixture_reaches_every_branch():
    """the corpus exercises what it is meant to: errors, every SBD path, NUL bytes, escapes, the JSON limits"""
    text, js = _run(0, None), _run(1, None)
    for s in ("NAK  ", "ACK:A ", "Label:_?", " CONT'd", " ERRORS", "SEQ:", "FNO:", "REG:AB123 ", "\0"):
        assert s in text["stdout"], s
    for s in ('"label":"_d"', '"reg":"..AB123"', '"more":true', '"header":"', '"flight":', '"msg_num_seq":', "\\u0001",
              '\\"', "\\\\", "\\t", "\\n", "\\r", "\\u007f"):
        assert s in js["stdout"], s
    assert '"station":"STN-01"' in _run(1, "STN-01")["stdout"]
    assert "broken/orphan" in text["stderr"] and "with errors" in text["stderr"]
    assert len(text["stdout"].splitlines()) > len(js["stdout"].splitlines())      # errors dropped in JSON mode
    assert max(len(l) for l in js["stdout"].splitlines()) > 2000                    # the escape limit is reached


@pytest.mark.parametrize("js,station", RUNS)
def test_model_equals_reference(js, station):
    ref = _run(js, station)
    m = am.Acars(json=js, station=station, origin=ORIGIN)
    assert m.feed(model_msgs()) == ref["stdout"]
    assert m.stats_text() == ref["stderr"]


@pytest.mark.parametrize("js,station", RUNS)
def test_library_equals_reference(js, station):
    ref = _run(js, station)
    a = irdm.AcarsPrinter(json=js, station=station, origin=ORIGIN)
    assert a.feed(lib_msgs()).decode("latin-1") == ref["stdout"]
    assert a.stats_text().decode("latin-1") == ref["stderr"]
    st = a.stats()
    mine = am.Acars(json=js, station=station, origin=ORIGIN)
    mine.feed(model_msgs())
    assert st == mine.st
    a.close()


@pytest.mark.parametrize("js,station", RUNS)
def test_chunking_independence(js, station):
    """the same messages one at a time, in uneven batches and all at once: the same bytes"""
    msgs = lib_msgs()
    one = irdm.AcarsPrinter(json=js, station=station, origin=ORIGIN)
    a = b"".join(one.feed([m]) for m in msgs)
    uneven = irdm.AcarsPrinter(json=js, station=station, origin=ORIGIN)
    b, i, k = b"", 0, 1
    while i < len(msgs):
        b += uneven.feed(msgs[i:i + k])
        i += k
        k = k % 7 + 2
    allat = irdm.AcarsPrinter(json=js, station=station, origin=ORIGIN)
    assert a == b == allat.feed(msgs) == _run(js, station)["stdout"].encode("latin-1")
    assert one.stats_text() == uneven.stats_text() == allat.stats_text()


def test_wall_clock_origin_without_a_fixed_one():
    """without an origin the first printed message reads CLOCK_REALTIME: the text lines carry today's date"""
    before = time.strftime("%Y-%m-%d", time.gmtime())
    out = irdm.AcarsPrinter(json=False).feed(lib_msgs()[:3]).decode("latin-1")
    after = time.strftime("%Y-%m-%d", time.gmtime())
    assert out.startswith("ACARS: ") and (before in out or after in out)


def test_small_buffer_is_refused():
    L = irdm.lib()
    a = irdm.AcarsPrinter(origin=ORIGIN)
    msgs = lib_msgs()[:2]
    arr = (irdm.IdaMessage * 2)(*msgs)
    buf = C.create_string_buffer(16)
    assert L.irdm_acars_feed(a._h, arr, 2, buf, 16) == -1
    assert L.irdm_acars_feed(None, arr, 2, buf, 16) == -1


# ---- the new C-ABI types against include/irdm_hip.h ----
def _struct_fields(name):
    src = open(HEADER).read()
    m = re.search(r"typedef struct \{([^}]*)\}\s*%s;" % name, src)
    assert m, name
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        typ, rest = decl.split(None, 1) if not decl.startswith("const ") else ("const char*", decl.split("*", 1)[1])
        for part in rest.split(","):
            part = part.strip().lstrip("*")
            fields.append((typ, re.sub(r"\[.*\]", "", part).strip(), re.search(r"\[(\d+)\]", part)))
    return fields


SIZES = {"uint8_t": 1, "int32_t": 4, "uint64_t": 8, "int64_t": 8, "double": 8, "float": 4, "const char*": 8}


@pytest.mark.parametrize("cname,py", [("irdm_ida_message_t", irdm.IdaMessage), ("irdm_acars_config_t", irdm.AcarsConfig),
                                      ("irdm_acars_stats_t", irdm.AcarsStats)])
def test_struct_layout_matches_header(cname, py):
    fields = _struct_fields(cname)
    assert [f[1] for f in fields] == [f[0] for f in py._fields_]
    off = 0
    for typ, name, arr in fields:
        size = SIZES[typ]
        off = (off + size - 1) // size * size
        assert getattr(py, name).offset == off, (cname, name)
        off += size * (int(arr.group(1)) if arr else 1)
    assert C.sizeof(py) == (off + 7) // 8 * 8 if cname != "irdm_acars_stats_t" else C.sizeof(py) == off
    assert C.sizeof(irdm.IdaMessage) == 288 and C.sizeof(irdm.AcarsConfig) == 32 and C.sizeof(irdm.AcarsStats) == 36
