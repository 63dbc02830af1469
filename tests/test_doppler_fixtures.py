"""--position's positioning engine (csrc/doppler.cpp) against the reference's own doppler_pos.c.

tests/golden/doppler_fixtures.json holds a synthetic IRA measurement corpus (its provenance says how it was made) and, for
height aiding at 0 m and at 300 m, what the reference's doppler_pos.c returned at every solve of the stream-time schedule
(every doppler_solution_t field as an exact double) and the POSITION lines it printed.  The library must return the same
doubles bit for bit through irdm_doppler_add / irdm_doppler_solve, and print the same bytes through the batch formatter.
No GPU: the engine is host code."""
import json
import math
import os

import pytest

import irdm

HERE = os.path.dirname(os.path.abspath(__file__))
FIX = json.load(open(os.path.join(HERE, "golden", "doppler_fixtures.json")))
FIELDS = ("lat", "lon", "alt", "hdop")


def records():
    out = []
    for r in FIX["records"]:
        d = irdm.Decoded()
        d.type, d.sat_id = r[0], r[1]
        d.pos_xyz[:] = r[2:5]
        d.lat, d.lon, d.frequency = (float.fromhex(v) for v in r[5:8])
        d.timestamp = r[8]
        d.id = len(out)
        out.append(d)
    return out


def scheduled_solves(dop, recs, origin, end_ns):
    """the schedule by hand: a solve for tick T before the first record at or past T s, the ticks up to end_ns, a final one"""
    got, tick = [], 10
    for d in recs:
        while d.timestamp - origin >= tick * 10**9:
            got.append((tick,) + dop.solve())
            tick += 10
        dop.add(d)
    while end_ns - origin >= tick * 10**9:
        got.append((tick,) + dop.solve())
        tick += 10
    got.append((-1,) + dop.solve())
    return got


def ecef(lat, lon, h):
    la, lo = math.radians(lat), math.radians(lon)
    e2 = 2 / 298.257223563 - (1 / 298.257223563) ** 2
    n = 6378137.0 / math.sqrt(1 - e2 * math.sin(la) ** 2)
    return ((n + h) * math.cos(la) * math.cos(lo), (n + h) * math.cos(la) * math.sin(lo), (n * (1 - e2) + h) * math.sin(la))


def test_corpus_covers_the_paths():
    kinds = {(r[0], r[1]) for r in FIX["records"]}
    assert (1, 0) in kinds and (2, 17) in kinds and (0, 17) in kinds          # sat 0, an IBC and an undecoded record
    lats = [float.fromhex(r[5]) for r in FIX["records"]]
    assert max(lats) > 90                                                    # coordinates out of range
    span = (FIX["records"][-1][8] - FIX["records"][0][8]) / 1e9
    assert span > 40 * 60                                                    # measurements age past 30 min
    assert "doppler_pos.c" in FIX["provenance"] and "verbose = 1" in FIX["provenance"]
    assert {run["height_m"] for run in FIX["runs"]} == {0.0, 300.0}
    # what the reference's own verbose diagnostics counted on this corpus: every screening path of add_measurement and
    # solve is taken at both heights
    for run in FIX["runs"]:
        paths = run["reference_paths"]
        for k in ("velocity_rejects", "gap_resets", "visibility_rejects", "satellite_drops", "jump_rejects", "jump_accepts"):
            assert paths[k] >= 1, (run["height_m"], k)


@pytest.mark.parametrize("run", range(2))
def test_solutions_bit_for_bit(run):
    spec = FIX["runs"][run]
    dop = irdm.Doppler(spec["height_m"], FIX["origin_ns"])
    got = scheduled_solves(dop, records(), FIX["origin_ns"], FIX["end_ns"])
    want = spec["solves"]
    assert len(got) == len(want)
    for (tick, ret, s), w in zip(got, want):
        assert (tick, ret) == (w[0], w[1])
        assert [getattr(s, f).hex() for f in FIELDS] == [float.fromhex(v).hex() for v in w[2:6]], tick
        assert (s.n_measurements, s.n_satellites, s.converged) == tuple(w[6:9]), tick
    # the last solution of each phase lies near that phase's receiver: 20 km (phase 1: five clean passes and a biased
    # satellite the screening drops), 1 km (phase 2, reached after the jump guard gave in)
    for truth, lo, hi, tol in ((FIX["truth"][0], 0, 700, 20e3), (FIX["truth"][1], 2860, 10**9, 1e3)):
        last = [w for w in want if w[1] and lo < (w[0] if w[0] > 0 else 10**9) <= hi][-1]
        a = ecef(float.fromhex(last[2]), float.fromhex(last[3]), truth["height_m"])
        b = ecef(truth["lat"], truth["lon"], truth["height_m"])
        assert math.dist(a, b) < tol, (last[0], math.dist(a, b))


@pytest.mark.parametrize("run", range(2))
@pytest.mark.parametrize("batch", (1, 7, 4096))
def test_formatted_lines_byte_for_byte(run, batch):
    spec = FIX["runs"][run]
    dop = irdm.Doppler(spec["height_m"], FIX["origin_ns"])
    recs = records()
    text = "".join(dop.format_batch(recs[i:i + batch]) for i in range(0, len(recs), batch))
    text += dop.finish(FIX["end_ns"])
    assert text == spec["stderr"]
    assert "POSITION: waiting" in text and text.count("POSITION: ") >= 100


def test_schedule_on_stream_time():
    """records spanning 0-75 s, no measurement usable: solves at 10 .. 70 s and at the end, the waiting line only at 60 s
    and at the end; the same records that do solve print a line at every tick"""
    origin = 1_700_000_000_000_000_000
    dop = irdm.Doppler(0.0, origin)
    recs = []
    for k in range(76):
        d = irdm.Decoded()
        d.type, d.timestamp = 0, origin + k * 10**9 + 123
        recs.append(d)
    text = dop.format_batch(recs[:33]) + dop.format_batch(recs[33:]) + dop.finish(origin + 75 * 10**9)
    assert text == "POSITION: waiting (0 sats, 0 meas)\n" * 2
    # the corpus's records, shifted so that the first solve succeeds early: one line per tick between the first and the
    # last solution; the direct solves tell which ticks ran
    full = records()
    t_first = next(w[0] for w in FIX["runs"][0]["solves"] if w[1])
    base = FIX["origin_ns"] + (t_first - 30) * 10**9
    window = [d for d in full if base <= d.timestamp < base + 75 * 10**9]
    for d in window:
        d.timestamp = d.timestamp - base + origin
    a = irdm.Doppler(0.0, origin)
    text = a.format_batch(window) + a.finish(origin + 75 * 10**9)
    b = irdm.Doppler(0.0, origin)
    solves = scheduled_solves(b, window, origin, origin + 75 * 10**9)
    assert [t for t, _, _ in solves] == [10, 20, 30, 40, 50, 60, 70, -1]
    want = ""
    for t, r, s in solves:
        if r:
            want += "POSITION: %.6f, %.6f (HDOP=%.1f, %d sats, %d meas)\n" % (s.lat, s.lon, s.hdop, s.n_satellites,
                                                                            s.n_measurements)
        elif t in (60, -1):
            want += "POSITION: waiting (%d sats, %d meas)\n" % (s.n_satellites, s.n_measurements)
    assert text == want and sum(r for _, r, _ in solves) >= 1


def test_only_ira_records_are_measurements():
    dop = irdm.Doppler(0.0, FIX["origin_ns"])
    recs = records()
    taken = [dop.add(d) for d in recs]
    assert sum(taken) >= 500
    for d, t in zip(recs, taken):
        if d.type != 1 or d.sat_id == 0 or not -90 <= d.lat <= 90 or not -180 <= d.lon <= 180:
            assert t == 0
