#!/usr/bin/env python3
"""What --prime costs: the batch of tools/batch_rate.py (N recordings of the bench scene's generator, one seed each, written
to /dev/shm in this call so that their pages are warm) through ONE run of this commit's binary, wall time from process start
to exit, without and with --prime, alternating, --pairs times, per format.  Priming feeds 512 FFT frames more per recording
through the same pipeline (4.2 Mi samples at 10 MS/s beside a recording's 64 Mi): the expectation is a few per cent, and this
tool is what says whether that is so.

  python3 tools/prime_rate.py --out profiles/prime_rate.json
"""
import argparse
import json
import os
import re
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "iridium-sniffer_amd"))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
EXE = os.path.join(ROOT, "iridium-sniffer_amd", "iridium-sniffer-hip")

import batch_rate       # noqa: E402  (write_scenes: the same recordings)


def run(files, args, fmt, prime):
    """one process over all the files: wall seconds start to exit, its stderr"""
    cmd = [EXE] + sum((["-f", f] for f in files), []) + ["-r", str(args.fs), "--format", fmt, "--timing"] + (["--prime"] if prime else [])
    t0 = time.perf_counter()
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    wall = time.perf_counter() - t0
    if r.returncode != 0:
        raise SystemExit("%s failed (exit %d): %s" % (" ".join(cmd[:4]), r.returncode, r.stderr.decode("latin-1")[-2000:]))
    return wall, r.stderr.decode("latin-1"), r.stdout.count(b"\n")


def measure(args, fmt):
    files = batch_rate.write_scenes(args, fmt, args.tmp)
    try:
        rec = dict(format=fmt, files=args.files, samples_per_file=args.samples, pairs=[])
        run(files[:1], args, fmt, False)              # (the binary's pages warm before the first timed pair)
        for pair in range(args.pairs):
            one = dict(pair=pair)
            for prime in (False, True):
                w, err, lines = run(files, args, fmt, prime)
                tagged = [int(v) for v in re.findall(r"tagged (\d+) bursts", err)]
                assert len(tagged) == args.files, err[-2000:]
                one["primed" if prime else "plain"] = dict(wall_s=round(w, 4), lines=lines, tagged=sum(tagged))
            rec["pairs"].append(one)
        plain = [p["plain"]["wall_s"] for p in rec["pairs"]]
        primed = [p["primed"]["wall_s"] for p in rec["pairs"]]
        mean = lambda v: sum(v) / len(v)            # noqa: E731
        rec.update(plain_wall_s=[min(plain), max(plain)], primed_wall_s=[min(primed), max(primed)],
                   mean_extra_s=round(mean(primed) - mean(plain), 4), mean_extra_percent=round(100.0 * (mean(primed) / mean(plain) - 1.0), 2),
                   extra_per_recording_ms=round(1e3 * (mean(primed) - mean(plain)) / args.files, 2),
                   plain_spread_s=round(max(plain) - min(plain), 4),
                   extra_lines=rec["pairs"][0]["primed"]["lines"] - rec["pairs"][0]["plain"]["lines"])
        return rec
    finally:
        for f in files:
            os.remove(f)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--files", type=int, default=8)
    ap.add_argument("--samples", type=int, default=64 << 20)
    ap.add_argument("--fs", type=int, default=10_000_000)
    ap.add_argument("--density", type=float, default=10.0, help="bursts per Msample (the bench's default)")
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--formats", default="cf32,ci8")
    ap.add_argument("--tmp", default="/dev/shm")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    runs = []
    for fmt in args.formats.split(","):
        rec = measure(args, fmt)
        print(json.dumps(rec), flush=True)
        runs.append(rec)
    out = dict(what="N recordings through one run of the binary, without and with --prime, alternating; wall time from process start "
                    "to exit, files in /dev/shm written in the same call; lines: what the run printed on stdout",
               tool="python3 tools/prime_rate.py --files %d --pairs %d" % (args.files, args.pairs), gpu="MI355X (gfx950), one device",
               runs=runs)
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(out, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
