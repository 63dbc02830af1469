#!/usr/bin/env python3
"""Rate of the I/Q exchange kernel (csrc/iq_swap.hpp, irdm_swap_iq_device) per 64 Mi-sample chunk, for component widths of
1, 2 and 4 bytes (ci8, ci16, cf32), beside a device-to-device copy of the same bytes in the same process -- the copy moves
the same traffic, one read and one write of every byte.

  events   in one process, per width and round: `reps` exchanges in place, then `reps` copies of the same buffer into a
           second one, each series between two events on one stream; microseconds per chunk, and the share of the HBM
           roofline (8 TB/s) over 2 x bytes.  The rounds alternate kernel and copy; the copy's spread between rounds is the
           yardstick for the difference.
  kernel   one `rocprofv3 --kernel-trace --stats` run of its own (no counters) of the same worker: the kernel's own span.

  python3 tools/iq_swap_rate.py --out profiles/iq_swap_rate.json
"""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "iridium-sniffer_amd"))

HBM_BYTES_PER_S = 8.0e12
WIDTHS = ((1, "ci8", 0), (2, "ci16", 1), (4, "cf32", 2))          # component bytes, name, IRDM_FMT_*


def worker(args):
    import torch
    import irdm
    s = torch.cuda.Stream()                  # (a stream of its own: the library then launches on it and does not wait)
    out = []
    for width, name, fmt in WIDTHS:
        nbytes = 2 * width * args.chunk
        a = torch.randint(0, 256, (nbytes,), dtype=torch.uint8, device="cuda:0")
        b = torch.empty_like(a)
        before = a[:4096].clone()
        torch.cuda.synchronize()
        for rnd in range(args.rounds + 1):                           # (round 0 warms up and is dropped)
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
            with torch.cuda.stream(s):
                ev[0].record(s)
                for _ in range(args.reps):
                    assert irdm.swap_iq_device(a.data_ptr(), args.chunk, fmt, 0, s.cuda_stream) == 0
                ev[1].record(s)
                ev[2].record(s)
                for _ in range(args.reps):
                    b.copy_(a, non_blocking=True)
                ev[3].record(s)
            torch.cuda.synchronize()
            if rnd:
                k_us, c_us = (ev[0].elapsed_time(ev[1]) * 1e3 / args.reps, ev[2].elapsed_time(ev[3]) * 1e3 / args.reps)
                out.append(dict(width=width, format=name, round=rnd, bytes=nbytes, kernel_us=round(k_us, 1), copy_us=round(c_us, 1),
                                kernel_roofline=round(2 * nbytes / (k_us * 1e-6) / HBM_BYTES_PER_S, 3),
                                copy_roofline=round(2 * nbytes / (c_us * 1e-6) / HBM_BYTES_PER_S, 3)))
        # an even number of exchanges: the buffer is what it was
        assert (args.reps * (args.rounds + 1)) % 2 == 1 or bool((a[:4096] == before).all())
        del a, b
    print(json.dumps(dict(runs=out, launches_per_width=args.reps * (args.rounds + 1))), flush=True)


def spawn(argv, timeout=600):
    r = subprocess.run(argv, capture_output=True, text=True, timeout=timeout)
    if r.returncode != 0:
        sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
        raise SystemExit("%s failed (exit %d)" % (" ".join(argv[:6]), r.returncode))
    return json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--worker", action="store_true")
    ap.add_argument("--chunk", type=int, default=64 << 20)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--scratch", default=None, help="where the profiler's output goes before it is read (default: the system's)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.worker:
        return worker(args)
    common = [sys.executable, os.path.abspath(__file__), "--worker", "--chunk", str(args.chunk), "--reps", str(args.reps),
              "--rounds", str(args.rounds)]
    out = dict(what="iq_swap_kernel per chunk of %d samples beside a device-to-device copy of the same bytes (events, one process, "
                    "alternating rounds), and the kernel's span under rocprofv3 --kernel-trace --stats in a run of its own" % args.chunk,
               tool="python3 tools/iq_swap_rate.py", gpu="MI355X (gfx950), one device", hbm_roofline_bytes_per_s=HBM_BYTES_PER_S)
    out["events"] = spawn(common)
    print(json.dumps(out["events"]), flush=True)
    with tempfile.TemporaryDirectory(dir=args.scratch) as d:
        info = spawn(["rocprofv3", "--kernel-trace", "--stats", "-d", d, "-o", "sw", "--output-format", "csv", "--"] + common)
        files = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
        if not files:
            raise SystemExit("no kernel_stats.csv under %s" % d)
        traced = []
        for row in csv.DictReader(open(files[0])):
            name = row.get("Name") or row.get("KernelName") or row.get("kernel")
            if "iq_swap_kernel" in name:
                calls = int(row.get("Calls") or row.get("calls"))
                total_ns = float(row.get("TotalDurationNs") or 0) or float(row.get("total_ms", 0)) * 1e6
                assert calls == info["launches_per_width"], (name, calls, info["launches_per_width"])
                traced.append(dict(kernel=name, calls=calls, us_per_chunk=round(total_ns / calls / 1e3, 1)))
        out["kernel_trace"] = sorted(traced, key=lambda r: r["kernel"])
    print(json.dumps(out["kernel_trace"]), flush=True)
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(out, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
