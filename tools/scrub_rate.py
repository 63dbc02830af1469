#!/usr/bin/env python3
"""Rate of the scrub kernel (csrc/scrub.hpp, irdm_scrub_device) per 64 Mi-sample cf32 chunk (512 MiB, resident) on three
inputs -- a clean chunk, a chunk with 1 % bad samples, a chunk that is all NaN -- beside iq_swap_kernel on the same buffer in
the same process as the yardstick (one read and one write of every byte).

  events   in one process, per input and round: `reps` launches between two events on one stream -- the scrub without
           statistics (scrub_kernel<false>, on the stream without waiting), then the exchange (applied an even number of
           times: the buffer is what it was).  A bad chunk is clean after its first pass, so for the two bad inputs every
           launch is preceded by a device-to-device copy that restores the chunk, and the same copies alone are timed as a
           third series: scrub_us is the difference.  Microseconds per chunk.
  kernel   per input one `rocprofv3 --kernel-trace --stats` run of its own (no counters) of the same worker, which there
           also makes `reps` calls WITH statistics (scrub_kernel<true>: the counting, the shuffles and the atomics; each call
           waits for its figures, so only the trace times it): the kernels' own spans.

  python3 tools/scrub_rate.py --out profiles/scrub_rate.json
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

INPUTS = ("clean", "sparse", "nan")
FMT_CF32 = 2


def make_input(torch, kind, chunk):
    x = torch.randn(2 * chunk, dtype=torch.float32, device="cuda:0")
    if kind == "sparse":
        bad = torch.rand(chunk, device="cuda:0") < 0.01
        x.view(chunk, 2)[bad, 0] = float("inf")
    elif kind == "nan":
        x.fill_(float("nan"))
    return x


def worker(args):
    import torch
    import irdm
    s = torch.cuda.Stream()                  # (a stream of its own: the library then launches on it and does not wait)
    out = []
    for kind in args.inputs.split(","):
        pristine = make_input(torch, kind, args.chunk)
        a = pristine.clone()
        restore = kind != "clean"
        torch.cuda.synchronize()
        for rnd in range(args.rounds + 1):                           # (round 0 warms up and is dropped)
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(6)]
            with torch.cuda.stream(s):
                ev[0].record(s)
                for _ in range(args.reps):
                    if restore:
                        a.copy_(pristine, non_blocking=True)
                    assert irdm.scrub_device(a.data_ptr(), args.chunk, FMT_CF32, 40, False, 0, s.cuda_stream)[0] == 0
                ev[1].record(s)
                ev[2].record(s)
                for _ in range(args.reps if restore else 0):
                    a.copy_(pristine, non_blocking=True)
                ev[3].record(s)
                ev[4].record(s)
                for _ in range(args.reps):
                    assert irdm.swap_iq_device(a.data_ptr(), args.chunk, FMT_CF32, 0, s.cuda_stream) == 0
                ev[5].record(s)
            torch.cuda.synchronize()
            if rnd:
                both, copy, swap = (ev[2 * i].elapsed_time(ev[2 * i + 1]) * 1e3 / args.reps for i in range(3))
                out.append(dict(input=kind, round=rnd, bytes=8 * args.chunk, scrub_us=round(both - copy, 1), restore_copy_us=round(copy, 1),
                                swap_us=round(swap, 1)))
        assert args.reps % 2 == 0                                    # (the exchanges cancel)
        # with statistics: the counting kernel; the figures are the input's
        figures = None
        for _ in range(args.reps):
            a.copy_(pristine)
            torch.cuda.synchronize()
            rc, st = irdm.scrub_device(a.data_ptr(), args.chunk, FMT_CF32, 40)
            assert rc == 0
            figures = dict(n_zeroed=int(st.n_zeroed), n_nonfinite=int(st.n_nonfinite), n_over=int(st.n_over))
        want = int((~torch.isfinite(pristine.view(args.chunk, 2))).any(dim=1).sum())
        assert figures["n_zeroed"] == want and bool(torch.isfinite(a).all()), (figures, want)
        out[-1]["figures"] = figures
        del a, pristine
    print(json.dumps(dict(runs=out, launches=args.reps * (args.rounds + 1), counted_launches=args.reps)), flush=True)


def spawn(argv, timeout=600):
    r = subprocess.run(argv, capture_output=True, text=True, timeout=timeout)
    if r.returncode != 0:
        sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
        raise SystemExit("%s failed (exit %d)" % (" ".join(argv[:6]), r.returncode))
    return json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--worker", action="store_true")
    ap.add_argument("--inputs", default=",".join(INPUTS))
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
    out = dict(what="scrub_kernel per cf32 chunk of %d samples on a clean chunk, one with 1 %% bad samples and one that is all NaN, beside "
                    "iq_swap_kernel<4> on the same buffer (events, one process; the bad inputs restored by a copy before every launch, "
                    "the copies' own time taken off), and the kernels' spans under rocprofv3 --kernel-trace --stats, one run per input"
                    % args.chunk,
               tool="python3 tools/scrub_rate.py", gpu="MI355X (gfx950), one device")
    out["events"] = spawn(common)
    print(json.dumps(out["events"]), flush=True)
    out["kernel_trace"] = {}
    for kind in args.inputs.split(","):
        with tempfile.TemporaryDirectory(dir=args.scratch) as d:
            spawn(["rocprofv3", "--kernel-trace", "--stats", "-d", d, "-o", "sb", "--output-format", "csv", "--"] + common + ["--inputs", kind])
            files = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
            if not files:
                raise SystemExit("no kernel_stats.csv under %s" % d)
            traced = []
            for row in csv.DictReader(open(files[0])):
                name = row.get("Name") or row.get("KernelName") or row.get("kernel")
                if "scrub_kernel" in name or "iq_swap_kernel" in name:
                    calls = int(row.get("Calls") or row.get("calls"))
                    total_ns = float(row.get("TotalDurationNs") or 0) or float(row.get("total_ms", 0)) * 1e6
                    traced.append(dict(kernel=name, calls=calls, us_per_chunk=round(total_ns / calls / 1e3, 1)))
            out["kernel_trace"][kind] = sorted(traced, key=lambda r: r["kernel"])
        print(kind, json.dumps(out["kernel_trace"][kind]), flush=True)
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(out, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
