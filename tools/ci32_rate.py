#!/usr/bin/env python3
"""Cost of the int32 load stage (IRDM_FMT_CI32) beside cf32's: both move 8 bytes per sample, so any difference is the
conversion's instructions (one v_cvt_f32_i32 per component and a packed multiply per sample).

One process under `rocprofv3 --kernel-trace`: the bench's 10 MHz scene as cf32 and, quantised at scale 2^33, as ci32, each
through a context of its own (pipeline_depth 0, the chunk resident), fed alternately: `rounds` times `steps` feeds of cf32,
then of ci32.  From the trace, per round and format, the mean span per launch of K1 (fft_mag_p32_kernel<13, F>) and of the
register decimator (fir_decimate_kernel_f<40, F>).  The spread of the cf32 rounds is the yardstick for the difference.

  python3 tools/ci32_rate.py --steps 6 --warmup 2 --rounds 3 --out profiles/ci32_rate.json
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
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)

KERNELS = (("k1", "fft_mag_p32_kernel<13, %d,", "fft_mag_p32_kernelILi13ELi%dE"),
           ("decimator", "fir_decimate_kernel_f<40, %d>", "fir_decimate_kernel_fILi40ELi%dE"))
FORMATS = (("cf32", 2), ("ci32", 8))


def worker(args):
    import torch
    import bench
    import irdm
    x, nb = bench.build_scene(torch, "cuda:0", args.fs, args.chunk, args.density, seed=1)
    v = torch.clamp(torch.round(x.to(torch.float64) * 2.0 ** 33), -2.0 ** 31, 2.0 ** 31 - 1).to(torch.int32)
    torch.cuda.synchronize()
    ctx = {}
    for name, code in FORMATS:
        p = irdm.Pipeline(args.fs, fmt=code, max_chunk_samples=args.chunk, max_bursts_per_chunk=8192, pipeline_depth=0)
        p.set_option("packed_records", 1)
        ctx[name] = (p, x if code == 2 else v)
    frames = {name: 0 for name, _ in FORMATS}
    try:
        for name, _ in FORMATS:                         # warm-up: both contexts, outside the rounds that are read
            p, buf = ctx[name]
            for _ in range(args.warmup):
                p.feed_device(buf.data_ptr(), args.chunk)
                p.poll_bursts_raw()
                p.drop_frames()
                p.poll_demods_packed_raw()
        for _ in range(args.rounds):
            for name, _ in FORMATS:
                p, buf = ctx[name]
                for _ in range(args.steps):
                    p.feed_device(buf.data_ptr(), args.chunk)
                    p.poll_bursts_raw()
                    p.drop_frames()
                    frames[name] += len(p.poll_demods_packed_raw())
        torch.cuda.synchronize()
    finally:
        for p, _ in ctx.values():
            p.close()
    print(json.dumps(dict(bursts_per_chunk=nb, feeds_per_round=args.steps, warmup_feeds=args.warmup, rounds=args.rounds,
                          frames_per_feed={k: round(f / (args.rounds * args.steps), 1) for k, f in frames.items()})), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--worker", action="store_true")
    ap.add_argument("--fs", type=int, default=10_000_000)
    ap.add_argument("--chunk", type=int, default=64 << 20)
    ap.add_argument("--density", type=float, default=10.0, help="bursts per Msample (the bench's default)")
    ap.add_argument("--steps", type=int, default=6)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--scratch", default=None, help="where the profiler's output goes before it is read (default: the system's)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.worker:
        return worker(args)
    common = ["--fs", str(args.fs), "--chunk", str(args.chunk), "--density", str(args.density), "--steps", str(args.steps),
              "--warmup", str(args.warmup), "--rounds", str(args.rounds)]
    with tempfile.TemporaryDirectory(dir=args.scratch) as d:
        r = subprocess.run(["rocprofv3", "--kernel-trace", "-d", d, "-o", "ci32", "--output-format", "csv", "--",
                            sys.executable, os.path.abspath(__file__), "--worker"] + common, capture_output=True, text=True, timeout=900)
        if r.returncode != 0:
            sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
            raise SystemExit("the traced run failed (exit %d)" % r.returncode)
        info = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
        files = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
        if not files:
            raise SystemExit("no kernel_trace.csv under %s" % d)
        rows = []
        for row in csv.DictReader(open(files[0])):
            name = row.get("Kernel_Name") or row.get("Name") or row.get("KernelName")
            rows.append((int(row["Start_Timestamp"]), int(row["End_Timestamp"]), name))
    rows.sort()
    out = dict(what="K1 (fft_mag_p32_kernel<13, F>) and the register decimator (fir_decimate_kernel_f<40, F>) for cf32 and ci32 on "
                    "the bench's scene, one process under rocprofv3 --kernel-trace, the formats fed alternately; us per launch, "
                    "per round of feeds",
               tool="python3 tools/ci32_rate.py --steps %d --warmup %d --rounds %d" % (args.steps, args.warmup, args.rounds),
               gpu="MI355X (gfx950), one device", fs=args.fs, chunk=args.chunk, run=info)
    for label, pat, mangled in KERNELS:
        for name, code in FORMATS:
            spans = [e - s for s, e, k in rows if k and (pat % code in k or mangled % code in k)]
            per_feed = len(spans) // (args.warmup + args.rounds * args.steps) if spans else 0
            assert per_feed >= 1 and len(spans) == per_feed * (args.warmup + args.rounds * args.steps), (label, name, len(spans))
            timed = spans[per_feed * args.warmup:]
            per_round = per_feed * args.steps
            us = [round(sum(timed[i * per_round:(i + 1) * per_round]) / per_round / 1e3, 2) for i in range(args.rounds)]
            out["%s_%s" % (label, name)] = dict(launches_per_feed=per_feed, us_per_launch_by_round=us,
                                                us_per_launch=round(sum(timed) / len(timed) / 1e3, 2))
            print(json.dumps({("%s_%s" % (label, name)): out["%s_%s" % (label, name)]}), flush=True)
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(out, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
