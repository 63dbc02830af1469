#!/usr/bin/env python3
"""Cost of option "burst_resample" (csrc/burst_resample.hpp, burst_resample_kernel) on the bench's scene declared at 10.24 MS/s
(1025/1024), 64 Mi-sample chunks.

  kernel      one `rocprofv3 --kernel-trace --stats` run of its own (no counters): the scene through a context with the
              option on at pipeline_depth 0, the chunk resident; the kernel's span per chunk, beside the decimator's and the
              demodulator's last kernel of the same run, and the multiply-adds it needs (2 x 20 per output) over that span.
  throughput  the scene device-resident at pipeline_depth 3, packed records polled per chunk, the chunk fed in place: one
              process, the option off, then on, alternating (profiler off)

The same capture through --resample-to (K0r, 1000/1024) is tools/resample_rate.py's measurement.

  python3 tools/burst_resample_rate.py --steps 10 --warmup 3 --out profiles/burst_resample_rate.json
"""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "iridium-sniffer_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)

TAPS = 20                             # per phase: 2 x TAPS fused multiply-adds per complex output


def scene(args, torch, bench):
    # (the bench's scene as it is: built for 10 MS/s, declared at args.fs)
    return bench.build_scene(torch, "cuda:0", args.scene_fs, args.chunk, args.density, seed=1)


def poll_all(p):
    p.poll_bursts_raw()
    p.drop_frames()
    return len(p.poll_demods_packed_raw())


def worker_kernel(args):
    """what the profiler watches: `warmup + steps` feeds of the resident chunk with the option on"""
    import torch
    import bench
    import irdm
    x, nb = scene(args, torch, bench)
    p = irdm.Pipeline(args.fs, fmt=irdm.FMT_CF32, max_chunk_samples=args.chunk, max_bursts_per_chunk=8192, pipeline_depth=0)
    p.set_option("packed_records", 1)
    p.set_option("burst_resample", 1)
    frames = 0
    for _ in range(args.warmup + args.steps):
        p.feed_device(x.data_ptr(), args.chunk)
        frames += poll_all(p)
    torch.cuda.synchronize()
    launches, outputs = p.stat("burst_resample_launches"), p.stat("scratch_peak")
    ratio = p.burst_resample_ratio()
    p.close()
    print(json.dumps(dict(feeds=args.warmup + args.steps, bursts_per_chunk=nb, launches=launches, frames=frames, ratio=list(ratio),
                          row_outputs_peak=outputs)), flush=True)


def worker_throughput(args):
    import ctypes as C
    import torch
    import bench
    import irdm
    x, nb = scene(args, torch, bench)
    L = irdm.lib()
    ctx = {}
    for name in ("off", "on"):
        p = irdm.Pipeline(args.fs, fmt=irdm.FMT_CF32, max_chunk_samples=args.chunk, max_bursts_per_chunk=8192, pipeline_depth=3)
        p.set_option("packed_records", 1)
        if name == "on":
            p.set_option("burst_resample", 1)
        ring_ptr, ring_len = p.ring()
        for k in range(ring_len // args.chunk):
            assert L.irdm_device_copy(C.c_void_p(ring_ptr + k * args.chunk * 8), C.c_void_p(x.data_ptr()), args.chunk * 8) == 0
        ctx[name] = p
    out = []
    try:
        for rnd in range(args.rounds):
            for name in ("off", "on"):
                p = ctx[name]
                frames = 0
                for k in range(args.warmup + args.steps):
                    if k == args.warmup:
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        frames = 0
                    p.feed_device(p.ingest_ptr(args.chunk), args.chunk)
                    frames += poll_all(p)
                p.flush()
                frames += poll_all(p)
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
                rec = dict(option=name, round=rnd, gsamples_per_s=round(args.steps * args.chunk / dt / 1e9, 2),
                           frames_per_step=round(frames / args.steps, 1))
                rec.update(launches=p.stat("burst_resample_launches"))
                out.append(rec)
                p.reset()
    finally:
        for p in ctx.values():
            p.close()
    print(json.dumps(dict(bursts_per_chunk=nb, runs=out)), flush=True)


def spawn(argv, timeout=600):
    r = subprocess.run(argv, capture_output=True, text=True, timeout=timeout)
    if r.returncode != 0:
        sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
        raise SystemExit("%s failed (exit %d)" % (" ".join(argv[:6]), r.returncode))
    return json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])


def traced(args, worker, common):
    """one profiler run of a worker: (its JSON line, {kernel name: (calls, total ns)})"""
    with tempfile.TemporaryDirectory(dir=args.scratch) as d:
        info = spawn(["rocprofv3", "--kernel-trace", "--stats", "-d", d, "-o", "br", "--output-format", "csv", "--",
                      sys.executable, os.path.abspath(__file__), "--worker", worker] + common)
        files = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
        if not files:
            raise SystemExit("no kernel_stats.csv under %s" % d)
        stats = {}
        for row in csv.DictReader(open(files[0])):
            name = row.get("Name") or row.get("KernelName") or row.get("kernel")
            total_ns = float(row.get("TotalDurationNs") or 0) or float(row.get("total_ms", 0)) * 1e6
            stats[name] = (int(row.get("Calls") or row.get("calls")), total_ns)
    return info, stats


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--worker", choices=("kernel", "throughput"), default=None)
    ap.add_argument("--fs", type=int, default=10_240_000, help="the rate the context is declared at")
    ap.add_argument("--scene-fs", type=int, default=10_000_000, help="the rate the bench's scene is built for")
    ap.add_argument("--chunk", type=int, default=64 << 20)
    ap.add_argument("--density", type=float, default=10.0, help="bursts per Msample (the bench's default)")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3, help="throughput: off / on pairs")
    ap.add_argument("--scratch", default=None, help="where the profiler's output goes before it is read (default: the system's)")
    ap.add_argument("--skip", default="", help="comma list of parts to leave out: kernel, throughput")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.worker:
        return {"kernel": worker_kernel, "throughput": worker_throughput}[args.worker](args)
    common = ["--fs", str(args.fs), "--scene-fs", str(args.scene_fs), "--chunk", str(args.chunk), "--density", str(args.density), "--steps", str(args.steps),
              "--warmup", str(args.warmup)]
    skip = set(args.skip.split(","))
    out = dict(what="option burst_resample: burst_resample_kernel's span per chunk under rocprofv3 --kernel-trace --stats (a run of "
                    "its own, no counters; pipeline_depth 0); device-resident throughput with the option off and on in one process "
                    "(pipeline_depth 3, profiler off)",
               tool="python3 tools/burst_resample_rate.py --steps %d --warmup %d" % (args.steps, args.warmup),
               gpu="MI355X (gfx950), one device", fs=args.fs, chunk=args.chunk)
    if "kernel" not in skip:
        info, stats = traced(args, "kernel", common)

        def span(pat):
            hit = [(c, t) for k, (c, t) in stats.items() if pat in k]
            return sum(c for c, _ in hit), sum(t for _, t in hit)
        calls, total = span("burst_resample_kernel")
        assert calls == info["launches"] and calls > 0, (calls, info, sorted(stats))
        us = total / calls / 1e3
        fma = 2.0 * TAPS * info["row_outputs_peak"]           # (an upper estimate: the largest batch's padded rows)
        rec = dict(info, us_per_chunk=round(us, 1), fma_per_chunk_at_most=fma, commit_us_per_chunk=round(span("burst_resample_commit")[1] / calls / 1e3, 1))
        for label, pat in (("decimator", "fir_decimate"), ("demod_par", "demod_par_kernel")):
            c, t = span(pat)
            rec["%s_us_per_chunk" % label] = round(t / max(info["feeds"], 1) / 1e3, 1)
            rec["%s_launches" % label] = c
        print(json.dumps(rec), flush=True)
        out["kernel"] = rec
    if "throughput" not in skip:
        out["throughput"] = spawn([sys.executable, os.path.abspath(__file__), "--worker", "throughput", "--rounds", str(args.rounds)] + common)
        print(json.dumps(out["throughput"]), flush=True)
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(out, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
