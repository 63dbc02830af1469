#!/usr/bin/env python3
"""Cost of option "spectrum_frames" (KS, csrc/detect.hip: spectrum_partial_kernel + spectrum_rows_kernel) on the bench's
10 MHz scene, 64 Mi-sample chunks.

  kernel      per R (1220: about a second per row; 16), in a `rocprofv3 --kernel-trace --stats` run of its own: the spans of
              the two KS kernels per chunk, their algorithmic bytes -- the plane read once, 4 B per sample, plus the rows
              written -- over that time as bytes/s and as a fraction of the 8 TB/s HBM roofline; K1 (fft_mag_p32_kernel) from
              the same trace as the yardstick: 12 B per sample (cf32 in, the plane out)
  throughput  device-resident end to end at pipeline_depth 3, packed records polled per chunk, the chunk fed in place: one
              process, the option off, then on, alternating (profiler off)

  python3 tools/spectrum_rate.py --steps 10 --warmup 3 --out profiles/spectrum_rate.json --stats-out profiles/spectrum_kernel_stats
"""
import argparse
import csv
import glob
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "iridium-sniffer_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)

HBM_BYTES_PER_S = 8e12
ROWS = (1220, 16)


def scene_and_context(args, depth, R):
    import torch
    import bench
    import irdm
    x, nb = bench.build_scene(torch, "cuda:0", args.fs, args.chunk, args.density, seed=1)
    p = irdm.Pipeline(args.fs, fmt=irdm.FMT_CF32, max_chunk_samples=args.chunk, max_bursts_per_chunk=8192, pipeline_depth=depth)
    p.set_option("packed_records", 1)
    if R:
        p.set_option("spectrum_frames", R)
    return torch, irdm, x, nb, p


def poll(p, spectrum):
    p.poll_bursts_raw()
    p.drop_frames()
    n = len(p.poll_demods_packed_raw())
    rows = len(p.poll_spectrum()[0]) if spectrum else 0
    return n, rows


def worker_trace(args):
    """what the profiler watches: the resident chunk fed `steps` times with the option at args.rows"""
    torch, irdm, x, nb, p = scene_and_context(args, 0, args.rows)
    try:
        rows = 0
        for _ in range(args.warmup + args.steps):
            p.feed_device(x.data_ptr(), args.chunk)
            rows += poll(p, True)[1]
        p.flush()
        rows += poll(p, True)[1]
        torch.cuda.synchronize()
        print(json.dumps(dict(rows=rows, feeds=args.warmup + args.steps, frames_per_feed=args.chunk // p.fft_size, n=p.fft_size)), flush=True)
    finally:
        p.close()


def worker_throughput(args):
    import ctypes as C
    torch, irdm, x, nb, p_off = scene_and_context(args, 3, 0)
    p_on = scene_and_context(args, 3, args.rows)[4]
    L = irdm.lib()
    out = []
    try:
        for p in (p_off, p_on):
            ring_ptr, ring_len = p.ring()
            for k in range(ring_len // args.chunk):
                assert L.irdm_device_copy(C.c_void_p(ring_ptr + k * args.chunk * 8), C.c_void_p(x.data_ptr()), args.chunk * 8) == 0
        for rnd in range(args.rounds):
            for name, p in (("off", p_off), ("on", p_on)):
                frames = rows = 0
                for k in range(args.warmup + args.steps):
                    if k == args.warmup:
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        frames = rows = 0
                    p.feed_device(p.ingest_ptr(args.chunk), args.chunk)
                    a, b = poll(p, name == "on")
                    frames, rows = frames + a, rows + b
                p.flush()
                a, b = poll(p, name == "on")
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
                out.append(dict(option=name, round=rnd, gsamples_per_s=round(args.steps * args.chunk / dt / 1e9, 2),
                                frames_per_step=round((frames + a) / args.steps, 1), rows=rows + b))
                p.reset()
    finally:
        p_off.close()
        p_on.close()
    print(json.dumps(dict(rows_of=args.rows, bursts_per_chunk=nb, runs=out)), flush=True)


def spawn(argv, timeout=600):
    r = subprocess.run(argv, capture_output=True, text=True, timeout=timeout)
    if r.returncode != 0:
        sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
        raise SystemExit("%s failed (exit %d)" % (" ".join(argv[:6]), r.returncode))
    return json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])


def traced(args, R, common):
    """one profiler run at R: per kernel (calls, total ms) from its *kernel_stats.csv"""
    with tempfile.TemporaryDirectory(dir=args.scratch) as d:
        info = spawn(["rocprofv3", "--kernel-trace", "--stats", "-d", d, "-o", "ks", "--output-format", "csv", "--",
                      sys.executable, os.path.abspath(__file__), "--worker", "trace", "--rows", str(R)] + common)
        files = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
        if not files:
            raise SystemExit("no kernel_stats.csv under %s" % d)
        if args.stats_out:
            shutil.copy(files[0], "%s_r%d.csv" % (args.stats_out, R))
        stats = {}
        for row in csv.DictReader(open(files[0])):
            name = row.get("Name") or row.get("KernelName") or row.get("kernel")
            total_ns = float(row.get("TotalDurationNs") or 0) or float(row.get("total_ms", 0)) * 1e6
            stats[name] = (int(row.get("Calls") or row.get("calls")), total_ns)
    def of(sub):
        hit = [(c, t) for k, (c, t) in stats.items() if sub in k]
        return sum(c for c, _ in hit), sum(t for _, t in hit)
    feeds, n, frames = info["feeds"], info["n"], info["frames_per_feed"]
    pc, pt = of("spectrum_partial_kernel")
    rc_, rt = of("spectrum_rows_kernel")
    kc, kt = of("fft_mag_p32_kernel")
    assert pc == feeds and rc_ == feeds and kc == feeds, (pc, rc_, kc, feeds)
    ks_us, k1_us = (pt + rt) / feeds / 1e3, kt / feeds / 1e3
    rows_per_feed = info["rows"] / feeds
    alg = 4.0 * n * frames + 8.0 * n * rows_per_feed                  # the plane once, mean + peak of every row
    k1_alg = 12.0 * n * frames
    rec = dict(rows_of=R, feeds=feeds, rows_per_feed=round(rows_per_feed, 2),
               partial_us_per_chunk=round(pt / feeds / 1e3, 1), rows_us_per_chunk=round(rt / feeds / 1e3, 1),
               ks_us_per_chunk=round(ks_us, 1), algorithmic_bytes=int(alg), ks_GBps=round(alg / (ks_us * 1e-6) / 1e9, 1),
               hbm_roofline_fraction=round(alg / (ks_us * 1e-6) / HBM_BYTES_PER_S, 3),
               k1_us_per_chunk=round(k1_us, 1), k1_GBps=round(k1_alg / (k1_us * 1e-6) / 1e9, 1),
               ks_over_k1_bandwidth=round((alg / ks_us) / (k1_alg / k1_us), 3))
    return rec


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--worker", choices=("trace", "throughput"), default=None)
    ap.add_argument("--rows", type=int, default=ROWS[0])
    ap.add_argument("--fs", type=int, default=10_000_000)
    ap.add_argument("--chunk", type=int, default=64 << 20)
    ap.add_argument("--density", type=float, default=10.0, help="bursts per Msample (the bench's default)")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3, help="throughput: off / on pairs")
    ap.add_argument("--scratch", default=None, help="where the profiler's output goes before it is read (default: the system's)")
    ap.add_argument("--stats-out", default=None, help="keep each trace's kernel statistics as PREFIX_r<R>.csv")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.worker == "trace":
        return worker_trace(args)
    if args.worker == "throughput":
        return worker_throughput(args)
    common = ["--fs", str(args.fs), "--chunk", str(args.chunk), "--density", str(args.density), "--steps", str(args.steps),
              "--warmup", str(args.warmup)]
    kernel = []
    for R in ROWS:
        kernel.append(traced(args, R, common))
        print(json.dumps(kernel[-1]), flush=True)
    thr = spawn([sys.executable, os.path.abspath(__file__), "--worker", "throughput", "--rows", str(ROWS[0]), "--rounds", str(args.rounds)] + common)
    print(json.dumps(thr), flush=True)
    out = dict(what="option spectrum_frames (KS) on the bench's scene: kernel spans under rocprofv3 --kernel-trace --stats (pipeline_depth 0, "
                    "a run per R), device-resident throughput with the option off and on in one process (pipeline_depth 3, profiler off)",
               tool="python3 tools/spectrum_rate.py --steps %d --warmup %d" % (args.steps, args.warmup),
               gpu="MI355X (gfx950), one device", hbm_roofline_bytes_per_s=HBM_BYTES_PER_S, fs=args.fs, chunk=args.chunk,
               kernel=kernel, throughput=thr)
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(out, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
