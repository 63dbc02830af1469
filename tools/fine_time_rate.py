#!/usr/bin/env python3
"""Cost of option "fine_time" (csrc/fine_time.hpp, fine_time_kernel) on the bench's 10 MHz scene, 64 Mi-sample chunks.

  kernel      one `rocprofv3 --kernel-trace --stats` run of its own (no counters): the scene through a context with the
              options fine_time, fine_freq and symbol_clock on at pipeline_depth 0, the chunk resident; the kernel's span
              per chunk, beside symbol_clock_kernel's, fine_freq_kernel's, the decimator's and the demodulator's last kernel
              of the same run, and the binary64 operations the estimator needs (2 per sample of the window and point, 17
              points; a frame's window is taken as min(n, 1310) samples) over that span.
  throughput  the scene device-resident at pipeline_depth 3, packed records polled per chunk, the chunk fed in place: one
              process, the option off, then on, alternating (profiler off)

  python3 tools/fine_time_rate.py --steps 10 --warmup 3 --out profiles/fine_time_rate.json
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

GRID, OPS_PER_POINT, WINDOW = 17, 2, 1310         # Goertzel on a real input: one subtraction and one fused multiply-add per sample and point


def scene(args, torch, bench):
    return bench.build_scene(torch, "cuda:0", args.fs, args.chunk, args.density, seed=1)


def poll_all(p):
    p.poll_bursts_raw()
    p.drop_frames()
    p.poll_symbol_clock_raw()
    p.poll_fine_freq_raw()
    return len(p.poll_demods_packed_raw()), p.poll_fine_time_raw()


def worker_kernel(args):
    """what the profiler watches: `warmup + steps` feeds of the resident chunk with the option on"""
    import numpy as np
    import torch
    import bench
    import irdm
    x, nb = scene(args, torch, bench)
    p = irdm.Pipeline(args.fs, fmt=irdm.FMT_CF32, max_chunk_samples=args.chunk, max_bursts_per_chunk=8192, pipeline_depth=0)
    p.set_option("packed_records", 1)
    p.set_option("symbol_clock", 1)
    p.set_option("fine_freq", 1)
    p.set_option("fine_time", 1)
    frames = samples = launches = 0
    for _ in range(args.warmup + args.steps):
        p.feed_device(x.data_ptr(), args.chunk)
        n, fine = poll_all(p)
        frames += n
        if len(fine):
            launches += 1
            samples += int(np.minimum(np.frombuffer(fine.tobytes(), dtype=np.uint32).reshape(len(fine), 16)[:, 15], WINDOW).sum())
    torch.cuda.synchronize()
    st = p.fine_time()
    assert p.stat("fine_time_launches") == launches
    p.close()
    print(json.dumps(dict(feeds=args.warmup + args.steps, bursts_per_chunk=nb, launches=launches, frames=frames, frame_samples=samples,
                          frames_applied=int(st.frames_applied), frames_ambiguous=int(st.frames_ambiguous),
                          frames_invalid=int(st.frames_invalid), median_samples=st.median)), flush=True)


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
            p.set_option("fine_time", 1)
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
                    frames += poll_all(p)[0]
                p.flush()
                frames += poll_all(p)[0]
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
                rec = dict(option=name, round=rnd, gsamples_per_s=round(args.steps * args.chunk / dt / 1e9, 2),
                           frames_per_step=round(frames / args.steps, 1))
                if name == "on":
                    st = p.fine_time()
                    rec.update(frames_applied=int(st.frames_applied), median_samples=st.median)
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
        info = spawn(["rocprofv3", "--kernel-trace", "--stats", "-d", d, "-o", "ft", "--output-format", "csv", "--",
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
    ap.add_argument("--fs", type=int, default=10_000_000)
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
    common = ["--fs", str(args.fs), "--chunk", str(args.chunk), "--density", str(args.density), "--steps", str(args.steps),
              "--warmup", str(args.warmup)]
    skip = set(args.skip.split(","))
    out = dict(what="option fine_time: fine_time_kernel's span per chunk under rocprofv3 --kernel-trace --stats (a run of its "
                    "own, no counters; pipeline_depth 0; symbol_clock and fine_freq on beside it); device-resident throughput "
                    "with the option off and on in one process (pipeline_depth 3, profiler off)",
               tool="python3 tools/fine_time_rate.py --steps %d --warmup %d" % (args.steps, args.warmup),
               gpu="MI355X (gfx950), one device", fs=args.fs, chunk=args.chunk)
    if "kernel" not in skip:
        info, stats = traced(args, "kernel", common)

        def span(pat):
            hit = [(c, t) for k, (c, t) in stats.items() if pat in k]
            return sum(c for c, _ in hit), sum(t for _, t in hit)
        calls, total = span("fine_time_kernel")
        assert calls == info["launches"] and calls > 0, (calls, info, sorted(stats))
        us = total / calls / 1e3
        ops = float(OPS_PER_POINT) * GRID * info["frame_samples"] / calls
        rec = dict(info, us_per_chunk=round(us, 1), binary64_ops_per_chunk=ops, binary64_tops_per_s=round(ops / (us * 1e-6) / 1e12, 2))
        for label, pat in (("symbol_clock", "symbol_clock_kernel"), ("fine_freq", "fine_freq_kernel"), ("decimator", "fir_decimate"), ("demod_par", "demod_par_kernel")):
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
