#!/usr/bin/env python3
"""Cost of option "input_stats" (csrc/input_stats.hpp, input_stats_kernel) and of the cu8 load stage.

  kernel      per format (ci8, cu8, ci16-full, cf32), one `rocprofv3 --kernel-trace --stats` run of its own: the kernel's span
              per 64 Mi-sample chunk through irdm_input_stats_device on a device-resident buffer.  The kernel reads b_in bytes
              per sample and writes nothing but its sums: b_in * n bytes over the span as bytes/s and as a fraction of the
              8 TB/s HBM roofline.
  formats     the bench's 10 MHz scene quantised to ci8 and to cu8 (scale 512), each through a context of its own in the
              same traced run: the register decimator's and K1's spans per chunk, cu8 against ci8.
  throughput  the bench's scene device-resident at pipeline_depth 3, packed records polled per chunk, the chunk fed in place:
              one process, the option off, then on, alternating (profiler off)

  python3 tools/input_stats_rate.py --steps 10 --warmup 3 --out profiles/input_stats_rate.json
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

HBM_BYTES_PER_S = 8e12
FORMATS = (("ci8", 0, 2), ("cu8", 6, 2), ("ci16-full", 3, 4), ("cf32", 2, 8))


def worker_kernel(args):
    """what the profiler watches: irdm_input_stats_device over one resident buffer per format, `steps` times each"""
    import torch
    import irdm
    g = torch.Generator(device="cuda:0")
    g.manual_seed(3)
    res = {}
    for name, code, bps in FORMATS:
        if code == 2:
            x = torch.randn((args.chunk, 2), generator=g, device="cuda:0", dtype=torch.float32) * 0.3
        elif bps == 2:
            x = torch.randint(0, 256, (args.chunk, 2), generator=g, device="cuda:0", dtype=torch.uint8)
        else:
            x = torch.randint(-32768, 32768, (args.chunk, 2), generator=g, device="cuda:0", dtype=torch.int16)
        torch.cuda.synchronize()
        for _ in range(args.warmup + args.steps):
            st = irdm.input_stats_device(x.data_ptr(), args.chunk, code)
        res[name] = dict(n_samples=int(st.n_samples), rails=int(st.n_rail_lo[0] + st.n_rail_hi[0]))
        del x
    print(json.dumps(dict(calls=args.warmup + args.steps, formats=res)), flush=True)


def scene(args, torch, bench):
    return bench.build_scene(torch, "cuda:0", args.fs, args.chunk, args.density, seed=1)


def worker_formats(args):
    """the bench's scene as ci8 and as cu8 through a context each (pipeline_depth 0, the chunk resident)"""
    import torch
    import bench
    import irdm
    x, nb = scene(args, torch, bench)
    q8 = torch.clamp(torch.round(x * 512.0), -128, 127).to(torch.int8)
    u8 = torch.clamp(torch.round(x * 512.0 + 127.5), 0, 255).to(torch.uint8)
    del x
    torch.cuda.synchronize()
    out = {}
    for name, code, buf in (("ci8", irdm.FMT_CI8, q8), ("cu8", irdm.FMT_CU8, u8)):
        p = irdm.Pipeline(args.fs, fmt=code, max_chunk_samples=args.chunk, max_bursts_per_chunk=8192, pipeline_depth=0)
        p.set_option("packed_records", 1)
        frames = 0
        for _ in range(args.warmup + args.steps):
            p.feed_device(buf.data_ptr(), args.chunk)
            p.poll_bursts_raw()
            p.drop_frames()
            frames += len(p.poll_demods_packed_raw())
        torch.cuda.synchronize()
        out[name] = dict(frames_per_feed=round(frames / (args.warmup + args.steps), 1))
        p.close()
    print(json.dumps(dict(feeds=args.warmup + args.steps, bursts_per_chunk=nb, formats=out)), flush=True)


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
            p.set_option("input_stats", 1)
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
                    p.poll_bursts_raw()
                    p.drop_frames()
                    frames += len(p.poll_demods_packed_raw())
                p.flush()
                p.poll_bursts_raw()
                p.drop_frames()
                frames += len(p.poll_demods_packed_raw())
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
                rec = dict(option=name, round=rnd, gsamples_per_s=round(args.steps * args.chunk / dt / 1e9, 2),
                           frames_per_step=round(frames / args.steps, 1))
                if name == "on":
                    rec["n_samples"] = int(p.input_stats().n_samples)
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
        info = spawn(["rocprofv3", "--kernel-trace", "--stats", "-d", d, "-o", "is", "--output-format", "csv", "--",
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
    ap.add_argument("--worker", choices=("kernel", "formats", "throughput"), default=None)
    ap.add_argument("--fs", type=int, default=10_000_000)
    ap.add_argument("--chunk", type=int, default=64 << 20)
    ap.add_argument("--density", type=float, default=10.0, help="bursts per Msample (the bench's default)")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3, help="throughput: off / on pairs")
    ap.add_argument("--scratch", default=None, help="where the profiler's output goes before it is read (default: the system's)")
    ap.add_argument("--skip", default="", help="comma list of parts to leave out: kernel, formats, throughput")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.worker:
        return {"kernel": worker_kernel, "formats": worker_formats, "throughput": worker_throughput}[args.worker](args)
    common = ["--fs", str(args.fs), "--chunk", str(args.chunk), "--density", str(args.density), "--steps", str(args.steps),
              "--warmup", str(args.warmup)]
    skip = set(args.skip.split(","))
    out = dict(what="option input_stats: input_stats_kernel's span per chunk per format under rocprofv3 --kernel-trace --stats "
                    "(irdm_input_stats_device, a run of its own); the cu8 and ci8 instantiations of the register decimator and K1 on the "
                    "bench's scene in one traced run; device-resident throughput with the option off and on in one process "
                    "(pipeline_depth 3, profiler off)",
               tool="python3 tools/input_stats_rate.py --steps %d --warmup %d" % (args.steps, args.warmup),
               gpu="MI355X (gfx950), one device", hbm_roofline_bytes_per_s=HBM_BYTES_PER_S, fs=args.fs, chunk=args.chunk)
    if "kernel" not in skip:
        info, stats = traced(args, "kernel", common)
        rows = []
        for name, code, bps in FORMATS:
            hit = [(c, t) for k, (c, t) in stats.items() if "input_stats_kernel<%d>" % code in k or "input_stats_kernelILi%dE" % code in k]
            calls, total = sum(c for c, _ in hit), sum(t for _, t in hit)
            assert calls == info["calls"], (name, calls, info["calls"], sorted(stats))
            us = total / calls / 1e3
            alg = float(bps) * args.chunk
            rows.append(dict(format=name, bytes_per_sample=bps, us_per_chunk=round(us, 1), GBps=round(alg / (us * 1e-6) / 1e9, 1),
                             hbm_roofline_fraction=round(alg / (us * 1e-6) / HBM_BYTES_PER_S, 3),
                             gsamples_per_s=round(args.chunk / (us * 1e-6) / 1e9, 1)))
            print(json.dumps(rows[-1]), flush=True)
        out["kernel"] = rows
    if "formats" not in skip:
        info, stats = traced(args, "formats", common)
        rec = dict(feeds=info["feeds"], bursts_per_chunk=info["bursts_per_chunk"], frames_per_feed=info["formats"])
        for label, pat, mangled in (("decimator", "fir_decimate_kernel_f<40, %d>", "fir_decimate_kernel_fILi40ELi%dE"),
                                    ("k1", "fft_mag_p32_kernel<13, %d,", "fft_mag_p32_kernelILi13ELi%dE")):
            for name, code in (("ci8", 0), ("cu8", 6)):
                hit = [(c, t) for k, (c, t) in stats.items() if pat % code in k or mangled % code in k]
                calls, total = sum(c for c, _ in hit), sum(t for _, t in hit)
                rec["%s_%s_us_per_launch" % (label, name)] = round(total / max(calls, 1) / 1e3, 1)
                rec["%s_%s_launches" % (label, name)] = calls
        print(json.dumps(rec), flush=True)
        out["cu8_against_ci8"] = rec
    if "throughput" not in skip:
        out["throughput"] = spawn([sys.executable, os.path.abspath(__file__), "--worker", "throughput", "--rounds", str(args.rounds)] + common)
        print(json.dumps(out["throughput"]), flush=True)
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(out, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
