#!/usr/bin/env python3
"""Cost of saving the band (irdm_frontend_save, csrc/frontend.hip requant_kernel): a 50 MS/s ci8 capture, D = 5, the
bench's 10 MHz scene behind the front end (the capture of tools/frontend_rate.py).

  trace    the requantiser's span per 64 Mi-output chunk, ci8 and ci16, from a `rocprofv3 --kernel-trace --stats` run of its
           own (irdm_frontend_run_device on the resident capture, saving on, the sink discarding): bytes per second and the
           fraction of the 8 TB/s HBM roofline over the algorithmic bytes (8 + 2 or 8 + 4 per sample), K0 of the same trace
           beside it
  e2e      irdm_frontend_feed_device of the resident capture into a pipeline_depth 3 context, packed records polled per
           chunk, in one process: saving off, then on as ci8 / ci16 / cf32, each with the staged copy (the default) and with
           the kernel storing into the pinned slot itself (IRDM_SAVE_DIRECT=1), the variants in turn, `--rounds` times over

  python3 tools/saveband_rate.py --out profiles/saveband_rate.json [--trace-dir DIR]
"""
import argparse
import csv
import ctypes as C
import glob
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "iridium-sniffer_amd"))
sys.path.insert(0, ROOT)

HBM_BYTES_PER_S = 8e12
OUT_BYTES = {"ci8": 2, "ci16": 4, "cf32": 8}


def capture(torch, bench, irdm, args):
    """the bench's scene zero-stuffed by D, scaled by D, rotated by the shift, as ci8 (tools/frontend_rate.py)"""
    D, n = args.decim, args.chunk
    x, nb = bench.build_scene(torch, "cuda:0", args.fs, n, args.density, seed=1)
    fe = irdm.Frontend(args.fs * D, irdm.FMT_CI8, D, args.shift)
    q = int(round(fe.applied_shift_hz * 65536 / (args.fs * D)))
    fe.close()
    cap = torch.zeros(n * D, dtype=torch.complex64, device="cuda:0")
    cap[::D] = x.reshape(-1).view(torch.complex64) if x.dtype != torch.complex64 else x
    idx = (torch.arange(0, n * D, D, device="cuda:0", dtype=torch.int64) * q) % 65536
    cap[::D] *= torch.polar(torch.full_like(idx, float(D), dtype=torch.float32), idx.to(torch.float32) * (2.0 * np.pi / 65536.0))
    cap = torch.clamp(torch.round(torch.view_as_real(cap) * 256.0), -128, 127).to(torch.int8).reshape(-1)
    torch.cuda.synchronize()
    return cap, nb


def saving(irdm, fe, fmt, direct, count):
    """saving on with a sink that only counts (no copy on the host); returns the callback (to be kept alive)"""
    code = {"ci8": irdm.FMT_CI8, "ci16": irdm.FMT_CI16, "cf32": irdm.FMT_CF32}[fmt]

    def sink(user, ptr, n):
        count[0] += n
        return 0
    cb = irdm.BAND_SINK(sink)
    os.environ["IRDM_SAVE_DIRECT"] = "1" if direct else "0"
    cfg = irdm.FrontendSaveConfig(code, 1.0, 0, cb, None)
    if irdm.lib().irdm_frontend_save(fe.h, C.byref(cfg)) != 0:
        raise SystemExit("irdm_frontend_save failed")
    return cb


def worker_trace(args):
    import torch
    import bench
    import irdm
    D, n = args.decim, args.chunk
    cap, _ = capture(torch, bench, irdm, args)
    d_out = torch.empty(n + 4096, dtype=torch.complex64, device="cuda:0")
    L = irdm.lib()
    for fmt in ("ci8", "ci16"):
        fe = irdm.Frontend(args.fs * D, irdm.FMT_CI8, D, args.shift)
        count = [0]
        cb = saving(irdm, fe, fmt, False, count)
        for _ in range(args.warmup + args.steps):
            assert L.irdm_frontend_run_device(fe.h, C.c_void_p(cap.data_ptr()), n * D, C.c_void_p(d_out.data_ptr()), n + 4096, None) >= 0
        fe.close()
        del cb
    print(json.dumps(dict(chunks_per_format=args.warmup + args.steps)), flush=True)


def worker_e2e(args):
    import torch
    import bench
    import irdm
    D, n = args.decim, args.chunk
    cap, nb = capture(torch, bench, irdm, args)
    p = irdm.Pipeline(args.fs, fmt=irdm.FMT_CF32, max_chunk_samples=n, max_bursts_per_chunk=8192, pipeline_depth=3)
    p.set_option("packed_records", 1)
    variants = [("off", None, False)] + [("%s_%s" % (f, "direct" if d else "staged"), f, d) for f in ("ci8", "ci16", "cf32")
                                         for d in (False, True)]
    fes, keep, counts = {}, [], {}
    for name, fmt, direct in variants:
        fes[name] = irdm.Frontend(args.fs * D, irdm.FMT_CI8, D, args.shift)
        counts[name] = [0]
        if fmt:
            keep.append(saving(irdm, fes[name], fmt, direct, counts[name]))

    def poll():
        p.poll_bursts_raw()
        p.drop_frames()
        return len(p.poll_demods_packed_raw())

    runs = {name: [] for name, _, _ in variants}
    for _ in range(args.rounds):
        for name, fmt, _ in variants:
            fe = fes[name]
            fe.reset()
            p.reset()
            counts[name][0] = 0
            frames, t0 = 0, None
            for k in range(args.warmup + args.steps):
                if k == args.warmup:
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                fe.feed_device(p, cap.data_ptr(), n * D)
                frames += poll()
            fe.flush(p)
            frames += poll()
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            if fmt:
                want = ((args.warmup + args.steps) * n * D + D - 1) // D * OUT_BYTES[fmt]
                assert counts[name][0] == want, (name, counts[name][0], want)
            runs[name].append(round(args.steps * n * D / dt / 1e6, 1))
    print(json.dumps(dict(bursts_per_chunk=nb, input_msps=runs)), flush=True)


def kernel_stats(trace_dir):
    """(calls, total ns) per kernel family from rocprofv3's kernel statistics"""
    out = {}
    for path in glob.glob(os.path.join(trace_dir, "**", "*kernel_stats.csv"), recursive=True):
        for row in csv.DictReader(open(path)):
            name = row["Name"]
            for key, tag in (("requant_ci8", "requant_kernelILi128E"), ("requant_ci16", "requant_kernelILi32768E"),
                             ("requant_ci8", "requant_kernel<128"), ("requant_ci16", "requant_kernel<32768"),
                             ("k0", "frontend_kernel")):
                if tag in name:
                    c, t = out.get(key, (0, 0))
                    out[key] = (c + int(row["Calls"]), t + int(float(row["TotalDurationNs"])))
                    break
    return out


def child(args, mode, prefix=()):
    cmd = list(prefix) + [sys.executable, os.path.abspath(__file__), "--worker", mode, "--steps", str(args.steps), "--warmup",
                          str(args.warmup), "--rounds", str(args.rounds), "--chunk", str(args.chunk)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    if r.returncode != 0:
        sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
        raise SystemExit("%s failed (exit %d)" % (mode, r.returncode))
    return json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--worker", choices=("trace", "e2e"), default=None)
    ap.add_argument("--fs", type=int, default=10_000_000)
    ap.add_argument("--decim", type=int, default=5)
    ap.add_argument("--shift", type=float, default=11e6)
    ap.add_argument("--chunk", type=int, default=64 << 20, help="output samples per chunk")
    ap.add_argument("--density", type=float, default=10.0)
    ap.add_argument("--steps", type=int, default=6)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--trace-dir", default=None, help="where rocprofv3 writes (default: a temporary directory)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.worker == "trace":
        return worker_trace(args)
    if args.worker == "e2e":
        return worker_e2e(args)
    # the trace, in a run of its own (the program itself behind `--`)
    if args.trace_dir is None:
        args.trace_dir = tempfile.mkdtemp(prefix="saveband_trace_")
    os.makedirs(args.trace_dir, exist_ok=True)
    tr = child(args, "trace", ("rocprofv3", "--kernel-trace", "--stats", "-d", args.trace_dir, "--output-format", "csv", "--"))
    chunks = tr["chunks_per_format"]
    stats = kernel_stats(args.trace_dir)
    if not all(k in stats for k in ("requant_ci8", "requant_ci16", "k0")):
        raise SystemExit("the trace under %s names no requantiser / K0 launches: %r" % (args.trace_dir, stats))
    n = args.chunk
    kernels = {}
    for fmt in ("ci8", "ci16"):
        calls, ns = stats["requant_" + fmt]
        us = ns / chunks / 1e3
        alg = n * (8 + OUT_BYTES[fmt])
        kernels[fmt] = dict(launches_per_chunk=calls / chunks, us_per_chunk=round(us, 1), algorithmic_bytes=alg,
                            GBps=round(alg / (us * 1e-6) / 1e9, 1), hbm_roofline_fraction=round(alg / (us * 1e-6) / HBM_BYTES_PER_S, 3))
    calls, ns = stats["k0"]
    k0_us = ns / (2 * chunks) / 1e3
    k0_alg = n * args.decim * 2 + n * 8
    kernels["k0_ci8_in"] = dict(us_per_chunk=round(k0_us, 1), algorithmic_bytes=k0_alg, GBps=round(k0_alg / (k0_us * 1e-6) / 1e9, 1),
                                hbm_roofline_fraction=round(k0_alg / (k0_us * 1e-6) / HBM_BYTES_PER_S, 3))
    e2e = child(args, "e2e")
    med = {k: float(np.median(v)) for k, v in e2e["input_msps"].items()}
    out = dict(what="saving the band behind K0 at D = %d: a 50 MS/s ci8 capture, 64 Mi-output chunks" % args.decim,
               tool="python3 tools/saveband_rate.py --steps %d --warmup %d --rounds %d" % (args.steps, args.warmup, args.rounds),
               gpu="MI355X (gfx950), one device", hbm_roofline_bytes_per_s=HBM_BYTES_PER_S,
               kernel_trace=kernels, device_resident=dict(e2e, median_input_msps=med),
               notes="kernel_trace: rocprofv3 --kernel-trace --stats in a run of its own, total span of the kernel's launches "
                     "(16 pieces of 4 Mi samples per chunk) per 64 Mi-output chunk. device_resident: input samples per second "
                     "through irdm_frontend_feed_device + polls, pipeline_depth 3, the variants in turn in one process; "
                     "staged = kernel into device staging, copied on the front end's copy stream; direct = the kernel's stores "
                     "go to the pinned slot.")
    print(json.dumps(out, indent=1))
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(out, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
