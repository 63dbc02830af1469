#!/usr/bin/env python3
"""Throughput of the input formats: cf32, ci16 (narrowed to 8 bits, the reference's file path), ci16-full and sc16q11
(interleaved int16 at full precision, include/irdm_hip.h) on one scene.

The bench's scene and headline configuration: 10 MHz, device-resident chunks of 64 Mi samples written in place
(irdm_ingest_ptr, every slot of the history ring filled before the timed region) and fed with one chunk of look-ahead at
pipeline_depth 3, packed records polled after every chunk; then the same chunk from pinned host memory (irdm_feed_host,
the H2D copy inside the measurement).  The int16 formats get the same bytes, round(x * 131072) clipped.  Before it is
timed, each format's first chunk goes through a context of its own and a cf32 context fed the converted samples
(v.astype(np.float32) * scale; (v >> 8) / 128 for ci16): the compact records must be equal bit for bit.  Each format runs
in a process of its own; the parent prints one JSON line per format and a summary (and writes them to --out).

  python3 tools/format_rate.py --steps 20 --warmup 5 --out profiles/format_rate.json
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "iridium-sniffer_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)

FORMATS = ("cf32", "ci16", "ci16-full", "sc16q11")
STATS = ("scan_fast_chunks", "scan_fallbacks", "band_chunks", "band_aborts", "band_retries", "scan_dense_frames")


def run_format(args):
    import torch
    import bench
    import formats16 as f16
    import irdm
    code = {"cf32": irdm.FMT_CF32, "ci16": irdm.FMT_CI16, "ci16-full": irdm.FMT_CI16_FULL, "sc16q11": irdm.FMT_SC16Q11}[args.format]
    fs, n = args.fs, args.chunk
    x, nb = bench.build_scene(torch, "cuda:0", fs, n, args.density, seed=1)
    if code != irdm.FMT_CF32:
        x = torch.clamp(torch.round(x * 131072.0), -32768, 32767).to(torch.int16)
    torch.cuda.synchronize()
    host = x.reshape(-1).cpu().numpy()
    bps = 8 if code == irdm.FMT_CF32 else 4

    # the first chunk against the cf32 context on the converted samples
    check = "reference"
    if code != irdm.FMT_CF32:
        conv = ((host >> 8).astype(np.float32) / np.float32(128.0)).view(np.complex64) if code == irdm.FMT_CI16 \
            else f16.converted(host, code)
        got = f16.run(host, fs, code, depth=1, packed=True)
        records = f16.same_records(got, f16.run(conv, fs, irdm.FMT_CF32, depth=1, packed=True))
        check = "%d records equal to the cf32 context's" % records
    else:
        host = host.view(np.complex64)

    def poll(p):
        p.poll_bursts_raw()
        p.drop_frames()
        return len(p.poll_demods_packed_raw())

    # device-resident, in place, one chunk of look-ahead, pipeline_depth 3
    p = irdm.Pipeline(fs, fmt=code, max_chunk_samples=n, max_bursts_per_chunk=8192, pipeline_depth=3)
    p.set_option("packed_records", 1)
    try:
        ring_ptr, ring_len = p.ring()
        assert ring_len % n == 0, (ring_len, n)
        for k in range(ring_len // n):
            assert irdm.lib().irdm_device_copy(C.c_void_p(ring_ptr + k * n * bps), C.c_void_p(x.data_ptr()), n * bps) == 0
        pending = 0
        frames = 0
        t0 = None
        stage = {}
        for k in range(args.warmup + args.steps):
            if k == args.warmup:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                frames = 0
                stats0 = {s: p.stat(s) for s in STATS}
            p.feed_begin(p.ingest_ptr(n), n)
            pending += 1
            if pending > 1:
                p.feed_end()
                pending -= 1
            frames += poll(p)
            if k >= args.warmup:
                for key, v in p.timings().items():
                    stage[key] = stage.get(key, 0.0) + v
        while pending:
            p.feed_end()
            pending -= 1
        p.flush()
        frames += poll(p)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        stats = {s: p.stat(s) - stats0[s] for s in STATS}
    finally:
        p.close()
    device_msps = args.steps * n / dt / 1e6

    # pinned host memory, pipeline_depth 3
    hptr, hview = irdm.host_alloc(n * bps)
    hview[:] = host.view(np.uint8)
    p = irdm.Pipeline(fs, fmt=code, max_chunk_samples=n, max_bursts_per_chunk=8192, pipeline_depth=3)
    p.set_option("packed_records", 1)
    try:
        for _ in range(2):
            p.feed_host_ptr(hptr, n)
            poll(p)
        torch.cuda.synchronize()
        th = time.perf_counter()
        for _ in range(args.host_steps):
            p.feed_host_ptr(hptr, n)
            poll(p)
        p.flush()
        poll(p)
        torch.cuda.synchronize()
        hdt = time.perf_counter() - th
    finally:
        p.close()
        irdm.host_free(hptr)
    rec = dict(format=args.format, bytes_per_sample=bps, fs=fs, chunk=n, density=args.density, bursts_per_chunk=nb,
               steps=args.steps, frames_per_step=round(frames / args.steps, 1), device_msps=round(device_msps, 1),
               device_stage_ms={k: round(v / args.steps, 3) for k, v in stage.items()}, device_stats=stats,
               host_steps=args.host_steps, pinned_host_msps=round(args.host_steps * n / hdt / 1e6, 1),
               pinned_h2d_GBps=round(args.host_steps * n * bps / hdt / 1e9, 2), first_chunk=check)
    print(json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--format", choices=FORMATS + ("all",), default="all")
    ap.add_argument("--fs", type=int, default=10_000_000)
    ap.add_argument("--chunk", type=int, default=64 << 20)
    ap.add_argument("--density", type=float, default=10.0, help="bursts per Msample (the bench's default)")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--host-steps", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.format != "all":
        return run_format(args)
    recs = []
    for fmt in FORMATS:
        cmd = [sys.executable, os.path.abspath(__file__), "--format", fmt, "--fs", str(args.fs), "--chunk", str(args.chunk),
               "--density", str(args.density), "--steps", str(args.steps), "--warmup", str(args.warmup),
               "--host-steps", str(args.host_steps)]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
        if r.returncode != 0:
            sys.stderr.write(r.stderr[-3000:])
            raise SystemExit("%s run failed (%d)" % (fmt, r.returncode))
        recs.append(json.loads(r.stdout.strip().splitlines()[-1]))
        print(json.dumps(recs[-1]), flush=True)
    summary = dict(summary=True, device_msps={r["format"]: r["device_msps"] for r in recs},
                   pinned_host_msps={r["format"]: r["pinned_host_msps"] for r in recs})
    print(json.dumps(summary), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(dict(runs=recs, **summary), f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
