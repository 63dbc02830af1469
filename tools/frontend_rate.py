#!/usr/bin/env python3
"""Cost of the band-select front end (K0, csrc/frontend.hip): a 50 MHz capture, the band shifted to the centre, D = 5, in
front of the bench's 10 MHz pipeline.

The capture is the bench's scene zero-stuffed by D, scaled by D and rotated back by the shift: the filter's cut-off of
0.5 fs_out makes it a Nyquist filter (zeros at multiples of D), so the pipeline behind the front end sees the bench's
scene and does the bench's work.  Per format (cf32, ci8), each in a process of its own:

  kernel      irdm_frontend_run_device on the resident capture, one 64 Mi-output chunk per call: the kernel's own span on
              the device (irdm_frontend_kernel_clock), and the fraction of the 8 TB/s HBM roofline over its algorithmic
              bytes n_in (bps_in + 8 / D)
  device      irdm_frontend_feed_device of the resident capture into a pipeline_depth 3 context (converted in place into
              the history ring), packed records polled per chunk: INPUT samples per second -- beside the same context fed
              the pre-decimated cf32 in place (irdm_feed_device on its ingest slot), times D
  pinned      irdm_frontend_feed_host from pinned memory (ci8 only)

  python3 tools/frontend_rate.py --steps 10 --warmup 3 --out profiles/frontend_rate.json
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

FORMATS = ("cf32", "ci8")
HBM_BYTES_PER_S = 8e12
STATS = ("scan_fast_chunks", "scan_fallbacks", "band_chunks", "band_aborts", "scan_dense_frames")


def run_format(args):
    import torch
    import bench
    import irdm
    code = {"cf32": irdm.FMT_CF32, "ci8": irdm.FMT_CI8}[args.format]
    bps = 8 if code == irdm.FMT_CF32 else 2
    D, fs_out, n = args.decim, args.fs, args.chunk
    fs_in, n_in = fs_out * D, n * D
    L = irdm.lib()
    x, nb = bench.build_scene(torch, "cuda:0", fs_out, n, args.density, seed=1)
    fe = irdm.Frontend(fs_in, code, D, args.shift)
    q = int(round(fe.applied_shift_hz * 65536 / fs_in))
    # the capture: zero-stuffed, scaled by D, rotated by +q so that the front end's rotation by -q undoes it
    cap = torch.zeros(n_in, dtype=torch.complex64, device="cuda:0")
    cap[::D] = x.reshape(-1).view(torch.complex64) if x.dtype != torch.complex64 else x
    idx = (torch.arange(0, n_in, D, device="cuda:0", dtype=torch.int64) * q) % 65536
    cap[::D] *= torch.polar(torch.full_like(idx, float(D), dtype=torch.float32), idx.to(torch.float32) * (2.0 * np.pi / 65536.0))
    del idx
    if code == irdm.FMT_CI8:
        cap = torch.clamp(torch.round(torch.view_as_real(cap) * 256.0), -128, 127).to(torch.int8).reshape(-1)
    torch.cuda.synchronize()
    d_out = torch.empty(n + 4096, dtype=torch.complex64, device="cuda:0")

    # ---- the kernel alone ----
    for _ in range(2):
        assert L.irdm_frontend_run_device(fe.h, C.c_void_p(cap.data_ptr()), n_in, C.c_void_p(d_out.data_ptr()), n + 4096, None) >= 0
    fe.kernel_clock(reset=True)
    for _ in range(args.steps):
        assert L.irdm_frontend_run_device(fe.h, C.c_void_p(cap.data_ptr()), n_in, C.c_void_p(d_out.data_ptr()), n + 4096, None) == n
    k_ms, k_n = fe.kernel_clock()
    fe.close()
    kernel_us = k_ms / max(k_n, 1) * 1e3
    alg_bytes = n_in * (bps + 8.0 / D)
    y = d_out[:n].clone()                     # the decimated stream (chunks of a continuing stream: what the context is fed)
    torch.cuda.synchronize()

    def poll(p):
        p.poll_bursts_raw()
        p.drop_frames()
        return len(p.poll_demods_packed_raw())

    scans = []          # the detector's statistics of every timed context, in order: front end, direct(, pinned)

    def timed(step, p, finish):
        frames = 0
        t0 = None
        for k in range(args.warmup + args.steps):
            if k == args.warmup:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                frames = 0
            step()
            frames += poll(p)
        finish()
        frames += poll(p)
        torch.cuda.synchronize()
        scans.append({k: p.stat(k) for k in STATS})
        return time.perf_counter() - t0, frames

    def context():
        p = irdm.Pipeline(fs_out, fmt=irdm.FMT_CF32, max_chunk_samples=n, max_bursts_per_chunk=8192, pipeline_depth=3)
        p.set_option("packed_records", 1)
        return p

    # ---- device-resident, through the front end ----
    p, fe = context(), irdm.Frontend(fs_in, code, D, args.shift)
    try:
        dt, frames = timed(lambda: fe.feed_device(p, cap.data_ptr(), n_in), p, lambda: fe.flush(p))
    finally:
        p.close()
        fe.close()
    fe_msps = args.steps * n_in / dt / 1e6

    # ---- the same context fed the pre-decimated stream in place ----
    p = context()
    try:
        ring_ptr, ring_len = p.ring()
        for k in range(ring_len // n):
            assert L.irdm_device_copy(C.c_void_p(ring_ptr + k * n * 8), C.c_void_p(y.data_ptr()), n * 8) == 0
        ddt, dframes = timed(lambda: p.feed_device(p.ingest_ptr(n), n), p, p.flush)
    finally:
        p.close()
    direct_msps = args.steps * n / ddt / 1e6

    rec = dict(format=args.format, bytes_per_sample=bps, fs_in=fs_in, decim=D, shift_hz=args.shift, q=q, chunk_out=n,
               density=args.density, bursts_per_chunk=nb, steps=args.steps,
               kernel_us_per_chunk=round(kernel_us, 1), kernel_launches=k_n, algorithmic_bytes=int(alg_bytes),
               kernel_GBps=round(alg_bytes / (kernel_us * 1e-6) / 1e9, 1),
               hbm_roofline_fraction=round(alg_bytes / (kernel_us * 1e-6) / HBM_BYTES_PER_S, 3),
               device_input_msps=round(fe_msps, 1), device_frames_per_step=round(frames / args.steps, 1),
               direct_cf32_output_msps=round(direct_msps, 1), direct_cf32_input_equivalent_msps=round(direct_msps * D, 1),
               direct_frames_per_step=round(dframes / args.steps, 1), scan_stats_frontend=scans[0], scan_stats_direct=scans[1])

    # ---- from pinned host memory ----
    if code == irdm.FMT_CI8:
        hptr, hview = irdm.host_alloc(n_in * bps)
        hview[:] = cap.cpu().numpy().view(np.uint8)
        p, fe = context(), irdm.Frontend(fs_in, code, D, args.shift)
        try:
            hdt, _ = timed(lambda: L.irdm_frontend_feed_host(fe.h, p.h, C.c_void_p(hptr), n_in), p, lambda: fe.flush(p))
        finally:
            p.close()
            fe.close()
            irdm.host_free(hptr)
        rec.update(pinned_host_input_msps=round(args.steps * n_in / hdt / 1e6, 1),
                   pinned_h2d_GBps=round(args.steps * n_in * bps / hdt / 1e9, 2))
    print(json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--format", choices=FORMATS + ("all",), default="all")
    ap.add_argument("--fs", type=int, default=10_000_000, help="the pipeline's rate behind the front end")
    ap.add_argument("--decim", type=int, default=5)
    ap.add_argument("--shift", type=float, default=11e6)
    ap.add_argument("--chunk", type=int, default=64 << 20, help="output samples per chunk")
    ap.add_argument("--density", type=float, default=10.0, help="bursts per Msample (the bench's default)")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.format != "all":
        run_format(args)
        return
    runs = []
    for f in FORMATS:
        # a process per format (a fresh HIP context each)
        cmd = [sys.executable, os.path.abspath(__file__), "--format", f] + [a for a in sys.argv[1:] if not a.startswith("--out")
                                                                             and a != args.out]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
        if r.returncode != 0:
            sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
            raise SystemExit("format %s failed (exit %d)" % (f, r.returncode))
        line = [l for l in r.stdout.splitlines() if l.startswith("{")][-1]
        print(line, flush=True)
        runs.append(json.loads(line))
    out = dict(what="band-select front end (K0) at D = %d in front of the bench's pipeline" % args.decim,
               tool="python3 tools/frontend_rate.py --steps %d --warmup %d" % (args.steps, args.warmup),
               gpu="MI355X (gfx950), one device", hbm_roofline_bytes_per_s=HBM_BYTES_PER_S, runs=runs)
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(out, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
