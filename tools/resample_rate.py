#!/usr/bin/env python3
"""Cost of the front end's rational mode (K0r, csrc/resample.hip) beside the integer front end (K0) on the same device in
the same run.

Cases: 61.44 -> 12 MS/s (25/128), 61.44 -> 10 MS/s (125/768), 56 -> 10 MS/s (5/28), each in cf32 and ci8; the yardstick is
K0 at 50 MS/s, D = 5.  The capture is resident noise (sigma 0.05, clipped to the format): the kernel's time does not depend
on the data.  Per case, each in a process of its own:

  kernel      irdm_frontend_run_device on the resident capture, one chunk of --chunk outputs (64 Mi) per call: the kernel's
              own span on the device (irdm_frontend_kernel_clock) per chunk, and that span per output relative to K0's
  device      irdm_frontend_feed_device of the resident capture into a pipeline_depth 3 cf32 context at the output rate,
              packed records polled per chunk: INPUT samples per second end to end (on noise the detector scans and finds
              nothing to demodulate: this is the front end plus the detector, not the bench's scene)

  python3 tools/resample_rate.py --steps 5 --warmup 2 --out profiles/resample_rate.json
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "iridium-sniffer_amd"))

# name: (in_rate, out_rate); "k0" is the integer front end
CASES = {"k0_50_10": (50_000_000, 10_000_000), "61.44_12": (61_440_000, 12_000_000), "61.44_10": (61_440_000, 10_000_000),
         "56_10": (56_000_000, 10_000_000)}
FORMATS = ("cf32", "ci8")


def run_case(args):
    import torch
    import irdm
    fi, fo = CASES[args.case]
    code = {"cf32": irdm.FMT_CF32, "ci8": irdm.FMT_CI8}[args.format]
    lib = irdm.lib()
    fe = irdm.Frontend.rational(fi, code, fo, args.shift)
    L, M = fe.ratio
    n = args.chunk // L * L                       # whole periods per chunk: every call produces the same count
    n_in = n // L * M
    g = torch.Generator(device="cuda:0")
    g.manual_seed(1)
    if code == irdm.FMT_CF32:
        cap = torch.randn(2 * n_in, dtype=torch.float32, device="cuda:0", generator=g) * 0.05
    else:
        cap = torch.clamp(torch.round(torch.randn(2 * n_in, dtype=torch.float32, device="cuda:0", generator=g) * (0.05 * 128)),
                          -128, 127).to(torch.int8)
    d_out = torch.empty(n + 65536, dtype=torch.complex64, device="cuda:0")
    torch.cuda.synchronize()
    for _ in range(2):
        assert lib.irdm_frontend_run_device(fe.h, C.c_void_p(cap.data_ptr()), n_in, C.c_void_p(d_out.data_ptr()), n + 65536, None) >= 0
    fe.kernel_clock(reset=True)
    for _ in range(args.steps):
        assert lib.irdm_frontend_run_device(fe.h, C.c_void_p(cap.data_ptr()), n_in, C.c_void_p(d_out.data_ptr()), n + 65536, None) == n
    k_ms, k_n = fe.kernel_clock()
    ntaps = fe.ntaps
    fe.close()
    del d_out
    kernel_ms = k_ms / max(k_n, 1)

    p = irdm.Pipeline(fo, fmt=irdm.FMT_CF32, max_chunk_samples=(n + 32767) // 32768 * 32768, max_bursts_per_chunk=8192, pipeline_depth=3)
    p.set_option("packed_records", 1)
    fe = irdm.Frontend.rational(fi, code, fo, args.shift)
    frames = 0
    try:
        t0 = None
        for k in range(args.warmup + args.steps):
            if k == args.warmup:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
            fe.feed_device(p, cap.data_ptr(), n_in)
            p.poll_bursts_raw()
            p.drop_frames()
            frames += len(p.poll_demods_packed_raw())
        fe.flush(p)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
    finally:
        p.close()
        fe.close()
    print(json.dumps(dict(case=args.case, format=args.format, in_rate=fi, out_rate=fo, L=L, M=M, ntaps=ntaps, chunk_out=n,
                          chunk_in=n_in, steps=args.steps, kernel_ms_per_chunk=round(kernel_ms, 3), kernel_launches=k_n,
                          kernel_ns_per_output=round(kernel_ms * 1e6 / n, 4),
                          kernel_ms_per_64Mi_outputs=round(kernel_ms * (64 << 20) / n, 3),
                          device_input_msps=round(args.steps * n_in / dt / 1e6, 1),
                          device_output_msps=round(args.steps * n / dt / 1e6, 1), frames=frames)), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--case", choices=tuple(CASES) + ("all",), default="all")
    ap.add_argument("--format", choices=FORMATS, default="cf32")
    ap.add_argument("--shift", type=float, default=3e6)
    ap.add_argument("--chunk", type=int, default=64 << 20, help="output samples per chunk")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.case != "all":
        run_case(args)
        return
    runs = []
    for case in CASES:
        for f in FORMATS:
            # a process per case (a fresh HIP context each)
            cmd = [sys.executable, os.path.abspath(__file__), "--case", case, "--format", f, "--shift", str(args.shift),
                   "--chunk", str(args.chunk), "--steps", str(args.steps), "--warmup", str(args.warmup)]
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
            if r.returncode != 0:
                sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
                raise SystemExit("case %s %s failed (exit %d)" % (case, f, r.returncode))
            line = [l for l in r.stdout.splitlines() if l.startswith("{")][-1]
            print(line, flush=True)
            runs.append(json.loads(line))
    k0 = {r["format"]: r["kernel_ns_per_output"] for r in runs if r["case"] == "k0_50_10"}
    for r in runs:
        r["kernel_span_per_output_vs_k0"] = round(r["kernel_ns_per_output"] / k0[r["format"]], 2)
    out = dict(what="the front end's rational mode (K0r) beside the integer front end (K0, 50 MS/s, D = 5) in the same run",
               tool="python3 tools/resample_rate.py --steps %d --warmup %d --chunk %d" % (args.steps, args.warmup, args.chunk),
               gpu="MI355X (gfx950), one device", runs=runs)
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(out, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
