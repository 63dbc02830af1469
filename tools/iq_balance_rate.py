#!/usr/bin/env python3
"""Rate of the two I/Q imbalance kernels per resident 64 Mi-sample chunk in ci8, ci16 and cf32:
  iq_balance_kernel (csrc/iq_balance.hpp, irdm_iq_balance_device): reads b_in bytes per sample, writes 8;
  iq_moments_kernel (csrc/iq_moments.hpp, irdm_iq_moments_device without figures): reads b_in bytes per sample, writes
  nothing but a row per workgroup;
each beside a device-to-device copy that moves the same bytes in the same process (a copy of X bytes reads X and writes X:
the yardstick of the balance kernel copies (b_in + 8) / 2 bytes per sample, that of the moments kernel b_in / 2).

  events   per format and round: `reps` launches of the balance kernel, `reps` of its copy, `reps` of the moments kernel,
           `reps` of its copy, each series between two events on one stream; microseconds per chunk, the ratio kernel / copy
           and the share of the HBM roofline (8 TB/s) over the bytes moved.  The copy's spread between rounds is the yardstick
           for the difference.

  python3 tools/iq_balance_rate.py --out profiles/iq_balance_rate.json
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "iridium-sniffer_amd"))

HBM_BYTES_PER_S = 8.0e12
FORMATS = (("ci8", 0, 2), ("ci16", 1, 4), ("cf32", 2, 8))          # name, IRDM_FMT_*, bytes per sample


def worker(args):
    import torch
    import irdm
    s = torch.cuda.Stream()                  # (a stream of its own: the library then launches on it and does not wait)
    alpha, beta = irdm.iq_balance_coeffs(0.999, 4.99)
    out = []
    for name, fmt, bps in FORMATS:
        n = args.chunk
        if fmt == 2:
            a = torch.randn(2 * n, dtype=torch.float32, device="cuda:0").view(torch.uint8)
        else:
            a = torch.randint(0, 256, (bps * n,), dtype=torch.uint8, device="cuda:0")
        o = torch.empty(8 * n, dtype=torch.uint8, device="cuda:0")
        moved = {"balance": (bps + 8) * n, "moments": bps * n}
        src = {k: torch.empty(v // 2, dtype=torch.uint8, device="cuda:0") for k, v in moved.items()}
        dst = {k: torch.empty_like(v) for k, v in src.items()}
        torch.cuda.synchronize()
        for rnd in range(args.rounds + 1):                           # (round 0 warms up and is dropped)
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(8)]
            with torch.cuda.stream(s):
                ev[0].record(s)
                for _ in range(args.reps):
                    assert irdm.iq_balance_device(o.data_ptr(), a.data_ptr(), n, fmt, alpha, beta, 0, s.cuda_stream) == 0
                ev[1].record(s)
                ev[2].record(s)
                for _ in range(args.reps):
                    dst["balance"].copy_(src["balance"], non_blocking=True)
                ev[3].record(s)
                ev[4].record(s)
                for _ in range(args.reps):
                    assert irdm.iq_moments_device(a.data_ptr(), n, fmt, 0, s.cuda_stream, stats=False)[0] == 0
                ev[5].record(s)
                ev[6].record(s)
                for _ in range(args.reps):
                    dst["moments"].copy_(src["moments"], non_blocking=True)
                ev[7].record(s)
            torch.cuda.synchronize()
            if rnd:
                for i, kernel in enumerate(("balance", "moments")):
                    k_us = ev[4 * i].elapsed_time(ev[4 * i + 1]) * 1e3 / args.reps
                    c_us = ev[4 * i + 2].elapsed_time(ev[4 * i + 3]) * 1e3 / args.reps
                    out.append(dict(kernel=kernel, format=name, round=rnd, bytes_moved=moved[kernel], kernel_us=round(k_us, 1),
                                    copy_us=round(c_us, 1), kernel_over_copy=round(k_us / c_us, 3),
                                    kernel_roofline=round(moved[kernel] / (k_us * 1e-6) / HBM_BYTES_PER_S, 3),
                                    copy_roofline=round(moved[kernel] / (c_us * 1e-6) / HBM_BYTES_PER_S, 3)))
        # the figures of the chunk, with waiting: the kernel computes something
        rc, st = irdm.iq_moments_device(a.data_ptr(), n, fmt)
        assert rc == 0 and int(st.n_samples) == n and st.valid == 1, (name, rc)
        out[-1]["figures"] = dict(n_used=int(st.n_used), gain_db=round(st.gain_db, 6), phase_deg=round(st.phase_deg, 5))
        del a, o, src, dst
    print(json.dumps(dict(runs=out, launches_per_series=args.reps * (args.rounds + 1))), flush=True)


def summary(runs):
    """per kernel and format: the means over the rounds, and the copy's spread (max - min) as a share of its mean"""
    out = []
    for kernel in ("balance", "moments"):
        for name, _, _ in FORMATS:
            r = [x for x in runs if x["kernel"] == kernel and x["format"] == name]
            k = sum(x["kernel_us"] for x in r) / len(r)
            c = sum(x["copy_us"] for x in r) / len(r)
            spread = max(x["copy_us"] for x in r) - min(x["copy_us"] for x in r)
            out.append(dict(kernel=kernel, format=name, kernel_us=round(k, 1), copy_us=round(c, 1), kernel_over_copy=round(k / c, 3),
                            copy_spread_us=round(spread, 1), behind_copy_us=round(k - c, 1),
                            kernel_roofline=round(r[0]["bytes_moved"] / (k * 1e-6) / HBM_BYTES_PER_S, 3)))
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--worker", action="store_true")
    ap.add_argument("--chunk", type=int, default=64 << 20)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.worker:
        return worker(args)
    argv = [sys.executable, os.path.abspath(__file__), "--worker", "--chunk", str(args.chunk), "--reps", str(args.reps),
            "--rounds", str(args.rounds)]
    r = subprocess.run(argv, capture_output=True, text=True, timeout=600)
    if r.returncode != 0:
        sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
        raise SystemExit("the worker failed (exit %d)" % r.returncode)
    events = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    out = dict(what="iq_balance_kernel and iq_moments_kernel per chunk of %d samples in ci8, ci16 and cf32, each beside a device-to-device "
                    "copy that moves the same bytes (events, one process, %d launches per series, %d rounds after a warm-up round)"
                    % (args.chunk, args.reps, args.rounds),
               tool="python3 tools/iq_balance_rate.py", gpu="MI355X (gfx950), one device", hbm_roofline_bytes_per_s=HBM_BYTES_PER_S,
               summary=summary(events["runs"]), events=events)
    for row in out["summary"]:
        print(json.dumps(row), flush=True)
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(out, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
