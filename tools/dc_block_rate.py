#!/usr/bin/env python3
"""Rate of the DC tracker's kernels (csrc/dc_block.hpp) per resident 64 Mi-sample chunk in ci8, ci16 and cf32, blocks of 2^20:
  dc_sums_kernel   reads b_in bytes per sample, writes nothing but its atomics (what iq_moments_kernel moves);
  dc_close_kernel  one wavefront over the blocks the chunk closed;
  dc_sub_kernel    reads b_in bytes per sample, writes 8 (what iq_balance_kernel moves);
the first and the last beside a device-to-device copy that moves the same bytes in the same process (a copy of X bytes reads
X and writes X: the yardstick of the sums pass copies b_in / 2 bytes per sample, that of the subtraction (b_in + 8) / 2).

  events   per format and round: irdm_dc_block_time_device launches each kernel `reps` times between two events of its own;
           the copies run `reps` times between two events on a stream of the tool's.  Microseconds per chunk, the ratio
           kernel / copy and the share of the HBM roofline (8 TB/s) over the bytes moved.  The copy's spread between rounds is
           the yardstick for the difference.

  python3 tools/dc_block_rate.py --out profiles/dc_block_rate.json
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
    s = torch.cuda.Stream()
    out = []
    for name, fmt, bps in FORMATS:
        n = args.chunk
        if fmt == 2:
            a = (torch.randn(2 * n, dtype=torch.float32, device="cuda:0") * 0.1 + 0.03).view(torch.uint8)
        else:
            a = torch.randint(0, 256, (bps * n,), dtype=torch.uint8, device="cuda:0")
        o = torch.empty(8 * n, dtype=torch.uint8, device="cuda:0")
        moved = {"sums": bps * n, "sub": (bps + 8) * n}
        src = {k: torch.empty(v // 2, dtype=torch.uint8, device="cuda:0") for k, v in moved.items()}
        dst = {k: torch.empty_like(v) for k, v in src.items()}
        torch.cuda.synchronize()
        for rnd in range(args.rounds + 1):                           # (round 0 warms up and is dropped)
            us = irdm.dc_block_time_device(fmt, o.data_ptr(), a.data_ptr(), n, args.log2, args.reps)
            assert us is not None, name
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
            with torch.cuda.stream(s):
                for i, k in enumerate(("sums", "sub")):
                    ev[2 * i].record(s)
                    for _ in range(args.reps):
                        dst[k].copy_(src[k], non_blocking=True)
                    ev[2 * i + 1].record(s)
            torch.cuda.synchronize()
            if rnd:
                for i, k in enumerate(("sums", "sub")):
                    k_us = us[0] if k == "sums" else us[2]
                    c_us = ev[2 * i].elapsed_time(ev[2 * i + 1]) * 1e3 / args.reps
                    out.append(dict(kernel=k, format=name, round=rnd, bytes_moved=moved[k], kernel_us=round(k_us, 1),
                                    copy_us=round(c_us, 1), kernel_over_copy=round(k_us / c_us, 3),
                                    kernel_roofline=round(moved[k] / (k_us * 1e-6) / HBM_BYTES_PER_S, 3),
                                    copy_roofline=round(moved[k] / (c_us * 1e-6) / HBM_BYTES_PER_S, 3)))
                out.append(dict(kernel="close", format=name, round=rnd, blocks=n >> args.log2, kernel_us=round(us[1], 1)))
        del a, o, src, dst
    print(json.dumps(dict(runs=out, launches_per_series=args.reps * (args.rounds + 1))), flush=True)


def summary(runs):
    """per kernel and format: the means over the rounds, and the copy's spread (max - min)"""
    out = []
    for kernel in ("sums", "sub", "close"):
        for name, _, _ in FORMATS:
            r = [x for x in runs if x["kernel"] == kernel and x["format"] == name]
            k = sum(x["kernel_us"] for x in r) / len(r)
            if kernel == "close":
                out.append(dict(kernel=kernel, format=name, blocks=r[0]["blocks"], kernel_us=round(k, 1)))
                continue
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
    ap.add_argument("--log2", type=int, default=20)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.worker:
        return worker(args)
    argv = [sys.executable, os.path.abspath(__file__), "--worker", "--chunk", str(args.chunk), "--log2", str(args.log2),
            "--reps", str(args.reps), "--rounds", str(args.rounds)]
    r = subprocess.run(argv, capture_output=True, text=True, timeout=600)
    if r.returncode != 0:
        sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
        raise SystemExit("the worker failed (exit %d)" % r.returncode)
    events = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    out = dict(what="dc_sums_kernel, dc_close_kernel and dc_sub_kernel per chunk of %d samples in ci8, ci16 and cf32, blocks of 2^%d, "
                    "the sums pass and the subtraction each beside a device-to-device copy that moves the same bytes (events, one "
                    "process, %d launches per series, %d rounds after a warm-up round)" % (args.chunk, args.log2, args.reps, args.rounds),
               tool="python3 tools/dc_block_rate.py", gpu="MI355X (gfx950), one device", hbm_roofline_bytes_per_s=HBM_BYTES_PER_S,
               summary=summary(events["runs"]), events=events)
    for row in out["summary"]:
        print(json.dumps(row), flush=True)
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(out, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
