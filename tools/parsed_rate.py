#!/usr/bin/env python3
"""What --parsed costs the throughput path: option packed_records against parsed_records (the same compact frame records
plus ida_decode() of every frame on the device, ida_packed_kernel) on one scene.

10 MHz cf32, device-resident chunks of 64 Mi samples fed again and again, pipeline_depth 1, records polled after every
chunk.  The scene is the bench's (noise on the device, `--density` bursts per Msample at random channels and times) but
every burst is an IDA frame (tests/bitlayer.py): LCW, two 124-bit blocks and the tail block, a quarter of them at low
amplitude so that Chase decoding runs, one in six with a bad CRC.  Each mode runs in a process of its own; the parent
prints one JSON line per mode and one with the ratio (and writes them to --out).

  python3 tools/parsed_rate.py --steps 20 --warmup 3 --out profiles/parsed_rate.json
  rocprofv3 --kernel-trace --stats -d DIR -- python3 tools/parsed_rate.py --mode parsed --steps 5 --warmup 1
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "iridium-sniffer_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))


def build_ida_scene(torch, device, fs, n, density, seed):
    import bitlayer as bl
    import siggen
    g = torch.Generator(device=device)
    g.manual_seed(seed)
    x = torch.randn((n, 2), generator=g, device=device, dtype=torch.float32)
    x.mul_(0.002)
    rng = np.random.default_rng(seed + 1000)
    fft = 1 << int(round(np.log2(fs / 1000.0)))
    first = 520 * fft
    nb = int(round(density * n / 1e6))
    starts = np.sort(rng.integers(0, n - first - int(0.012 * fs), size=nb)) + first
    half_ch = int((fs / 2 - 60e3) // (1e6 / 24.0))
    for k, s in enumerate(starts):
        st = bl.ida_stream(k % 8, int(rng.integers(0, 21)), k & 1, [int(b) for b in rng.integers(0, 256, 20)], rng,
                           good_crc=k % 6 != 5)
        bits = bl.ida_frame(bl.lcw_bits(2, int(rng.integers(0, 32)), int(rng.integers(0, 1 << 21))), st, rng)
        quads = [0] * 16 + siggen.bits_to_quadrants("".join(str(b) for b in bits))
        ch = int(rng.integers(-half_ch, half_ch + 1)) or 1
        sig = siggen.make_burst(fs, quads, siggen.channel_freq(ch), rng.uniform(0, 2 * np.pi),
                                amp=0.0065 if k % 4 == 3 else 0.05)
        e = min(n, int(s) + len(sig))
        t = torch.from_numpy(np.ascontiguousarray(sig[:e - int(s)]).view(np.float32).reshape(-1, 2)).to(device)
        x[int(s):e] += t
    return x, nb


def run_mode(args):
    import torch
    import irdm
    fs, n = args.fs, args.chunk
    x, nb = build_ida_scene(torch, "cuda:0", fs, n, args.density, seed=4)
    torch.cuda.synchronize()
    p = irdm.Pipeline(fs, max_chunk_samples=n, max_bursts_per_chunk=4096, pipeline_depth=1)
    p.set_option("packed_records" if args.mode == "packed" else "parsed_records", 1)
    frames = idas = ok = 0
    try:
        t0 = None
        for k in range(args.warmup + args.steps):
            if k == args.warmup:
                t0 = time.perf_counter()
                frames = idas = ok = 0
            p.feed_device(x.data_ptr(), n, None)
            d = p.poll_demods_packed_raw()
            frames += len(d)
            if args.mode == "parsed":
                r = p._poll_raw(p.L.irdm_poll_ida_packed, irdm.IdaPacked, 4096)
                idas += len(r)
                ok += int(np.count_nonzero(r[:, :4].copy().view(np.int32))) if len(r) else 0
            p.poll_bursts_raw()
        p.flush()
        dt = time.perf_counter() - t0
    finally:
        p.close()
    rec = dict(mode=args.mode, fs=fs, chunk=n, steps=args.steps, density=args.density, bursts_per_chunk=nb,
               frames=frames, msps=round(args.steps * n / dt / 1e6, 1), seconds=round(dt, 4))
    if args.mode == "parsed":
        assert idas == frames, (idas, frames)
        rec.update(ida_records=idas, ida_ok=ok)
    print(json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--mode", choices=("packed", "parsed", "both"), default="both")
    ap.add_argument("--fs", type=int, default=10_000_000)
    ap.add_argument("--chunk", type=int, default=64 << 20)
    ap.add_argument("--density", type=float, default=10.0, help="bursts per Msample (the bench's default)")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=2, help="with --mode both: packed / parsed processes, alternating")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.mode != "both":
        return run_mode(args)
    recs = []
    for _ in range(args.rounds):
        for mode in ("packed", "parsed"):
            cmd = [sys.executable, os.path.abspath(__file__), "--mode", mode, "--fs", str(args.fs), "--chunk",
                   str(args.chunk), "--density", str(args.density), "--steps", str(args.steps), "--warmup", str(args.warmup)]
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
            if r.returncode != 0:
                sys.stderr.write(r.stderr[-3000:])
                raise SystemExit("%s run failed (%d)" % (mode, r.returncode))
            recs.append(json.loads(r.stdout.strip().splitlines()[-1]))
            print(json.dumps(recs[-1]), flush=True)
    best = {m: max(r["msps"] for r in recs if r["mode"] == m) for m in ("packed", "parsed")}
    summary = dict(summary=True, packed_msps=best["packed"], parsed_msps=best["parsed"],
                   parsed_over_packed=round(best["parsed"] / best["packed"], 4))
    print(json.dumps(summary), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(dict(runs=recs, **summary), f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
