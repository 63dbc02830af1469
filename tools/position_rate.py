#!/usr/bin/env python3
"""What --position costs the throughput path: option packed_records against frame_records (the same compact frame records
plus frame_decode() of every frame on the device, frame_packed_kernel) on one scene.

10 MHz cf32, device-resident chunks of 64 Mi samples fed again and again, pipeline_depth 1, records polled after every
chunk.  The scene is the bench's (noise on the device, `--density` bursts per Msample at random channels and times) but
every burst is an IRA frame (tests/bitlayer.py) with up to four paging blocks, a quarter of them at low amplitude so that
Chase decoding runs.  Each mode runs in a process of its own; the parent prints one JSON line per mode and one with the
ratio (and writes them to --out).  --mode decode runs the full-record path with decode_frames (frame_decode_kernel), for
comparing the two kernels' times under rocprofv3:

  python3 tools/position_rate.py --steps 15 --warmup 3 --out /tmp/rate.json
  rocprofv3 --kernel-trace --stats -d DIR -- python3 tools/position_rate.py --mode framed --steps 3 --warmup 1
  rocprofv3 --kernel-trace --stats -d DIR -- python3 tools/position_rate.py --mode decode --steps 3 --warmup 1
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

OPTION = {"packed": "packed_records", "framed": "frame_records", "decode": "decode_frames"}


def build_ira_scene(torch, device, fs, n, density, seed):
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
        pages = [(int(rng.integers(0, 2**32)), int(rng.integers(0, 32))) for _ in range(k % 5)]
        st = bl.ira_stream(int(rng.integers(1, 128)), int(rng.integers(0, 64)), int(rng.integers(-2047, 2048)),
                           int(rng.integers(-2047, 2048)), int(rng.integers(-2047, 2048)), pages, rng)
        bits = bl.ira_frame(st)
        if len(bits) % 2:
            bits.append(0)
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
    x, nb = build_ira_scene(torch, "cuda:0", fs, n, args.density, seed=4)
    torch.cuda.synchronize()
    p = irdm.Pipeline(fs, max_chunk_samples=n, max_bursts_per_chunk=4096, pipeline_depth=1)
    p.set_option(OPTION[args.mode], 1)
    frames = recs = ira = 0
    try:
        t0 = None
        for k in range(args.warmup + args.steps):
            if k == args.warmup:
                t0 = time.perf_counter()
                frames = recs = ira = 0
            p.feed_device(x.data_ptr(), n, None)
            if args.mode == "decode":
                frames += len(p.poll_demods())
                dec = p.poll_decoded()
                recs += len(dec)
                ira += sum(d.type == 1 for d in dec)
            else:
                frames += len(p.poll_demods_packed_raw())
                if args.mode == "framed":
                    r = p._poll_raw(p.L.irdm_poll_frame_packed, irdm.FramePacked, 4096)
                    recs += len(r)
                    ira += int(np.count_nonzero(r[:, 0] == 1)) if len(r) else 0
            p.poll_bursts_raw()
        p.flush()
        dt = time.perf_counter() - t0
    finally:
        p.close()
    rec = dict(mode=args.mode, fs=fs, chunk=n, steps=args.steps, density=args.density, bursts_per_chunk=nb,
               frames=frames, msps=round(args.steps * n / dt / 1e6, 1), seconds=round(dt, 4))
    if args.mode != "packed":
        assert recs == frames, (recs, frames)
        rec.update(frame_records=recs, ira=ira)
    print(json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--mode", choices=("packed", "framed", "decode", "both"), default="both")
    ap.add_argument("--fs", type=int, default=10_000_000)
    ap.add_argument("--chunk", type=int, default=64 << 20)
    ap.add_argument("--density", type=float, default=10.0, help="bursts per Msample (the bench's default)")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=2, help="with --mode both: packed / framed processes, alternating")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.mode != "both":
        return run_mode(args)
    recs = []
    for _ in range(args.rounds):
        for mode in ("packed", "framed"):
            cmd = [sys.executable, os.path.abspath(__file__), "--mode", mode, "--fs", str(args.fs), "--chunk",
                   str(args.chunk), "--density", str(args.density), "--steps", str(args.steps), "--warmup", str(args.warmup)]
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
            if r.returncode != 0:
                sys.stderr.write(r.stderr[-3000:])
                raise SystemExit("%s run failed (%d)" % (mode, r.returncode))
            recs.append(json.loads(r.stdout.strip().splitlines()[-1]))
            print(json.dumps(recs[-1]), flush=True)
    best = {m: max(r["msps"] for r in recs if r["mode"] == m) for m in ("packed", "framed")}
    summary = dict(summary=True, packed_msps=best["packed"], framed_msps=best["framed"],
                   framed_over_packed=round(best["framed"] / best["packed"], 4))
    print(json.dumps(summary), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(dict(runs=recs, **summary), f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
