#!/usr/bin/env python3
"""What running an archive of recordings through ONE context saves: N recordings (the bench scene's generator, one seed
each, written to /dev/shm in this call so that their pages are warm), wall time from process start to exit

  (a) as N runs of the PARENT commit's binary, one recording each,
  (b) as one run of this commit's binary with the N recordings behind -f,

alternating (a) and (b) --pairs times, per format (cf32, ci8); and (c) ONE recording through both binaries, alternating: the
batch machinery may cost a single file nothing, i.e. the two agree within the run-to-run spread seen in (a).  The per-file
reset time (this binary's --timing lines) is reported beside the parent's start-up figure.

The parent's binary is built from `git archive` of the parent commit (its own libirdm_hip.so beside it):

  git archive HEAD~1 | tar -x -C /tmp/parent && make -C /tmp/parent/iridium-sniffer_amd -j16
  python3 tools/batch_rate.py --parent-exe /tmp/parent/iridium-sniffer_amd/iridium-sniffer-hip --out profiles/batch_rate.json
"""
import argparse
import json
import os
import re
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "iridium-sniffer_amd"))
sys.path.insert(0, ROOT)
EXE = os.path.join(ROOT, "iridium-sniffer_amd", "iridium-sniffer-hip")


def write_scenes(args, fmt, tmp):
    """N scenes on the GPU (bench.build_scene), copied out and written; returns the paths"""
    import torch
    import bench
    paths = []
    for i in range(args.files):
        x, _ = bench.build_scene(torch, "cuda:0", args.fs, args.samples, args.density, seed=1 + i)
        x = torch.view_as_real(x.reshape(-1).view(torch.complex64)) if x.dtype != torch.float32 else x.reshape(-1, 2)
        if fmt == "ci8":
            x = torch.clamp(torch.round(x * 256.0), -128, 127).to(torch.int8)
        path = os.path.join(tmp, "irdm_batch_%d_%d.%s" % (os.getpid(), i, fmt))
        x.cpu().numpy().tofile(path)
        paths.append(path)
        del x
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    return paths


def run(exe, files, args, fmt):
    """one process: wall seconds start to exit, its stderr"""
    cmd = [exe] + sum((["-f", f] for f in files), []) + ["-r", str(args.fs), "--format", fmt, "--timing"]
    t0 = time.perf_counter()
    r = subprocess.run(cmd, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, timeout=600)
    wall = time.perf_counter() - t0
    if r.returncode != 0:
        raise SystemExit("%s failed (exit %d): %s" % (" ".join(cmd[:4]), r.returncode, r.stderr.decode("latin-1")[-2000:]))
    return wall, r.stderr.decode("latin-1")


def measure(args, fmt, tmp):
    files = write_scenes(args, fmt, tmp)
    try:
        rec = dict(format=fmt, files=args.files, samples_per_file=args.samples, a_parent_one_run_per_file=[], b_one_batch_run=[],
                   c_single_file=[])
        run(args.parent_exe, files[:1], args, fmt)            # (both binaries' pages warm before the first timed pair)
        run(EXE, files[:1], args, fmt)
        startups, resets, tagged = [], [], None
        for pair in range(args.pairs):
            walls = []
            for f in files:
                w, err = run(args.parent_exe, [f], args, fmt)
                walls.append(round(w, 4))
                m = re.search(r"startup ([0-9.]+) s", err)
                startups.append(float(m.group(1)))
            rec["a_parent_one_run_per_file"].append(dict(pair=pair, wall_s=round(sum(walls), 4), per_run_s=walls))
            w, err = run(EXE, files, args, fmt)
            resets += [float(v) for v in re.findall(r"reset ([0-9.]+) ms", err)]
            t = re.findall(r"tagged (\d+) bursts", err)
            assert len(t) == args.files and (tagged is None or t == tagged), t
            tagged = t
            rec["b_one_batch_run"].append(dict(pair=pair, wall_s=round(w, 4)))
        for pair in range(args.pairs):
            wp, _ = run(args.parent_exe, files[:1], args, fmt)
            wt, _ = run(EXE, files[:1], args, fmt)
            rec["c_single_file"].append(dict(pair=pair, parent_wall_s=round(wp, 4), this_wall_s=round(wt, 4)))
        a = [r["wall_s"] for r in rec["a_parent_one_run_per_file"]]
        b = [r["wall_s"] for r in rec["b_one_batch_run"]]
        per_run = [w for r in rec["a_parent_one_run_per_file"] for w in r["per_run_s"]]
        rec.update(ratio_a_over_b=[round(x / y, 3) for x, y in zip(a, b)], b_faster_in_every_pair=all(y < x for x, y in zip(a, b)),
                   parent_startup_s=[min(startups), max(startups)], reset_ms=[min(resets), max(resets)] if resets else None,
                   parent_single_run_s=[min(per_run), max(per_run)], tagged_per_file=[int(v) for v in tagged],
                   batch_msamples_per_s=[round(args.files * args.samples / y / 1e6, 1) for y in b],
                   parent_msamples_per_s=[round(args.files * args.samples / x / 1e6, 1) for x in a])
        return rec
    finally:
        for f in files:
            os.remove(f)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--parent-exe", required=True, help="the parent commit's iridium-sniffer-hip (its libirdm_hip.so beside it)")
    ap.add_argument("--files", type=int, default=8)
    ap.add_argument("--samples", type=int, default=64 << 20)
    ap.add_argument("--fs", type=int, default=10_000_000)
    ap.add_argument("--density", type=float, default=10.0, help="bursts per Msample (the bench's default)")
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--formats", default="cf32,ci8")
    ap.add_argument("--tmp", default="/dev/shm")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    runs = []
    for fmt in args.formats.split(","):
        rec = measure(args, fmt, args.tmp)
        print(json.dumps(rec), flush=True)
        runs.append(rec)
    out = dict(what="N recordings through one context (this commit's binary, -f N times) against N runs of the parent commit's binary; "
                    "wall time from process start to exit, files in /dev/shm written in the same call",
               tool="python3 tools/batch_rate.py --parent-exe <parent>/iridium-sniffer_amd/iridium-sniffer-hip --files %d --pairs %d" % (args.files, args.pairs),
               gpu="MI355X (gfx950), one device", runs=runs)
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(out, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
