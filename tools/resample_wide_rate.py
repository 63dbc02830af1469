#!/usr/bin/env python3
"""Cost of the front end's wide-ratio kernel (K0w, csrc/resample_wide.hip) beside K0r (csrc/resample.hip) on the same device
in the same process.

Cases: K0r at 11.2 -> 10 MS/s (25/28), the yardstick -- about as many multiply-adds per output as K0w has at a ratio near
1, its taps from scalar loads where K0w's come from vector loads; K0w forced at the same 25/28 (irdm_frontend_create_wide);
K0w at 10.025 -> 10 MS/s (400/401), 10.0025 -> 10 MS/s (4000/4001) and 8.01 -> 1 MS/s (100/801, eight times the taps per
output).  Each in cf32 and ci8.  The capture is resident noise (sigma 0.05, clipped to the format): the kernel's time does
not depend on the data.  Per case irdm_frontend_run_device on the resident capture, one chunk of --chunk outputs (64 Mi) per
call: the kernel's own span on the device (irdm_frontend_kernel_clock) per chunk, per output, and per output relative to
K0r's.

  python3 tools/resample_wide_rate.py --steps 5 --out profiles/resample_wide_rate.json
"""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "iridium-sniffer_amd"))

# name: (maker, in_rate, out_rate)
CASES = {"k0r_25_28": ("rational", 11_200_000, 10_000_000), "k0w_25_28": ("wide", 11_200_000, 10_000_000),
         "k0w_400_401": ("wide", 10_025_000, 10_000_000), "k0w_4000_4001": ("wide", 10_002_500, 10_000_000),
         "k0w_100_801": ("wide", 8_010_000, 1_000_000)}
FORMATS = ("cf32", "ci8")


def run_case(irdm, torch, name, fmt_name, chunk, steps):
    maker, fi, fo = CASES[name]
    code = {"cf32": irdm.FMT_CF32, "ci8": irdm.FMT_CI8}[fmt_name]
    lib = irdm.lib()
    fe = irdm.Frontend(fi, code, None, 0.03 * fi, 0, out_rate=fo, maker=maker)
    L, M = fe.ratio
    n = chunk // L * L                            # whole periods per chunk: every call produces the same count
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
    try:
        for _ in range(2):
            assert lib.irdm_frontend_run_device(fe.h, C.c_void_p(cap.data_ptr()), n_in, C.c_void_p(d_out.data_ptr()), n + 65536, None) >= 0
        fe.kernel_clock(reset=True)
        for _ in range(steps):
            assert lib.irdm_frontend_run_device(fe.h, C.c_void_p(cap.data_ptr()), n_in, C.c_void_p(d_out.data_ptr()), n + 65536, None) == n
        k_ms, k_n = fe.kernel_clock()
        ntaps = fe.ntaps
    finally:
        fe.close()
    del cap, d_out
    torch.cuda.empty_cache()
    kernel_ms = k_ms / max(k_n, 1)
    return dict(case=name, kernel="K0r" if maker == "rational" else "K0w", format=fmt_name, in_rate=fi, out_rate=fo, L=L, M=M,
                ntaps=ntaps, terms_per_output=round(ntaps / L, 1), chunk_out=n, chunk_in=n_in, steps=steps,
                kernel_ms_per_chunk=round(kernel_ms, 3), kernel_launches=k_n, kernel_ns_per_output=round(kernel_ms * 1e6 / n, 4),
                kernel_ms_per_64Mi_outputs=round(kernel_ms * (64 << 20) / n, 3),
                kernel_ps_per_term=round(kernel_ms * 1e9 / n / (ntaps / L), 2))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--chunk", type=int, default=64 << 20, help="output samples per chunk")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--case", choices=tuple(CASES), action="append", help="these cases only (for a counters run); no ratios then")
    ap.add_argument("--format", choices=FORMATS, action="append")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import irdm
    runs = []
    for f in args.format or FORMATS:
        for name in args.case or CASES:
            r = run_case(irdm, torch, name, f, args.chunk, args.steps)
            print(json.dumps(r), flush=True)
            runs.append(r)
    k0r = {r["format"]: r for r in runs if r["case"] == "k0r_25_28"}
    for r in runs if len(k0r) == len(args.format or FORMATS) else []:
        r["span_per_output_vs_k0r_25_28"] = round(r["kernel_ns_per_output"] / k0r[r["format"]]["kernel_ns_per_output"], 2)
        r["span_per_term_vs_k0r_25_28"] = round(r["kernel_ps_per_term"] / k0r[r["format"]]["kernel_ps_per_term"], 2)
    out = dict(what="the front end's wide-ratio kernel (K0w) beside K0r at 25/28 in the same process",
               tool="python3 tools/resample_wide_rate.py --steps %d --chunk %d" % (args.steps, args.chunk),
               gpu="MI355X (gfx950), one device", runs=runs)
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(out, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
