"""The host side of the frame line estimators (csrc/frame_line.hpp: the histogram's bins, the fold of a stream, the
quantiles) under AddressSanitizer and UndefinedBehaviorSanitizer, on the CPU: tests/line_hist_host.cpp, a program of its own
built here with g++ against the HIP emulation's headers.  A value far beyond a histogram's ends, NaN and +-Inf are clamped
in double, never converted to int first."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bins_and_quantiles_under_sanitizers():
    out = os.path.join(ROOT, "tests", "_build")
    os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, "line_hist_host")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-w", "-fsanitize=address,undefined,float-cast-overflow",
                           "-fno-sanitize-recover=undefined,float-cast-overflow", "-I" + os.path.join(ROOT, "tests", "hip_emul"),
                           "-I" + os.path.join(ROOT, "iridium-sniffer_amd", "csrc"), "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "line_hist_host.cpp"), "-o", exe, "-pthread"])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and p.stdout.strip() == "line_hist_host ok", p.stdout[-2000:] + p.stderr[-4000:]
