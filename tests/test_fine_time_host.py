"""The host side of the symbol timing estimator (csrc/fine_time.hpp: a record's tau, the fold of a stream, the summary) under
AddressSanitizer and UndefinedBehaviorSanitizer, on the CPU: tests/fine_time_host.cpp, a program of its own built here with
g++ against the HIP emulation's headers.  An ambiguous record (tau - c = +-2.6) and an invalid one keep the correlator's
place, a frame whose unique word failed is counted and enters no histogram, and uw_start + delta below zero goes back from
the timestamp."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_fold_under_sanitizers():
    out = os.path.join(ROOT, "tests", "_build")
    os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, "fine_time_host")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-w", "-fsanitize=address,undefined,float-cast-overflow",
                           "-fno-sanitize-recover=undefined,float-cast-overflow", "-I" + os.path.join(ROOT, "tests", "hip_emul"),
                           "-I" + os.path.join(ROOT, "iridium-sniffer_amd", "csrc"), "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "fine_time_host.cpp"), "-o", exe, "-pthread"])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and p.stdout.strip() == "fine_time_host ok", p.stdout[-2000:] + p.stderr[-4000:]
