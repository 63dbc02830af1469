"""TEST INFRASTRUCTURE: tests/_build/libirdm_emul_rw.so -- the emulated rational front end of tests/resample_emul_build.py (its
objects, as that module leaves them) plus the wide-ratio kernel's two sources, csrc/resample_wide.hip and
csrc/resample_wide.cpp, compiled the same way: g++ against the HIP emulation of tests/hip_emul with -ffp-contract=off.
irdm_frontend_create_wide / _create_resampler and everything behind them, K0w included, then run on the CPU
(tests/test_resample_wide_emul.py).  Never loaded by the product."""
import os
import subprocess

import emul_build
import frontend_emul_build
import resample_emul_build

SOURCES = ["resample_wide.hip", "resample_wide.cpp"]
SO = os.path.join(emul_build.ROOT, "tests", "_build", "libirdm_emul_rw.so")


def build(force=False):
    base = resample_emul_build.build(force=force)
    out = emul_build.OUT
    deps = [base, os.path.abspath(__file__)] + [os.path.join(emul_build.CSRC, f) for f in os.listdir(emul_build.CSRC)]
    if not force and os.path.exists(SO) and os.path.getmtime(SO) >= emul_build.newest(deps):
        return SO
    objs = [resample_emul_build._obj(out, n) for n in emul_build.SOURCES + frontend_emul_build.SOURCES + resample_emul_build.SOURCES]
    for name in SOURCES:
        dst = resample_emul_build._obj(out, name)[:-2] + ".cpp"
        open(dst, "w").write(emul_build.transform(name, open(os.path.join(emul_build.CSRC, name)).read()))
        obj = dst[:-4] + ".o"
        r = subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-ffp-contract=off", "-pthread", "-w", "-I" + emul_build.EMUL,
                            "-I" + out, "-I" + emul_build.CSRC, "-I" + os.path.join(emul_build.ROOT, "include"), "-c", dst, "-o", obj],
                           capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError("emulated wide resampler build failed:\n" + r.stderr[-4000:])
        objs.append(obj)
    subprocess.check_call(["g++", "-shared", "-pthread", "-o", SO] + objs)
    return SO


if __name__ == "__main__":
    print(build(force=True))
