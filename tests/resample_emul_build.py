"""TEST INFRASTRUCTURE: tests/_build/libirdm_emul_rs.so -- the emulated front-end build of tests/frontend_emul_build.py (its
objects, as that module leaves them) plus the rational mode's two sources, csrc/resample.hip and csrc/resample.cpp, compiled
the same way: g++ against the HIP emulation of tests/hip_emul with -ffp-contract=off.  irdm_frontend_create_rational and
everything behind it, kernel included, then run on the CPU (tests/test_resample_emul.py).  Never loaded by the product."""
import os
import subprocess

import emul_build
import frontend_emul_build

SOURCES = ["resample.hip", "resample.cpp"]
SO = os.path.join(emul_build.ROOT, "tests", "_build", "libirdm_emul_rs.so")


def _obj(out, name):
    return os.path.join(out, name.replace(".hip", "_hip").replace(".cpp", "_cpp") + ".o")


def build(force=False):
    base = frontend_emul_build.build(force=force)
    out = emul_build.OUT
    deps = [base, os.path.abspath(__file__)] + [os.path.join(emul_build.CSRC, f) for f in os.listdir(emul_build.CSRC)]
    if not force and os.path.exists(SO) and os.path.getmtime(SO) >= emul_build.newest(deps):
        return SO
    objs = [_obj(out, n) for n in emul_build.SOURCES + frontend_emul_build.SOURCES]
    for name in SOURCES:
        dst = _obj(out, name)[:-2] + ".cpp"
        open(dst, "w").write(emul_build.transform(name, open(os.path.join(emul_build.CSRC, name)).read()))
        obj = dst[:-4] + ".o"
        r = subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-ffp-contract=off", "-pthread", "-w", "-I" + emul_build.EMUL,
                            "-I" + out, "-I" + emul_build.CSRC, "-I" + os.path.join(emul_build.ROOT, "include"), "-c", dst, "-o", obj],
                           capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError("emulated resampler build failed:\n" + r.stderr[-4000:])
        objs.append(obj)
    subprocess.check_call(["g++", "-shared", "-pthread", "-o", SO] + objs)
    return SO


if __name__ == "__main__":
    print(build(force=True))
