"""TEST INFRASTRUCTURE: tests/_build/libirdm_emul_fe.so -- the emulated build of tests/emul_build.py (its objects, as that
module leaves them) plus the band-select front end's two sources, csrc/frontend.hip and csrc/frontend.cpp, compiled the same way:
g++ against the HIP emulation of tests/hip_emul with -ffp-contract=off.  The whole C-ABI of the front end, kernel included, then
runs on the CPU (tests/test_frontend_emul.py).  Never loaded by the product."""
import os
import subprocess

import emul_build

SOURCES = ["frontend.hip", "frontend.cpp"]
SO = os.path.join(emul_build.ROOT, "tests", "_build", "libirdm_emul_fe.so")


def build(force=False):
    base = emul_build.build(force=force)
    out = emul_build.OUT
    deps = [base, os.path.abspath(__file__)] + [os.path.join(emul_build.CSRC, f) for f in os.listdir(emul_build.CSRC)]
    if not force and os.path.exists(SO) and os.path.getmtime(SO) >= emul_build.newest(deps):
        return SO
    objs = [os.path.join(out, n.replace(".hip", "_hip").replace(".cpp", "_cpp") + ".o") for n in emul_build.SOURCES]
    for name in SOURCES:
        dst = os.path.join(out, name.replace(".hip", "_hip").replace(".cpp", "_cpp") + ".cpp")
        open(dst, "w").write(emul_build.transform(name, open(os.path.join(emul_build.CSRC, name)).read()))
        obj = dst[:-4] + ".o"
        r = subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-ffp-contract=off", "-pthread", "-w", "-I" + emul_build.EMUL,
                            "-I" + out, "-I" + emul_build.CSRC, "-I" + os.path.join(emul_build.ROOT, "include"), "-c", dst, "-o", obj],
                           capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError("emulated front-end build failed:\n" + r.stderr[-4000:])
        objs.append(obj)
    subprocess.check_call(["g++", "-shared", "-pthread", "-o", SO] + objs)
    return SO


if __name__ == "__main__":
    print(build(force=True))
