"""TEST INFRASTRUCTURE: tests/_build/libirdm_emul_rec.so -- the emulated build of tests/resample_emul_build.py (its objects,
as that module leaves them: the whole C-ABI with both front ends) plus csrc/recording.cpp, which includes no HIP header and
compiles unchanged.  irdm_recording_probe then comes from an emulated library as it comes from the product's
(tests/test_container_probe.py).  Never loaded by the product."""
import os
import subprocess

import emul_build
import frontend_emul_build
import resample_emul_build

SOURCES = ["recording.cpp"]
SO = os.path.join(emul_build.ROOT, "tests", "_build", "libirdm_emul_rec.so")


def build(force=False):
    base = resample_emul_build.build(force=force)
    out = emul_build.OUT
    deps = [base, os.path.abspath(__file__)] + [os.path.join(emul_build.CSRC, f) for f in os.listdir(emul_build.CSRC)]
    if not force and os.path.exists(SO) and os.path.getmtime(SO) >= emul_build.newest(deps):
        return SO
    objs = [resample_emul_build._obj(out, n) for n in emul_build.SOURCES + frontend_emul_build.SOURCES + resample_emul_build.SOURCES]
    for name in SOURCES:
        obj = resample_emul_build._obj(out, name)
        r = subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-pthread", "-Wall", "-I" + os.path.join(emul_build.ROOT, "include"),
                            "-c", os.path.join(emul_build.CSRC, name), "-o", obj], capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError("emulated build of %s failed:\n" % name + r.stderr[-4000:])
        objs.append(obj)
    subprocess.check_call(["g++", "-shared", "-pthread", "-o", SO] + objs)
    return SO


if __name__ == "__main__":
    print(build(force=True))
