"""The DPP controls of the HIP emulation (tests/hip_emul/hip/hip_runtime.h: update_dpp) against the ISA's definition, and the
wavefront reductions of csrc/scan_fast.hip -- wave_or_u32, wave_min_u32, wave_max_u64: row_shr:1/2/4/8, row_bcast:15,
row_bcast:31, the result read from lane 63 -- run through it on one wavefront against a plain loop over the 64 values
(tests/dpp_emul.cpp includes the product's text, cut out of scan_fast.hip unchanged).  No GPU.

Which lanes are checked: the product reads lane 63 only, and every lane of the emulated wavefront receives that value
from readlane -- all 64 are compared with the plain loop.  The six steps without the readlane leave an inclusive prefix
reduction in EVERY lane on the hardware (after the four row_shr steps lane l holds its row's lanes up to l; row_bcast:15
adds lane 15 of the row before to rows 1-3; row_bcast:31 adds lane 31 to rows 2-3): all 64 lanes are compared with that
prefix.  Single moves (row_mask = bank_mask = 0xf, bound_ctrl = false) are compared lane by lane, the lanes without a
source keeping `old`."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "iridium-sniffer_amd", "csrc")

U32 = np.uint32
EXTREME_LANES = (0, 15, 16, 31, 32, 63)


@pytest.fixture(scope="module")
def dpp():
    out_dir = os.path.join(ROOT, "tests", "_build")
    os.makedirs(out_dir, exist_ok=True)
    so = os.path.join(out_dir, "libdppemul.so")
    inc = os.path.join(out_dir, "dpp_reduce_emul.inc")
    src = os.path.join(ROOT, "tests", "dpp_emul.cpp")
    deps = [src, os.path.join(ROOT, "tests", "hip_emul", "hip", "hip_runtime.h"), os.path.join(CSRC, "scan_fast.hip"),
            os.path.abspath(__file__)]
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(d) for d in deps):
        text = open(os.path.join(CSRC, "scan_fast.hip")).read()
        m = re.search(r"// ---- wavefront reductions on the DPP network.*?(?=// Values that are wave-uniform)", text, re.S)
        assert m, "the reductions are no longer where this test cuts them out of scan_fast.hip"
        part = m.group(0)
        for name in ("wave_min_u32", "wave_or_u32", "wave_max_u64", "0x142", "0x143"):
            assert name in part, name
        open(inc, "w").write(part)
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off",
                               "-I" + os.path.join(ROOT, "tests", "hip_emul"), "-I" + out_dir, "-o", so, src])
    return C.CDLL(so)


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _product(L, v32, v64):
    v32 = np.ascontiguousarray(v32, U32)
    v64 = np.ascontiguousarray(v64, np.uint64)
    o, mn, mx = np.zeros(64, U32), np.zeros(64, U32), np.zeros(64, np.uint64)
    L.dpp_emul_product(_p(v32), _p(v64), _p(o), _p(mn), _p(mx))
    return o, mn, mx


def _plain(v32, v64):
    o, mn, mx = 0, 0xffffffff, 0
    for l in range(64):
        o |= int(v32[l])
        mn = min(mn, int(v32[l]))
        mx = max(mx, int(v64[l]))
    return o, mn, mx


def _cases():
    rng = np.random.default_rng(1234)
    for k in range(8):
        yield "random %d" % k, rng.integers(0, 1 << 32, 64, dtype=np.uint64).astype(U32), \
            rng.integers(0, 1 << 63, 64, dtype=np.uint64) * 2 + rng.integers(0, 2, 64, dtype=np.uint64)
    # keys whose high words tie: the low word decides
    hi = rng.integers(0, 4, 64, dtype=np.uint64) << np.uint64(32)
    yield "ties in the high word", rng.integers(0, 16, 64, dtype=np.uint64).astype(U32), hi | rng.integers(0, 1 << 32, 64, dtype=np.uint64)
    # the identity of each reduction in every lane
    yield "identity of or / max", np.zeros(64, U32), np.zeros(64, np.uint64)
    yield "identity of min", np.full(64, 0xffffffff, U32), np.zeros(64, np.uint64)
    for lane in EXTREME_LANES:
        v = np.zeros(64, U32)
        v[lane] = 0x80000001                         # or / max: the one lane that is not the identity
        w = np.full(64, 5, np.uint64)
        w[lane] = (np.uint64(7) << np.uint64(32)) | np.uint64(lane)
        yield "largest in lane %d" % lane, v, w
        v = np.full(64, 0xffffffff, U32)
        v[lane] = 3 + lane                           # min: the one lane below the identity
        w = np.full(64, (7 << 32) | 9, np.uint64)
        w[lane] = (np.uint64(7) << np.uint64(32)) | np.uint64(10)      # max decided by the low word, in that lane
        yield "smallest in lane %d" % lane, v, w


def test_product_reductions_equal_a_plain_loop(dpp):
    """wave_or_u32 / wave_min_u32 / wave_max_u64 as scan_fast.hip has them: the value every lane gets back (lane 63's) against
    a loop over the 64 inputs -- random lanes, the identity everywhere, the extreme in lane 0 / 15 / 16 / 31 / 32 / 63"""
    n = 0
    for name, v32, v64 in _cases():
        o, mn, mx = _product(dpp, v32, v64)
        po, pmn, pmx = _plain(v32, v64)
        assert (o == po).all(), (name, [hex(x) for x in o], hex(po))
        assert (mn == pmn).all(), (name, [hex(x) for x in mn], hex(pmn))
        assert (mx == pmx).all(), (name, [hex(x) for x in mx], hex(pmx))
        n += 1
    assert n == 8 + 3 + 2 * len(EXTREME_LANES)


def test_every_lane_holds_the_inclusive_prefix_after_the_six_steps(dpp):
    """the six steps without the readlane: lane l holds the reduction over lanes 0 .. l, as the ISA's definition of the six
    moves gives it -- all 64 lanes, for or and for min"""
    for name, v32, _ in _cases():
        v32 = np.ascontiguousarray(v32, U32)
        lo, lm = np.zeros(64, U32), np.zeros(64, U32)
        dpp.dpp_emul_lanes(_p(v32), _p(lo), _p(lm))
        want_or = np.bitwise_or.accumulate(v32)
        want_min = np.minimum.accumulate(v32)
        assert np.array_equal(lo, want_or), (name, lo, want_or)
        assert np.array_equal(lm, want_min), (name, lm, want_min)


def _isa_move(ctrl, old, src):
    """the ISA's DPP move for row_mask = bank_mask = 0xf, bound_ctrl = false: lanes without a source keep old"""
    out = old.copy()
    for l in range(64):
        if 0x111 <= ctrl <= 0x11f:                       # row_shr:n
            n = ctrl - 0x110
            if (l & 15) >= n:
                out[l] = src[l - n]
        elif ctrl == 0x138:                              # wave_shr:1
            if l >= 1:
                out[l] = src[l - 1]
        elif ctrl == 0x142:                              # row_bcast:15
            if l >= 16:
                out[l] = src[(l // 16) * 16 - 1]
        elif ctrl == 0x143:                              # row_bcast:31
            if l >= 32:
                out[l] = src[31]
        else:
            raise ValueError(ctrl)
    return out


@pytest.mark.parametrize("ctrl", [0x111, 0x118, 0x138, 0x142, 0x143])
def test_single_moves_lane_by_lane(dpp, ctrl):
    src = np.arange(64, dtype=np.int32) * 3 + 7
    old = -(np.arange(64, dtype=np.int32) + 1000)
    out = np.zeros(64, np.int32)
    assert dpp.dpp_emul_step(ctrl, _p(old), _p(src), _p(out)) == 0
    want = _isa_move(ctrl, old, src)
    assert np.array_equal(out, want), (hex(ctrl), out, want)
    if ctrl == 0x142:
        assert (out[:16] == old[:16]).all() and (out[16:32] == src[15]).all() and (out[32:48] == src[31]).all() and (out[48:] == src[47]).all()
    if ctrl == 0x143:
        assert (out[:32] == old[:32]).all() and (out[32:] == src[31]).all()
