"""TEST INFRASTRUCTURE: the input statistics of the int32 formats against the integer model (tests/ci32.py over
tests/inputstats_model.py), on whichever build irdm.lib() loads -- the GPU library (tests/test_gpu_ci32.py) or an emulated
one (tests/ci32_emul_run.py)."""
import numpy as np

import ci32
import formats16 as f16
import input_stats_checks as ic
import inputstats_model as im
import irdm

SIZES = (0, 1, 2, 3, 63, 64, 65, 255, 4101, (1 << 18) + 7)


def stage_one(x, fmt, off, what):
    d = im.DeviceInput(x, fmt, off)
    try:
        st = irdm.input_stats_device(d.ptr, d.n, fmt)
    finally:
        d.close()
    im.check(st, ci32.model(x, fmt), fmt, what)
    return st


def model_selfcheck():
    """the model's split sums against plain Python integers on a small stream with the extreme codes"""
    x = np.array([ci32.I32_MIN, ci32.I32_MAX, ci32.I32_MAX, ci32.I32_MIN, -5, 7, 2 ** 24 + 1, -(2 ** 30)] * 9, np.int32)
    m = ci32.model(x, irdm.FMT_CI32)
    for k in range(2):
        vals = [int(t) for t in x[k::2]]
        assert m["sum"][k] == sum(vals) / 2 ** 31 and m["sum_sq"][k] == sum(t * t for t in vals) / 2 ** 62
    assert m["abs_max"] == [np.float32(1.0), np.float32(1.0)] and m["code_min"] == [ci32.I32_MIN] * 2


def stage_cases():
    """irdm_input_stats_device: both formats; every size at a base 0 and 1 sample past a 16-byte boundary, rails at the first
    and the last sample; all-rail buffers: INT32_MIN everywhere (the sum of squares 2^62 n, past 64 bits from n = 4), INT32_MAX
    everywhere, the rails of format 9 and one code inside them"""
    model_selfcheck()
    count = 0
    for fmt in ci32.FORMATS:
        for n in SIZES:
            x = ci32.stats_input(fmt, n, seed=1000 * fmt + n % 997)
            for off in (0, 1):
                st = stage_one(x, fmt, off, "%s n %d off %d" % (ci32.NAMES[fmt], n, off))
                if n >= 2:                  # (n = 1: the last sample's rails overwrite the first's)
                    assert st.n_rail_lo[0] >= 1 and st.n_rail_hi[1] >= 1
                count += 1
    n = 4101
    for code, want_sq, want_abs in ((ci32.I32_MIN, float(n), 1.0), (ci32.I32_MAX, (2 ** 31 - 1) ** 2 * n / 2 ** 62, 1.0)):
        st = stage_one(np.full(2 * n, code, np.int32), irdm.FMT_CI32, 1, "all-rail ci32 %d" % code)
        assert list(st.n_rail_lo) == ([n, n] if code < 0 else [0, 0]) and list(st.n_rail_hi) == ([0, 0] if code < 0 else [n, n])
        assert list(st.code_min) == list(st.code_max) == [code, code]
        assert list(st.sum_sq) == [want_sq, want_sq] and list(st.abs_max) == [want_abs, want_abs]
        count += 1
    for code, lo, hi in ((-2 ** 23, n, 0), (2 ** 23 - 1, 0, n), (-2 ** 23 + 1, 0, 0), (2 ** 23 - 2, 0, 0), (2 ** 23, 0, n), (ci32.I32_MIN, n, 0)):
        st = stage_one(np.full(2 * n, code, np.int32), irdm.FMT_CI32_24, 0, "all-one-code ci32-24 %d" % code)
        assert list(st.n_rail_lo) == [lo, lo] and list(st.n_rail_hi) == [hi, hi], (code, list(st.n_rail_lo), list(st.n_rail_hi))
        count += 1
    return dict(cases=count)


def context_cuts(fs=2_000_000, secs=0.3):
    """option input_stats over one stream fed whole, in four chunks at pipeline_depth 1 and in ragged pieces, both formats:
    byte-identical structs, the model's"""
    out = {}
    for fmt in ci32.FORMATS:
        n = int(secs * fs) // 32768 * 32768
        v = ci32.stats_input(fmt, n, seed=40 + fmt)
        want = ci32.model(v, fmt)
        got = []
        for sizes, depth in (([n], 0), (f16.chunks_of(n, 4), 1), (ic.ragged_blocks(n), 0)):
            st, _ = ic.context_run(v, fs, fmt, sizes, depth)
            im.check(st, want, fmt, "context %s %d chunks" % (ci32.NAMES[fmt], len(sizes)))
            got.append(ic.struct_bytes(st))
        assert got[0] == got[1] == got[2]
        out[ci32.NAMES[fmt]] = n
    return out


def all_cases():
    res = stage_cases()
    res["context"] = context_cuts()
    return res
