"""TEST INFRASTRUCTURE: the case table of the front end's shared load stage (csrc/fe_stage.hpp), which
tests/test_gpu_fe_stage.py runs on the GPU and tests/test_fe_stage_emul.py, through tests/fe_stage_emul_run.py, on the CPU
emulation: whichever build irdm.lib() has loaded.  Every kernel instantiation that differs in the load stage -- K0's three
thread counts, K0r with and without its pad sample, K0w's two PAD instantiations -- takes every device format, fed three
ways, with a shift whose rotation index wraps inside a tile.  The references are the plain C models of the arithmetic
contract (tests/frontend_model.c, tests/resample_model.c), bit for bit; cu8 and the int32 formats go to the models as the
cf32 stream the load stage converts them to (exact in float)."""
import numpy as np

import ci32
import frontend_model as fm
import irdm
import resample_model as rm
import resample_wide_cases as wc

# name -> (kernel, capture rate, output rate, the input samples of one tile).  K0: NT * 8 * D inputs per tile, NT = 256 /
# 128 / 64 threads.  K0r: nper * M, nper <= 256 periods (5/28: M even, pad sample and magic multiply; 25/27: M odd, the slot
# is the staged index).  K0w: B * M / L (400/401: B = 2048, no pad; 100/801: B = 256, pad).
ROWS = {"k0_d2": ("k0", 4_000_000, 2_000_000, 256 * 8 * 2), "k0_d5": ("k0", 10_000_000, 2_000_000, 128 * 8 * 5),
        "k0_d16": ("k0", 32_000_000, 2_000_000, 64 * 8 * 16),
        "k0r_5_28": ("k0r", 56_000_000, 10_000_000, 256 * 28), "k0r_25_27": ("k0r", 2_700_000, 2_500_000, 256 * 27),
        "k0w_400_401": ("k0w", 10_025_000, 10_000_000, 2048 * 401 // 400 + 1), "k0w_100_801": ("k0w", 8_010_000, 1_000_000, 256 * 801 // 100 + 1)}
FORMATS = (irdm.FMT_CI8, irdm.FMT_CI16, irdm.FMT_CF32, irdm.FMT_CI16_FULL, irdm.FMT_SC16Q11, irdm.FMT_CU8, irdm.FMT_CI32,
           irdm.FMT_CI32_24)
NAMES = {**fm.NAMES, **ci32.NAMES, irdm.FMT_CU8: "cu8"}
Q_LIST = (14418, -32768)


def capture(fmt, n, seed):
    """n samples of format fmt over its whole code range, and the (stream, format) the models take for it"""
    if fmt == irdm.FMT_CU8:
        u = np.random.default_rng(seed).integers(0, 256, 2 * n, dtype=np.uint8)         # (tests/cu8_emul_run.py's)
        return u, (irdm.convert_cu8(u), irdm.FMT_CF32)
    if fmt in ci32.FORMATS:
        v = ci32.stats_input(fmt, n, seed)
        return v, (irdm.convert_ci32(v, fmt), irdm.FMT_CF32)
    x = fm.random_capture(fmt, n, seed)
    return x, (x, fmt)


def make_stage(kernel, fi, fmt, fo, shift):
    if kernel == "k0":
        st = fm.Stage(fi, fmt, fi // fo, shift)
        st.L, st.M = 1, fi // fo
        return st
    return rm.Stage(fi, fmt, fo, shift) if kernel == "k0r" else wc.Stage(fi, fmt, fo, shift)


def feeds_of(n, tile, per_phase):
    """whole; ragged -- 1 sample, one less than the taps of a phase (both shorter than the carried tail), a prime, two tiles
    and a bit (tiles wholly inside a chunk that does not start the stream), in turn; and the cut of the run after reset"""
    ragged = fm.ragged_feeds(n, max(2, per_phase), (997, 2 * tile + 13))
    assert ragged[0] == 1 and 1 < ragged[1] < per_phase and max(ragged) > 2 * tile and len(ragged) > 4
    return [n], ragged, [n // 3, n - n // 3]


def check_row(name, fmt, q):
    """four tiles' worth of inputs and an odd remainder: whole, then (the same object, irdm_frontend_reset) in two feeds,
    and on a fresh object in ragged feeds = the model.  Returns the number of outputs."""
    kernel, fi, fo, tile = ROWS[name]
    L, M = rm.ratio(fi, fo)
    n = 4 * tile + 777
    shift = q * fi / 65536.0
    assert fm.quantise(shift, fi) == q             # ((q n) mod 65536 wraps every few samples: many times within a tile)
    x, (xm, fmt_m) = capture(fmt, n, seed=100 * M + L + fmt)
    st = make_stage(kernel, fi, fmt, fo, shift)
    try:
        assert (st.L, st.M) == (L, M) and st.fe.out_rate == fo
        if kernel == "k0w":
            geo = irdm.Frontend.wide_geometry(fi, fo)
            assert geo["tile"] * M // L + 1 == tile and bool(((2 * M + L) // (2 * L)) % 2 == 0) == (name == "k0w_100_801"), geo
        taps = st.fe.taps()
        want = fm.run(xm, fmt_m, M, q, taps) if kernel == "k0" else rm.run(xm, fmt_m, L, M, q, taps)
        whole, ragged, halves = feeds_of(n, tile, -(-len(taps) // L))
        assert len(want) == rm.n_outputs(n, L, M)
        got = st.run(x, whole)
        assert wc.differ(got, want) is None, (name, NAMES[fmt], q, "whole", wc.differ(got, want))
        st.fe.reset()
        got = st.run(x, halves)
        assert wc.differ(got, want) is None, (name, NAMES[fmt], q, "after reset", wc.differ(got, want))
    finally:
        st.close()
    st = make_stage(kernel, fi, fmt, fo, shift)
    try:
        got = st.run(x, ragged)
    finally:
        st.close()
    assert wc.differ(got, want) is None, (name, NAMES[fmt], q, "ragged", wc.differ(got, want))
    return len(want)


def check(name):
    return {"%s_q%d" % (NAMES[fmt], q): check_row(name, fmt, q) for fmt in FORMATS for q in Q_LIST}
