"""TEST INFRASTRUCTURE: the checks of the input statistics that run on whichever build irdm.lib() loads -- the GPU library
(tests/test_gpu_input_stats.py) or an emulated one (tests/input_stats_emul_run.py)."""
import numpy as np

import cu8
import formats16 as f16
import inputstats_model as im
import irdm

SIZES = (0, 1, 3, 63, 64, 65, 255, 4101, (1 << 20) + 7)


def stage_one(x, fmt, off, what):
    d = im.DeviceInput(x, fmt, off)
    try:
        st = irdm.input_stats_device(d.ptr, d.n, fmt)
    finally:
        d.close()
    im.check(st, im.model(x, fmt), fmt, what)
    return st


def stage_cases():
    """irdm_input_stats_device against the model: every format; every size at a base 0, 1 and 3 samples past a 16-byte
    boundary, rails at the first and the last sample; an all-rail buffer; cf32 with NaN, Inf, +-1.0 and subnormals"""
    count = 0
    for fmt in im.FORMATS:
        for n in SIZES:
            x = im.with_rails_at_the_ends(im.random_input(fmt, n, seed=1000 * fmt + n % 997), fmt)
            for off in (0, 1, 3):
                stage_one(x, fmt, off, "%s n %d off %d" % (im.NAMES[fmt], n, off))
                count += 1
    # all-rail: every component -32768, n = 2^20: the sum of c^2 is 2^50 per component
    n = 1 << 20
    x = np.full(2 * n, -32768, np.int16)
    for fmt in (irdm.FMT_CI16, irdm.FMT_CI16_FULL, irdm.FMT_SC16Q11):
        st = stage_one(x, fmt, 1, "all-rail %s" % im.NAMES[fmt])
        assert list(st.n_rail_lo) == [n, n] and list(st.n_rail_hi) == [0, 0]
        if fmt == irdm.FMT_CI16_FULL:
            assert list(st.sum_sq) == [float(n), float(n)] and list(st.sum) == [-float(n), -float(n)]
        count += 1
    for fmt, code in ((irdm.FMT_CI8, -128), (irdm.FMT_CU8, 255), (irdm.FMT_CU8, 0)):
        st = stage_one(np.full(2 * 4101, code, im.DTYPES[fmt]), fmt, 3, "all-rail %s %d" % (im.NAMES[fmt], code))
        assert list(st.n_rail_lo)[0] + list(st.n_rail_hi)[0] == 4101
        count += 1
    for n in (1, 7, 65, 4101, (1 << 20) + 7):
        for off in (0, 1):
            st = stage_one(im.special_cf32(n, seed=n), irdm.FMT_CF32, off, "cf32 specials n %d off %d" % (n, off))
            count += 1
    assert st.n_nonfinite[0] + st.n_nonfinite[1] > 0
    return dict(cases=count)


def struct_bytes(st):
    return bytes(st)


def context_scene():
    """the 2 MHz cu8 scene of tests/test_cu8_emul.py"""
    return 2_000_000, cu8.cu8_scene(2_000_000, 1.2, 6, seed=162)


def context_run(u, fs, fmt, sizes, depth=0, feed="host", stats=True, reset_first=False):
    """one stream through a context with option input_stats; returns (the struct, the record queues)"""
    per = 1 if fmt == irdm.FMT_CF32 else 2
    p = irdm.Pipeline(fs, fmt=fmt, max_chunk_samples=max(sizes), max_bursts_per_chunk=1024, pipeline_depth=depth)
    try:
        p.set_option("keep_frame_samples", 1)
        if stats:
            p.set_option("input_stats", 1)
        if reset_first:
            # a first stream that leaves totals behind, then irdm_reset: they start over
            p.feed_host(np.ascontiguousarray(u[:32768 * per * 3]))
            if depth:
                p.flush()
            assert p.input_stats().n_samples == 32768 * 3
            p.poll_bursts(), p.poll_frames(), p.poll_demods()
            p.reset(start_time_ns=1700000000 * 10**9)
            assert p.input_stats().n_samples == 0
        pending, off = [], 0
        for c in sizes:
            part = np.ascontiguousarray(u[off * per:(off + c) * per])
            off += c
            if feed == "host":
                p.feed_host(part)
            else:
                import ctypes as C
                ptr = p.ingest_ptr(c)
                assert ptr
                assert irdm.lib().irdm_device_upload(C.c_void_p(ptr), part.ctypes.data_as(C.c_void_p), part.nbytes) == 0
                p.feed_begin(ptr, c)
                pending.append(c)
                if len(pending) > 1:
                    p.feed_end()
                    pending.pop(0)
        while pending:
            p.feed_end()
            pending.pop(0)
        if depth:
            p.flush()
        st = p.input_stats() if stats else None
        res = dict(tagged=p.tagged, n_samples=p.sample_count, bursts=p.poll_bursts())
        res["infos"], res["samples"] = p.poll_frames()
        res["demods"] = p.poll_demods()
        return st, res
    finally:
        p.close()


def ragged_blocks(n, block=32768):
    """n samples in chunks of 5, 1, 17, 2, ... feed blocks, the remainder on the last"""
    out, k, left = [], 0, n // block
    while left > 0:
        b = min(left, (5, 1, 17, 2)[k % 4])
        out.append(b * block)
        left -= b
        k += 1
    out[-1] += n % block
    return out


def context_cuts():
    """the option over the scene fed whole, in four chunks and in ragged pieces: byte-identical structs, the model's"""
    fs, u = context_scene()
    n = len(u) // 2
    want = im.model(u, irdm.FMT_CU8)
    got = []
    for sizes, depth in (([n], 0), (f16.chunks_of(n, 4), 1), (ragged_blocks(n), 0)):
        st, _ = context_run(u, fs, irdm.FMT_CU8, sizes, depth)
        im.check(st, want, irdm.FMT_CU8, "context %d chunks" % len(sizes))
        got.append(struct_bytes(st))
    assert got[0] == got[1] == got[2]
    return dict(n_samples=n, rails=want["n_rail_lo"] + want["n_rail_hi"])


def frontend_run(make_fe, u, fmt, feeds, out_cap):
    """the capture through irdm_frontend_run_device with the statistics on; returns the struct"""
    import ctypes as C
    per = 1 if fmt == irdm.FMT_CF32 else 2
    L = irdm.lib()
    fe = make_fe()
    d_out = L.irdm_device_alloc(0, out_cap * 8)
    try:
        fe.input_stats_enable(True)
        pos = 0
        for f in feeds:
            part = np.ascontiguousarray(u[pos * per:(pos + f) * per])
            d_in = irdm.device_buffer(part if len(part) else np.zeros(2, u.dtype))
            try:
                assert L.irdm_frontend_run_device(fe.h, C.c_void_p(d_in), f, C.c_void_p(d_out), out_cap, None) >= 0
            finally:
                irdm.device_free(d_in)
            pos += f
        st = fe.input_stats()
        fe.reset()
        assert fe.input_stats().n_samples == 0
        return st
    finally:
        L.irdm_device_free(d_out)
        fe.close()


def frontend_cuts(n=5 * 4096 + 777):
    """the front end's getter over a cu8 capture, K0 at D = 5: whole and in ragged feeds, byte-identical, the model's;
    irdm_frontend_reset starts over"""
    import frontend_model as fm
    u = np.random.default_rng(77).integers(0, 256, 2 * n, dtype=np.uint8)
    u[:64] = 0
    u[-64:] = 255
    want = im.model(u, irdm.FMT_CU8)
    got = []
    for feeds in ([n], fm.ragged_feeds(n, 223, (997, 4099))):
        st = frontend_run(lambda: irdm.Frontend(10_000_000, irdm.FMT_CU8, 5, 1_000_000.0), u, irdm.FMT_CU8, feeds, n // 5 + 64)
        im.check(st, want, irdm.FMT_CU8, "front end %d feeds" % len(feeds))
        got.append(struct_bytes(st))
    assert got[0] == got[1]
    return dict(n_samples=n)
