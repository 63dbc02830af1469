"""Helpers of the full-precision int16 format tests (tests/test_gpu_formats16.py, tests/formats16_emul_run.py).

The contract (include/irdm_hip.h, IRDM_FMT_CI16_FULL / IRDM_FMT_SC16Q11): a context in either format produces exactly the
records of a cf32 context fed v.astype(np.float32) * scale.  run() feeds one stream through one context and returns every
record queue it filled; same_records() compares two such runs field by field, floats by their bits."""
import ctypes as C

import numpy as np

import irdm
import siggen

FORMATS = (irdm.FMT_CI16_FULL, irdm.FMT_SC16Q11)
NAMES = {irdm.FMT_CI16_FULL: "ci16-full", irdm.FMT_SC16Q11: "sc16q11"}


def converted(x, fmt):
    """interleaved int16 -> the cf32 stream a context in format fmt sees"""
    return (np.asarray(x, np.int16).astype(np.float32) * np.float32(irdm.FMT_SCALE[fmt])).view(np.complex64)


def int16_scene(fs, secs, nb, seed, scale=131072.0):
    n = int(secs * fs) // 32768 * 32768
    iq, _ = siggen.standard_scene(fs, n, nb, seed=seed)
    return siggen.to_ci16(iq, scale)


def chunks_of(n, parts, block=32768):
    """n samples in `parts` chunks of whole feed blocks, the remainder on the last (a ragged end)"""
    blocks = n // block
    cuts = [blocks * (i + 1) // parts for i in range(parts)]
    out, prev = [], 0
    for c in cuts:
        if c > prev:
            out.append((c - prev) * block)
            prev = c
    out[-1] += n - sum(out)
    return out


def run(x, fs, fmt, chunks=None, depth=0, feed="host", packed=False, options=None):
    """Feed x (cf32 samples, or interleaved int16) through one context.

    feed: "host" irdm_feed_host from pageable memory; "pinned" irdm_feed_host from an irdm_host_alloc buffer; "device"
    irdm_feed_device from a device buffer per chunk; "ingest_lookahead" every chunk written in place (irdm_ingest_ptr)
    and begun before the previous one is ended.  packed: options packed_records, parsed_records and frame_records (the
    compact queues); otherwise the full records with the frames' samples."""
    per = 1 if fmt == irdm.FMT_CF32 else 2
    n = len(x) // per
    sizes = list(chunks or [n])
    assert sum(sizes) == n
    p = irdm.Pipeline(fs, fmt=fmt, max_chunk_samples=max(sizes), max_bursts_per_chunk=1024, pipeline_depth=depth)
    L = irdm.lib()
    pinned = []
    try:
        opts = {"packed_records": 1, "parsed_records": 1, "frame_records": 1} if packed else {"keep_frame_samples": 1}
        opts.update(options or {})
        for k, v in opts.items():
            p.set_option(k, v)
        pending = []
        off = 0
        for c in sizes:
            part = np.ascontiguousarray(x[off * per:(off + c) * per])
            off += c
            if feed == "host":
                p.feed_host(part)
            elif feed == "pinned":
                if not pinned:
                    pinned.append(irdm.host_alloc(max(sizes) * per * part.itemsize))
                ptr, view = pinned[0]
                view[:part.nbytes] = part.view(np.uint8)
                p.feed_host_ptr(ptr, c)
            elif feed == "device":
                ptr = irdm.device_buffer(part)
                try:
                    p.feed_device(ptr, c)
                finally:
                    irdm.device_free(ptr)
            elif feed == "ingest_lookahead":
                ptr = p.ingest_ptr(c)
                assert ptr, "irdm_ingest_ptr refused a chunk of %d samples" % c
                assert L.irdm_device_upload(C.c_void_p(ptr), part.ctypes.data_as(C.c_void_p), part.nbytes) == 0
                p.feed_begin(ptr, c)
                pending.append(c)
                if len(pending) > 1:
                    p.feed_end()
                    pending.pop(0)
            else:
                raise ValueError(feed)
        while pending:
            p.feed_end()
            pending.pop(0)
        if depth:
            p.flush()
        res = dict(tagged=p.tagged, n_samples=p.sample_count, bursts=p.poll_bursts())
        if packed:
            res.update(packed=p.poll_demods_packed(), ida=p.poll_ida_packed(), frame=p.poll_frame_packed())
        else:
            res["infos"], res["samples"] = p.poll_frames()
            res["demods"] = p.poll_demods()
        return res
    finally:
        p.close()
        for ptr, _ in pinned:
            irdm.host_free(ptr)


def _struct_fields(s):
    """(name, raw bytes) of every field of a ctypes record: floats compare by their bits, padding is left out"""
    raw = bytes(s)
    t = type(s)
    return [(name, raw[getattr(t, name).offset:getattr(t, name).offset + getattr(t, name).size])
            for name, *_ in t._fields_]


def same_records(a, b):
    """two run() results hold the same records, bit for bit; returns the number of records compared"""
    assert a["tagged"] == b["tagged"] and a["n_samples"] == b["n_samples"], (a["tagged"], b["tagged"])
    n = 0
    for key in ("bursts", "infos", "demods", "packed", "ida", "frame"):
        if key not in a and key not in b:
            continue
        assert len(a[key]) == len(b[key]), (key, len(a[key]), len(b[key]))
        for ra, rb in zip(a[key], b[key]):
            for (name, va), (_, vb) in zip(_struct_fields(ra), _struct_fields(rb)):
                assert va == vb, (key, name, getattr(ra, "id", None))
            n += 1
    if "samples" in a or "samples" in b:
        assert len(a["samples"]) == len(b["samples"])
        for sa, sb in zip(a["samples"], b["samples"]):
            assert np.array_equal(np.asarray(sa).view(np.uint32), np.asarray(sb).view(np.uint32))
    return n
