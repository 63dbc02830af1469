"""Writers of self-describing recordings for the container tests (tests/test_container_probe.py,
tests/test_gpu_containers.py): WAV / RF64, SigMF and SDRangel's .sdriq, built with struct from the layouts that
include/irdm_hip.h states for irdm_recording_probe -- not from the programs that write such files."""
import json
import struct
import zlib

import numpy as np

PCM, FLOAT, EXTENSIBLE = 1, 3, 0xFFFE


def chunk(tag, body):
    """one RIFF chunk: word-aligned, an odd size is followed by one pad byte"""
    assert len(tag) == 4
    return tag + struct.pack("<I", len(body)) + body + (b"\0" if len(body) & 1 else b"")


def fmt_chunk(tag, channels, rate, bits, size=16):
    block = channels * bits // 8
    if size == 40:
        body = struct.pack("<HHIIHH", EXTENSIBLE, channels, rate, rate * block, block, bits)
        body += struct.pack("<HHI", 22, bits, 3) + struct.pack("<H", tag) + bytes.fromhex("000000001000800000aa00389b71")
    else:
        body = struct.pack("<HHIIHH", tag, channels, rate, rate * block, block, bits)
        if size == 18:
            body += struct.pack("<H", 0)
    assert len(body) == size
    return chunk(b"fmt ", body)


def systemtime(y, mo, d, h, mi, s, ms, dow=0):
    return struct.pack("<8H", y, mo, dow, d, h, mi, s, ms)


def auxi_chunk(start, stop, centre_hz, extra=b""):
    """the binary auxi: two SYSTEMTIMEs (UTC), then a u32 centre frequency in Hz"""
    return chunk(b"auxi", systemtime(*start) + systemtime(*stop) + struct.pack("<I", centre_hz) + extra)


def wav(data, tag=PCM, channels=2, rate=2_000_000, bits=16, fmt_size=16, before=(), after=(), data_size=None, riff=b"RIFF",
        ds64_data=None):
    """a WAV file's bytes: RIFF/WAVE, [ds64], fmt, `before` chunks, data (declared size data_size if given), `after` chunks"""
    data = bytes(data)
    body = b"WAVE"
    if ds64_data is not None:
        body += chunk(b"ds64", struct.pack("<QQQI", 0, ds64_data, 0, 0))
    body += fmt_chunk(tag, channels, rate, bits, fmt_size)
    for c in before:
        body += c
    body += b"data" + struct.pack("<I", len(data) if data_size is None else data_size) + data + (b"\0" if len(data) & 1 else b"")
    for c in after:
        body += c
    size = len(body) if riff == b"RIFF" and len(body) < 2 ** 32 else 0xFFFFFFFF
    return riff + struct.pack("<I", size) + body


def sigmf_meta(datatype, rate, frequency=None, datetime=None, header_bytes=None, trailing_bytes=None, dataset=None,
               num_channels=None, captures=None, rate_text=None):
    """the text of a .sigmf-meta file; rate_text writes core:sample_rate verbatim (2.4e6)"""
    g = {"core:datatype": datatype, "core:version": "1.0.0", "core:sample_rate": "@RATE@",
         "core:description": "a \"quoted\" \\ description with é and nested {braces} [brackets]"}
    if trailing_bytes is not None:
        g["core:trailing_bytes"] = trailing_bytes
    if dataset is not None:
        g["core:dataset"] = dataset
    if num_channels is not None:
        g["core:num_channels"] = num_channels
    c = {"core:sample_start": 0}
    if frequency is not None:
        c["core:frequency"] = frequency
    if datetime is not None:
        c["core:datetime"] = datetime
    if header_bytes is not None:
        c["core:header_bytes"] = header_bytes
    doc = {"global": g, "captures": [c] if captures is None else captures,
           "annotations": [{"core:sample_start": 10, "core:sample_count": 5, "core:label": "x", "ok": True, "none": None}]}
    text = json.dumps(doc, indent=2)
    return text.replace('"@RATE@"', rate_text if rate_text is not None else repr(rate))


def sdriq_header(rate, centre_hz, start, sample_size, crc=None):
    """the 32-byte header: u32 rate, u64 centre, u64 start time, u32 sample size, u32 0, u32 CRC-32 of the first 28 bytes"""
    h = struct.pack("<IQQII", rate, centre_hz, start, sample_size, 0)
    assert len(h) == 28
    return h + struct.pack("<I", zlib.crc32(h) & 0xFFFFFFFF if crc is None else crc)


def interleave(iq):
    x = np.empty(2 * len(iq), dtype=np.float32)
    x[0::2] = iq.real
    x[1::2] = iq.imag
    return x


def quantise(iq, scale, lo, hi, dtype):
    """interleaved integer samples: clip(round(x * scale))"""
    return np.clip(np.round(interleave(iq).astype(np.float64) * scale), lo, hi).astype(dtype)
