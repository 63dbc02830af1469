"""irdm_recording_probe (include/irdm_hip.h, csrc/recording.cpp) and the command line's container options, without a GPU.

The files are built with struct in tmp_path (tests/containers.py) from the layouts the header states -- the binary auxi
chunk and the .sdriq header as this project documents them, not as the programs that write them were checked to do -- and
probed through irdm.py, which loads the library the way tests/test_capi_exports.py does.  --probe, --format beside a
container and mixed rates in a batch end before any device call, so they run here too."""
import calendar
import os
import struct
import subprocess

import numpy as np
import pytest

import containers as ct
import irdm

EXE = os.path.join(os.path.dirname(irdm.LIB_PATH), "iridium-sniffer-hip")
START = (2023, 11, 14, 22, 13, 20, 250)         # 1700000000.250 UTC
STOP = (2023, 11, 14, 22, 14, 20, 0)
START_NS = 1700000000_250_000_000


@pytest.fixture(scope="module", autouse=True)
def built():
    irdm.build()


def probe(path, container=0):
    return irdm.recording_probe(path, container)


def put(tmp_path, name, data):
    p = tmp_path / name
    p.write_bytes(data if isinstance(data, bytes) else data.encode())
    return p


def samples(n, dtype, seed=1):
    info = np.iinfo(dtype)
    return np.random.default_rng(seed).integers(info.min, info.max, 2 * n, dtype=dtype, endpoint=True).tobytes()


def expect(path, kind, fmt, rate, offset, nbytes, container=0, data=None):
    rc, i, msg = probe(path, container)
    assert rc == 0, msg
    assert (i.kind, i.format, i.sample_rate) == (kind, fmt, rate), (i.kind, i.format, i.sample_rate)
    assert (i.data_offset, i.data_bytes) == (offset, nbytes), (i.data_offset, i.data_bytes)
    assert os.fsdecode(i.data_path) == str(data or path)
    return i


def refused(path, *words, container=0):
    rc, _, msg = probe(path, container)
    assert rc == -1, (rc, msg)
    for w in words:
        assert w in msg, msg
    return msg


# ---- WAV / RF64 ----

@pytest.mark.parametrize("tag,bits,dtype,fmt", [(ct.PCM, 8, np.uint8, irdm.FMT_CU8), (ct.PCM, 16, np.int16, irdm.FMT_CI16_FULL),
                                                (ct.PCM, 32, np.int32, irdm.FMT_CI32), (ct.FLOAT, 32, None, irdm.FMT_CF32)])
@pytest.mark.parametrize("fmt_size", [16, 18, 40])
def test_wav_sample_formats(tmp_path, tag, bits, dtype, fmt, fmt_size):
    """8 / 16 / 32-bit PCM and 32-bit float, with the plain, the 18-byte and the extensible fmt chunk (the tag then sits in
    the sub-format GUID)"""
    n = 1000
    data = samples(n, dtype) if dtype else np.arange(2 * n, dtype=np.float32).tobytes()
    p = put(tmp_path, "a.wav", ct.wav(data, tag=tag, bits=bits, rate=2_400_000, fmt_size=fmt_size))
    i = expect(p, irdm.CONTAINER_WAV, fmt, 2_400_000, 12 + 8 + fmt_size + 8, len(data))
    assert not i.has_center and not i.has_start
    assert p.read_bytes()[i.data_offset:i.data_offset + i.data_bytes] == data


def test_wav_extensions_and_forced_kind(tmp_path):
    """.wav / .wave / .rf64 without regard to case; any other name is a raw file (return 1) unless the kind is forced; the
    contents are never sniffed"""
    w = ct.wav(samples(64, np.int16))
    for name in ("a.WAV", "b.wave", "c.Rf64"):
        expect(put(tmp_path, name, w), irdm.CONTAINER_WAV, irdm.FMT_CI16_FULL, 2_000_000, 44, 256)
    raw = put(tmp_path, "d.cs16", w)
    assert probe(raw)[0] == 1
    expect(raw, irdm.CONTAINER_WAV, irdm.FMT_CI16_FULL, 2_000_000, 44, 256, container=irdm.CONTAINER_WAV)
    refused(put(tmp_path, "e.wav", samples(64, np.int16)), "not a RIFF")


def test_wav_open_ended_and_rf64(tmp_path):
    """a data size of 0 or 0xFFFFFFFF, or one past the end of the file, means to the end of the file (rounded down to whole
    samples); RF64 / BW64 take the size from ds64"""
    data = samples(500, np.int16) + b"\x01\x02"              # 2002 bytes: 500 samples and a ragged end
    for size in (0, 0xFFFFFFFF, 1 << 20):
        p = put(tmp_path, "open%d.wav" % (size & 0xff), ct.wav(data, data_size=size))
        expect(p, irdm.CONTAINER_WAV, irdm.FMT_CI16_FULL, 2_000_000, 44, 2000)
    whole = samples(500, np.int16)
    tail = [ct.chunk(b"LIST", b"\x7f" * 4000)]
    for riff in (b"RF64", b"BW64"):
        p = put(tmp_path, "big.rf64", ct.wav(whole, data_size=0xFFFFFFFF, riff=riff, ds64_data=len(whole), after=tail))
        expect(p, irdm.CONTAINER_WAV, irdm.FMT_CI16_FULL, 2_000_000, 12 + 36 + 24 + 8, 2000)
    # RF64 whose ds64 was never filled in (a recorder that was killed): to the end of the file
    p = put(tmp_path, "killed.rf64", ct.wav(whole, data_size=0xFFFFFFFF, riff=b"RF64", ds64_data=0))
    expect(p, irdm.CONTAINER_WAV, irdm.FMT_CI16_FULL, 2_000_000, 12 + 36 + 24 + 8, 2000)


def test_wav_chunks_around_data(tmp_path):
    """an odd-sized chunk in front of data is followed by one pad byte; chunks behind data are not samples"""
    data = samples(300, np.int16)
    odd = ct.chunk(b"junk", b"x" * 13)
    assert len(odd) == 8 + 14
    p = put(tmp_path, "a.wav", ct.wav(data, before=[odd], after=[ct.chunk(b"LIST", b"\xff\x7f" * 5000)]))
    i = expect(p, irdm.CONTAINER_WAV, irdm.FMT_CI16_FULL, 2_000_000, 44 + 22, len(data))
    assert p.read_bytes()[i.data_offset:i.data_offset + i.data_bytes] == data


def test_wav_refusals(tmp_path):
    """mono, packed 24-bit, an unknown depth and truncated headers: -1 and a message that says what and where"""
    refused(put(tmp_path, "mono.wav", ct.wav(samples(10, np.int16), channels=1)), "1 channel", "2 (I, Q)")
    refused(put(tmp_path, "p24.wav", ct.wav(b"\0" * 600, bits=24)), "24 bits per sample")
    refused(put(tmp_path, "f64.wav", ct.wav(b"\0" * 640, tag=ct.FLOAT, bits=64)), "64 bits per sample")
    refused(put(tmp_path, "pcm12.wav", ct.wav(b"\0" * 640, bits=12)), "12 bits per sample")
    whole = ct.wav(samples(10, np.int16))
    refused(put(tmp_path, "t8.wav", whole[:8]), "truncated header", "8 bytes")
    refused(put(tmp_path, "t30.wav", whole[:30]), "truncated", "'fmt '", "offset 12")
    refused(put(tmp_path, "t36.wav", whole[:36]), "truncated", "no data chunk")
    refused(tmp_path / "missing.wav", "cannot open")


def test_wav_auxi_and_file_name(tmp_path):
    """the binary auxi chunk gives start time and centre; one whose year is implausible (SDR#'s XML auxi) is ignored, and the
    centre then comes from _<digits>Hz / _<digits>kHz in the name; with neither there is no centre"""
    data = samples(100, np.int16)
    aux = ct.auxi_chunk(START, STOP, 1_626_000_000, extra=b"\0" * 128)
    i = expect(put(tmp_path, "SDRSharp_20231114_221320Z_1622000000Hz_IQ.wav", ct.wav(data, before=[aux])), irdm.CONTAINER_WAV,
               irdm.FMT_CI16_FULL, 2_000_000, 44 + len(aux), len(data))
    assert i.has_start and i.start_time_ns == START_NS
    assert i.has_center and i.center_frequency == 1_626_000_000.0
    assert START_NS == (calendar.timegm((2023, 11, 14, 22, 13, 20)) * 1000 + 250) * 1_000_000
    # behind the data chunk as well
    i = expect(put(tmp_path, "after.wav", ct.wav(data, after=[ct.auxi_chunk(START, STOP, 1_626_500_000)])), irdm.CONTAINER_WAV,
               irdm.FMT_CI16_FULL, 2_000_000, 44, len(data))
    assert i.has_start and i.has_center and i.center_frequency == 1_626_500_000.0
    xml = ct.chunk(b"auxi", b"<?xml version=\"1.0\"?><Definition><CenterFrequency>1626000000</CenterFrequency></Definition>")
    i = expect(put(tmp_path, "SDRSharp_20231114_221320Z_1622000000Hz_IQ.wav", ct.wav(data, before=[xml])), irdm.CONTAINER_WAV,
               irdm.FMT_CI16_FULL, 2_000_000, 44 + len(xml), len(data))
    assert not i.has_start and i.has_center and i.center_frequency == 1_622_000_000.0
    i = expect(put(tmp_path, "SDRuno_20200907_184033Z_1626270kHz.wav", ct.wav(data)), irdm.CONTAINER_WAV, irdm.FMT_CI16_FULL,
               2_000_000, 44, len(data))
    assert i.has_center and i.center_frequency == 1_626_270_000.0 and not i.has_start
    i = expect(put(tmp_path, "plain_20200907.wav", ct.wav(data)), irdm.CONTAINER_WAV, irdm.FMT_CI16_FULL, 2_000_000, 44, len(data))
    assert not i.has_center and not i.has_start


# ---- SigMF ----

def test_sigmf_either_path_and_fields(tmp_path):
    """either file of the pair; header_bytes, trailing_bytes, a rate written 2.4e6, a datetime with more fractional digits than
    nanoseconds"""
    data = b"H" * 24 + samples(400, np.int16) + b"T" * 10 + b"x"
    d = put(tmp_path, "rec.sigmf-data", data)
    m = put(tmp_path, "rec.sigmf-meta", ct.sigmf_meta("ci16_le", None, rate_text="2.4e6", frequency=1.6265e9,
                                                      datetime="2023-11-14T22:13:20.1234567891Z", header_bytes=24, trailing_bytes=11))
    for path in (m, d):
        i = expect(path, irdm.CONTAINER_SIGMF, irdm.FMT_CI16_FULL, 2_400_000, 24, 1600, data=d)
        assert i.has_center and i.center_frequency == 1.6265e9
        assert i.has_start and i.start_time_ns == 1700000000_123_456_789
        assert i.n_captures == 1


@pytest.mark.parametrize("datatype,fmt,per", [("cf32_le", irdm.FMT_CF32, 8), ("ci16_le", irdm.FMT_CI16_FULL, 4), ("ci8", irdm.FMT_CI8, 2),
                                               ("cu8", irdm.FMT_CU8, 2), ("ci32_le", irdm.FMT_CI32, 8)])
def test_sigmf_datatypes(tmp_path, datatype, fmt, per):
    d = put(tmp_path, "a.sigmf-data", b"\0" * (per * 100 + 1))
    put(tmp_path, "a.sigmf-meta", ct.sigmf_meta(datatype, 10_000_000))
    i = expect(d, irdm.CONTAINER_SIGMF, fmt, 10_000_000, 0, per * 100, data=d)
    assert not i.has_center and not i.has_start


def test_sigmf_dataset_datetimes_and_captures(tmp_path):
    """core:dataset names the data file in the metadata's directory; datetimes with no, three and nine fractional digits;
    several capture segments: the first one's values, and the count"""
    d = put(tmp_path, "samples.bin", samples(64, np.int8))
    for text, ns in (("2023-11-14T22:13:20Z", 1700000000_000_000_000), ("2023-11-14T22:13:20.250Z", START_NS),
                     ("2023-11-14T22:13:20.000000001Z", 1700000000_000_000_001), ("2023-11-14T23:13:20.5+01:00", 1700000000_500_000_000)):
        m = put(tmp_path, "meta.sigmf-meta", ct.sigmf_meta("ci8", 2_000_000, dataset="samples.bin", datetime=text, frequency=1626000000))
        i = expect(m, irdm.CONTAINER_SIGMF, irdm.FMT_CI8, 2_000_000, 0, 128, data=d)
        assert i.has_start and i.start_time_ns == ns, (text, i.start_time_ns)
    caps = [{"core:sample_start": 0, "core:frequency": 1.625e9}, {"core:sample_start": 32, "core:frequency": 1.626e9}]
    m = put(tmp_path, "meta.sigmf-meta", ct.sigmf_meta("ci8", 2_000_000, dataset="samples.bin", captures=caps))
    i = expect(m, irdm.CONTAINER_SIGMF, irdm.FMT_CI8, 2_000_000, 0, 128, data=d)
    assert i.n_captures == 2 and i.center_frequency == 1.625e9 and not i.has_start


def test_sigmf_refusals(tmp_path):
    """cf64_le and ci16_be by name; a fractional rate; two channels; a first capture that does not start at 0; broken JSON;
    a missing data file; .sigmf archives"""
    put(tmp_path, "a.sigmf-data", b"\0" * 64)
    for dt in ("cf64_le", "ci16_be"):
        m = put(tmp_path, "a.sigmf-meta", ct.sigmf_meta(dt, 2_000_000))
        refused(m, "core:datatype", '"%s"' % dt)
    refused(put(tmp_path, "a.sigmf-meta", ct.sigmf_meta("ci8", None, rate_text="2400000.5")), "core:sample_rate", "2400000.5")
    refused(put(tmp_path, "a.sigmf-meta", ct.sigmf_meta("ci8", 2_000_000, num_channels=2)), "core:num_channels")
    refused(put(tmp_path, "a.sigmf-meta", ct.sigmf_meta("ci8", 2_000_000, captures=[{"core:sample_start": 5}])), "core:sample_start")
    refused(put(tmp_path, "a.sigmf-meta", ct.sigmf_meta("ci8", 2_000_000, header_bytes=65)), "core:header_bytes")
    refused(put(tmp_path, "a.sigmf-meta", ct.sigmf_meta("ci8", 2_000_000)[:-30]), "malformed JSON", "at byte")
    refused(put(tmp_path, "lonely.sigmf-meta", ct.sigmf_meta("ci8", 2_000_000)), "cannot open the data file")
    refused(put(tmp_path, "orphan.sigmf-data", b"\0" * 64), "cannot open the metadata file")
    refused(put(tmp_path, "archive.sigmf", b"\0" * 1024), "archives")


# ---- SDRangel .sdriq ----

def test_sdriq(tmp_path):
    """sample sizes 16 and 24, start times in seconds and in milliseconds, a bad CRC, a short header"""
    body16, body24 = samples(200, np.int16) + b"z", (np.arange(-400, 400, dtype=np.int32) * 20000).tobytes() + b"zzz"
    i = expect(put(tmp_path, "a.sdriq", ct.sdriq_header(2_000_000, 1_626_000_000, 1_700_000_000, 16) + body16), irdm.CONTAINER_SDRIQ,
               irdm.FMT_CI16_FULL, 2_000_000, 32, 800)
    assert i.has_center and i.center_frequency == 1_626_000_000.0 and i.has_start and i.start_time_ns == 1_700_000_000 * 10 ** 9
    i = expect(put(tmp_path, "b.SDRIQ", ct.sdriq_header(6_000_000, 10_000_000_000, 1_700_000_000_250, 24) + body24), irdm.CONTAINER_SDRIQ,
               irdm.FMT_CI32_24, 6_000_000, 32, 3200)
    assert i.center_frequency == 1e10 and i.start_time_ns == START_NS
    # the threshold between the two units: 10^11
    # (seconds just below it do not fit 64 bits of nanoseconds: the largest second count tried here is in the year 2540)
    for t, ns in ((18_000_000_000, 18_000_000_000 * 10 ** 9), (100_000_000_000, 100_000_000_000 * 10 ** 6)):
        i = expect(put(tmp_path, "c.sdriq", ct.sdriq_header(2_000_000, 1, t, 16)), irdm.CONTAINER_SDRIQ, irdm.FMT_CI16_FULL, 2_000_000, 32, 0)
        assert i.start_time_ns == ns
    good = ct.sdriq_header(2_000_000, 1_626_000_000, 1_700_000_000, 24)
    bad = good[:4] + bytes([good[4] ^ 1]) + good[5:]
    refused(put(tmp_path, "crc.sdriq", bad + body24), "CRC-32")
    refused(put(tmp_path, "size.sdriq", ct.sdriq_header(2_000_000, 1, 1, 32)), "sample size 32")
    refused(put(tmp_path, "short.sdriq", good[:20]), "truncated header", "20 bytes")


# ---- the command line, before any device call ----

def cli(*args):
    return subprocess.run([EXE] + [str(a) for a in args], capture_output=True, text=True, timeout=60)


def test_cli_probe_lines(tmp_path):
    """--probe: one line per input on stdout, exit 0, nothing on stderr; a malformed header is reported instead (exit 2 as the
    only input, 1 among others)"""
    data = samples(1000, np.int16)
    w = put(tmp_path, "rec_1626000000Hz.wav", ct.wav(data, before=[ct.auxi_chunk(START, STOP, 1_626_000_000)]))
    q = put(tmp_path, "rec.sdriq", ct.sdriq_header(2_000_000, 1_626_100_000, 1_700_000_100, 24) + samples(500, np.int32))
    raw = put(tmp_path, "rec.cf32", b"\0" * 8004)
    r = cli("-f", w, "-f", q, "-f", raw, "--probe")
    assert r.returncode == 0 and r.stderr == "", r.stderr
    assert r.stdout.splitlines() == [
        "probe: %s container=wav format=ci16-full rate=2000000 centre=1626000000 start=1700000000.250000000 offset=88 bytes=4000 data=%s" % (w, w),
        "probe: %s container=sdriq format=ci32-24 rate=2000000 centre=1626100000 start=1700000100.000000000 offset=32 bytes=4000 data=%s" % (q, q),
        "probe: %s container=raw format=cf32 rate=- centre=- start=- offset=0 bytes=8000 data=%s" % (raw, raw)]
    r = cli("-f", raw, "-r", 2000000, "--probe", "--container", "raw")
    assert r.returncode == 0 and " rate=2000000 " in r.stdout
    r = cli("-f", w, "--container", "raw", "--probe")
    assert r.returncode == 0 and "container=raw format=ci8" in r.stdout
    bad = put(tmp_path, "bad.wav", ct.wav(data, channels=1))
    r = cli("-f", bad, "--probe")
    assert r.returncode == 2 and r.stdout == "" and "1 channel" in r.stderr
    r = cli("-f", bad)
    assert r.returncode == 2 and r.stdout == "" and "1 channel" in r.stderr
    r = cli("-f", w, "-f", bad, "--probe")
    assert r.returncode == 1 and len(r.stdout.splitlines()) == 1 and "1 channel" in r.stderr


def test_cli_refusals_before_any_device_call(tmp_path):
    """--format beside a container, mixed rates and mixed formats in a batch, differing centres behind a front end, stdin with
    --container: exit 2, nothing on stdout"""
    data = samples(1000, np.int16)
    a = put(tmp_path, "a.wav", ct.wav(data, rate=2_000_000))
    b = put(tmp_path, "b.wav", ct.wav(data, rate=4_000_000))
    f32 = put(tmp_path, "c.wav", ct.wav(b"\0" * 800, tag=ct.FLOAT, bits=32))
    q1 = put(tmp_path, "q1.sdriq", ct.sdriq_header(10_000_000, 1_626_000_000, 1_700_000_000, 16) + data)
    q2 = put(tmp_path, "q2.sdriq", ct.sdriq_header(10_000_000, 1_626_500_000, 1_700_000_000, 16) + data)
    r = cli("-f", a, "--format", "ci16-full")
    assert r.returncode == 2 and r.stdout == "" and "--format" in r.stderr and "container" in r.stderr
    r = cli("-f", a, "-f", b)
    assert r.returncode == 2 and r.stdout == "" and "one sample rate" in r.stderr and "4000000" in r.stderr
    r = cli("-f", a, "-f", f32)
    assert r.returncode == 2 and r.stdout == "" and "different sample formats" in r.stderr
    r = cli("-f", q1, "-f", q2, "--band-center", 1626000000, "--decimate", 5)
    assert r.returncode == 2 and r.stdout == "" and "one centre frequency" in r.stderr
    r = cli("-f", "-", "--container", "wav")
    assert r.returncode == 2 and r.stdout == "" and "standard input" in r.stderr
    r = cli("-f", a, "--container", "flac")
    assert r.returncode == 2 and "wav, sigmf, sdriq or raw" in r.stderr
    # a raw file still needs -r
    r = cli("-f", put(tmp_path, "x.cf32", b"\0" * 80))
    assert r.returncode == 2 and r.stderr.startswith("usage:")


def test_python_mirror_matches_the_header():
    """irdm.RecordingInfo is irdm_recording_info_t (x86-64 SysV): 56 bytes of fields and the 4096-byte path"""
    import ctypes as C
    assert C.sizeof(irdm.RecordingInfo) == 56 + 4096
    assert irdm.RecordingInfo.start_time_ns.offset == 32 and irdm.RecordingInfo.data_path.offset == 56
    assert (irdm.FMT_CI32, irdm.FMT_CI32_24) == (8, 9)
    v = np.array([-2 ** 31, 2 ** 31 - 1, 2 ** 24 + 1, 2 ** 24 + 3, -(2 ** 24 + 1), 1], dtype=np.int32)
    x = irdm.convert_ci32(v).view(np.float32)
    # INT32_MAX rounds up to 2^31: exactly 1.0; ties go to even
    assert x.tolist() == [-1.0, 1.0, 2.0 ** -7, (2.0 ** 24 + 4) / 2.0 ** 31, -(2.0 ** -7), 2.0 ** -31]
    assert irdm.convert_ci32(v, irdm.FMT_CI32_24).view(np.float32)[5] == 2.0 ** -23


# ---- the review's corner cases, and the probe from an emulated library ----

def test_dates_that_do_not_exist_are_refused(tmp_path):
    """day 31 of a 30-day month, 29 February of a common year: a SigMF datetime is refused, an auxi chunk ignored; 29 February
    2024 is a date"""
    put(tmp_path, "a.sigmf-data", b"\0" * 64)
    for text in ("2023-02-31T00:00:00Z", "2023-02-29T12:00:00Z", "2023-04-31T00:00:00Z", "2023-13-01T00:00:00Z"):
        refused(put(tmp_path, "a.sigmf-meta", ct.sigmf_meta("ci8", 2_000_000, datetime=text)), "core:datetime", text)
    i = expect(put(tmp_path, "a.sigmf-meta", ct.sigmf_meta("ci8", 2_000_000, datetime="2024-02-29T00:00:01Z")), irdm.CONTAINER_SIGMF,
               irdm.FMT_CI8, 2_000_000, 0, 64, data=tmp_path / "a.sigmf-data")
    assert i.start_time_ns == calendar.timegm((2024, 2, 29, 0, 0, 1)) * 10 ** 9
    data = samples(100, np.int16)
    aux = ct.auxi_chunk((2023, 2, 31, 1, 2, 3, 4), STOP, 1_626_000_000)
    i = expect(put(tmp_path, "feb.wav", ct.wav(data, before=[aux])), irdm.CONTAINER_WAV, irdm.FMT_CI16_FULL, 2_000_000, 44 + len(aux), len(data))
    assert not i.has_start and not i.has_center


def test_the_first_data_chunk_holds_the_samples(tmp_path):
    data = samples(100, np.int16)
    p = put(tmp_path, "two.wav", ct.wav(data, after=[ct.chunk(b"data", b"\x55" * 4000), ct.auxi_chunk(START, STOP, 1_626_000_000)]))
    i = expect(p, irdm.CONTAINER_WAV, irdm.FMT_CI16_FULL, 2_000_000, 44, len(data))
    assert i.has_center                      # (the scan goes on behind the second one)


def test_a_data_path_that_does_not_fit_is_refused(tmp_path):
    """the metadata's directory plus core:dataset past the struct's 4095 bytes: -1 and a message about the path, not a cut
    path (no file can be made at such an absolute path here; under a relative one it could exist)"""
    d = tmp_path
    while len(str(d)) < 3900:
        d = d / ("d" * 200)
    d.mkdir(parents=True)
    name = "s" * 250 + ".bin"
    m = put(d, "m.sigmf-meta", ct.sigmf_meta("ci8", 2_000_000, dataset=name))
    assert len(str(m)) < 4096 <= len(str(d / name))
    refused(m, "path", "4095")
    (d / "t.bin").write_bytes(b"\0" * 64)
    expect(put(d, "m.sigmf-meta", ct.sigmf_meta("ci8", 2_000_000, dataset="t.bin")), irdm.CONTAINER_SIGMF, irdm.FMT_CI8, 2_000_000, 0, 64,
           data=d / "t.bin")


def test_format_beside_a_container_is_refused_under_probe_too(tmp_path):
    a = put(tmp_path, "a.wav", ct.wav(samples(100, np.int16)))
    r = cli("-f", a, "--probe", "--format", "cf32")
    assert r.returncode == 2 and r.stdout == "" and "--format" in r.stderr
    r = cli("-f", a, "--probe", "--format", "cf32", "--container", "raw")
    assert r.returncode == 0 and "container=raw format=cf32" in r.stdout


def test_format_bytes():
    L = irdm.lib()
    assert [L.irdm_format_bytes(f) for f in range(-1, 11)] == [0, 2, 4, 8, 4, 4, 0, 2, 0, 8, 8, 0]


def test_probe_from_an_emulated_library(tmp_path):
    """csrc/recording.cpp linked into the CPU emulation build (tests/recording_emul_build.py): the same answers"""
    import json
    import sys
    import recording_emul_build
    env = dict(os.environ, IRDM_LIB=recording_emul_build.build())
    p = subprocess.run([sys.executable, os.path.join(os.path.dirname(os.path.abspath(__file__)), "probe_emul_run.py"), str(tmp_path)],
                       env=env, capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    res = json.loads([l for l in p.stdout.splitlines() if l.startswith("RESULT ")][-1][7:])
    assert res["wav"] == [0, irdm.CONTAINER_WAV, irdm.FMT_CI16_FULL, 2_400_000, 1_626_000_000.0, START_NS, 88, 800]
    assert res["sigmf"] == [0, irdm.CONTAINER_SIGMF, irdm.FMT_CI32, 2_400_000, 1.6265e9, 800]
    assert res["sdriq"] == [0, irdm.CONTAINER_SDRIQ, irdm.FMT_CI32_24, 2_000_000, 1_700_000_000 * 10 ** 9, 32, 800]
    assert res["mono"][0] == -1 and "1 channel" in res["mono"][1] and res["raw"] == 1
    assert res["format_bytes"] == [0, 2, 4, 8, 4, 4, 0, 2, 0, 8, 8, 0]
