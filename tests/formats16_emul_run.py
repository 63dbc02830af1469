"""TEST INFRASTRUCTURE: the full-precision int16 formats (IRDM_FMT_CI16_FULL, IRDM_FMT_SC16Q11) end to end on the CPU
emulation (tests/_build/libirdm_emul.so, tests/emul_build.py).  Every run equals the emulated cf32 context on the converted
samples record for record and bit for bit, and the oracle on the converted stream under the parity rules
(tests/parity.py).  Started by tests/test_formats16_emul.py in a process of its own with IRDM_LIB pointing at the emulated
build.  Usage: python formats16_emul_run.py <case>"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "iridium-sniffer_amd"))

import formats16 as f16     # noqa: E402
import irdm                 # noqa: E402
import orc                  # noqa: E402
import parity               # noqa: E402


def check(x, fs, fmt, **kw):
    """the int16 context vs the cf32 context on the converted samples (bitwise) and the oracle"""
    y = f16.converted(x, fmt)
    got = f16.run(x, fs, fmt, **kw)
    n = f16.same_records(got, f16.run(y, fs, irdm.FMT_CF32, **kw))
    s = parity.compare(got, orc.run_stream(y, fs))
    s["records"] = n
    return s


def main():
    case = sys.argv[1]
    assert "libirdm_emul" in irdm.LIB_PATH, irdm.LIB_PATH
    res = {}
    if case == "2mhz":
        # 2048-point frames (the generic K1), the any-M decimator (M = 20): its general path reads through burst_sample
        fs = 2_000_000
        x = f16.int16_scene(fs, 1.2, 6, seed=16)
        n = len(x) // 2
        for fmt in f16.FORMATS:
            name = f16.NAMES[fmt]
            res[name + "_whole"] = check(x, fs, fmt)
            res[name + "_chunked_depth1"] = check(x, fs, fmt, chunks=f16.chunks_of(n, 4), depth=1)
            res[name + "_sequential_scan"] = check(x, fs, fmt, options={"scan_mode": 1})
    elif case == "12mhz":
        # 16384-point frames (K1 p32<14>), the register-resident decimator at M = 48, two chunks
        fs = 12_000_000
        x = f16.int16_scene(fs, 0.85, 3, seed=12)
        fmt = irdm.FMT_SC16Q11
        res["sc16q11_two_chunks_depth1"] = check(x, fs, fmt, chunks=f16.chunks_of(len(x) // 2, 2), depth=1)
    else:
        raise SystemExit("unknown case")
    print("RESULT " + json.dumps(res))


if __name__ == "__main__":
    main()
