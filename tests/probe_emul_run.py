"""TEST INFRASTRUCTURE: irdm_recording_probe from whichever library IRDM_LIB names (tests/test_container_probe.py starts this
with an emulated build): one WAV, one SigMF pair, one .sdriq file and one malformed header, written to the directory given.
Usage: python probe_emul_run.py <dir>"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "iridium-sniffer_amd"))

import containers as ct     # noqa: E402
import irdm                 # noqa: E402


def main():
    d = sys.argv[1]
    assert "libirdm_emul" in irdm.LIB_PATH, irdm.LIB_PATH
    data = np.arange(400, dtype=np.int16).tobytes()
    out = {}

    def put(name, body):
        p = os.path.join(d, name)
        open(p, "wb").write(body if isinstance(body, bytes) else body.encode())
        return p

    rc, i, msg = irdm.recording_probe(put("a.wav", ct.wav(data, rate=2_400_000, before=[ct.auxi_chunk((2023, 11, 14, 22, 13, 20, 250),
                                                                                                      (2023, 11, 14, 22, 14, 20, 0), 1_626_000_000)])))
    out["wav"] = [rc, i.kind, i.format, i.sample_rate, i.center_frequency, i.start_time_ns, i.data_offset, i.data_bytes]
    put("b.sigmf-data", data)
    rc, i, msg = irdm.recording_probe(put("b.sigmf-meta", ct.sigmf_meta("ci32_le", None, rate_text="2.4e6", frequency=1.6265e9)))
    out["sigmf"] = [rc, i.kind, i.format, i.sample_rate, i.center_frequency, i.data_bytes]
    rc, i, msg = irdm.recording_probe(put("c.sdriq", ct.sdriq_header(2_000_000, 1_626_000_000, 1_700_000_000, 24) + data))
    out["sdriq"] = [rc, i.kind, i.format, i.sample_rate, i.start_time_ns, i.data_offset, i.data_bytes]
    rc, i, msg = irdm.recording_probe(put("d.wav", ct.wav(data, channels=1)))
    out["mono"] = [rc, msg]
    out["raw"] = irdm.recording_probe(put("e.cf32", data))[0]
    out["format_bytes"] = [int(irdm.lib().irdm_format_bytes(f)) for f in range(-1, 11)]
    print("RESULT " + json.dumps(out))


if __name__ == "__main__":
    main()
