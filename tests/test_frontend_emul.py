"""The band-select front end (csrc/frontend.hip, csrc/frontend.cpp) without a GPU: the product's sources on the HIP emulation
(tests/frontend_emul_build.py), driven by tests/frontend_emul_run.py in a process of its own.  The kernel equals the plain
C restatement of the arithmetic contract (tests/frontend_model.c) bit for bit; the model stays inside the derived fp32 bound
of a float64 evaluation; the taps meet the stated response; the feeder composes with the pipeline."""
import ctypes as C
import json
import math
import os
import re
import subprocess
import sys

import pytest

import frontend_emul_build
import frontend_model as fm
import irdm

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


@pytest.fixture(scope="module")
def emul_lib():
    return frontend_emul_build.build()


def run_case(lib, case, timeout=1800):
    env = dict(os.environ, IRDM_LIB=lib)
    p = subprocess.run([sys.executable, os.path.join(HERE, "frontend_emul_run.py"), case], env=env, capture_output=True,
                       text=True, timeout=timeout)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    line = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")][-1]
    return json.loads(line[7:])


def test_kernel_equals_model_all_formats_decimations_shifts(emul_lib):
    """five formats x D in {2,3,4,5,6,8,16} x q zero / positive / negative / near +-32768, whole and in ragged feeds"""
    res = run_case(emul_lib, "matrix")
    assert len(res) == 5 * len(fm.D_LIST) * 6
    assert all(v > 4000 for v in res.values())


def test_same_bytes_whole_in_blocks_and_ragged(emul_lib):
    """one stream per D fed whole, in blocks of 32768 D samples, and in feeds of 1, ntaps - 1 and primes"""
    res = run_case(emul_lib, "blocks")
    assert set(res) == {"D%d" % d for d in fm.D_LIST}
    assert all(v > 65536 for v in res.values())


def test_model_within_fp32_bound_of_float64(emul_lib):
    """|y - y64| <= (ntaps + 8) 2^-24 sum|h| max|r| per component (asserted in the runner, figures returned)"""
    res = run_case(emul_lib, "float64")
    assert len(res) == 5 * len(fm.D_LIST) * 3
    assert all(err <= bound for err, bound in res.values())


def test_taps_meet_the_stated_response(emul_lib):
    """>= 80 dB from 0.58 fs_out on, <= 0.002 dB of ripple up to 0.42 fs_out, ntaps as the design rule gives them"""
    res = run_case(emul_lib, "taps")
    want_taps = {2: 89, 3: 133, 5: 223, 16: 711}
    for d in fm.D_LIST:
        r = res["D%d" % d]
        print("D %d: %d taps, ripple %.5f dB, attenuation %.2f dB" % (d, r["ntaps"], r["ripple_db"], r["atten_db"]))
        assert r["atten_db"] >= 80.0, (d, r)
        assert r["ripple_db"] <= 0.002, (d, r)
        if d in want_taps:
            assert r["ntaps"] == want_taps[d], (d, r)


def test_feeder_composes_with_the_pipeline(emul_lib):
    """irdm_frontend_feed_host + irdm_frontend_flush in front of the emulated pipeline (depth 0 and 1, ragged feeds) against
    the oracle run on the model's output, under tests/parity.py's rules"""
    res = run_case(emul_lib, "compose")
    for name, s in res.items():
        assert s["bursts"] >= 2 and s["demods"] >= 2, (name, s)


def test_config_struct_layout_matches_the_header(tmp_path):
    """irdm_frontend_config_t: sizeof and every offset as gcc lays the header's struct out"""
    names = [n for n, _ in irdm.FrontendConfig._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "irdm_hip.h"\nint main(void) {\n'
                   '    printf("%zu", sizeof(irdm_frontend_config_t));\n' +
                   "".join('    printf(" %%zu", offsetof(irdm_frontend_config_t, %s));\n' % n for n in names) +
                   '    return 0;\n}\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I" + os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    got = [int(v) for v in subprocess.check_output([str(exe)], text=True).split()]
    assert got == [C.sizeof(irdm.FrontendConfig)] + [getattr(irdm.FrontendConfig, n).offset for n in names]
    # and the header declares exactly these fields
    hdr = open(os.path.join(ROOT, "include", "irdm_hip.h")).read()
    body = re.search(r"typedef struct \{([^}]*)\} irdm_frontend_config_t;", hdr).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert re.findall(r"(\w+);", body) == names


def test_wideband_scene_model_then_oracle():
    """Scene selection for the GPU signal test (tests/test_gpu_frontend.py), on the CPU: a 50 MHz ci8 capture, the band 11 MHz
    above its centre, D = 5; six in-band bursts and three strong ones 0.65-0.82 fs_out from the band centre.  Model ->
    oracle at 10 MHz gives all six payloads and nothing from out of band."""
    import hashlib
    import orc
    x, expect, q = fm.wideband_scene()
    s = fm.SCENE
    # the default capture is the bytes it was before wideband_scene() took a scene
    assert (q, len(x)) == (14418, 74973184)
    assert hashlib.sha256(x.tobytes()).hexdigest() == "b5d430bcef80c6759616fe96bbab86f4b35b9811024a426b4098ced89802d623"
    assert hashlib.sha256(json.dumps(expect).encode()).hexdigest() == "ee12d86885208dc5d47f31e4011c902c54c7c688237a823dad41599251b5c936"
    taps = fm.design_taps(s["fs_in"], s["D"])
    y = fm.run(x, irdm.FMT_CI8, s["D"], q, taps)
    ref = orc.run_stream(y, s["fs_in"] // s["D"], center_frequency=1622000000.0 + q * s["fs_in"] / 65536.0)
    assert len(expect) == s["n_inband"] == 6
    fm.check_scene_demods(ref.demods, expect)


@pytest.mark.parametrize("scene,out_rate", [(fm.SCENE_61M44_D6, 10_240_000), (fm.SCENE_50M_D4, 12_500_000)],
                         ids=["61.44M_by_6", "50M_by_4"])
def test_wideband_scenes_at_other_output_rates_model_then_oracle(scene, out_rate):
    """Scene selection for tests/test_gpu_rates.py, on the CPU: 61.44 MS/s ci16 by 6 -> 10.24 MHz and 50 MS/s ci8 by 4 ->
    12.5 MHz.  Model -> oracle gives at least 5 frames at both; at 12.5 MHz (a multiple of 250 kHz) every in-band payload
    whole and nothing from out of band.  (At 10.24 MHz the oracle decodes every payload of this scene too, but the margin
    of a decimation by 40.96 rounded to 41 is not measured, so the GPU test asserts no payloads there.)"""
    import orc
    s = scene
    assert s["fs_in"] // s["D"] == out_rate and s["fs_in"] % s["D"] == 0
    assert max(abs(c) for c in s["inband_channels"]) * (1e6 / 24.0) + 1234.0 <= 0.42 * out_rate
    assert min(abs(f) for f in s["outband_hz"]) >= 0.65 * out_rate
    assert s["start0"] * out_rate > 530 * (1 << int(round(math.log2(out_rate / 1000.0))))       # behind the priming frames
    x, expect, q = fm.wideband_scene(s)
    taps = fm.design_taps(s["fs_in"], s["D"])
    y = fm.run(x, s["fmt"], s["D"], q, taps)
    ref = orc.run_stream(y, out_rate, center_frequency=1622000000.0 + q * s["fs_in"] / 65536.0)
    assert len(expect) == s["n_inband"]
    assert sum(1 for f in ref.frames if f.drop_reason == 0) >= 5 and len(ref.demods) >= 5
    if out_rate % 250_000 == 0:
        fm.check_scene_demods(ref.demods, expect)
