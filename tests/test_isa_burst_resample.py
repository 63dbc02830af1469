"""burst_resample_kernel's code object (csrc/burst_resample.hpp through csrc/state.cpp, compiled to gfx950 assembly; no GPU
needed): no private segment, no spilled registers, and the tap loop -- the stretch from the first fused multiply-add to the
last -- made of fused multiply-adds, LDS reads and waits alone (and the register moves that put an odd tap where a packed
multiply-add's operand selection reaches it): 2 x 20 of the former, the 20 taps in registers before it."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "iridium-sniffer_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not present")
    out = str(tmp_path_factory.mktemp("br_isa") / "state.s")
    subprocess.run([HIPCC, "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "--offload-arch=gfx950", "-x", "hip",
                    "--cuda-device-only", "-S", os.path.join(CSRC, "state.cpp"), "-o", out], check=True, capture_output=True)
    return open(out).read()


def kernel_text(asm, name):
    m = re.search(r"^(_ZN4irdm\d+%s\w*):[^\n]*\n(.*?)\n\.Lfunc_end" % name, asm, flags=re.M | re.S)
    assert m, name
    return m.group(1), m.group(2)


def metadata(asm, symbol, key):
    block = re.search(r"- \.agpr_count:.*?\.name:\s+%s\n.*?\.wavefront_size" % re.escape(symbol), asm, flags=re.S)
    if block is None:
        block = [b for b in asm.split("  - .a") if re.search(r"\.name:\s+%s\b" % re.escape(symbol), b)][0]
    else:
        block = block.group(0)
    return int(re.search(r"\.%s:\s*(\d+)" % key, block).group(1))


def test_no_scratch_no_spills_and_a_loop_of_fmas_and_lds_reads(asm):
    symbol, body = kernel_text(asm, "burst_resample_kernel")
    for key in ("private_segment_fixed_size", "vgpr_spill_count", "sgpr_spill_count"):
        assert metadata(asm, symbol, key) == 0, key
    assert not re.findall(r"^\s+scratch_\w+", body, flags=re.M)
    ins = [l.split()[0] for l in body.splitlines() if re.match(r"^\s+[a-z]", l)]
    fma = [i for i, op in enumerate(ins) if op in ("v_fma_f32", "v_fmac_f32", "v_pk_fma_f32")]
    count = sum(2 if ins[i] == "v_pk_fma_f32" else 1 for i in fma)
    assert count == 40, count
    loop = ins[fma[0]:fma[-1] + 1]
    other = sorted(set(op for op in loop if not (op in ("v_fma_f32", "v_fmac_f32", "v_pk_fma_f32", "v_mov_b32_e32", "s_waitcnt", "s_nop") or
                                                 op.startswith("ds_read") or op.startswith("ds_load"))))
    assert not other, other
    reads = [op for op in ins if op.startswith("ds_read") or op.startswith("ds_load")]
    assert reads and all(op in ("ds_read_b64", "ds_read2_b64", "ds_read_b128", "ds_read2st64_b64") for op in reads), sorted(set(reads))
    # the taps: 16-byte loads from the phase-major table
    assert ins.count("global_load_dwordx4") >= 5
