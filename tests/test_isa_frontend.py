"""The band-select front end's code object (csrc/frontend.hip compiled to gfx950 assembly, no GPU needed): no store or atomic
issued by the scalar unit, no scalar-cache write-back, no scratch memory (no spills, no private segment), and the tap loop
in packed fused multiply-adds.  In the manner of tests/test_isa_store_hazard.py, which also scans the file for the
wide-store hazard."""
import os
import re
import shutil
import subprocess

import pytest

import test_isa_store_hazard as hazard

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
# mnemonics of the scalar unit that write memory, spelt in pieces: scalar stores (plain, buffer, scratch), scalar atomics
# (plain, buffer) and the scalar data cache's write-back / discard
SCALAR_WRITES = re.compile(r"\bs_(?:buffer_|scratch_)?(?:" + "sto" + "re|ato" + r"mic)_\w+|\bs_dcache_(?:" + "w" + "b|disc" + r"ard)\w*")


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not present")
    return hazard._asm("frontend.hip", str(tmp_path_factory.mktemp("fe_isa")))


def test_the_pattern_sees_what_it_looks_for():
    for word in ("s_" + "store_dword s4, s[0:1], 0x0", "s_buffer_" + "store_dwordx2 s[4:5], s[0:3], 0", "s_scratch_" + "store_dword s1, s2",
                 "s_" + "atomic_add s1, s[2:3], 0x0", "s_buffer_" + "atomic_swap s1, s[4:7], 0", "s_dcache_" + "wb", "s_dcache_" + "discard s[0:1], 0"):
        assert SCALAR_WRITES.search("\t" + word), word
    for word in ("s_load_dwordx8 s[4:11], s[26:27], 0x0", "global_store_dwordx2 v[0:1], v[2:3], off", "ds_write_b64 v1, v[2:3]"):
        assert not SCALAR_WRITES.search("\t" + word), word


def test_no_scalar_writes_no_scratch_packed_fma(asm):
    kernels = re.findall(r"^(_ZN4irdm\w*frontend\w*):", asm, flags=re.M)
    assert len([k for k in kernels if "frontend_kernel" in k]) == 15 and any("tail" in k for k in kernels), kernels
    assert not SCALAR_WRITES.findall(asm)
    assert not re.findall(r"^\s+scratch_\w+", asm, flags=re.M)
    sizes = [int(v) for v in re.findall(r"\.private_segment_fixed_size:\s*(\d+)", asm)]
    spills = [int(v) for v in re.findall(r"\.(?:vgpr|sgpr)_spill_count:\s*(\d+)", asm)]
    assert len(sizes) >= 16 and not any(sizes), sizes
    # (SGPRs may spill into VGPR lanes: v_writelane / v_readlane, no memory; VGPR spills would be scratch)
    assert not any(int(v) for v in re.findall(r"\.vgpr_spill_count:\s*(\d+)", asm)), spills
    assert len(re.findall(r"\bv_pk_fma_f32\b", asm)) >= 15 * 64
    assert not hazard.hazards(asm)
