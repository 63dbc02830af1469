"""The wide-ratio kernel's code object (csrc/resample_wide.hip compiled to gfx950 assembly with the Makefile's flags, no GPU
needed), in the style of tests/test_isa_resample.py: from the kernels' metadata, no scratch memory and no spilled VGPR;
the multiply-adds packed; and registers and LDS -- static from the metadata, dynamic from
irdm_frontend_wide_geometry -- that fit the workgroups per CU the launch geometry is chosen for."""
import ctypes as C
import os
import re

import pytest

import resample_wide_cases as wc
import resample_wide_emul_build
import test_isa_frontend as k0
import test_isa_store_hazard as hazard

LDS_PER_CU = 160 * 1024
VGPRS_PER_SIMD = 512            # per lane; a workgroup of 256 threads puts one wavefront on each of the CU's four SIMDs


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    if not os.path.exists(k0.HIPCC):
        pytest.skip("hipcc not present")
    return hazard._asm("resample_wide.hip", str(tmp_path_factory.mktemp("rw_isa")))


def metadata(asm):
    """{kernel name: {field: int}} from the code object's metadata"""
    out = {}
    for block in asm.split("  - .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", block).group(1)
        out[name] = {k: int(v) for k, v in re.findall(r"^    \.(\w+):\s+(\d+)\s*$", "    .agpr_count:" + block, flags=re.M)}
    return out


def test_no_scratch_no_spills_packed_fma_and_the_assumed_occupancy(asm):
    md = {n: f for n, f in metadata(asm).items() if "resample_wide_kernel" in n}
    assert len(md) == 2, sorted(md)                          # with and without pad samples
    assert not re.findall(r"^\s+scratch_\w+", asm, flags=re.M)
    for name, f in md.items():
        assert f["private_segment_fixed_size"] == 0 and f["vgpr_spill_count"] == 0 and f["sgpr_spill_count"] == 0, (name, f)
        assert f["max_flat_workgroup_size"] == 256 and f["wavefront_size"] == 64, (name, f)
    # the multiply-adds are packed: both components of an output in one instruction
    for name in md:
        body = asm.split("\n%s:" % name, 1)[1].split("s_endpgm", 1)[0]
        ins = [l.split()[0] for l in body.splitlines() if re.match(r"^\s+[a-z]", l)]
        assert ins.count("v_pk_fma_f32") == 2 * 8, name     # (a block of the tap loop, and the block behind the loop)
    assert not hazard.hazards(asm)
    # occupancy: the geometry of every tested ratio and of the corners of the domain
    L = C.CDLL(resample_wide_emul_build.build())
    rates = [v[:2] for v in wc.PAIRS.values()] + [(32_768_000, 2_500_000), (2_400_000, 2_500_000), (31_250_000, 2_000_000)]
    seen = set()
    for fi, fo in rates:
        nt, b, lds, wg = C.c_int(0), C.c_int(0), C.c_int(0), C.c_int(0)
        assert L.irdm_frontend_wide_geometry(fi, fo, C.byref(nt), C.byref(b), C.byref(lds), C.byref(wg)) == 0, (fi, fo)
        seen.add(wg.value)
        for name, f in md.items():
            assert wg.value * (f["group_segment_fixed_size"] + lds.value) <= LDS_PER_CU, (fi, fo, name, lds.value, wg.value)
            assert wg.value * max(f["vgpr_count"] + f["agpr_count"], 1) <= VGPRS_PER_SIMD, (fi, fo, name, f)
    assert 4 in seen
