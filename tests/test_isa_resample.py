"""The rational front end's code object (csrc/resample.hip compiled to gfx950 assembly, no GPU needed), under the scan
tests/test_isa_frontend.py applies to K0: no store or atomic issued by the scalar unit, no scalar-cache write-back, no
scratch memory (no VGPR spills, no private segment), and the tap loop in packed fused multiply-adds."""
import os
import re

import pytest

import test_isa_frontend as k0
import test_isa_store_hazard as hazard


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    if not os.path.exists(k0.HIPCC):
        pytest.skip("hipcc not present")
    return hazard._asm("resample.hip", str(tmp_path_factory.mktemp("rs_isa")))


def test_no_scalar_writes_no_scratch_packed_fma(asm):
    kernels = re.findall(r"^(_ZN4irdm\w*resample_kernel\w*):", asm, flags=re.M)
    assert len(kernels) == 4, kernels                      # 5 .. 8 outputs per lane
    assert not k0.SCALAR_WRITES.findall(asm)
    assert not re.findall(r"^\s+scratch_\w+", asm, flags=re.M)
    sizes = [int(v) for v in re.findall(r"\.private_segment_fixed_size:\s*(\d+)", asm)]
    assert len(sizes) == 4 and not any(sizes), sizes
    assert not any(int(v) for v in re.findall(r"\.vgpr_spill_count:\s*(\d+)", asm))
    # the tap loop's body between its two scheduling barriers: nothing but packed FMAs (and waits), 4 x 5 and 2 x 6, 7, 8 of them
    bodies = re.findall(r"; sched_barrier[^\n]*\n(.*?); sched_barrier", asm, flags=re.S)
    loops = []
    for b in bodies:
        ins = [l.split()[0] for l in b.splitlines() if re.match(r"^\s+[a-z]", l)]
        if ins and all(i in ("v_pk_fma_f32", "s_waitcnt", "s_nop") for i in ins):
            loops.append(ins.count("v_pk_fma_f32"))
    assert sorted(loops) == [12, 14, 16, 20], loops
    assert not hazard.hazards(asm)
