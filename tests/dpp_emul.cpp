// dpp_emul.cpp -- TEST INFRASTRUCTURE: the wavefront reductions of csrc/scan_fast.hip (wave_or_u32, wave_min_u32,
// wave_max_u64: four row_shr steps, row_bcast:15, row_bcast:31 on the DPP network) executed by the HIP emulation of
// tests/hip_emul/hip/hip_runtime.h, one wavefront of 64 lanes, so that the emulation of the DPP controls can be checked
// against a plain loop without a GPU (tests/test_dpp_emul.py).
//
// The test cuts dpp_reduce_emul.inc out of csrc/scan_fast.hip: the text from "wavefront reductions on the DPP network" up to
// the uni() helpers, unchanged.
#include <hip/hip_runtime.h>

namespace irdm {
#include "dpp_reduce_emul.inc"

// the product's three reductions: every lane stores what the function returned to it (the value read from lane 63)
__global__ void dpp_product_kernel(const unsigned *v32, const unsigned long long *v64, unsigned *out_or, unsigned *out_min,
                                   unsigned long long *out_max)
{
    const int l = threadIdx.x;
    out_or[l] = wave_or_u32(v32[l]);
    out_min[l] = wave_min_u32(v32[l]);
    out_max[l] = wave_max_u64(v64[l]);
}

// the same six steps without the final readlane: what every lane holds after them
__global__ void dpp_lanes_kernel(const unsigned *v32, unsigned *lanes_or, unsigned *lanes_min)
{
    const int l = threadIdx.x;
    unsigned a = v32[l], b = v32[l];
    IRDM_DPP_REDUCE(a, op_or_u32, 0u);
    IRDM_DPP_REDUCE(b, op_min_u32, 0xffffffffu);
    lanes_or[l] = a;
    lanes_min[l] = b;
}

// one DPP move: out[l] = update_dpp(old[l], src[l], ctrl) with row_mask = bank_mask = 0xf, bound_ctrl = false
template <int CTRL>
__global__ void dpp_step_kernel(const int *old, const int *src, int *out)
{
    const int l = threadIdx.x;
    out[l] = __builtin_amdgcn_update_dpp(old[l], src[l], CTRL, 0xf, 0xf, false);
}
}  // namespace irdm

using namespace irdm;

extern "C" {

void dpp_emul_product(const unsigned *v32, const unsigned long long *v64, unsigned *out_or, unsigned *out_min,
                      unsigned long long *out_max)
{
    hipLaunchKernelGGL(dpp_product_kernel, dim3(1), dim3(64), 0, (hipStream_t)0, v32, v64, out_or, out_min, out_max);
}

void dpp_emul_lanes(const unsigned *v32, unsigned *lanes_or, unsigned *lanes_min)
{
    hipLaunchKernelGGL(dpp_lanes_kernel, dim3(1), dim3(64), 0, (hipStream_t)0, v32, lanes_or, lanes_min);
}

int dpp_emul_step(int ctrl, const int *old, const int *src, int *out)
{
    switch (ctrl) {
    case 0x111: hipLaunchKernelGGL(dpp_step_kernel<0x111>, dim3(1), dim3(64), 0, (hipStream_t)0, old, src, out); return 0;
    case 0x118: hipLaunchKernelGGL(dpp_step_kernel<0x118>, dim3(1), dim3(64), 0, (hipStream_t)0, old, src, out); return 0;
    case 0x138: hipLaunchKernelGGL(dpp_step_kernel<0x138>, dim3(1), dim3(64), 0, (hipStream_t)0, old, src, out); return 0;
    case 0x142: hipLaunchKernelGGL(dpp_step_kernel<0x142>, dim3(1), dim3(64), 0, (hipStream_t)0, old, src, out); return 0;
    case 0x143: hipLaunchKernelGGL(dpp_step_kernel<0x143>, dim3(1), dim3(64), 0, (hipStream_t)0, old, src, out); return 0;
    }
    return -1;
}
}
