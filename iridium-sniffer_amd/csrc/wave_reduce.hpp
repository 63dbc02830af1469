// wave_reduce.hpp -- a wavefront's reductions into lane 0 by shuffles of 32-bit words (a 64-bit value travels as its two
// halves).  Every lane of the wavefront calls them; the tree is fixed, so a floating-point sum is reproducible.
#pragma once
#include <hip/hip_runtime.h>

namespace irdm {

__device__ __forceinline__ unsigned long long wave_down64(unsigned long long v, int d)
{
    const unsigned lo = __shfl_down((unsigned)v, d), hi = __shfl_down((unsigned)(v >> 32), d);
    return ((unsigned long long)hi << 32) | lo;
}
__device__ __forceinline__ unsigned wave_sum(unsigned v)
{
    for (int d = 32; d > 0; d >>= 1) v += __shfl_down(v, d);
    return v;
}
__device__ __forceinline__ unsigned long long wave_sum(unsigned long long v)
{
    for (int d = 32; d > 0; d >>= 1) v += wave_down64(v, d);
    return v;
}
__device__ __forceinline__ double wave_sum(double v)
{
    for (int d = 32; d > 0; d >>= 1) v += __builtin_bit_cast(double, wave_down64(__builtin_bit_cast(unsigned long long, v), d));
    return v;
}
__device__ __forceinline__ int wave_min(int v)
{
    for (int d = 32; d > 0; d >>= 1) {
        const int o = __shfl_down(v, d);
        v = o < v ? o : v;
    }
    return v;
}
template <typename T>
__device__ __forceinline__ T wave_max(T v)
{
    for (int d = 32; d > 0; d >>= 1) {
        const T o = __shfl_down(v, d);
        v = o > v ? o : v;
    }
    return v;
}

}  // namespace irdm
