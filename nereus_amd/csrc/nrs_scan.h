// nrs_scan.h — the integer scans of the add-ons that order their outputs without atomics: the surface extraction (nrs_kernels_surface.h),
// the diffuse particles (nrs_kernels_diffuse.h), the cull of the sinks (nrs_kernels_inflow.h).  The scanned value is a uint32_t or a uint2 (two
// sums side by side).  It includes nothing of the project (nrs_surface.hip has no nrs_math.h).  A step's scans have their own shapes elsewhere.
#pragma once
#include <hip/hip_runtime.h>

namespace nrs {

constexpr int SCAN_BLOCK = 1024; // threads of the one workgroup that scans a list of workgroup totals

__device__ __forceinline__ uint32_t scan_shfl_up(uint32_t v, uint32_t d) { return (uint32_t)__shfl_up((int)v, d, 64); }
__device__ __forceinline__ uint2 scan_shfl_up(uint2 v, uint32_t d) { return make_uint2(scan_shfl_up(v.x, d), scan_shfl_up(v.y, d)); }

// inclusive scan over the 64 lanes of a wave
template <typename T> __device__ __forceinline__ T wave_scan(T v)
{
    const uint32_t lane = threadIdx.x & 63u;
#pragma unroll
    for (uint32_t d = 1; d < 64; d <<= 1) {
        const T o = scan_shfl_up(v, d);
        if (lane >= d) v += o;
    }
    return v;
}
// exclusive scan over the NT threads of a workgroup; every thread calls it.  wsum: NT / 64 words of LDS, free again on return.
// total, unless null: the sum over the workgroup, in every thread
template <int NT, typename T> __device__ __forceinline__ T block_scan(T v, T *wsum, T *total = nullptr)
{
    const T incl = wave_scan(v);
    const uint32_t w = threadIdx.x >> 6;
    if ((threadIdx.x & 63u) == 63u) wsum[w] = incl;
    __syncthreads();
    T before = T(), all = T();
#pragma unroll
    for (uint32_t i = 0; i < NT / 64; ++i) {
        const T s = wsum[i];
        before += i < w ? s : T();
        all += s;
    }
    __syncthreads(); // (wsum may be used again)
    if (total) *total = all;
    return before + incl - v;
}
// exclusive scan of tot[0 .. nb) in place by one workgroup of SCAN_BLOCK threads, SCAN_BLOCK entries per pass with the carry handed on;
// returns the total in every thread
template <typename T> __device__ __forceinline__ T scan_list(T *__restrict__ tot, uint32_t nb, T *wsum)
{
    T carry = T();
    for (uint32_t base = 0; base < nb; base += SCAN_BLOCK) {
        const uint32_t idx = base + threadIdx.x;
        const T v = idx < nb ? tot[idx] : T();
        T all;
        const T ex = block_scan<SCAN_BLOCK>(v, wsum, &all);
        if (idx < nb) tot[idx] = carry + ex;
        carry += all;
    }
    return carry;
}

} // namespace nrs
