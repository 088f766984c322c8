// seb_scan.h — the exclusive scan over per-tile sums that the plans of the memtable write side (k_write_scan)
// and of the Get path's compaction (k_gc_scan) share: one workgroup of kScanWidth lanes per array, a carry
// from one stretch of kScanWidth tiles to the next.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "seb_kernels.h"

namespace seb {

// x[0, count) = its exclusive scan in place, *total = its sum.  Called by every lane of a workgroup of
// kScanWidth lanes.
__device__ __forceinline__ void scan_tile_sums(uint64_t *x, uint64_t count, uint64_t *total) {
    constexpr uint32_t SW = kScanWidth;
    __shared__ uint64_t X[SW];
    __shared__ uint64_t carry_s;
    const uint32_t tid = threadIdx.x;
    if (tid == 0) carry_s = 0;
    __syncthreads();
    for (uint64_t base = 0; base < count; base += SW) {
        const uint64_t v = base + tid < count ? x[base + tid] : 0;
        X[tid] = v;
        __syncthreads();
        for (uint32_t d = 1; d < SW; d <<= 1) {
            const uint64_t a = tid >= d ? X[tid - d] : 0;
            __syncthreads();
            X[tid] += a;
            __syncthreads();
        }
        const uint64_t carry = carry_s;
        if (base + tid < count) x[base + tid] = carry + X[tid] - v;
        __syncthreads();
        if (tid == SW - 1) carry_s = carry + X[tid];
        __syncthreads();
    }
    if (tid == 0) *total = carry_s;
}

}  // namespace seb
