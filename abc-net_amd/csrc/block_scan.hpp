// Workgroup-wide exclusive prefix sum (order-preserving compaction in extract.hip and assemble.hip).
#pragma once
#include <hip/hip_runtime.h>

// exclusive prefix sum of v over a workgroup of XT threads (v may pack two 16-bit counters); wt = LDS scratch [XT / 64 + 1].
// Every thread of the workgroup must call it (it synchronises).
template <int XT>
__device__ inline unsigned block_excl_scan(unsigned v, unsigned* wt, unsigned* total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned t = __shfl_up(inc, o);
        if (lane >= o) inc += t;
    }
    __syncthreads();  // wt may still be read from the previous call
    if (lane == 63) wt[wave] = inc;
    __syncthreads();
    if (wave == 0) {
        const unsigned x = lane < XT / 64 ? wt[lane] : 0u;
        unsigned s = x;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const unsigned t = __shfl_up(s, o);
            if (lane >= o) s += t;
        }
        if (lane < XT / 64) wt[lane] = s - x;
        if (lane == XT / 64 - 1) wt[XT / 64] = s;
    }
    __syncthreads();
    *total = wt[XT / 64];
    return wt[wave] + inc - v;
}
