// What the device text writers (molblock.hip, smiles.hip) share: contiguous ranges of rows per thread, the 64-bit workgroup scan and
// the prefix rule that packs a batch's texts back to back.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace text_pack {

typedef unsigned long long u64;

// rows [lo, hi) of thread tid when n rows are dealt out in contiguous ranges over MT threads
template <int MT>
__device__ inline void my_range(int n, int tid, int& lo, int& hi) {
    const int per = (n + MT - 1) / MT;
    lo = min(tid * per, n);
    hi = min(lo + per, n);
}

// exclusive prefix sum of a 64-bit value over the workgroup (the unclipped running total of a batch may pass 2^32);
// wt = LDS scratch [MT / 64 + 1].  Every thread must call it (it synchronises).
template <int MT>
__device__ inline u64 block_excl_scan64(u64 v, u64* wt, u64* total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    u64 inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const u64 t = __shfl_up(inc, o);
        if (lane >= o) inc += t;
    }
    __syncthreads();
    if (lane == 63) wt[wave] = inc;
    __syncthreads();
    if (threadIdx.x == 0) {
        u64 s = 0;
#pragma unroll
        for (int i = 0; i < MT / 64; ++i) {
            const u64 x = wt[i];
            wt[i] = s;
            s += x;
        }
        wt[MT / 64] = s;
    }
    __syncthreads();
    *total = wt[MT / 64];
    return wt[wave] + inc - v;
}

// The prefix rule for image b of a batch whose lengths are lens[0 .. B) (a negative length counts as 0): the unclipped running
// total in front of the image and through it, and the largest running total through an image 0 .. b that is <= cap_text -- an image
// is written iff through <= cap_text, and offsets[b + 1] = fits either way.  Every thread must call it; all get the same values.
struct Span { u64 before, through, fits; };
template <int MT>
__device__ inline Span prefix_rule(const int* lens, int b, int64_t cap_text) {
    __shared__ u64 wt64[MT / 64 + 1];
    __shared__ u64 edge[2];
    __shared__ u64 fits;
    const int tid = threadIdx.x;
    if (tid == 0) fits = 0;
    int lo, hi;
    my_range<MT>(b + 1, tid, lo, hi);
    u64 mine = 0;
    for (int i = lo; i < hi; ++i) mine += (u64)max(lens[i], 0);
    u64 all;
    u64 run = block_excl_scan64<MT>(mine, wt64, &all);      // (its barriers publish fits = 0)
    u64 best = 0;
    for (int i = lo; i < hi; ++i) {
        if (i == b) edge[0] = run;
        run += (u64)max(lens[i], 0);
        if (run <= (u64)cap_text) best = run;      // (the totals never decrease: the last one that fits is the largest)
    }
    if (lo < hi && hi == b + 1) edge[1] = run;
    if (best) atomicMax(&fits, best);
    __syncthreads();
    Span s;
    s.before = edge[0], s.through = edge[1], s.fits = fits;
    return s;
}

}  // namespace text_pack
