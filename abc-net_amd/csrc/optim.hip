// torch.optim.Adam over arbitrary lists of f32 device tensors in ONE launch (abcnet_amd.optim.Adam; reference: train.py:55,141).
//
// The host hands a device table of segments {p, g, m, v, n, first_chunk, cls}: a segment is a run of elements whose four
// arrays are each contiguous (one tensor, or a whole arena of adjacent tensors coalesced on the host).  Workgroup b takes
// chunks b, b + grid, ... of the concatenated segments; chunk k is AM_CHUNK elements of the segment whose first_chunk is the last
// one <= k (binary search over the table; uniform, so scalar loads).  The hyper-parameters arrive by value, one class per distinct
// (param group, step count), bias corrections computed on the host as torch does.  Per element the arithmetic is
// adam_kernel's (misc.hip).
#include "common.hpp"
#include "../../include/abcnet_hip.h"
#include "capi_util.hpp"

namespace {

constexpr int AM_THREADS = 256;
constexpr int AM_CHUNK = AM_THREADS * 4;   // elements per workgroup and pass: one 16-byte vector per thread and array
constexpr int AM_GRID = 2048;              // persistent grid striding over the chunks, as adam_kernel strides over the arena
                                           // (16 vectors in flight per thread: 168 VGPRs, 3 waves / SIMD, 26 % slower)

__device__ inline void adam_elem(float& p, float g, float& m, float& v, const abc_adam_class& c) {
    const float gg = g + c.weight_decay * p;
    m = m + (gg - m) * (1.f - c.beta1);
    v = v * c.beta2 + (1.f - c.beta2) * gg * gg;
    p -= c.step_size * m / (sqrtf(v) / c.bc2_sqrt + c.eps);
}

__global__ __launch_bounds__(AM_THREADS) void adam_multi_kernel(const abc_adam_multi_desc d) {
    const int t = threadIdx.x;
    for (int64_t chunk = blockIdx.x; chunk < d.chunk_total; chunk += gridDim.x) {
        int lo = 0, hi = d.nseg - 1;
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (d.segs[mid].first_chunk <= chunk) lo = mid; else hi = mid - 1;
        }
        const abc_adam_seg s = d.segs[lo];
        if (s.cls < 0 || s.cls >= d.nclass) continue;
        const abc_adam_class c = d.cls[s.cls];
        const int64_t e0 = (chunk - s.first_chunk) * AM_CHUNK;
        if (e0 < 0 || e0 >= s.n) continue;
        const int64_t e1 = (e0 + AM_CHUNK < s.n) ? e0 + AM_CHUNK : s.n;
        if ((((uintptr_t)s.p | (uintptr_t)s.g | (uintptr_t)s.m | (uintptr_t)s.v) & 15) == 0) {
            const int nv = (int)((e1 - e0) >> 2);
            if (t < nv) {
                f32x4 p = ((f32x4*)(s.p + e0))[t], g = ((const f32x4*)(s.g + e0))[t];
                f32x4 m = ((f32x4*)(s.m + e0))[t], v = ((f32x4*)(s.v + e0))[t];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    float pp = p[j], mm = m[j], vv = v[j];
                    adam_elem(pp, g[j], mm, vv, c);
                    p[j] = pp; m[j] = mm; v[j] = vv;
                }
                ((f32x4*)(s.p + e0))[t] = p; ((f32x4*)(s.m + e0))[t] = m; ((f32x4*)(s.v + e0))[t] = v;
            }
            const int64_t i = e0 + (int64_t)nv * 4 + t;   // the segment's last 0-3 elements
            if (i < e1) {
                float pp = s.p[i], mm = s.m[i], vv = s.v[i];
                adam_elem(pp, s.g[i], mm, vv, c);
                s.p[i] = pp; s.m[i] = mm; s.v[i] = vv;
            }
        } else {
            for (int64_t i = e0 + t; i < e1; i += AM_THREADS) {
                float pp = s.p[i], mm = s.m[i], vv = s.v[i];
                adam_elem(pp, s.g[i], mm, vv, c);
                s.p[i] = pp; s.m[i] = mm; s.v[i] = vv;
            }
        }
    }
}

}  // namespace

extern "C" int abc_adam_multi_chunk(void) { return AM_CHUNK; }

extern "C" int abc_adam_multi(const abc_adam_multi_desc* d, abc_stream_t stream) {
    if (d->nseg < 1 || !d->segs) return abc_fail(ABC_EINVAL, "adam_multi: empty segment table");
    if (d->nclass < 1 || d->nclass > ABC_ADAM_MAX_CLASSES) return abc_fail(ABC_EINVAL, "adam_multi: 1..ABC_ADAM_MAX_CLASSES classes");
    if (d->chunk_total < 1 || d->chunk_total > 0x7fffffff) return abc_fail(ABC_EINVAL, "adam_multi: chunk_total out of range");
    const int64_t nb = d->chunk_total < AM_GRID ? d->chunk_total : AM_GRID;
    hipLaunchKernelGGL(adam_multi_kernel, dim3((unsigned)nb), dim3(AM_THREADS), 0, (hipStream_t)stream, *d);
    return abc_check_launch("adam_multi");
}
