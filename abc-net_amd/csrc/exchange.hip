// The bf16 wire format of the data-parallel gradient exchange (GradReducer mode "direct", wire_dtype "bf16"):
// pack (f32 -> bf16), the rank-ordered f32 sum of the received rows (-> bf16), unpack (bf16 -> f32).  Pure streaming kernels.
//
// Rounding is round-to-nearest-even on the f32 bit pattern, in INTEGER arithmetic: (u + 0x7FFF + ((u >> 16) & 1)) >> 16, any NaN
// to a quiet NaN.  Subnormals are rounded (not flushed) and a finite value above the largest bf16 carries into the exponent and
// becomes Inf whatever float mode the kernel runs under -- nothing here depends on how a conversion instruction treats them.
//
// Layout of every kernel: the destination's first `head` elements (those in front of its first 16-byte boundary) and the last
// n - head - 8 * units elements are written one by one by sixteen threads of workgroup 0; in between, one thread per unit of 8
// elements writes with 16-byte stores to 16-byte-aligned addresses.  The unit's loads are 16-byte loads too, typed as vectors of
// ELEMENT alignment: a source that shares the destination's phase (every bucket of the training step) is read at aligned addresses,
// any other one at the address it has -- global memory takes both, and hipcc emits the same global_load_dwordx4 for either.
#include "common.hpp"
#include "../../include/abcnet_hip.h"
#include "capi_util.hpp"

namespace {

typedef float f32x4_e __attribute__((ext_vector_type(4), aligned(4)));      // element-aligned 16 bytes of f32
typedef unsigned u32x4_e __attribute__((ext_vector_type(4), aligned(2)));   // element-aligned 16 bytes of bf16

__device__ inline unsigned rne_bits(unsigned u) {
    const unsigned r = (u + 0x7FFFu + ((u >> 16) & 1u)) >> 16;
    return (u & 0x7FFFFFFFu) > 0x7F800000u ? ((u >> 16) | 0x40u) : r;      // NaN: keep sign and top payload bits, set the quiet bit
}
__device__ inline unsigned rne_bits(float x) { return rne_bits(__float_as_uint(x)); }
__device__ inline float widen_lo(unsigned w) { return __uint_as_float(w << 16); }
__device__ inline float widen_hi(unsigned w) { return __uint_as_float(w & 0xFFFF0000u); }
__device__ inline float widen(uint16_t h) { return __uint_as_float((unsigned)h << 16); }

__device__ inline f32x4 load_f32x4(const float* p) { const f32x4_e t = *(const f32x4_e*)p; return (f32x4){t[0], t[1], t[2], t[3]}; }
__device__ inline u32x4 load_bf16x8(const uint16_t* p) { const u32x4_e t = *(const u32x4_e*)p; return (u32x4){t[0], t[1], t[2], t[3]}; }

// the one-by-one elements: thread t < 8 owns element t of the head, thread 8 + t element t of the tail; -1: none
__device__ inline int64_t edge_element(int64_t head, int64_t units, int64_t n) {
    const int t = threadIdx.x;
    if (blockIdx.x != 0 || t >= 16) return -1;
    const int64_t e = t < 8 ? t : head + 8 * units + (t - 8);
    return (t < 8 ? e < head : e < n) ? e : -1;
}

__global__ __launch_bounds__(256) void pack_bf16_kernel(const float* __restrict__ src, uint16_t* __restrict__ dst, int64_t n, int64_t head, int64_t units) {
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < units; i += stride) {
        const int64_t e = head + 8 * i;
        const f32x4 a = load_f32x4(src + e), b = load_f32x4(src + e + 4);
        u32x4 o;
        o[0] = rne_bits(a[0]) | (rne_bits(a[1]) << 16); o[1] = rne_bits(a[2]) | (rne_bits(a[3]) << 16);
        o[2] = rne_bits(b[0]) | (rne_bits(b[1]) << 16); o[3] = rne_bits(b[2]) | (rne_bits(b[3]) << 16);
        *(u32x4*)(dst + e) = o;
    }
    const int64_t e = edge_element(head, units, n);
    if (e >= 0) dst[e] = (uint16_t)rne_bits(src[e]);
}

__global__ __launch_bounds__(256) void unpack_bf16_kernel(const uint16_t* __restrict__ src, float* __restrict__ dst, int64_t n, int64_t head, int64_t units) {
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < units; i += stride) {
        const int64_t e = head + 8 * i;
        const u32x4 v = load_bf16x8(src + e);
        *(f32x4*)(dst + e) = (f32x4){widen_lo(v[0]), widen_hi(v[0]), widen_lo(v[1]), widen_hi(v[1])};
        *(f32x4*)(dst + e + 4) = (f32x4){widen_lo(v[2]), widen_hi(v[2]), widen_lo(v[3]), widen_hi(v[3])};
    }
    const int64_t e = edge_element(head, units, n);
    if (e >= 0) dst[e] = widen(src[e]);
}

// dst[i] = bf16(((f32(recv[0][i]) + f32(recv[1][i])) + f32(recv[2][i])) + ...): plain f32 adds in ascending row order
__global__ __launch_bounds__(256) void reduce_bf16_kernel(const uint16_t* __restrict__ recv, uint16_t* __restrict__ dst, int W, int64_t n, int64_t head, int64_t units) {
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < units; i += stride) {
        const int64_t e = head + 8 * i;
        float acc[8];
        {
            const u32x4 v = load_bf16x8(recv + e);
#pragma unroll
            for (int j = 0; j < 4; ++j) { acc[2 * j] = widen_lo(v[j]); acc[2 * j + 1] = widen_hi(v[j]); }
        }
#pragma unroll 4
        for (int q = 1; q < W; ++q) {
            const u32x4 v = load_bf16x8(recv + (int64_t)q * n + e);
#pragma unroll
            for (int j = 0; j < 4; ++j) { acc[2 * j] = acc[2 * j] + widen_lo(v[j]); acc[2 * j + 1] = acc[2 * j + 1] + widen_hi(v[j]); }
        }
        u32x4 o;
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = rne_bits(acc[2 * j]) | (rne_bits(acc[2 * j + 1]) << 16);
        *(u32x4*)(dst + e) = o;
    }
    const int64_t e = edge_element(head, units, n);
    if (e >= 0) {
        float acc = widen(recv[e]);
        for (int q = 1; q < W; ++q) acc = acc + widen(recv[(int64_t)q * n + e]);
        dst[e] = (uint16_t)rne_bits(acc);
    }
}

// elements of `esize` bytes in front of dst's first 16-byte boundary (at most n), and the whole 8-element units after them
inline void split(const void* dst, int esize, int64_t n, int64_t* head, int64_t* units) {
    int64_t h = (int64_t)((16 - ((uintptr_t)dst & 15)) & 15) / esize;
    if (h > n) h = n;
    *head = h;
    *units = (n - h) / 8;
}
// one thread per unit: the grid follows n (the largest gradient bucket, ~2 M elements, is 1024 workgroups); the grid-stride loop
// only serves sizes beyond 2^31 threads
inline dim3 grid_for(int64_t units) {
    int64_t nb = (units + 255) / 256;
    if (nb < 1) nb = 1;
    if (nb > (1 << 23)) nb = 1 << 23;
    return dim3((unsigned)nb);
}

}  // namespace

extern "C" int abc_grad_pack_bf16(const float* src, void* dst, int64_t n, abc_stream_t stream) {
    if (n < 1) return abc_fail(ABC_EINVAL, "grad_pack_bf16: n < 1");
    if (!src || !dst) return abc_fail(ABC_EINVAL, "grad_pack_bf16: null pointer");
    if (((uintptr_t)src & 3) || ((uintptr_t)dst & 1)) return abc_fail(ABC_EINVAL, "grad_pack_bf16: pointers must be element-aligned (f32: 4 bytes, bf16: 2)");
    int64_t head, units;
    split(dst, 2, n, &head, &units);
    hipLaunchKernelGGL(pack_bf16_kernel, grid_for(units), dim3(256), 0, (hipStream_t)stream, src, (uint16_t*)dst, n, head, units);
    return abc_check_launch("grad_pack_bf16");
}

extern "C" int abc_grad_unpack_bf16(const void* src, float* dst, int64_t n, abc_stream_t stream) {
    if (n < 1) return abc_fail(ABC_EINVAL, "grad_unpack_bf16: n < 1");
    if (!src || !dst) return abc_fail(ABC_EINVAL, "grad_unpack_bf16: null pointer");
    if (((uintptr_t)src & 1) || ((uintptr_t)dst & 3)) return abc_fail(ABC_EINVAL, "grad_unpack_bf16: pointers must be element-aligned (bf16: 2 bytes, f32: 4)");
    int64_t head, units;
    split(dst, 4, n, &head, &units);
    hipLaunchKernelGGL(unpack_bf16_kernel, grid_for(units), dim3(256), 0, (hipStream_t)stream, (const uint16_t*)src, dst, n, head, units);
    return abc_check_launch("grad_unpack_bf16");
}

extern "C" int abc_grad_reduce_bf16(const void* recv, void* dst, int32_t W, int64_t n, abc_stream_t stream) {
    if (n < 1) return abc_fail(ABC_EINVAL, "grad_reduce_bf16: n < 1");
    if (W < 1 || W > 64) return abc_fail(ABC_EINVAL, "grad_reduce_bf16: 1 <= W <= 64");
    if (!recv || !dst) return abc_fail(ABC_EINVAL, "grad_reduce_bf16: null pointer");
    if (((uintptr_t)recv & 1) || ((uintptr_t)dst & 1)) return abc_fail(ABC_EINVAL, "grad_reduce_bf16: pointers must be 2-byte aligned");
    int64_t head, units;
    split(dst, 2, n, &head, &units);
    hipLaunchKernelGGL(reduce_bf16_kernel, grid_for(units), dim3(256), 0, (hipStream_t)stream, (const uint16_t*)recv, (uint16_t*)dst, (int)W, n, head, units);
    return abc_check_launch("grad_reduce_bf16");
}
