// Input images on the device: src/utils.py:42-81 (the image half of MolecularImageDataset.__getitem__) and
// src/utils_for_test.py:21-27, from the raw 8-bit renders.
//
// The reference resizes, pads, thresholds and noises every 512 x 512 image on a DataLoader worker (two 512 x 512 uniform
// fields per image) and ships it as f32.  Here the host ships the uint8 render and ten int32 per image (abcnet_amd/augment.py
// draws the reference's scalars) and one launch writes the f32 batch where the network reads it.  One thread = 8 consecutive
// output pixels of a row: the source row bytes with 8-byte loads (the copied axis), two 16-byte stores.  The noise hash's
// key premix is uniform per image; a pixel pays one finaliser per field.
#include "common.hpp"
#include "../../include/abcnet_hip.h"
#include "capi_util.hpp"

namespace {

constexpr int ITHR = 256;
constexpr int VEC = 8;

// the contract of one image's parameter row (host check at call time and device check per image)
__host__ __device__ inline bool img_params_ok(const int32_t* P, int S, int mode, int max_h, int pitch) {
    const int sh = P[ABC_IMG_SRC_H], sw = P[ABC_IMG_SRC_W];
    if (sh < 1 || sw < 1 || sh > max_h || sw > pitch) return false;
    if (mode == ABC_IMG_TEST) return sh == S && sw == S;
    const int rows = P[ABC_IMG_ROWS], cols = P[ABC_IMG_COLS], ddx = P[ABC_IMG_DDX], ddy = P[ABC_IMG_DDY];
    return rows >= 1 && cols >= 1 && rows <= S && cols <= S && ddx >= 0 && ddy >= 0 && ddx <= S - rows && ddy <= S - cols;
}

// OpenCV's INTER_LINEAR source taps of destination index d, n source samples resized to m:
// f = (float)((d + 0.5) * (n / m) - 0.5), s = floor(f), f -= s, clamped at both edges with weight (1, 0)
__device__ inline void lin_taps(int d, int n, double scale, int& s0, int& s1, float& f) {
#pragma clang fp contract(off)
    float fx = (float)(((double)d + 0.5) * scale - 0.5);
    int sx = (int)floorf(fx);
    fx -= (float)sx;
    if (sx < 0) { sx = 0; fx = 0.f; }
    if (sx >= n - 1) { sx = n - 1; fx = 0.f; }
    s0 = sx;
    s1 = min(sx + 1, n - 1);
    f = fx;
}

// horizontal pass of source row `row` for destination columns c0 .. c0 + 7 (only those in [0, cols) are meaningful); scale = sw / cols.
// The products and the sum are plain expressions under contract(off): every one rounded on its own, never an fma (the __f*_rn
// helpers are header functions whose bodies the pragma does not reach -- hipcc fused them)
__device__ inline void hpass(const uint8_t* row, int c0, int cols, int sw, double scale, float* v) {
#pragma clang fp contract(off)
    if (cols == sw) {
        // copied axis: the (at most two) aligned 8-byte words holding columns c0 .. c0 + 7 that lie inside the row
        const int a = c0 >> 3, sh = c0 & 7;
        const uint64_t* r64 = (const uint64_t*)row;
        const uint64_t w0 = (a >= 0 && 8 * a < cols) ? r64[a] : 0ull;
        const uint64_t w1 = (sh && a + 1 >= 0 && 8 * (a + 1) < cols) ? r64[a + 1] : 0ull;
        const uint64_t t = sh ? (w0 >> (8 * sh)) | (w1 << (64 - 8 * sh)) : w0;
#pragma unroll
        for (int j = 0; j < VEC; ++j) v[j] = (float)(uint32_t)((t >> (8 * j)) & 0xFFu);
        return;
    }
#pragma unroll
    for (int j = 0; j < VEC; ++j) {
        const int c = c0 + j;
        v[j] = 255.f;
        if (c < 0 || c >= cols) continue;
        int s0, s1;
        float f;
        lin_taps(c, sw, scale, s0, s1, f);
        const float a = (float)row[s0] * (1.f - f);
        const float b = (float)row[s1] * f;
        v[j] = a + b;
    }
}

// train_cut: the largest byte b with b / 255.f < 0.6f (abc_build_images computes it): the verdict for pixels whose axes are both copied
__global__ __launch_bounds__(ITHR) void build_images_kernel(const abc_image_desc d, int train_cut) {
#pragma clang fp contract(off)
    const int b = blockIdx.y, S = d.S;
    const int npix = S * S;                                   // (S <= 8192: pixel indices fit 32 bits)
    const int p0 = (blockIdx.x * ITHR + threadIdx.x) * VEC;
    if (p0 >= npix) return;
    const int x = p0 / S, y0 = p0 - x * S;
    const int32_t* P = d.params + (size_t)b * ABC_IMG_NPARAM;
    f32x4* o = (f32x4*)(d.out + (size_t)b * npix + p0);
    if (!img_params_ok(P, S, d.mode, d.src_max_h, d.src_pitch)) {
        const f32x4 q = {__builtin_nanf(""), __builtin_nanf(""), __builtin_nanf(""), __builtin_nanf("")};
        o[0] = q;
        o[1] = q;
        return;
    }
    const uint8_t* src = d.src + (size_t)b * d.src_stride;
    bool ink[VEC];
    uint32_t salt_thr = 0u, pepper_thr = 0u;
    if (d.mode == ABC_IMG_TEST) {
        const uint64_t t = *(const uint64_t*)(src + (size_t)x * d.src_pitch + y0);
#pragma unroll
        for (int j = 0; j < VEC; ++j) ink[j] = (int)((t >> (8 * j)) & 0xFFu) <= d.test_max_ink;
    } else {
        const int sh = P[ABC_IMG_SRC_H], sw = P[ABC_IMG_SRC_W], rows = P[ABC_IMG_ROWS], cols = P[ABC_IMG_COLS];
        const int r = x - P[ABC_IMG_DDX], c0 = y0 - P[ABC_IMG_DDY];
        salt_thr = (uint32_t)P[ABC_IMG_SALT_THR];
        pepper_thr = (uint32_t)P[ABC_IMG_PEPPER_THR];
#pragma unroll
        for (int j = 0; j < VEC; ++j) ink[j] = false;    // the white canvas: 255 / 255 < 0.6 is false
        const bool copied = rows == sh && cols == sw;
        if (r >= 0 && r < rows && c0 + VEC > 0 && c0 < cols) {
            float v[VEC];
            const double hscale = cols == sw ? 1.0 : (double)sw / (double)cols;
            if (rows == sh) {
                hpass(src + (size_t)r * d.src_pitch, c0, cols, sw, hscale, v);
            } else {
                int s0, s1;
                float fy;
                lin_taps(r, sh, (double)sh / (double)rows, s0, s1, fy);
                float w[VEC];
                hpass(src + (size_t)s0 * d.src_pitch, c0, cols, sw, hscale, v);
                hpass(src + (size_t)s1 * d.src_pitch, c0, cols, sw, hscale, w);
                const float gy = 1.f - fy;
#pragma unroll
                for (int j = 0; j < VEC; ++j) {
                    const float a = v[j] * gy;
                    const float b = w[j] * fy;
                    v[j] = a + b;
                }
            }
#pragma unroll
            for (int j = 0; j < VEC; ++j) {
                const int c = c0 + j;
                // both axes copied: v is a byte, and train_cut is the same float32 division's verdict on bytes
                ink[j] = c >= 0 && c < cols && (copied ? v[j] <= (float)train_cut : v[j] / 255.f < 0.6f);
            }
        }
    }
    float y[VEC];
    const uint32_t seed = abc_noise_seed((uint32_t)P[ABC_IMG_KEY_LO], (uint32_t)P[ABC_IMG_KEY_HI]);    // (uniform: once per wave)
#pragma unroll
    for (int j = 0; j < VEC; ++j) {
        const uint32_t p = (uint32_t)(p0 + j);
        bool on = ink[j];
        if (salt_thr) on = on || abc_noise_hash(2u * p, seed) < salt_thr;
        if (pepper_thr) on = on && !(abc_noise_hash(2u * p + 1u, seed) < pepper_thr);
        y[j] = on ? 1.f : 0.f;
    }
    o[0] = (f32x4){y[0], y[1], y[2], y[3]};
    o[1] = (f32x4){y[4], y[5], y[6], y[7]};
}

}  // namespace

extern "C" int abc_build_images(const abc_image_desc* d, abc_stream_t stream) {
    if (!d->out || !d->src || !d->params) return abc_fail(ABC_EINVAL, "build_images: null pointer");
    if (d->B < 1 || d->B > 65535) return abc_fail(ABC_EINVAL, "build_images: B must be 1 .. 65535");
    if (d->mode != ABC_IMG_TRAIN && d->mode != ABC_IMG_TEST) return abc_fail(ABC_EINVAL, "build_images: mode");
    if (d->S < VEC || d->S > 8192 || d->S % VEC)
        return abc_fail(ABC_EUNSUPPORTED, "build_images: S must be a multiple of 8 in 8 .. 8192 (8 pixels per thread)");
    if (d->src_pitch < 16 || d->src_pitch > 1024 || d->src_pitch % 16 || d->src_max_h < 1 || d->src_max_h > 1024)
        return abc_fail(ABC_EUNSUPPORTED, "build_images: src_pitch (multiple of 16) and src_max_h must be at most 1024");
    if (d->src_stride % 16 || d->src_stride < (int64_t)d->src_max_h * d->src_pitch)
        return abc_fail(ABC_EINVAL, "build_images: src_stride below src_max_h * src_pitch or not a multiple of 16");
    if (((uintptr_t)d->src | (uintptr_t)d->out) % 16) return abc_fail(ABC_EINVAL, "build_images: src and out must be 16-byte aligned");
    if (d->test_max_ink < -1 || d->test_max_ink > 255) return abc_fail(ABC_EINVAL, "build_images: test_max_ink must be a byte (or -1)");
    if (d->params_host) {
        for (int b = 0; b < d->B; ++b)
            if (!img_params_ok(d->params_host + (size_t)b * ABC_IMG_NPARAM, d->S, d->mode, d->src_max_h, d->src_pitch))
                return abc_fail(ABC_EINVAL, d->mode == ABC_IMG_TEST
                                ? "build_images: test mode needs S x S sources"
                                : "build_images: an image's rows / cols / offsets leave the S x S canvas, or its source its slot");
    }
    const int64_t per_img = (int64_t)d->S * d->S / VEC;
    const dim3 grid((unsigned)((per_img + ITHR - 1) / ITHR), (unsigned)d->B);
    // utils.py:63's float32 (v / 255) < 0.6 on every byte value (IEEE division and compare on the host, as on the device)
    int train_cut = -1;
    for (int v = 0; v < 256; ++v)
        if ((float)v / 255.f < 0.6f) train_cut = v;
    hipLaunchKernelGGL(build_images_kernel, grid, dim3(ITHR), 0, (hipStream_t)stream, *d, train_cut);
    return abc_check_launch("build_images");
}
