// Raw grey scans of any size into the network's input: what the reference leaves to an offline step (binarize.py, an Otsu
// threshold whose results it stores under processed_images/) composed with utils_for_test.py:21-27, plus the crop and the fit
// that a scan needs and a rendered 512 x 512 file does not.  The contract in full: include/abcnet_hip.h (abc_scan_desc) and
// DESIGN.md section 7.  Everything is integer arithmetic except sigma(t), two double multiplies and one divide of exact integers.
//
// Five launches on the caller's stream, in order (no parallel branch, no sync, no allocation):
//   zero       hist[B][256] <- 0
//   histogram  grid (row chunks, B): 16-byte loads along rows, columns >= src_w masked, one u32 histogram per wave in LDS
//              (LDS atomics), merged, one global atomicAdd per non-zero bin
//   threshold  one 256-thread workgroup per image: 64-bit scans of h and v * h, thread t evaluates sigma(t), arg-max with the
//              smallest t at the maximum, polarity, the ink count, and the four box words reset
//   box        grid as the histogram: per-workgroup min / max of the ink rows and columns, then atomicMin / atomicMax
//   fit+write  one thread = 8 consecutive canvas pixels (two 16-byte stores): every workgroup derives the geometry from the
//              box words, counts ink over each pixel's source box from aligned 8-byte row loads; workgroup 0 of an image
//              writes its geometry row
#include "common.hpp"
#include "../../include/abcnet_hip.h"
#include "capi_util.hpp"

namespace {

constexpr int STHR = 256;
constexpr int VEC = 8;
constexpr int SCAN_ROWS = 64;      // source rows per workgroup of the histogram and box passes
// the words of abc_scan_desc.box per image
enum { BOX_Y0 = 0, BOX_Y1, BOX_X0, BOX_X1, BOX_THR, BOX_INV, BOX_STATUS, BOX_INK };

__host__ __device__ inline bool scan_params_ok(const int32_t* P, int max_h, int pitch) {
    const int sh = P[ABC_SCAN_SRC_H], sw = P[ABC_SCAN_SRC_W];
    return sh >= 1 && sw >= 1 && sh <= max_h && sw <= pitch;
}

__global__ __launch_bounds__(STHR) void scan_zero_kernel(uint32_t* hist) {
    hist[(size_t)blockIdx.x * 256 + threadIdx.x] = 0u;
}

// the 16 source bytes at columns 16 v .. 16 v + 15 of row y (inside the pitch: 16 v < src_w <= pitch, a multiple of 16)
__device__ inline u32x4 load_vec(const uint8_t* src, int pitch, int y, int v) {
    return *(const u32x4*)(src + (size_t)y * pitch + 16 * v);
}

__global__ __launch_bounds__(STHR) void scan_hist_kernel(const abc_scan_desc d) {
    __shared__ uint32_t wh[STHR / 64][256];
    const int b = blockIdx.y;
    const int32_t* P = d.params + (size_t)b * ABC_SCAN_NPARAM;
    if (!scan_params_ok(P, d.src_max_h, d.src_pitch)) return;      // (uniform)
    const int sh = P[ABC_SCAN_SRC_H], sw = P[ABC_SCAN_SRC_W];
    const int r0 = blockIdx.x * SCAN_ROWS;
    if (r0 >= sh) return;
    const int nrow = min(SCAN_ROWS, sh - r0);
    const int vpr = (sw + 15) >> 4;
    const int wave = threadIdx.x >> 6;
    for (int i = threadIdx.x; i < (STHR / 64) * 256; i += STHR) (&wh[0][0])[i] = 0u;
    __syncthreads();
    const uint8_t* src = d.src + (size_t)b * d.src_stride;
    uint32_t* h = wh[wave];
    // a thread adds a run of equal bytes once (the paper of a scan is one value for whole rows: 64 lanes on one LDS word otherwise)
    int run_v = 0;
    uint32_t run_n = 0u;
    for (int i = threadIdx.x; i < nrow * vpr; i += STHR) {
        const int y = i / vpr, v = i - y * vpr;
        const u32x4 q = load_vec(src, d.src_pitch, r0 + y, v);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const uint32_t w = q[k];
            const int c = 16 * v + 4 * k;                 // column of the word's first byte
            if (c >= sw) break;
            const int lo = (int)(w & 0xFFu);
            if (c + 4 <= sw && w == (uint32_t)lo * 0x01010101u) {    // a flat word: four at once
                if (lo == run_v) { run_n += 4u; continue; }
                if (run_n) atomicAdd(&h[run_v], run_n);
                run_v = lo;
                run_n = 4u;
                continue;
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (c + j >= sw) break;
                const int bv = (int)((w >> (8 * j)) & 0xFFu);
                if (bv == run_v) { run_n += 1u; continue; }
                if (run_n) atomicAdd(&h[run_v], run_n);
                run_v = bv;
                run_n = 1u;
            }
        }
    }
    if (run_n) atomicAdd(&h[run_v], run_n);
    __syncthreads();
    uint32_t s = 0u;
#pragma unroll
    for (int k = 0; k < STHR / 64; ++k) s += wh[k][threadIdx.x];
    if (s) atomicAdd(&d.hist[(size_t)b * 256 + threadIdx.x], s);
}

__global__ __launch_bounds__(256) void scan_threshold_kernel(const abc_scan_desc d) {
#pragma clang fp contract(off)
    __shared__ uint64_t sw0[2][256], ss0[2][256];
    __shared__ double bs[256];
    __shared__ int bt[256];
    const int b = blockIdx.x, t = threadIdx.x;
    int32_t* box = d.box + (size_t)b * ABC_SCAN_NBOX;
    const int32_t* P = d.params + (size_t)b * ABC_SCAN_NPARAM;
    if (!scan_params_ok(P, d.src_max_h, d.src_pitch)) {      // (uniform)
        if (t == 0) {
            box[BOX_Y0] = 0x7FFFFFFF; box[BOX_Y1] = -1; box[BOX_X0] = 0x7FFFFFFF; box[BOX_X1] = -1;
            box[BOX_THR] = -1; box[BOX_INV] = 0; box[BOX_STATUS] = ABC_SCAN_BAD_PARAMS; box[BOX_INK] = 0;
        }
        return;
    }
    const int64_t N = (int64_t)P[ABC_SCAN_SRC_H] * P[ABC_SCAN_SRC_W];
    const uint64_t hv = d.hist[(size_t)b * 256 + t];
    // inclusive scans of h and v * h, 64 bits, ping-pong in LDS (integer adds: exact in any order)
    int cur = 0;
    sw0[0][t] = hv;
    ss0[0][t] = hv * (uint64_t)t;
    __syncthreads();
    for (int o = 1; o < 256; o <<= 1) {
        uint64_t a = sw0[cur][t], c = ss0[cur][t];
        if (t >= o) { a += sw0[cur][t - o]; c += ss0[cur][t - o]; }
        sw0[cur ^ 1][t] = a;
        ss0[cur ^ 1][t] = c;
        cur ^= 1;
        __syncthreads();
    }
    const int64_t w0 = (int64_t)sw0[cur][t], s0 = (int64_t)ss0[cur][t], S = (int64_t)ss0[cur][255];
    const int64_t w1 = N - w0;
    double sigma = -1.0;      // (not admissible: below every admissible value, which is >= 0)
    if (w0 > 0 && w1 > 0) {
        const int64_t dd = S * w0 - N * s0;      // |dd| < 2^56
        const double x = (double)dd;
        const double num = x * x;
        const double den = (double)w0 * (double)w1;
        sigma = num / den;
    }
    bs[t] = sigma;
    bt[t] = t;
    __syncthreads();
    for (int o = 128; o >= 1; o >>= 1) {
        if (t < o) {
            const double u = bs[t + o];
            const int ut = bt[t + o];
            if (u > bs[t] || (u == bs[t] && ut < bt[t])) { bs[t] = u; bt[t] = ut; }
        }
        __syncthreads();
    }
    if (t == 0) {
        box[BOX_Y0] = 0x7FFFFFFF; box[BOX_Y1] = -1; box[BOX_X0] = 0x7FFFFFFF; box[BOX_X1] = -1;
        if (bs[0] < 0.0) {
            box[BOX_THR] = -1; box[BOX_INV] = 0; box[BOX_STATUS] = ABC_SCAN_CONSTANT; box[BOX_INK] = 0;
        } else {
            const int thr = bt[0];
            const int64_t dark = (int64_t)sw0[cur][thr];
            const int inv = d.polarity == ABC_SCAN_LIGHT || (d.polarity == ABC_SCAN_AUTO && 2 * dark > N);
            box[BOX_THR] = thr; box[BOX_INV] = inv; box[BOX_STATUS] = 0; box[BOX_INK] = (int32_t)(inv ? N - dark : dark);
        }
    }
}

// bit j of the result: byte j of w is ink
__device__ inline uint32_t ink_bits(uint32_t w, int thr, int inv) {
    uint32_t m = 0u;
#pragma unroll
    for (int j = 0; j < 4; ++j) m |= (uint32_t)(((int)((w >> (8 * j)) & 0xFFu) <= thr) != (inv != 0)) << j;
    return m;
}

__global__ __launch_bounds__(STHR) void scan_box_kernel(const abc_scan_desc d) {
    __shared__ int red[4][STHR / 64];
    const int b = blockIdx.y;
    int32_t* box = d.box + (size_t)b * ABC_SCAN_NBOX;
    if (box[BOX_STATUS] != 0) return;      // (uniform: BAD_PARAMS or CONSTANT, written by the launch before)
    const int32_t* P = d.params + (size_t)b * ABC_SCAN_NPARAM;
    const int sh = P[ABC_SCAN_SRC_H], sw = P[ABC_SCAN_SRC_W];
    const int r0 = blockIdx.x * SCAN_ROWS;
    if (r0 >= sh) return;
    const int nrow = min(SCAN_ROWS, sh - r0);
    const int vpr = (sw + 15) >> 4;
    const int thr = box[BOX_THR], inv = box[BOX_INV];
    const uint8_t* src = d.src + (size_t)b * d.src_stride;
    int ymin = 0x7FFFFFFF, ymax = -1, xmin = 0x7FFFFFFF, xmax = -1;
    for (int i = threadIdx.x; i < nrow * vpr; i += STHR) {
        const int y = i / vpr, v = i - y * vpr;
        const u32x4 q = load_vec(src, d.src_pitch, r0 + y, v);
        uint32_t m = 0u;
#pragma unroll
        for (int k = 0; k < 4; ++k) m |= ink_bits(q[k], thr, inv) << (4 * k);
        const int valid = sw - 16 * v;      // >= 1
        if (valid < 16) m &= (1u << valid) - 1u;
        if (m) {
            ymin = min(ymin, r0 + y);
            ymax = max(ymax, r0 + y);
            xmin = min(xmin, 16 * v + (__ffs((int)m) - 1));
            xmax = max(xmax, 16 * v + (31 - __clz((int)m)));
        }
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        ymin = min(ymin, __shfl_xor(ymin, o));
        ymax = max(ymax, __shfl_xor(ymax, o));
        xmin = min(xmin, __shfl_xor(xmin, o));
        xmax = max(xmax, __shfl_xor(xmax, o));
    }
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { red[0][wave] = ymin; red[1][wave] = ymax; red[2][wave] = xmin; red[3][wave] = xmax; }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 1; k < STHR / 64; ++k) {
            ymin = min(ymin, red[0][k]); ymax = max(ymax, red[1][k]); xmin = min(xmin, red[2][k]); xmax = max(xmax, red[3][k]);
        }
        if (ymax >= 0) {
            atomicMin(&box[BOX_Y0], ymin);
            atomicMax(&box[BOX_Y1], ymax);
            atomicMin(&box[BOX_X0], xmin);
            atomicMax(&box[BOX_X1], xmax);
        }
    }
}

// the fit of a bh x bw box into the S x S canvas with `margin`: never upscales
__host__ __device__ inline void scan_fit(int bh, int bw, int S, int margin, int& rows, int& cols) {
    const int L = S - 2 * margin, m = bh > bw ? bh : bw;
    if (m <= L) { rows = bh; cols = bw; return; }
    const int64_t r = (int64_t)bh * L / m, c = (int64_t)bw * L / m;
    rows = r < 1 ? 1 : (int)r;
    cols = c < 1 ? 1 : (int)c;
}

__global__ __launch_bounds__(STHR) void scan_write_kernel(const abc_scan_desc d) {
    const int b = blockIdx.y, S = d.S;
    const int npix = S * S;                                   // (S <= 8192: pixel indices fit 32 bits)
    const int32_t* box = d.box + (size_t)b * ABC_SCAN_NBOX;
    const int status = box[BOX_STATUS], thr = box[BOX_THR], inv = box[BOX_INV];
    int y0 = 0, x0 = 0, bh = 0, bw = 0, rows = 0, cols = 0, ddx = 0, ddy = 0;
    if (status == 0) {
        y0 = box[BOX_Y0]; x0 = box[BOX_X0];
        bh = box[BOX_Y1] - y0 + 1; bw = box[BOX_X1] - x0 + 1;
        scan_fit(bh, bw, S, d.margin, rows, cols);
        ddx = (S - rows) / 2; ddy = (S - cols) / 2;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        int32_t* g = d.geom + (size_t)b * ABC_SCAN_NGEOM;
        g[ABC_SCAN_G_THR] = thr; g[ABC_SCAN_G_INVERTED] = inv; g[ABC_SCAN_G_STATUS] = status;
        g[ABC_SCAN_G_Y0] = y0; g[ABC_SCAN_G_X0] = x0; g[ABC_SCAN_G_BH] = bh; g[ABC_SCAN_G_BW] = bw;
        g[ABC_SCAN_G_ROWS] = rows; g[ABC_SCAN_G_COLS] = cols; g[ABC_SCAN_G_DDX] = ddx; g[ABC_SCAN_G_DDY] = ddy;
        g[ABC_SCAN_G_INK] = box[BOX_INK];
    }
    const int p0 = (blockIdx.x * STHR + threadIdx.x) * VEC;
    if (p0 >= npix) return;
    f32x4* o = (f32x4*)(d.out + (size_t)b * npix + p0);
    if (status & ABC_SCAN_BAD_PARAMS) {
        const f32x4 q = {__builtin_nanf(""), __builtin_nanf(""), __builtin_nanf(""), __builtin_nanf("")};
        o[0] = q;
        o[1] = q;
        return;
    }
    float y[VEC];
#pragma unroll
    for (int j = 0; j < VEC; ++j) y[j] = 0.f;
    const int x = p0 / S, yc0 = p0 - x * S;
    const int r = x - ddx, c0 = yc0 - ddy;
    if (status == 0 && r >= 0 && r < rows && c0 + VEC > 0 && c0 < cols) {
        // the pixel's source box: rows ya .. yb, columns xa[j] .. xb[j] (inclusive, inside the bounding box)
        const int ya = y0 + (int)((uint32_t)(r * bh) / (uint32_t)rows);
        const int yb = y0 + (int)(((uint32_t)((r + 1) * bh) + (uint32_t)rows - 1u) / (uint32_t)rows) - 1;
        int xa[VEC], xb[VEC];
        uint32_t n[VEC];
        // floor(c bw / cols) as quotient and remainder, stepped from column to column: q(c + 1) = q(c) + bw / cols (+ 1 when the
        // remainders carry); the box of c ends at ceil((c + 1) bw / cols) - 1 = q(c + 1) - (remainder of c + 1 == 0)
        const int cs = max(c0, 0);
        const uint32_t dq = (uint32_t)bw / (uint32_t)cols, dr = (uint32_t)bw - dq * (uint32_t)cols;
        uint32_t q = (uint32_t)(cs * bw) / (uint32_t)cols, rem = (uint32_t)(cs * bw) - q * (uint32_t)cols;
#pragma unroll
        for (int j = 0; j < VEC; ++j) {
            const int c = c0 + j;
            n[j] = 0u;
            xa[j] = 0;
            xb[j] = -1;                                       // (an empty range: outside the placed drawing)
            if (c < 0 || c >= cols) continue;
            xa[j] = x0 + (int)q;
            q += dq;
            rem += dr;
            if (rem >= (uint32_t)cols) { rem -= (uint32_t)cols; ++q; }
            xb[j] = x0 + (int)q - (rem == 0u ? 1 : 0);
        }
        const uint8_t* src = d.src + (size_t)b * d.src_stride;
        for (int yy = ya; yy <= yb; ++yy) {
            const uint64_t* row = (const uint64_t*)(src + (size_t)yy * d.src_pitch);
            int have = -1;                                    // the aligned 8-byte word whose ink bits `bits` holds
            uint32_t bits = 0u;
#pragma unroll
            for (int j = 0; j < VEC; ++j) {
                for (int w = xa[j] >> 3; w <= (xb[j] >> 3) && xb[j] >= 0; ++w) {
                    if (w != have) {      // (8 w <= xb < src_w <= pitch, a multiple of 16: the word lies inside the row)
                        const uint64_t t = row[w];
                        bits = ink_bits((uint32_t)t, thr, inv) | (ink_bits((uint32_t)(t >> 32), thr, inv) << 4);
                        have = w;
                    }
                    const int lo = max(xa[j] - 8 * w, 0), hi = min(xb[j] - 8 * w, 7);
                    n[j] += (uint32_t)__popc((bits >> lo) & ((2u << (hi - lo)) - 1u));
                }
            }
        }
        const uint64_t nrows = (uint64_t)(yb - ya + 1);
#pragma unroll
        for (int j = 0; j < VEC; ++j) {
            const uint64_t a = nrows * (uint64_t)(xb[j] - xa[j] + 1);
            y[j] = (n[j] >= 1u && (uint64_t)n[j] * 256u >= (uint64_t)d.cover_q8 * a) ? 1.f : 0.f;
        }
    }
    o[0] = (f32x4){y[0], y[1], y[2], y[3]};
    o[1] = (f32x4){y[4], y[5], y[6], y[7]};
}

}  // namespace

extern "C" int abc_scan_desc_size(void) { return (int)sizeof(abc_scan_desc); }

extern "C" int abc_build_scan_images(const abc_scan_desc* d, abc_stream_t stream) {
    if (!d) return abc_fail(ABC_EINVAL, "build_scan_images: null descriptor");
    if (!d->out || !d->src || !d->params || !d->hist || !d->box || !d->geom) return abc_fail(ABC_EINVAL, "build_scan_images: null pointer");
    if (d->B < 1 || d->B > 65535) return abc_fail(ABC_EINVAL, "build_scan_images: B must be 1 .. 65535");
    if (d->S < VEC || d->S > 8192 || d->S % VEC)
        return abc_fail(ABC_EUNSUPPORTED, "build_scan_images: S must be a multiple of 8 in 8 .. 8192 (8 pixels per thread)");
    if (d->src_pitch < 16 || d->src_pitch > 4096 || d->src_pitch % 16 || d->src_max_h < 1 || d->src_max_h > 4096)
        return abc_fail(ABC_EUNSUPPORTED, "build_scan_images: src_pitch (multiple of 16) and src_max_h must be at most 4096");
    if (d->src_stride % 16 || d->src_stride < (int64_t)d->src_max_h * d->src_pitch)
        return abc_fail(ABC_EINVAL, "build_scan_images: src_stride below src_max_h * src_pitch or not a multiple of 16");
    if (((uintptr_t)d->src | (uintptr_t)d->out) % 16) return abc_fail(ABC_EINVAL, "build_scan_images: src and out must be 16-byte aligned");
    if (((uintptr_t)d->hist | (uintptr_t)d->box | (uintptr_t)d->geom | (uintptr_t)d->params) % 4)
        return abc_fail(ABC_EINVAL, "build_scan_images: hist, box, geom and params must be 4-byte aligned");
    if (d->margin < 0 || 2 * (int64_t)d->margin >= d->S) return abc_fail(ABC_EINVAL, "build_scan_images: margin must leave 0 <= 2 margin < S");
    if (d->cover_q8 < 0 || d->cover_q8 > 256) return abc_fail(ABC_EINVAL, "build_scan_images: cover_q8 must be 0 .. 256");
    if (d->polarity != ABC_SCAN_DARK && d->polarity != ABC_SCAN_LIGHT && d->polarity != ABC_SCAN_AUTO)
        return abc_fail(ABC_EINVAL, "build_scan_images: polarity");
    if (d->params_host) {
        for (int b = 0; b < d->B; ++b)
            if (!scan_params_ok(d->params_host + (size_t)b * ABC_SCAN_NPARAM, d->src_max_h, d->src_pitch))
                return abc_fail(ABC_EINVAL, "build_scan_images: an image's src_h / src_w is below 1 or leaves its slot");
    }
    hipStream_t s = (hipStream_t)stream;
    const dim3 chunks((unsigned)((d->src_max_h + SCAN_ROWS - 1) / SCAN_ROWS), (unsigned)d->B);
    hipLaunchKernelGGL(scan_zero_kernel, dim3((unsigned)d->B), dim3(256), 0, s, d->hist);
    hipLaunchKernelGGL(scan_hist_kernel, chunks, dim3(STHR), 0, s, *d);
    hipLaunchKernelGGL(scan_threshold_kernel, dim3((unsigned)d->B), dim3(256), 0, s, *d);
    hipLaunchKernelGGL(scan_box_kernel, chunks, dim3(STHR), 0, s, *d);
    const int64_t per_img = (int64_t)d->S * d->S / VEC;
    hipLaunchKernelGGL(scan_write_kernel, dim3((unsigned)((per_img + STHR - 1) / STHR), (unsigned)d->B), dim3(STHR), 0, s, *d);
    return abc_check_launch("build_scan_images");
}
