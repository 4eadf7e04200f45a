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
// abc_build_scan_images_clean (the contract: abc_scan_clean_desc) puts four launches between the threshold and the box -- cells,
// union, flatten, decide, below -- and launches the box and fit+write kernels with a mask argument: nine launches, the same way.
// abc_split_scan_pages (the contract: abc_scan_split_desc) runs the same front over pages and gives every kept group of cells a
// canvas of its own: ten launches, at the end of this file.
#include "common.hpp"
#include "../../include/abcnet_hip.h"
#include "capi_util.hpp"
#include "block_scan.hpp"

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

// what the masked box and write passes of abc_build_scan_images_clean read beside abc_scan_desc: one keep byte per cell of the
// capacity grid (image b at keep + b * stride, cell (cy, cx) at cy * cap_cw + cx), cells of 1 << shift pixels
struct scan_mask {
    const uint8_t* keep;
    int64_t stride;
    int cap_cw, shift;
};

__device__ inline const scan_mask& mask_of(const scan_mask& k) { return k; }
// the image whose source output b reads under a mask, and whether the ink in cell (cy, cx) of that image counts for b
__device__ inline int mask_source(const scan_mask&, int b) { return b; }
__device__ inline bool mask_keeps(const scan_mask& k, int b, int, int cy, int cx) {
    const uint8_t* kr = k.keep + (size_t)b * k.stride + (size_t)cy * k.cap_cw;
    return kr[cx];
}

// what the fit+write pass of abc_split_scan_pages reads beside abc_scan_desc: output b is a canvas, its source the page of its
// drawings row (page 0 for an unused canvas, which reads no source), and a cell's ink counts when the cell's canvas is b
struct split_mask {
    const int32_t* canvas;         // [P][ncap]: the canvas of every cell of the capacity grid, -1 for none
    const int32_t* drawings;       // [D][ABC_SCAN_NDRAWING]
    int ncap, cap_cw, shift;
};

__device__ inline const split_mask& mask_of(const split_mask& k) { return k; }
__device__ inline int mask_source(const split_mask& k, int b) { return max(k.drawings[(size_t)b * ABC_SCAN_NDRAWING + ABC_SCAN_D_PAGE], 0); }
__device__ inline bool mask_keeps(const split_mask& k, int b, int page, int cy, int cx) {
    return k.canvas[(size_t)page * k.ncap + (size_t)cy * k.cap_cw + cx] == b;
}

// launched with d alone this is the box pass of abc_build_scan_images as it always was (the same kernel arguments, the same code);
// launched with d and a scan_mask it drops the ink outside kept cells
template <class... M>
__global__ __launch_bounds__(STHR) void scan_box_kernel(const abc_scan_desc d, const M... mk) {
    constexpr bool MASKED = sizeof...(M) != 0;
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
        if constexpr (MASKED) {
            if (m) {      // (a 16-byte vector lies in one cell, or at cell 8 in the two cells 2 v and 2 v + 1 < cap_cw = pitch / 8)
                const scan_mask& k = mask_of(mk...);
                const uint8_t* kr = k.keep + (size_t)b * k.stride + (size_t)((r0 + y) >> k.shift) * k.cap_cw;
                if (k.shift == 3) m &= (kr[2 * v] ? 0x00FFu : 0u) | (kr[2 * v + 1] ? 0xFF00u : 0u);
                else if (!kr[(16 * v) >> k.shift]) m = 0u;
            }
        }
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

// launched with d alone this is the fit+write pass of abc_build_scan_images as it always was; launched with d and a scan_mask it
// counts n over the ink of kept cells only; launched with d and a split_mask it writes canvas b from its page's source
template <class... M>
__global__ __launch_bounds__(STHR) void scan_write_kernel(const abc_scan_desc d, const M... mk) {
    constexpr bool MASKED = sizeof...(M) != 0;
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
        int sb = b;
        if constexpr (MASKED) sb = mask_source(mask_of(mk...), b);
        const uint8_t* src = d.src + (size_t)sb * d.src_stride;
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
                        if constexpr (MASKED) {      // (cells are multiples of 8 wide: an aligned 8-byte word lies in one cell)
                            const auto& k = mask_of(mk...);
                            if (!mask_keeps(k, b, sb, yy >> k.shift, (8 * w) >> k.shift)) bits = 0u;
                        }
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

// ---- the cell component filter of abc_build_scan_images_clean: four launches between the threshold and the masked box ----
//   cells      grid as the histogram: ink per cell of 64 source rows in LDS, each cell of the capacity grid stored once (its ink,
//              itself as its parent when occupied, a zero weight): the sequence resets the whole of its scratch here
//   union      one thread per cell of the capacity grid: union-find, the larger root hung under the smaller by compare-and-swap
//   flatten    one thread per cell: parent <- root, the cell's ink added to the root's weight (integer atomics, one per root and wave)
//   decide     one 1024-thread workgroup per image: H, the keep byte of every cell, the stats row, the debug slices, the status
// then the masked box and the masked fit+write.  Every loop that follows parents has the static bound ncap (the cells of the
// capacity grid); parents only decrease, so a correct run cannot reach it; a run that does sets the fail word and never spins.
constexpr int CTHR = 256;          // threads per workgroup of the union and flatten launches
constexpr int DTHR = 1024;         // threads of the decide launch's one workgroup per image
constexpr int CELL_LDS = 4096;     // cells of 64 source rows: (64 / cell) * ceil(4096 / cell) <= 8 * 512
// the words of an image's meta block in the scratch
enum { META_FAIL = 0, META_NWORD = 4 };

// an image's slice of abc_scan_clean_desc.scratch: ink, parent and weight per cell, one keep byte per cell, the meta words
struct clean_view {
    uint32_t* ink;
    int* parent;
    uint32_t* weight;
    uint8_t* keep;
    int* meta;
};

__host__ __device__ inline int64_t clean_keep_words(int64_t ncap) { return (ncap + 3) / 4; }
// int32 words of scratch per image, a multiple of 4 (16 bytes)
__host__ __device__ inline int64_t clean_image_words(int64_t ncap) {
    return (3 * ncap + clean_keep_words(ncap) + META_NWORD + 3) / 4 * 4;
}

__device__ inline clean_view clean_slice(void* scratch, int b, int ncap) {
    int32_t* w = (int32_t*)scratch + (size_t)b * clean_image_words(ncap);
    clean_view v;
    v.ink = (uint32_t*)w;
    v.parent = w + ncap;
    v.weight = (uint32_t*)(w + 2 * (size_t)ncap);
    v.keep = (uint8_t*)(w + 3 * (size_t)ncap);
    v.meta = w + 3 * (size_t)ncap + clean_keep_words(ncap);
    return v;
}

// the grid of cells a launch works on, derived on the host once
struct clean_grid {
    int shift;                     // cell = 1 << shift
    int cap_ch, cap_cw, ncap;      // the capacity grid and its cells
};

__global__ __launch_bounds__(STHR) void clean_cells_kernel(const abc_scan_desc d, const abc_scan_clean_desc q, const clean_grid G) {
    __shared__ uint32_t cnt[CELL_LDS];
    const int b = blockIdx.y;
    const int32_t* box = d.box + (size_t)b * ABC_SCAN_NBOX;
    if (box[BOX_STATUS] != 0) return;      // (uniform: BAD_PARAMS or CONSTANT; no later launch reads this image's scratch)
    const int32_t* P = d.params + (size_t)b * ABC_SCAN_NPARAM;
    const int sh = P[ABC_SCAN_SRC_H], sw = P[ABC_SCAN_SRC_W];
    const int r0 = blockIdx.x * SCAN_ROWS;
    const int crows = SCAN_ROWS >> G.shift;                  // rows of cells of this workgroup: 64 is a multiple of every cell
    const int ncell = crows * G.cap_cw;                       // <= CELL_LDS
    for (int i = threadIdx.x; i < ncell; i += STHR) cnt[i] = 0u;
    __syncthreads();
    if (r0 < sh) {                                            // (uniform)
        const int nrow = min(SCAN_ROWS, sh - r0);
        const int vpr = (sw + 15) >> 4;
        const int thr = box[BOX_THR], inv = box[BOX_INV];
        const uint8_t* src = d.src + (size_t)b * d.src_stride;
        for (int i = threadIdx.x; i < nrow * vpr; i += STHR) {
            const int y = i / vpr, v = i - y * vpr;
            const u32x4 w = load_vec(src, d.src_pitch, r0 + y, v);
            uint32_t m = 0u;
#pragma unroll
            for (int k = 0; k < 4; ++k) m |= ink_bits(w[k], thr, inv) << (4 * k);
            const int valid = sw - 16 * v;      // >= 1
            if (valid < 16) m &= (1u << valid) - 1u;
            if (!m) continue;
            uint32_t* row = cnt + (y >> G.shift) * G.cap_cw;
            if (G.shift == 3) {                               // two cells per vector: 2 v + 1 < cap_cw = pitch / 8
                const uint32_t lo = (uint32_t)__popc(m & 0xFFu), hi = (uint32_t)__popc(m >> 8);
                if (lo) atomicAdd(&row[2 * v], lo);
                if (hi) atomicAdd(&row[2 * v + 1], hi);
            } else {
                atomicAdd(&row[(16 * v) >> G.shift], (uint32_t)__popc(m));
            }
        }
    }
    __syncthreads();
    const clean_view V = clean_slice(q.scratch, b, G.ncap);
    const int cy0 = blockIdx.x * crows;
    for (int i = threadIdx.x; i < ncell; i += STHR) {
        const int cy = cy0 + i / G.cap_cw;
        if (cy >= G.cap_ch) break;                            // (the last workgroup's rows past the capacity grid)
        const int c = cy0 * G.cap_cw + i;
        const uint32_t n = cnt[i];
        V.ink[c] = n;
        V.parent[c] = n ? c : -1;
        V.weight[c] = 0u;
    }
    if (blockIdx.x == 0 && threadIdx.x < META_NWORD) V.meta[threadIdx.x] = 0;
}

// parents are read and written by atomics alone inside the union launch: they live in L2, no CU's L1 holds a copy that matters
__device__ inline int clean_parent(const int* parent, int c) { return __hip_atomic_load(parent + c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// the root of c, following at most `bound` parents; ok = false when the bound is reached (cannot happen: parent[x] <= x)
__device__ inline int clean_find(const int* parent, int c, int bound, bool& ok) {
    for (int it = 0; it < bound; ++it) {
        const int p = clean_parent(parent, c);
        if (p == c) return c;
        c = p;
    }
    ok = false;
    return c;
}

// one set of a and b: only a root is ever rewritten, and only to a smaller index, so the root of a set is its smallest cell.  Every
// failed compare-and-swap means that another thread hung that root meanwhile; fewer than ncap roots exist: `bound` tries suffice
__device__ inline void clean_unite(int* parent, int a, int b, int bound, bool& ok) {
    for (int it = 0; it < bound && ok; ++it) {
        a = clean_find(parent, a, bound, ok);
        b = clean_find(parent, b, bound, ok);
        if (a == b || !ok) return;
        if (a < b) { const int t = a; a = b; b = t; }
        if (atomicCAS(&parent[a], a, b) == a) return;
    }
    ok = false;
}

__global__ __launch_bounds__(CTHR) void clean_union_kernel(const abc_scan_desc d, const abc_scan_clean_desc q, const clean_grid G) {
    const int b = blockIdx.y;
    if (d.box[(size_t)b * ABC_SCAN_NBOX + BOX_STATUS] != 0) return;
    const int c = blockIdx.x * CTHR + threadIdx.x;
    if (c >= G.ncap) return;
    const clean_view V = clean_slice(q.scratch, b, G.ncap);
    if (!V.ink[c]) return;
    const int cy = c / G.cap_cw, cx = c - cy * G.cap_cw;
    bool ok = true;
    // W, NW, N, NE.  An occupied N stands for all four: NW and NE are N's own W and E neighbours, and W reaches N as its NE
    if (cy > 0 && V.ink[c - G.cap_cw]) {
        clean_unite(V.parent, c, c - G.cap_cw, G.ncap, ok);
    } else {
        if (cx > 0 && V.ink[c - 1]) clean_unite(V.parent, c, c - 1, G.ncap, ok);
        if (cy > 0 && cx > 0 && V.ink[c - G.cap_cw - 1]) clean_unite(V.parent, c, c - G.cap_cw - 1, G.ncap, ok);
        if (cy > 0 && cx + 1 < G.cap_cw && V.ink[c - G.cap_cw + 1]) clean_unite(V.parent, c, c - G.cap_cw + 1, G.ncap, ok);
    }
    if (!ok) atomicOr(&V.meta[META_FAIL], 1);
}

__global__ __launch_bounds__(CTHR) void clean_flatten_kernel(const abc_scan_desc d, const abc_scan_clean_desc q, const clean_grid G) {
    const int b = blockIdx.y;
    if (d.box[(size_t)b * ABC_SCAN_NBOX + BOX_STATUS] != 0) return;      // (uniform)
    const int c = blockIdx.x * CTHR + threadIdx.x;
    const clean_view V = clean_slice(q.scratch, b, G.ncap);
    const uint32_t n = c < G.ncap ? V.ink[c] : 0u;
    int r = -1;
    bool todo = false;
    if (n) {
        bool ok = true;
        r = clean_find(V.parent, c, G.ncap, ok);             // (no root changes in this launch: r is final)
        if (!ok) atomicOr(&V.meta[META_FAIL], 1);
        else if (r != c) atomicMin(&V.parent[c], r);          // (still a cell of c's set on every path that runs through c)
        todo = ok;
    }
    // the weights: a wave's 64 consecutive cells mostly share a root, and a page's cells all add to one word.  The lanes that share
    // the first live lane's root sum in the wave and add once, until no lane is left (every lane of the wave runs every round)
    const int lane = threadIdx.x & 63;
    for (int round = 0; round < 64; ++round) {                // (a round retires its first live lane at least: 64 suffice)
        const unsigned long long live = __ballot(todo);
        if (!live) break;
        const int lead = __ffsll((long long)live) - 1;
        const int rr = __shfl(r, lead);
        const bool mine = todo && r == rr;
        uint32_t s = mine ? n : 0u;
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) s += __shfl_xor(s, o);
        if (lane == lead) atomicAdd(&V.weight[rr], s);
        if (mine) todo = false;
    }
}

// sums (and one maximum) of a DTHR workgroup; every thread calls it, every thread gets the result
__device__ inline void clean_reduce(int64_t (&v)[4], int& mx, int64_t (*red)[5]) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] += __shfl_xor(v[k], o);
        mx = max(mx, __shfl_xor(mx, o));
    }
    const int wave = threadIdx.x >> 6;
    __syncthreads();                                          // (red may still be read from the call before)
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int k = 0; k < 4; ++k) red[wave][k] = v[k];
        red[wave][4] = mx;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = 0;
    mx = 0;
    for (int w = 0; w < DTHR / 64; ++w) {
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] += red[w][k];
        mx = max(mx, (int)red[w][4]);
    }
}

__global__ __launch_bounds__(DTHR) void clean_decide_kernel(const abc_scan_desc d, const abc_scan_clean_desc q, const clean_grid G) {
    __shared__ int64_t red[DTHR / 64][5];
    const int b = blockIdx.x, t = threadIdx.x;
    int32_t* box = d.box + (size_t)b * ABC_SCAN_NBOX;
    int32_t* st = q.stats + (size_t)b * ABC_SCAN_NCLEAN;
    int32_t* lab = q.labels_out ? q.labels_out + (size_t)b * G.ncap : nullptr;
    uint8_t* kep = q.keep_out ? q.keep_out + (size_t)b * G.ncap : nullptr;
    if (box[BOX_STATUS] != 0) {                               // (uniform) CONSTANT or BAD_PARAMS: as today, a zero stats row
        if (t < ABC_SCAN_NCLEAN) st[t] = 0;
        for (int c = t; c < G.ncap; c += DTHR) {
            if (lab) lab[c] = -1;
            if (kep) kep[c] = 0;
        }
        return;
    }
    const clean_view V = clean_slice(q.scratch, b, G.ncap);
    const bool failed = V.meta[META_FAIL] != 0;               // (uniform)
    // the components, the occupied cells and the heaviest weight
    int64_t s[4] = {0, 0, 0, 0};
    int H = 0;
    for (int c = t; c < G.ncap; c += DTHR) {
        if (!V.ink[c]) continue;
        s[0] += 1;
        if (V.parent[c] == c) { s[1] += 1; H = max(H, (int)V.weight[c]); }
    }
    clean_reduce(s, H, red);
    const int occupied = (int)s[0], components = (int)s[1];
    // the keep rule per cell, from its root's weight
    int64_t u[4] = {0, 0, 0, 0};
    int unused = 0;
    for (int c = t; c < G.ncap; c += DTHR) {
        const uint32_t n = failed ? 0u : V.ink[c];
        int label = -1, keep = 0;
        if (n) {
            label = V.parent[c];
            const int64_t w = (int64_t)V.weight[label];
            keep = w >= (int64_t)q.min_ink && 256 * w >= (int64_t)q.keep_q8 * (int64_t)H;
            if (keep) { u[0] += n; u[1] += label == c; }
        }
        V.keep[c] = (uint8_t)keep;
        if (lab) lab[c] = label;
        if (kep) kep[c] = (uint8_t)keep;
    }
    clean_reduce(u, unused, red);
    if (t == 0) {
        const int ink = box[BOX_INK];
        if (failed) {
            for (int k = 0; k < ABC_SCAN_NCLEAN; ++k) st[k] = 0;
            box[BOX_STATUS] = ABC_SCAN_CLEAN_FAILED;
        } else {
            st[ABC_SCAN_C_COMPONENTS] = components; st[ABC_SCAN_C_KEPT] = (int)u[1]; st[ABC_SCAN_C_INK_KEPT] = (int)u[0];
            st[ABC_SCAN_C_INK_DROPPED] = ink - (int)u[0]; st[ABC_SCAN_C_HEAVIEST] = H; st[ABC_SCAN_C_OCCUPIED] = occupied;
            if ((int64_t)q.min_ink > (int64_t)H) box[BOX_STATUS] = ABC_SCAN_NO_COMPONENT;      // nothing kept
        }
    }
}

// ---- abc_split_scan_pages: a page into its drawings, one canvas each.  Ten launches: zero, histogram, threshold, cells and flatten
// are the kernels above, run over the pages with the per-page box words in the scratch; between and after them
//   union      one thread per cell: an occupied cell unions with the occupied cells in the preceding half of its window
//   rank       one workgroup per page: H, the keep rule per root, the kept roots' ranks in label order by a scan with a running
//              carry over the grid in cell order, every cell's rank (-1: none), the page row, the page's list of taken roots
//   pack       one workgroup: first and taken per page by a scan over the pages, total, the drawings rows, the canvases' box
//              words reset, every cell's rank turned into its canvas
//   box        grid as the histogram: min / max per canvas in an LDS table of the page's slots, then one atomic per touched word
//   fit+write  scan_write_kernel over the D canvases with a split_mask
constexpr int SPLIT_K = ABC_SCAN_SPLIT_MAX_PER_PAGE;

// the split's slices of abc_scan_split_desc.scratch and its sizes, derived on the host once
struct split_view {
    clean_grid G;
    int32_t* pbox;                 // [P][ABC_SCAN_NBOX]: the box words of the pages (abc_scan_desc.box is the canvases')
    void* cells;                   // the clean_slice of every page
    int32_t* canvas;               // [P][ncap]: after rank a cell's rank in its page, after pack its canvas
    int32_t* list;                 // [P][SPLIT_K][2]: label and weight of the page's taken groups in order
    int P, D, K, reach;
};

__host__ __device__ inline int64_t split_canvas_words(int64_t P, int64_t ncap) { return (P * ncap + 3) / 4 * 4; }

__global__ __launch_bounds__(CTHR) void split_union_kernel(const abc_scan_desc d, const split_view W) {
    const clean_grid& G = W.G;
    const int b = blockIdx.y;
    if (d.box[(size_t)b * ABC_SCAN_NBOX + BOX_STATUS] != 0) return;
    const int c = blockIdx.x * CTHR + threadIdx.x;
    if (c >= G.ncap) return;
    const clean_view V = clean_slice(W.cells, b, G.ncap);
    if (!V.ink[c]) return;
    const int cy = c / G.cap_cw, cx = c - cy * G.cap_cw;
    bool ok = true;
    // the cells before c in cell order within Chebyshev distance reach: the rows above in full, this row to the left (the other
    // half of the window is joined by its own cells).  No occupied cell stands for another here: that holds at reach 1 alone
    for (int y = max(cy - W.reach, 0); y <= cy; ++y) {
        const int xe = y < cy ? min(cx + W.reach, G.cap_cw - 1) : cx - 1;
        for (int x = max(cx - W.reach, 0); x <= xe; ++x) {
            const int n = y * G.cap_cw + x;
            if (V.ink[n]) clean_unite(V.parent, c, n, G.ncap, ok);
        }
    }
    if (!ok) atomicOr(&V.meta[META_FAIL], 1);
}

__global__ __launch_bounds__(DTHR) void split_rank_kernel(const abc_scan_desc d, const abc_scan_split_desc q, const split_view W) {
    __shared__ int64_t red[DTHR / 64][5];
    __shared__ unsigned wt[DTHR / 64 + 1];
    const clean_grid& G = W.G;
    const int p = blockIdx.x, t = threadIdx.x;
    const int32_t* box = d.box + (size_t)p * ABC_SCAN_NBOX;
    int32_t* row = q.pages + (size_t)p * ABC_SCAN_NPAGE;
    int32_t* rank = W.canvas + (size_t)p * G.ncap;
    int32_t* lab = q.labels_out ? q.labels_out + (size_t)p * G.ncap : nullptr;
    const clean_view V = clean_slice(W.cells, p, G.ncap);
    const int status = box[BOX_STATUS];
    const bool failed = status == 0 && V.meta[META_FAIL] != 0;      // (uniform; a skipped page's scratch is not read)
    if (status != 0 || failed) {                                     // no drawings: the status and zeros
        if (t < ABC_SCAN_NPAGE) row[t] = t == ABC_SCAN_P_STATUS ? (failed ? ABC_SCAN_CLEAN_FAILED : status) : 0;
        for (int c = t; c < G.ncap; c += DTHR) {
            rank[c] = -1;
            if (lab) lab[c] = -1;
        }
        return;
    }
    // the groups, the occupied cells and the heaviest weight
    int64_t s[4] = {0, 0, 0, 0};
    int H = 0;
    for (int c = t; c < G.ncap; c += DTHR) {
        if (!V.ink[c]) continue;
        s[0] += 1;
        if (V.parent[c] == c) { s[1] += 1; H = max(H, (int)V.weight[c]); }
    }
    clean_reduce(s, H, red);
    // the kept roots in cell order, which is label order: a root's rank is the number of kept roots before it
    int64_t u[4] = {0, 0, 0, 0};
    int unused = 0;
    unsigned carry = 0u;
    int32_t* list = W.list + (size_t)p * SPLIT_K * 2;
    for (int c0 = 0; c0 < G.ncap; c0 += DTHR) {
        const int c = c0 + t;
        bool keep = false;
        int64_t w = 0;
        if (c < G.ncap && V.ink[c] && V.parent[c] == c) {
            w = (int64_t)V.weight[c];
            keep = w >= (int64_t)q.min_ink && 256 * w >= (int64_t)q.keep_q8 * (int64_t)H;
        }
        unsigned tot;
        const unsigned r = carry + block_excl_scan<DTHR>(keep ? 1u : 0u, wt, &tot);
        carry += tot;
        const bool taken = keep && r < (unsigned)W.K;
        if (keep) u[0] += w;
        if (taken) { list[2 * r] = c; list[2 * r + 1] = (int32_t)w; }
        if (c < G.ncap) rank[c] = taken ? (int)r : -1;
    }
    __threadfence_block();
    __syncthreads();
    // every other cell takes its root's rank (roots are written above and only read here)
    for (int c = t; c < G.ncap; c += DTHR) {
        const int label = V.ink[c] ? V.parent[c] : -1;
        if (label >= 0 && label != c) rank[c] = rank[label];
        if (lab) lab[c] = label;
    }
    clean_reduce(u, unused, red);
    if (t == 0) {
        const int kept = (int)carry;
        row[ABC_SCAN_P_STATUS] = (kept == 0 ? ABC_SCAN_NO_COMPONENT : 0) | (kept > W.K ? ABC_SCAN_SPLIT_PAGE_FULL : 0);
        row[ABC_SCAN_P_GROUPS] = (int)s[1];
        row[ABC_SCAN_P_KEPT] = kept;
        row[ABC_SCAN_P_FIRST] = 0;                                  // (pack's)
        row[ABC_SCAN_P_TAKEN] = min(kept, W.K);                     // (what the page asks for: pack cuts it at D)
        row[ABC_SCAN_P_INK_KEPT] = (int)u[0];
        row[ABC_SCAN_P_INK_DROPPED] = box[BOX_INK] - (int)u[0];
        row[ABC_SCAN_P_OCCUPIED] = (int)s[0];
    }
}

__global__ __launch_bounds__(DTHR) void split_pack_kernel(const abc_scan_desc d, const abc_scan_split_desc q, const split_view W) {
    __shared__ unsigned wt[DTHR / 64 + 1];
    const clean_grid& G = W.G;
    const int t = threadIdx.x;
    // first and taken, page by page without holes
    unsigned carry = 0u, truth = 0u;
    for (int p0 = 0; p0 < W.P; p0 += DTHR) {
        const int p = p0 + t;
        int32_t* row = q.pages + (size_t)p * ABC_SCAN_NPAGE;
        const unsigned want = p < W.P ? (unsigned)row[ABC_SCAN_P_TAKEN] : 0u;
        const unsigned kept = p < W.P ? (unsigned)row[ABC_SCAN_P_KEPT] : 0u;
        unsigned tot, tot_kept;
        const unsigned before = carry + block_excl_scan<DTHR>(want, wt, &tot);
        block_excl_scan<DTHR>(kept, wt, &tot_kept);
        carry += tot;
        truth += tot_kept;
        if (p < W.P) {
            const unsigned first = min(before, (unsigned)W.D), taken = min(want, (unsigned)W.D - first);
            row[ABC_SCAN_P_FIRST] = (int)first;
            row[ABC_SCAN_P_TAKEN] = (int)taken;
            if (taken < want) row[ABC_SCAN_P_STATUS] |= ABC_SCAN_SPLIT_BATCH_FULL;
        }
    }
    const int written = (int)min(carry, (unsigned)W.D);
    if (t == 0) { q.total[0] = written; q.total[1] = (int)truth; }
    __threadfence_block();
    __syncthreads();
    // the drawings rows and the canvases' box words: the taken groups, then the unused canvases
    for (int64_t i = t; i < (int64_t)W.P * SPLIT_K; i += DTHR) {
        const int p = (int)(i / SPLIT_K), r = (int)(i - (int64_t)p * SPLIT_K);
        const int32_t* row = q.pages + (size_t)p * ABC_SCAN_NPAGE;
        if (r >= row[ABC_SCAN_P_TAKEN]) continue;
        const int j = row[ABC_SCAN_P_FIRST] + r;                    // < D
        const int32_t* e = W.list + ((size_t)p * SPLIT_K + r) * 2;
        const int32_t* pb = W.pbox + (size_t)p * ABC_SCAN_NBOX;
        int32_t* dr = q.drawings + (size_t)j * ABC_SCAN_NDRAWING;
        dr[ABC_SCAN_D_PAGE] = p; dr[ABC_SCAN_D_LABEL] = e[0]; dr[ABC_SCAN_D_WEIGHT] = e[1]; dr[ABC_SCAN_D_RANK] = r;
        int32_t* box = d.box + (size_t)j * ABC_SCAN_NBOX;
        box[BOX_Y0] = 0x7FFFFFFF; box[BOX_Y1] = -1; box[BOX_X0] = 0x7FFFFFFF; box[BOX_X1] = -1;
        box[BOX_THR] = pb[BOX_THR]; box[BOX_INV] = pb[BOX_INV]; box[BOX_STATUS] = 0; box[BOX_INK] = e[1];
    }
    for (int j = written + t; j < W.D; j += DTHR) {
        int32_t* dr = q.drawings + (size_t)j * ABC_SCAN_NDRAWING;
        dr[ABC_SCAN_D_PAGE] = -1; dr[ABC_SCAN_D_LABEL] = -1; dr[ABC_SCAN_D_WEIGHT] = 0; dr[ABC_SCAN_D_RANK] = -1;
        int32_t* box = d.box + (size_t)j * ABC_SCAN_NBOX;
        box[BOX_Y0] = 0x7FFFFFFF; box[BOX_Y1] = -1; box[BOX_X0] = 0x7FFFFFFF; box[BOX_X1] = -1;
        box[BOX_THR] = -1; box[BOX_INV] = 0; box[BOX_STATUS] = ABC_SCAN_NO_COMPONENT; box[BOX_INK] = 0;
    }
    // every cell's rank into its canvas
    for (int p = 0; p < W.P; ++p) {
        const int32_t* row = q.pages + (size_t)p * ABC_SCAN_NPAGE;
        const int first = row[ABC_SCAN_P_FIRST], taken = row[ABC_SCAN_P_TAKEN];
        int32_t* cv = W.canvas + (size_t)p * G.ncap;
        int32_t* co = q.canvas_out ? q.canvas_out + (size_t)p * G.ncap : nullptr;
        for (int c = t; c < G.ncap; c += DTHR) {
            const int r = cv[c];
            const int j = r >= 0 && r < taken ? first + r : -1;
            cv[c] = j;
            if (co) co[c] = j;
        }
    }
}

__global__ __launch_bounds__(STHR) void split_box_kernel(const abc_scan_desc d, const abc_scan_split_desc q, const split_view W) {
    __shared__ int tab[SPLIT_K][4];                               // BOX_Y0 .. BOX_X1 of the page's slots (4 SPLIT_K <= STHR)
    const clean_grid& G = W.G;
    const int p = blockIdx.y;
    const int32_t* row = q.pages + (size_t)p * ABC_SCAN_NPAGE;
    const int first = row[ABC_SCAN_P_FIRST], taken = row[ABC_SCAN_P_TAKEN];
    if (taken == 0) return;                                       // (uniform: also every page without drawings)
    const int32_t* P = d.params + (size_t)p * ABC_SCAN_NPARAM;
    const int sh = P[ABC_SCAN_SRC_H], sw = P[ABC_SCAN_SRC_W];
    const int r0 = blockIdx.x * SCAN_ROWS;
    if (r0 >= sh) return;
    if (threadIdx.x < 4 * taken) tab[threadIdx.x >> 2][threadIdx.x & 3] = (threadIdx.x & 1) ? -1 : 0x7FFFFFFF;
    __syncthreads();
    const int nrow = min(SCAN_ROWS, sh - r0);
    const int vpr = (sw + 15) >> 4;
    const int32_t* pb = W.pbox + (size_t)p * ABC_SCAN_NBOX;
    const int thr = pb[BOX_THR], inv = pb[BOX_INV];
    const uint8_t* src = d.src + (size_t)p * d.src_stride;
    const int32_t* cv = W.canvas + (size_t)p * G.ncap;
    // a thread keeps the extent of the slot it met last and adds it to the table when the slot changes
    int slot = -1, ymin = 0x7FFFFFFF, ymax = -1, xmin = 0x7FFFFFFF, xmax = -1;
    auto flush = [&]() {
        if (slot < 0) return;
        atomicMin(&tab[slot][BOX_Y0], ymin); atomicMax(&tab[slot][BOX_Y1], ymax);
        atomicMin(&tab[slot][BOX_X0], xmin); atomicMax(&tab[slot][BOX_X1], xmax);
    };
    // the ink bits m (bit i: column x + i) of row y belong to canvas j
    auto add = [&](int j, uint32_t m, int y, int x) {
        if (!m || j < 0) return;
        const int sl = j - first;                                 // 0 .. taken - 1: a page's canvases are consecutive
        if (sl != slot) { flush(); slot = sl; ymin = 0x7FFFFFFF; ymax = -1; xmin = 0x7FFFFFFF; xmax = -1; }
        ymin = min(ymin, y); ymax = max(ymax, y);
        xmin = min(xmin, x + (__ffs((int)m) - 1)); xmax = max(xmax, x + (31 - __clz((int)m)));
    };
    for (int i = threadIdx.x; i < nrow * vpr; i += STHR) {
        const int y = i / vpr, v = i - y * vpr;
        const u32x4 w = load_vec(src, d.src_pitch, r0 + y, v);
        uint32_t m = 0u;
#pragma unroll
        for (int k = 0; k < 4; ++k) m |= ink_bits(w[k], thr, inv) << (4 * k);
        const int valid = sw - 16 * v;      // >= 1
        if (valid < 16) m &= (1u << valid) - 1u;
        if (!m) continue;
        // (a 16-byte vector lies in one cell, or at cell 8 in the two cells 2 v and 2 v + 1 < cap_cw = pitch / 8)
        const int32_t* cr = cv + (size_t)((r0 + y) >> G.shift) * G.cap_cw;
        if (G.shift == 3) {
            add(cr[2 * v], m & 0xFFu, r0 + y, 16 * v);
            add(cr[2 * v + 1], m >> 8, r0 + y, 16 * v + 8);
        } else {
            add(cr[(16 * v) >> G.shift], m, r0 + y, 16 * v);
        }
    }
    flush();
    __syncthreads();
    if (threadIdx.x < 4 * taken) {
        const int sl = threadIdx.x >> 2, w = threadIdx.x & 3;
        if (tab[sl][BOX_Y1] >= 0) {                               // a slot this workgroup's rows touched
            int32_t* box = d.box + (size_t)(first + sl) * ABC_SCAN_NBOX;
            if (w & 1) atomicMax(&box[w], tab[sl][w]);
            else atomicMin(&box[w], tab[sl][w]);
        }
    }
}

}  // namespace

extern "C" int abc_scan_desc_size(void) { return (int)sizeof(abc_scan_desc); }

// the guards of abc_build_scan_images, shared with abc_build_scan_images_clean: 0 when d may be launched
static int scan_guards(const abc_scan_desc* d) {
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
    return 0;
}

extern "C" int abc_build_scan_images(const abc_scan_desc* d, abc_stream_t stream) {
    if (const int rc = scan_guards(d)) return rc;
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

extern "C" int abc_scan_clean_desc_size(void) { return (int)sizeof(abc_scan_clean_desc); }

static int clean_shift(int cell) { return cell == 8 ? 3 : cell == 16 ? 4 : cell == 32 ? 5 : cell == 64 ? 6 : -1; }

extern "C" int64_t abc_scan_clean_scratch_bytes(int32_t B, int32_t src_max_h, int32_t src_pitch, int32_t cell) {
    if (B < 1 || B > 65535 || src_max_h < 1 || src_max_h > 4096 || src_pitch < 16 || src_pitch > 4096 || src_pitch % 16 || clean_shift(cell) < 0)
        return abc_fail(ABC_EINVAL, "scan_clean_scratch_bytes: B, src_max_h, src_pitch or cell outside abc_build_scan_images_clean's limits");
    const int64_t ncap = (int64_t)((src_max_h + cell - 1) / cell) * ((src_pitch + cell - 1) / cell);
    return (int64_t)B * clean_image_words(ncap) * 4;
}

extern "C" int abc_build_scan_images_clean(const abc_scan_desc* d, const abc_scan_clean_desc* q, abc_stream_t stream) {
    if (const int rc = scan_guards(d)) return rc;
    if (!q) return abc_fail(ABC_EINVAL, "build_scan_images_clean: null cleaning descriptor");
    const int shift = clean_shift(q->cell);
    if (shift < 0) return abc_fail(ABC_EUNSUPPORTED, "build_scan_images_clean: cell must be 8, 16, 32 or 64");
    if (q->min_ink < 0) return abc_fail(ABC_EINVAL, "build_scan_images_clean: min_ink must be >= 0");
    if (q->keep_q8 < 0 || q->keep_q8 > 256) return abc_fail(ABC_EINVAL, "build_scan_images_clean: keep_q8 must be 0 .. 256");
    if (!q->scratch || !q->stats) return abc_fail(ABC_EINVAL, "build_scan_images_clean: null pointer");
    if ((uintptr_t)q->scratch % 16) return abc_fail(ABC_EINVAL, "build_scan_images_clean: scratch must be 16-byte aligned");
    if (((uintptr_t)q->stats | (uintptr_t)q->labels_out) % 4)
        return abc_fail(ABC_EINVAL, "build_scan_images_clean: stats and labels_out must be 4-byte aligned");
    clean_grid G;
    G.shift = shift;
    G.cap_ch = (d->src_max_h + q->cell - 1) >> shift;
    G.cap_cw = (d->src_pitch + q->cell - 1) >> shift;
    G.ncap = G.cap_ch * G.cap_cw;                              // <= 512 * 512
    scan_mask k;
    k.keep = (const uint8_t*)q->scratch + 3 * (size_t)G.ncap * 4;      // (clean_slice: the keep bytes follow ink, parent and weight)
    k.stride = clean_image_words(G.ncap) * 4;
    k.cap_cw = G.cap_cw;
    k.shift = shift;
    hipStream_t s = (hipStream_t)stream;
    const dim3 chunks((unsigned)((d->src_max_h + SCAN_ROWS - 1) / SCAN_ROWS), (unsigned)d->B);
    const dim3 cells((unsigned)((G.ncap + CTHR - 1) / CTHR), (unsigned)d->B);
    hipLaunchKernelGGL(scan_zero_kernel, dim3((unsigned)d->B), dim3(256), 0, s, d->hist);
    hipLaunchKernelGGL(scan_hist_kernel, chunks, dim3(STHR), 0, s, *d);
    hipLaunchKernelGGL(scan_threshold_kernel, dim3((unsigned)d->B), dim3(256), 0, s, *d);
    hipLaunchKernelGGL(clean_cells_kernel, chunks, dim3(STHR), 0, s, *d, *q, G);
    hipLaunchKernelGGL(clean_union_kernel, cells, dim3(CTHR), 0, s, *d, *q, G);
    hipLaunchKernelGGL(clean_flatten_kernel, cells, dim3(CTHR), 0, s, *d, *q, G);
    hipLaunchKernelGGL(clean_decide_kernel, dim3((unsigned)d->B), dim3(DTHR), 0, s, *d, *q, G);
    hipLaunchKernelGGL(scan_box_kernel, chunks, dim3(STHR), 0, s, *d, k);
    const int64_t per_img = (int64_t)d->S * d->S / VEC;
    hipLaunchKernelGGL(scan_write_kernel, dim3((unsigned)((per_img + STHR - 1) / STHR), (unsigned)d->B), dim3(STHR), 0, s, *d, k);
    return abc_check_launch("build_scan_images_clean");
}

extern "C" int abc_scan_split_desc_size(void) { return (int)sizeof(abc_scan_split_desc); }

extern "C" int64_t abc_scan_split_scratch_bytes(int32_t P, int32_t src_max_h, int32_t src_pitch, int32_t cell, int32_t D) {
    if (P < 1 || P > 65535 || D < 1 || D > 65535 || src_max_h < 1 || src_max_h > 4096 || src_pitch < 16 || src_pitch > 4096 ||
        src_pitch % 16 || clean_shift(cell) < 0)
        return abc_fail(ABC_EINVAL, "scan_split_scratch_bytes: P, D, src_max_h, src_pitch or cell outside abc_split_scan_pages' limits");
    const int64_t ncap = (int64_t)((src_max_h + cell - 1) / cell) * ((src_pitch + cell - 1) / cell);
    // the pages' box words, their cells, every cell's canvas, the pages' lists (the canvases' own words are d->box: D sizes nothing here)
    return ((int64_t)P * ABC_SCAN_NBOX + (int64_t)P * clean_image_words(ncap) + split_canvas_words(P, ncap) + (int64_t)P * SPLIT_K * 2) * 4;
}

extern "C" int abc_split_scan_pages(const abc_scan_desc* d, const abc_scan_split_desc* q, abc_stream_t stream) {
    if (const int rc = scan_guards(d)) return rc;
    if (!q) return abc_fail(ABC_EINVAL, "split_scan_pages: null splitting descriptor");
    const int shift = clean_shift(q->cell);
    if (shift < 0) return abc_fail(ABC_EUNSUPPORTED, "split_scan_pages: cell must be 8, 16, 32 or 64");
    if (q->canvases < 1 || q->canvases > 65535) return abc_fail(ABC_EINVAL, "split_scan_pages: canvases must be 1 .. 65535");
    if (q->max_per_page < 1 || q->max_per_page > SPLIT_K) return abc_fail(ABC_EINVAL, "split_scan_pages: max_per_page must be 1 .. 64");
    if (q->reach < 1 || q->reach > ABC_SCAN_SPLIT_MAX_REACH) return abc_fail(ABC_EINVAL, "split_scan_pages: reach must be 1 .. 4");
    if (q->min_ink < 0) return abc_fail(ABC_EINVAL, "split_scan_pages: min_ink must be >= 0");
    if (q->keep_q8 < 0 || q->keep_q8 > 256) return abc_fail(ABC_EINVAL, "split_scan_pages: keep_q8 must be 0 .. 256");
    if (!q->scratch || !q->pages || !q->drawings || !q->total) return abc_fail(ABC_EINVAL, "split_scan_pages: null pointer");
    if ((uintptr_t)q->scratch % 16) return abc_fail(ABC_EINVAL, "split_scan_pages: scratch must be 16-byte aligned");
    if (((uintptr_t)q->pages | (uintptr_t)q->drawings | (uintptr_t)q->total | (uintptr_t)q->labels_out | (uintptr_t)q->canvas_out) % 4)
        return abc_fail(ABC_EINVAL, "split_scan_pages: pages, drawings, total, labels_out and canvas_out must be 4-byte aligned");
    split_view W;
    W.G.shift = shift;
    W.G.cap_ch = (d->src_max_h + q->cell - 1) >> shift;
    W.G.cap_cw = (d->src_pitch + q->cell - 1) >> shift;
    W.G.ncap = W.G.cap_ch * W.G.cap_cw;                        // <= 512 * 512
    W.P = d->B; W.D = q->canvases; W.K = q->max_per_page; W.reach = q->reach;
    W.pbox = (int32_t*)q->scratch;
    int32_t* cells = W.pbox + (size_t)W.P * ABC_SCAN_NBOX;
    W.cells = cells;
    W.canvas = cells + (size_t)W.P * clean_image_words(W.G.ncap);
    W.list = W.canvas + split_canvas_words(W.P, W.G.ncap);
    abc_scan_desc pg = *d;                                       // the pages as the kernels above take images: their box words
    pg.box = W.pbox;
    abc_scan_clean_desc qc = {};                                 // (the cells and flatten kernels read the scratch alone)
    qc.scratch = W.cells;
    qc.cell = q->cell;
    split_mask k;
    k.canvas = W.canvas;
    k.drawings = q->drawings;
    k.ncap = W.G.ncap; k.cap_cw = W.G.cap_cw; k.shift = shift;
    hipStream_t s = (hipStream_t)stream;
    const dim3 chunks((unsigned)((d->src_max_h + SCAN_ROWS - 1) / SCAN_ROWS), (unsigned)W.P);
    const dim3 cellgrid((unsigned)((W.G.ncap + CTHR - 1) / CTHR), (unsigned)W.P);
    hipLaunchKernelGGL(scan_zero_kernel, dim3((unsigned)W.P), dim3(256), 0, s, pg.hist);
    hipLaunchKernelGGL(scan_hist_kernel, chunks, dim3(STHR), 0, s, pg);
    hipLaunchKernelGGL(scan_threshold_kernel, dim3((unsigned)W.P), dim3(256), 0, s, pg);
    hipLaunchKernelGGL(clean_cells_kernel, chunks, dim3(STHR), 0, s, pg, qc, W.G);
    hipLaunchKernelGGL(split_union_kernel, cellgrid, dim3(CTHR), 0, s, pg, W);
    hipLaunchKernelGGL(clean_flatten_kernel, cellgrid, dim3(CTHR), 0, s, pg, qc, W.G);
    hipLaunchKernelGGL(split_rank_kernel, dim3((unsigned)W.P), dim3(DTHR), 0, s, pg, *q, W);
    hipLaunchKernelGGL(split_pack_kernel, dim3(1), dim3(DTHR), 0, s, *d, *q, W);
    hipLaunchKernelGGL(split_box_kernel, chunks, dim3(STHR), 0, s, *d, *q, W);
    const int64_t per_img = (int64_t)d->S * d->S / VEC;
    hipLaunchKernelGGL(scan_write_kernel, dim3((unsigned)((per_img + STHR - 1) / STHR), (unsigned)W.D), dim3(STHR), 0, s, *d, k);
    return abc_check_launch("split_scan_pages");
}
