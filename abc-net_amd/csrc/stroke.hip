// Stroke width of a binary drawing, normalised: despeckle, thin toward the skeleton (Guo-Hall, two subiterations), dilate by a
// disk.  The contract in full: include/abcnet_hip.h (abc_stroke_desc) and DESIGN.md section 7.
//
// One launch, one workgroup per image.  The image lives in LDS as bits, inside a frame of paper: row y is W = ceil(S / 32) words
// plus one border word, bit j of word w is the pixel of column 32 w + j (S is a multiple of 8, so the last word of a row may be
// ragged: its upper bits stay 0 throughout); PAD paper rows lie above and below.  The border word of row y is the right
// neighbour of its last word and the left neighbour of the first word of row y + 1, so no read of a pass tests a bound: the
// word (y, w) is img[(y + PAD) * Wp + w + 1], Wp = W + 1.  A 512 x 512 image takes 35 KB, a 1024 x 1024 one 136 KB of the
// CU's 160 KB.
//   pack       16-byte loads, one thread = 4 pixels = one nibble, OR-ed into its word with an LDS atomic (ink is sparse: a paper
//              nibble costs nothing)
//   a pass     (despeckle, a subiteration, the dilation) in two phases: every thread computes the new value of its words into
//              registers from the eight neighbour planes -- shifts of the three rows, with carries from the adjacent words -- as
//              bit-sliced Boolean arithmetic on the word, no per-pixel loop; a barrier; then it applies them.  One copy of the
//              image is enough, and every pass reads the state as it was before the pass.  A deleting pass skips paper words.
//   unpack     16-byte stores of 0.0f / 1.0f
// A thread owns WPT consecutive words, WPT odd: the lanes of a wave read at an odd stride, which is conflict-free.
// Everything is integer; plain C++.
#include "common.hpp"
#include "../../include/abcnet_hip.h"
#include "capi_util.hpp"

namespace {

enum { PASS_ISOLATED = 0, PASS_A = 1, PASS_B = 2, PASS_DILATE = 3 };
constexpr int PAD = 3;      // paper rows above and below: the largest radius

// words of LDS an S x S image takes with its frame
__host__ __device__ constexpr int frame_words(int S) { return (S + 2 * PAD) * (((S + 31) >> 5) + 1) + 1; }

// bit j: exactly one of the four bits j is set
__device__ inline uint32_t exactly_one(uint32_t a, uint32_t b, uint32_t c, uint32_t d) {
    return ((a ^ b) ^ (c ^ d)) & ~((a & b) | (c & d));
}

// bit j: at least two of the four bits j are set
__device__ inline uint32_t two_or_more(uint32_t a, uint32_t b, uint32_t c, uint32_t d) {
    return (a & b) | (c & d) | ((a ^ b) & (c ^ d));
}

// the pixels of the word at i (a word of the canvas, value c != 0) that the pass deletes
__device__ inline uint32_t flagged(const uint32_t* img, uint32_t c, int i, int Wp, int pass) {
    const uint32_t nl = img[i - Wp - 1], nc = img[i - Wp], nr = img[i - Wp + 1];
    const uint32_t cl = img[i - 1], cr = img[i + 1];
    const uint32_t sl = img[i + Wp - 1], sc = img[i + Wp], sr = img[i + Wp + 1];
    // the neighbour planes: bit j is the neighbour of the pixel at bit j (west is the column before: one bit down)
    const uint32_t p2 = nc, p6 = sc;
    const uint32_t p8 = (c << 1) | (cl >> 31), p4 = (c >> 1) | (cr << 31);
    const uint32_t p9 = (nc << 1) | (nl >> 31), p3 = (nc >> 1) | (nr << 31);
    const uint32_t p7 = (sc << 1) | (sl >> 31), p5 = (sc >> 1) | (sr << 31);
    if (pass == PASS_ISOLATED) return c & ~(p2 | p3 | p4 | p5 | p6 | p7 | p8 | p9);
    const uint32_t c1 = exactly_one(~p2 & (p3 | p4), ~p4 & (p5 | p6), ~p6 & (p7 | p8), ~p8 & (p9 | p2));
    const uint32_t a1 = p9 | p2, a2 = p3 | p4, a3 = p5 | p6, a4 = p7 | p8;
    const uint32_t b1 = p2 | p3, b2 = p4 | p5, b3 = p6 | p7, b4 = p8 | p9;
    // 2 <= min(N1, N2) <= 3: both at least 2, not both 4
    const uint32_t n_ok = two_or_more(a1, a2, a3, a4) & two_or_more(b1, b2, b3, b4) & ~(a1 & a2 & a3 & a4 & b1 & b2 & b3 & b4);
    const uint32_t m = pass == PASS_A ? ((p6 | p7 | ~p9) & p8) : ((p2 | p3 | ~p5) & p4);
    return c & c1 & n_ok & ~m;
}

// the word at i of the image dilated by disk(r), r = 1 .. 3 <= PAD, before the cut to the canvas
__device__ inline uint32_t dilated(const uint32_t* img, int i, int Wp, int r) {
    uint32_t out = 0u;
    for (int dy = -r; dy <= r; ++dy) {
        const int k2 = r * r - dy * dy;
        const int dxm = k2 >= 9 ? 3 : (k2 >= 4 ? 2 : (k2 >= 1 ? 1 : 0));      // the largest dx with dx^2 <= k2
        const int j = i + dy * Wp;
        const uint32_t l = img[j - 1], c = img[j], rr = img[j + 1];
        uint32_t acc = c;
        for (int dx = 1; dx <= dxm; ++dx) acc |= (c << dx) | (l >> (32 - dx)) | (c >> dx) | (rr << (32 - dx));
        out |= acc;
    }
    return out;
}

// the canvas bits of word w of a row: all of a full word, the low S - 32 w of a ragged one, none of the border word (w = W)
__device__ inline uint32_t canvas_bits(int w, int S) {
    const int valid = S - 32 * w;
    return valid >= 32 ? 0xFFFFFFFFu : (valid > 0 ? (1u << valid) - 1u : 0u);
}

// LW: the words of LDS the framed image may take; NT threads; a thread owns the WPT consecutive words from first + t * WPT
template <int LW, int NT, int WPT>
__global__ __launch_bounds__(NT) void stroke_kernel(const abc_stroke_desc d) {
    __shared__ uint32_t img[LW];
    __shared__ int red[2][NT / 64];
    const int b = blockIdx.x, t = threadIdx.x, S = d.S;
    const int Wp = ((S + 31) >> 5) + 1, nvec = S * S / 4;
    // the words of rows 0 .. S - 1, border words included: S * Wp <= WPT * NT and frame_words(S) <= LW (the launcher's choice)
    const int first = PAD * Wp + 1, count = S * Wp;
    int32_t* st = d.stats + (size_t)b * ABC_STROKE_NSTAT;
    const float* src = d.src + (size_t)b * S * S;
    float* dst = d.dst + (size_t)b * S * S;
    if (d.skip && d.skip[(size_t)b * d.skip_stride] != 0) {      // (uniform)
        if (src != dst)
            for (int i = t; i < nvec; i += NT) ((u32x4*)dst)[i] = ((const u32x4*)src)[i];
        if (t == 0) {
            st[ABC_STROKE_ITERATIONS] = 0; st[ABC_STROKE_CONVERGED] = 0; st[ABC_STROKE_INK_IN] = 0; st[ABC_STROKE_INK_OUT] = 0;
            st[ABC_STROKE_SKIPPED] = 1;
        }
        return;
    }
    // pack
    for (int i = t; i < frame_words(S); i += NT) img[i] = 0u;
    __syncthreads();
    int ink_in = 0, ink_out = 0;
    for (int i = t; i < nvec; i += NT) {
        const f32x4 q = ((const f32x4*)src)[i];
        const uint32_t nib = (uint32_t)(q[0] > 0.5f) | ((uint32_t)(q[1] > 0.5f) << 1) | ((uint32_t)(q[2] > 0.5f) << 2) | ((uint32_t)(q[3] > 0.5f) << 3);
        if (nib) {
            const int p = 4 * i, y = p / S, x = p - y * S;      // (x a multiple of 4: the nibble lies inside one word)
            atomicOr(&img[first + y * Wp + (x >> 5)], nib << (x & 31));
            ink_in += __popc(nib);
        }
    }
    __syncthreads();
    // The new values of a thread's words wait in nw[] for the barrier.  The sweep is a real loop -- unrolled, the compiler lifts
    // the reads of all WPT neighbourhoods to its top and spills -- so nw[] is filled as a shift register: static indices only.
    uint32_t nw[WPT];
    auto sweep = [&](int pass) -> int {
        uint32_t any = 0u;
#pragma unroll 1
        for (int k = 0; k < WPT; ++k) {
            const int i = t * WPT + k;
            uint32_t v = 0u;
            if (i < count) {
                if (pass == PASS_DILATE) {
                    v = dilated(img, first + i, Wp, d.radius) & canvas_bits(i % Wp, S);
                } else {
                    const uint32_t c = img[first + i];
                    if (c) v = flagged(img, c, first + i, Wp, pass);      // (a border word is paper: never here)
                }
            }
            any |= v;
#pragma unroll
            for (int j = 0; j + 1 < WPT; ++j) nw[j] = nw[j + 1];
            nw[WPT - 1] = v;
        }
        return any != 0u;
    };
    // a deleting pass: nonzero when this thread deleted something
    auto remove = [&](int pass) -> int {
        const int mine = sweep(pass);
        __syncthreads();
#pragma unroll
        for (int k = 0; k < WPT; ++k)
            if (nw[k]) img[first + t * WPT + k] &= ~nw[k];
        __syncthreads();
        return mine;
    };
    if (d.drop_isolated) remove(PASS_ISOLATED);
    int iters = 0, conv = 0;
    if (d.max_iter != 0) {
        for (;;) {      // (every test below is uniform)
            int mine = remove(PASS_A);
            mine |= remove(PASS_B);
            const int changed = __syncthreads_or(mine);
            ++iters;
            if (!changed) { conv = 1; break; }
            if (d.max_iter > 0 && iters >= d.max_iter) break;
        }
    }
    if (d.radius > 0) {
        sweep(PASS_DILATE);
        __syncthreads();
#pragma unroll
        for (int k = 0; k < WPT; ++k)
            if (t * WPT + k < count) img[first + t * WPT + k] = nw[k];
        __syncthreads();
    }
    // unpack (every read of src lies before the barriers above: src == dst is safe)
    for (int i = t; i < nvec; i += NT) {
        const int p = 4 * i, y = p / S, x = p - y * S;
        const uint32_t nib = (img[first + y * Wp + (x >> 5)] >> (x & 31)) & 15u;
        const f32x4 q = {(nib & 1u) ? 1.f : 0.f, (nib & 2u) ? 1.f : 0.f, (nib & 4u) ? 1.f : 0.f, (nib & 8u) ? 1.f : 0.f};
        ((f32x4*)dst)[i] = q;
        ink_out += __popc(nib);
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        ink_in += __shfl_xor(ink_in, o);
        ink_out += __shfl_xor(ink_out, o);
    }
    if ((t & 63) == 0) { red[0][t >> 6] = ink_in; red[1][t >> 6] = ink_out; }
    __syncthreads();
    if (t == 0) {
        int a = 0, c = 0;
#pragma unroll
        for (int k = 0; k < NT / 64; ++k) { a += red[0][k]; c += red[1][k]; }
        st[ABC_STROKE_ITERATIONS] = iters; st[ABC_STROKE_CONVERGED] = conv; st[ABC_STROKE_INK_IN] = a; st[ABC_STROKE_INK_OUT] = c;
        st[ABC_STROKE_SKIPPED] = 0;
    }
}

// the three sizes of the framed image: (largest S, threads); words per thread = ceil(S * Wp / threads)
static_assert(frame_words(256) <= 2360 && 256 * 9 <= 9 * 256, "S <= 256");
static_assert(frame_words(512) <= 8808 && 512 * 17 <= 9 * 1024, "S <= 512");
static_assert(frame_words(ABC_STROKE_MAX_SIZE) <= 33992 && ABC_STROKE_MAX_SIZE * 33 <= 33 * 1024, "S <= 1024");
static_assert(33992 * 4 + 2 * 16 * 4 <= 160 * 1024, "the largest image fits the LDS of a CU");

}  // namespace

extern "C" int abc_stroke_desc_size(void) { return (int)sizeof(abc_stroke_desc); }

extern "C" int abc_normalize_strokes(const abc_stroke_desc* d, abc_stream_t stream) {
    if (!d) return abc_fail(ABC_EINVAL, "normalize_strokes: null descriptor");
    if (!d->src || !d->dst || !d->stats) return abc_fail(ABC_EINVAL, "normalize_strokes: null pointer");
    if (d->B < 1) return abc_fail(ABC_EINVAL, "normalize_strokes: B must be at least 1");
    if (d->S < 8 || d->S > ABC_STROKE_MAX_SIZE || d->S % 8)
        return abc_fail(ABC_EINVAL, "normalize_strokes: S must be a multiple of 8 in 8 .. ABC_STROKE_MAX_SIZE (1024: the image is held in LDS)");
    if (d->radius < 0 || d->radius > 3) return abc_fail(ABC_EINVAL, "normalize_strokes: radius must be 0 .. 3");
    if (d->max_iter < ABC_STROKE_UNTIL_STABLE) return abc_fail(ABC_EINVAL, "normalize_strokes: max_iter must be 0, k >= 1 or ABC_STROKE_UNTIL_STABLE (-1)");
    if (d->drop_isolated != 0 && d->drop_isolated != 1) return abc_fail(ABC_EINVAL, "normalize_strokes: drop_isolated must be 0 or 1");
    if (((uintptr_t)d->src | (uintptr_t)d->dst) % 16) return abc_fail(ABC_EINVAL, "normalize_strokes: src and dst must be 16-byte aligned");
    if (((uintptr_t)d->stats | (uintptr_t)d->skip) % 4) return abc_fail(ABC_EINVAL, "normalize_strokes: stats and skip must be 4-byte aligned");
    if (d->skip && d->skip_stride < 1) return abc_fail(ABC_EINVAL, "normalize_strokes: skip_stride must be at least 1 when skip is given");
    const uintptr_t bytes = (uintptr_t)d->B * d->S * d->S * sizeof(float), s0 = (uintptr_t)d->src, d0 = (uintptr_t)d->dst;
    if (s0 != d0 && s0 < d0 + bytes && d0 < s0 + bytes)
        return abc_fail(ABC_EINVAL, "normalize_strokes: src and dst overlap without being the same buffer");
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((unsigned)d->B);
    // the smallest of three LDS images that holds the framed canvas: more workgroups per CU for the smaller ones
    if (d->S <= 256) hipLaunchKernelGGL((stroke_kernel<2360, 256, 9>), grid, dim3(256), 0, s, *d);
    else if (d->S <= 512) hipLaunchKernelGGL((stroke_kernel<8808, 1024, 9>), grid, dim3(1024), 0, s, *d);
    else hipLaunchKernelGGL((stroke_kernel<33992, 1024, 33>), grid, dim3(1024), 0, s, *d);
    return abc_check_launch("normalize_strokes");
}
