// The heads' weight gradients: the 1x1 kernel abc_wgrad routes a head's descriptor to, and the fused-heads conv2 gradient with its reductions.
//
// Weight gradient of a head's 1x1 convolution: dW[a][b] = sum_p dL[a][p] * act(H[p][b]) with dL the channel-planar
// f32 gradient map (the reference's NCHW logits layout, unet.py:119) and H the NHWC feature map (BN + LeakyReLU +
// dropout applied on load).  HBM-bound on dL (hc x pixels x 4 B, 212 MB for the 360-channel head): dL is already
// pixel-contiguous per row, i.e. exactly the A-operand layout of the MFMA, so it goes global -> registers with each
// lane reading 256 contiguous bytes per 128-pixel chunk (a whole chunk prefetched ahead); only H is staged and
// transposed through LDS.  Workgroup = 8 waves = 4 m-tiles x 2 halves of the 128 b-channels; grid = m-groups x
// K-splits, slabs reduced by abc_wgrad_reduce like every other weight gradient.
#include "wgrad_parts.hpp"
#include "capi_util.hpp"
#include "heads_fused.hpp"

namespace {

struct HeadK {
    const float* dl;
    const float *psc, *psh, *psl;  // per-row transform of dL (scale = d(loss weight), shift 0, slope 1) or null
    const void* q;
    const float *qsc, *qsh, *qsl;
    float* partial;
    float* rowsum;   // [nsplit][Ca_pad] or null
    int HW, hc, ldq, cq_off, nchunks, nsplit, mtiles, Ca_pad;
    float drop_p;
    uint32_t drop_seed;
    const uint32_t* drop_salt;
    unsigned bytesP, bytesQ;
    int cpad_blk;    // BLK: dl = bf16 [chunk][cpad_blk rows][128 pixels], written by the fused heads kernel (heads_fused.hip)
    const uint8_t* keep;   // BLK: the fused kernel's dropout keep bits, 16 bytes per pixel (byte kk + 8 h = channels 16 kk + 8 h ..), or null
    const uint64_t* tiles; // BLK: abc_heads_fused_desc.dl_tiles (bit 4 mt + w of a chunk's word: rows 32 mt .., pixels 32 w .. of dl are written), or null = all are
};

constexpr int HQ_PSW = 320;  // pixel stride of the [pixel][128 channel] bf16 LDS image (wgrad Q layout)
constexpr int HP_RSW = 272;  // row stride of the [dL row][128 pixel] bf16 LDS image: 16 consecutive rows = 16 distinct 16-byte bank slots
constexpr int HEAD_PBUF = 128 * HP_RSW, HEAD_QBUF = 128 * HQ_PSW;
constexpr int HEAD_LDS = 2 * (HEAD_PBUF + HEAD_QBUF) + 3 * 128 * 4;

// dL used to go global -> registers with each lane reading ITS row (256 contiguous bytes per chunk): 64 lanes = 64 rows
// 36 KB apart, i.e. 64 cache lines touched per load instruction for 16 useful bytes each -- the kernel ran at the texture
// addresser's line rate, 7.9 us per 128-pixel chunk (1.7 TB/s for all heads together).  Now both operands are loaded
// coalesced (a wave instruction = two whole 512-byte rows of dL) one chunk ahead, transformed, and written to LDS as bf16:
// dL as [row][pixel] (the A fragment of a K-step is one ds_read_b128), the features as [pixel][channel] (read transposed).
template <bool BLK>
__device__ inline void head_wgrad_body(const HeadK& a, const int split, const int mg) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 31, h = lane >> 5;
    const int mi = wave & 3, nh = wave >> 2;
    if (split >= a.nsplit || mg * 4 >= a.mtiles) return;   // (batched launch: the grid is sized for the largest head)
    const int mt = mg * 4 + mi;
    // (wave-uniform IN A SCALAR REGISTER: an MFMA under a lane-dependent branch is not safe, the instruction ignores EXEC)
    const bool active = __builtin_amdgcn_readfirstlane(mt) < a.mtiles;
    const bool ptrans = a.psc != nullptr;
    const int c0 = (int)((long long)split * a.nchunks / a.nsplit), c1 = (int)((long long)(split + 1) * a.nchunks / a.nsplit);

    const __amdgpu_buffer_rsrc_t rsP = abc_make_rsrc(a.dl, a.bytesP), rsQ = abc_make_rsrc(a.q, a.bytesQ);
    // Q staging: 128 pixels x 16 segments of 8 channels over 512 threads -> 4 per thread, same channel segment always
    const int part = tid & 15, pix0 = tid >> 4;  // segment i: pixel pix0 + 32 i
    const bool qtrans = a.qsc != nullptr;
    float* sCoef = (float*)(smem + 2 * (HEAD_PBUF + HEAD_QBUF));  // [3][128]
    if (qtrans && tid < 128) {
        sCoef[tid] = a.qsc[a.cq_off + tid]; sCoef[128 + tid] = a.qsh[a.cq_off + tid]; sCoef[256 + tid] = a.qsl[a.cq_off + tid];
    }
    // P staging: 128 rows x 32 segments of 4 pixels -> 8 per thread; segment i of a thread: row prow0 + 16 i, pixels 4 pseg ..
    const int pseg = tid & 31, prow0 = tid >> 5;
    float psc[8], psh[8], psl[8], rsum[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int co = mg * 128 + prow0 + 16 * i;
        const bool ok = co < a.hc;
        psc[i] = (ok && ptrans) ? a.psc[co] : 1.f; psh[i] = (ok && ptrans) ? a.psh[co] : 0.f; psl[i] = (ok && ptrans) ? a.psl[co] : 1.f;
        rsum[i] = 0.f;
    }
    __syncthreads();
    const float dscale = a.drop_p > 0.f ? 1.0f / (1.0f - a.drop_p) : 1.0f;
    const uint32_t dseed = a.drop_seed + ((a.drop_p > 0.f && a.drop_salt) ? *a.drop_salt : 0u);
    // TWO chunks of prefetch in flight (two named register sets): with one, an iteration was the loaded HBM latency
    // (~4 us for 96 KB per CU) plus the commit -- the 16 MFMAs per wave of a chunk hide nothing.  Loads are issued
    // unconditionally (past the last chunk with an out-of-range offset: zeros, no traffic) so that vmcnt stays exact.
    u32x4 qreg0[4], preg0[8], qreg1[4], preg1[8];
    // (BLK with the fused kernel's keep bits: the four pixels' mask bytes of this thread's channel segment ride in preg[4],
    //  which the blocked form does not use for d(logits))
    const bool kmask = BLK && a.keep != nullptr && a.drop_p > 0.f;
    const __amdgpu_buffer_rsrc_t rsK = abc_make_rsrc(kmask ? a.keep : (const uint8_t*)a.q, kmask ? (unsigned)a.nchunks * 2048u : 0u);
    const unsigned kbyte = (unsigned)((part & 1) * 8 + (part >> 1));
    const int CPI = a.HW / 128;  // chunks per image
    // BLK with the fused kernel's tile mask (the bond types): the 16 bits of this m-group's four row tiles x the chunk's four
    // 32-pixel quarters, workgroup-uniform and in a scalar register.  d(logits) is zero wherever a bit is clear, and the buffer is
    // NOT written there: a 16-byte piece of P (rows of tile i of the group, pixels of quarter (tid & 15) >> 2) whose bit is clear
    // is loaded with the out-of-range offset (zeros, no traffic -- the memory there is never read).  A chunk with all 16 bits clear
    // adds +0 to every accumulator and row sum (finite features): all of its loads go out of range (issued all the same, so that
    // vmcnt stays exact), and it is neither committed to LDS nor multiplied.  The barriers and the buffer parity do not depend on it.
    auto tmask16 = [&](int c) -> uint32_t {
        if (!BLK || a.tiles == nullptr) return 0xFFFFu;
        if (c >= c1) return 0u;
        return (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(a.tiles[c] >> (16 * mg))) & 0xFFFFu;
    };
    auto issue = [&](int c, const uint32_t m16, u32x4 (&qreg)[4], u32x4 (&preg)[8]) {
        const bool live = c < c1 && m16 != 0u;
        const int b = c / CPI, pp0 = (c - b * CPI) * 128;
        const unsigned qoff = live ? (unsigned)(((unsigned)(c * 128 + pix0) * (unsigned)a.ldq + (unsigned)(a.cq_off + part * 8)) * 2u) : 0x80000000u;
#pragma unroll
        for (int i = 0; i < 4; ++i) qreg[i] = __builtin_amdgcn_raw_buffer_load_b128(rsQ, live ? qoff + (unsigned)(i * 32 * a.ldq * 2) : qoff, 0, 0);
        if constexpr (BLK) {
            if (kmask) {
                const unsigned koff = live ? (unsigned)(c * 128 + pix0) * 16u + kbyte : 0x80000000u;
#pragma unroll
                for (int i = 0; i < 4; ++i) preg[4][i] = (unsigned)__builtin_amdgcn_raw_buffer_load_b8(rsK, live ? koff + (unsigned)(i * 32 * 16) : koff, 0, 0);
            }
            // the chunk's 128 rows are ONE contiguous 32 KB block: 16-byte piece q = tid + 512 i = (row q >> 4, pixels 8 (q & 15) ..)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int row = mg * 128 + (tid >> 4) + 32 * i;
                const bool bit = (m16 >> (4 * i + ((tid & 15) >> 2))) & 1u;   // (row >> 5 = 4 mg + i: tile i of the group)
                const unsigned poff = (live && bit && row < a.cpad_blk) ? (unsigned)((((unsigned)c * (unsigned)a.cpad_blk + (unsigned)row) * 128u + 8u * (tid & 15)) * 2u) : 0x80000000u;
                preg[i] = __builtin_amdgcn_raw_buffer_load_b128(rsP, poff, 0, 0);
            }
        } else {
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int co = mg * 128 + prow0 + 16 * i;
            const unsigned poff = (live && co < a.hc) ? (unsigned)((((unsigned)(b * a.hc + co)) * (unsigned)a.HW + (unsigned)(pp0 + 4 * pseg)) * 4u) : 0x80000000u;
            preg[i] = __builtin_amdgcn_raw_buffer_load_b128(rsP, poff, 0, 0);
        }
        }
    };
    auto commit = [&](int c, char* sP, char* sQ, const u32x4 (&qreg)[4], const u32x4 (&preg)[8]) {
        float qsc[8], qsh[8], qsl[8];
        if (qtrans) {
#pragma unroll
            for (int j = 0; j < 8; ++j) { qsc[j] = sCoef[part * 8 + j]; qsh[j] = sCoef[128 + part * 8 + j]; qsl[j] = sCoef[256 + part * 8 + j]; }
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int pix = pix0 + 32 * i;
            const uint32_t eoff = (uint32_t)(c * 128 + pix) * (uint32_t)a.ldq + (uint32_t)(a.cq_off + part * 8);
            float v[8];
#pragma unroll
            for (int j = 0; j < 4; ++j) { v[2 * j] = __uint_as_float(qreg[i][j] << 16); v[2 * j + 1] = __uint_as_float(qreg[i][j] & 0xFFFF0000u); }
            if (qtrans) {
#pragma unroll
                for (int j = 0; j < 8; ++j) v[j] = abc_act(v[j], qsc[j], qsh[j], qsl[j]);
            }
            if (BLK && kmask) {
                const unsigned kb = preg[4][i];
#pragma unroll
                for (int j = 0; j < 8; ++j) v[j] = ((kb >> j) & 1u) ? v[j] * dscale : 0.f;
            } else if (a.drop_p > 0.f) {
#pragma unroll
                for (int j = 0; j < 8; ++j) v[j] = abc_drop_keep(eoff + j, dseed, a.drop_p) ? v[j] * dscale : 0.f;
            }
            *(bf16x8*)(sQ + pix * HQ_PSW + part * 16) = pack_frag<bf16>(v);
        }
        if constexpr (BLK) {
            // already bf16 in the operand layout: a copy, with the row sums (bias gradient) on the way
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                float f = 0.f;
#pragma unroll
                for (int j = 0; j < 4; ++j) f += __uint_as_float(preg[i][j] << 16) + __uint_as_float(preg[i][j] & 0xFFFF0000u);
                rsum[i] += f;
                *(u32x4*)(sP + ((tid >> 4) + 32 * i) * HP_RSW + (tid & 15) * 16) = preg[i];
            }
            return;
        }
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const bool ok = mg * 128 + prow0 + 16 * i < a.hc;
            float f[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                f[j] = __uint_as_float(preg[i][j]);
                if (ptrans) f[j] = abc_act(f[j], psc[i], psh[i], psl[i]);
                if (!ok) f[j] = 0.f;
            }
            rsum[i] += (f[0] + f[1]) + (f[2] + f[3]);   // sum over pixels of the transformed dL = the conv's bias gradient
            bf16x4 o;
#pragma unroll
            for (int j = 0; j < 4; ++j) o[j] = (bf16)f[j];
            *(bf16x4*)(sP + (prow0 + 16 * i) * HP_RSW + pseg * 8) = o;
        }
    };

    f32x16 acc[2];
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int k = 0; k < 16; ++k) acc[j][k] = 0.f;

    const int sub = 16 * ((lane >> 4) & 1) + 4 * (lane & 3);
    const int qlane = (64 * h + ((lane & 15) >> 2)) * HQ_PSW + sub * 2;  // + 8 kk pixels + b-tile * 64 bytes
    // K order inside a chunk: MFMA K-step kk covers pixels {64 h + 8 kk + j}: the same pixel set for both operands
    const int plane = (mi * 32 + r) * HP_RSW + (64 * h) * 2;              // + 8 kk pixels

    auto compute = [&](const char* sP, const char* sQ) {
#pragma unroll
        for (int kk = 0; kk < 8; ++kk) {
            const bf16x8 fa = *(const bf16x8*)(sP + plane + kk * 16);
            const char* qb = sQ + qlane + kk * 8 * HQ_PSW + nh * 128;
            const bf16x8 fb0 = tr_read8(qb, qb + 4 * HQ_PSW);
            const bf16x8 fb1 = tr_read8(qb + 64, qb + 64 + 4 * HQ_PSW);
            acc[0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa, fb0, acc[0], 0, 0, 0);
            acc[1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa, fb1, acc[1], 0, 0, 0);
        }
    };

    constexpr int BUF = HEAD_PBUF + HEAD_QBUF;
    char* const b0 = smem;
    char* const b1 = smem + BUF;
    // the tile masks of chunks c .. c + 3, read one pair ahead of the loads they steer (issue(c + 2) needs its mask at once)
    uint32_t mA = tmask16(c0), mB = tmask16(c0 + 1), mC = tmask16(c0 + 2), mD = tmask16(c0 + 3);
    issue(c0, mA, qreg0, preg0);
    issue(c0 + 1, mB, qreg1, preg1);
    if (c0 < c1 && mA != 0u) commit(c0, b0, b0 + HEAD_PBUF, qreg0, preg0);
    __syncthreads();
    // even chunks (relative) live in LDS buffer 0 and come from register set 0, odd ones buffer 1 / set 1
    for (int c = c0; c < c1; c += 2) {
        const uint32_t mE = tmask16(c + 4), mF = tmask16(c + 5);
        issue(c + 2, mC, qreg0, preg0);
        if (active && mA != 0u) compute(b0, b0 + HEAD_PBUF);
        if (c + 1 < c1 && mB != 0u) commit(c + 1, b1, b1 + HEAD_PBUF, qreg1, preg1);
        __syncthreads();
        if (c + 1 < c1) {
            issue(c + 3, mD, qreg1, preg1);
            if (active && mB != 0u) compute(b1, b1 + HEAD_PBUF);
            if (c + 2 < c1 && mC != 0u) commit(c + 2, b0, b0 + HEAD_PBUF, qreg0, preg0);
            __syncthreads();
        }
        mA = mC; mB = mD; mC = mE; mD = mF;
    }
    if (BLK && a.rowsum != nullptr) {
        // a row's 16 pieces sit in 16 consecutive lanes
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            float v = rsum[i];
#pragma unroll
            for (int m = 8; m >= 1; m >>= 1) v += __shfl_xor(v, m);
            const int row = mg * 128 + (tid >> 4) + 32 * i;
            if ((tid & 15) == 0 && row < a.Ca_pad) a.rowsum[(size_t)split * a.Ca_pad + row] = v;
        }
    } else if (a.rowsum != nullptr) {
        // a row's 32 segments sit in the 32 lanes of one half-wave
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            float v = rsum[i];
#pragma unroll
            for (int m = 16; m >= 1; m >>= 1) v += __shfl_xor(v, m);
            const int row = mg * 128 + prow0 + 16 * i;
            if (pseg == 0 && row < a.Ca_pad) a.rowsum[(size_t)split * a.Ca_pad + row] = v;
        }
    }
    if (active) {
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            float* out = a.partial + ((size_t)split * a.Ca_pad + mt * 32) * 128 + (nh * 2 + j) * 32 + r;
#pragma unroll
            for (int k = 0; k < 16; ++k) {
                const int arow = (k & 3) + 8 * (k >> 2) + 4 * h;
                out[(size_t)arow * 128] = acc[j][k];
            }
        }
    }
}

// dL planar f32 (x) activated NHWC bf16 features, 1x1, 128 b-channels, whole 128-pixel chunks per image
__global__ __launch_bounds__(512, 2) void head_wgrad_kernel(const HeadK a) { head_wgrad_body<false>(a, blockIdx.x, blockIdx.y); }
// all heads in one launch (blockIdx.z = head), as abc_heads_batch does for the forward and the data gradient
struct HeadWgBatch { HeadK k[8]; int first[9]; };
__global__ __launch_bounds__(512, 2) void head_wgrad_batch_kernel(const HeadWgBatch bt) { head_wgrad_body<false>(bt.k[blockIdx.z], blockIdx.x, blockIdx.y); }
// ... with d(logits) from the fused heads kernel's blocked bf16 buffer (abc_heads_fused_wgrad).  A DENSE one-dimensional grid:
// workgroup id -> (head, K-split, m-group) through the prefix table `first` (m-groups of a split adjacent: they stage the same
// feature chunks).  As a (split, m-group, head) box sized for the largest head the grid was half empty workgroups; every one of
// them still claims a CU's 150 KB of LDS for its moment, the dispatcher dealt the ~256 real ones unevenly -- some CUs ran two
// one after the other while others idled: waves alive for 82 us of a 162 us launch (SQ_WAVE_CYCLES against GRBM_GUI_ACTIVE).
__global__ __launch_bounds__(512, 2) void head_wgrad_blocked_kernel(const HeadWgBatch bt) {
    const int id = blockIdx.x;
    int hd = 0;
    while (hd < 7 && id >= bt.first[hd + 1]) ++hd;
    const HeadK& k = bt.k[hd];
    const int units = (k.mtiles + 3) >> 2, local = id - bt.first[hd];
    head_wgrad_body<true>(k, local / units, local % units);
}

static void head_fill(HeadK& k, const abc_wgrad_desc* d) {
    k.dl = (const float*)d->p.x; k.psc = d->p.scale; k.psh = d->p.shift; k.psl = d->p.slope;
    k.q = d->q.x; k.qsc = d->q.scale; k.qsh = d->q.shift; k.qsl = d->q.slope;
    k.partial = d->partial; k.rowsum = d->rowsum_partial; k.HW = d->Hg * d->Wg; k.hc = d->Ca; k.ldq = d->q.ldx; k.cq_off = d->cq_off;
    k.nchunks = d->B * k.HW / 128; k.nsplit = d->nsplit; k.mtiles = abc_cdiv(d->Ca, 32); k.Ca_pad = k.mtiles * 32;
    k.drop_p = d->q.drop_p; k.drop_seed = d->q.drop_seed; k.drop_salt = d->q.drop_salt;
    k.bytesP = (unsigned)((int64_t)d->B * d->Ca * k.HW * 4); k.bytesQ = (unsigned)((int64_t)d->B * k.HW * d->q.ldx * 2);
    k.cpad_blk = 0; k.keep = nullptr; k.tiles = nullptr;
}

// both operands lie on the gradient's own grid
static bool head_dims_ok(const abc_wgrad_desc* d) { return d->p.Hx == d->Hg && d->p.Wx == d->Wg && d->q.Hx == d->Hg && d->q.Wx == d->Wg; }

}  // namespace

int abc_wgrad_head_ok(const abc_wgrad_desc* d) {
    if (!d->p.planar || d->dtype_p != ABC_F32 || d->dtype_q != ABC_BF16 || d->dtype_c != ABC_BF16) return 0;
    if (d->ntaps != 1 || d->tap_dy[0] != 0 || d->tap_dx[0] != 0 || d->stride != 1 || d->Cb != 128 || d->cp_off != 0) return 0;
    if (d->q.pool || d->q.planar || d->p.pool || d->p.drop_p > 0.f || (d->Hg * d->Wg) % 128) return 0;
    if (d->p.ctot != d->Ca) return 0;
    const int64_t bp = (int64_t)d->B * d->Ca * d->Hg * d->Wg * 4, bq = (int64_t)d->B * d->Hg * d->Wg * d->q.ldx * 2;
    return bp < (int64_t(1) << 31) && bq < (int64_t(1) << 31) && (d->q.ldx % 8) == 0 && (d->cq_off % 8) == 0;
}

int abc_wgrad_head_launch(const abc_wgrad_desc* d, abc_stream_t stream) {
    if (!head_dims_ok(d)) return abc_fail(ABC_EINVAL, "wgrad: dims mismatch");
    HeadK k;
    head_fill(k, d);
    static unsigned long long lds_ok = 0;
    if (int rc = abc_allow_lds((const void*)head_wgrad_kernel, 160 * 1024, &lds_ok)) return rc;
    hipLaunchKernelGGL(head_wgrad_kernel, dim3(d->nsplit, abc_cdiv(k.mtiles, 4)), dim3(512), HEAD_LDS, (hipStream_t)stream, k);
    return abc_check_launch("head_wgrad");
}

// The heads' 1x1 weight gradients (unet.py:70 under autograd) of all heads in one launch: descs[0..n) as abc_wgrad takes
// them one by one (each with its OWN partial / rowsum_partial slabs), n <= 8.  ABC_EUNSUPPORTED unless every one of them
// is served by the heads kernel (the router's first question: abc_wgrad_head_ok).
extern "C" int abc_wgrad_heads_batch(const abc_wgrad_desc* descs, int32_t n, abc_stream_t stream) {
    if (n < 1 || n > 8) return abc_fail(ABC_EINVAL, "wgrad_heads_batch: 1..8 heads");
    HeadWgBatch bt;
    int gx = 0, gy = 0;
    for (int i = 0; i < n; ++i) {
        const abc_wgrad_desc* d = descs + i;
        if (d->nsplit < 1 || d->ntaps != 1 || !abc_wgrad_head_ok(d)) return abc_fail(ABC_EUNSUPPORTED, "wgrad_heads_batch: not a heads' 1x1 weight gradient");
        if (!head_dims_ok(d)) return abc_fail(ABC_EINVAL, "wgrad: dims mismatch");
        head_fill(bt.k[i], d);
        gx = bt.k[i].nsplit > gx ? bt.k[i].nsplit : gx;
        gy = abc_cdiv(bt.k[i].mtiles, 4) > gy ? abc_cdiv(bt.k[i].mtiles, 4) : gy;
    }
    for (int i = n; i < 8; ++i) bt.k[i] = bt.k[0];
    static unsigned long long lds_ok = 0;
    if (int rc = abc_allow_lds((const void*)head_wgrad_batch_kernel, 160 * 1024, &lds_ok)) return rc;
    hipLaunchKernelGGL(head_wgrad_batch_kernel, dim3(gx, gy, n), dim3(512), HEAD_LDS, (hipStream_t)stream, bt);
    return abc_check_launch("wgrad_heads_batch");
}

// K-splits of the blocked weight gradient (heads 5, 6, 7: the five small heads' gradients come out of the fused kernel
// itself): ONE round of ~256 workgroups (the kernel holds 150 KB of LDS) shared out over the heads by the cost of a
// 128-pixel chunk (the feature tile is staged and activated once per workgroup, the d(logits) rows on top)
static void hf_splits(int nchunk, int* nsplit) {
    double cost[HF_NH], tot = 0;
    int units[HF_NH];
    for (int i = 5; i < HF_NH; ++i) {
        units[i] = abc_cdiv(hf_tiles(i), 4);
        cost[i] = 4.0 + 1.5 * (double)hf_tiles(i) / units[i] / 4.0;
        tot += units[i] * cost[i];
    }
    for (int i = 0; i < HF_NH; ++i) {
        if (i < 5) { nsplit[i] = 0; continue; }
        int n = (int)(256.0 * cost[i] / tot);
        n = n < 1 ? 1 : n;
        nsplit[i] = n > nchunk ? nchunk : n;
    }
}

extern "C" int64_t abc_heads_fused_wgrad_floats(const abc_heads_fused_desc* d) {
    int ns[HF_NH];
    const int nchunk = d->B * d->h * d->w / 128;
    hf_splits(nchunk, ns);
    int64_t n = (int64_t)(nchunk + 16) * HF_SMALL_ROWS * 129;      // the fused kernel's partials of the small heads + their first reduction
    for (int i = 5; i < HF_NH; ++i) n += (int64_t)ns[i] * hf_tiles(i) * 32 * (128 + 1);
    return n;
}

// slabs -> conv2.weight.grad / conv2.bias.grad: packed rows back to channels (hf_row_of_chan), times the head's loss factor
// (abc_loss_finalize's chan_scale), fixed summation order.  Heads 5-7: the K-split slabs of the blocked kernel; heads 0-4: the
// per-chunk partial rows [chunk][21][128 weights | 1 bias] the fused kernel left.
struct HeadFusedRedK {
    const float* partial[HF_NH]; const float* rowsum[HF_NH];
    float* dw[HF_NH]; float* db[HF_NH];
    const float* chan_scale;
    const float* small2;
    int nsplit[HF_NH], chan_off[HF_NH];
};
// first stage for the small heads: [nchunk][21][129] -> 16 row slices [16][21][129] (grid = 21 x 16: enough loads in flight)
__global__ __launch_bounds__(192) void head_fused_small_reduce_kernel(const float* part, int nchunk, float* out) {
    const int row = blockIdx.x, sl = blockIdx.y, c2 = threadIdx.x;
    if (c2 >= 129) return;
    const float* p = part + (size_t)row * 129 + c2;
    const size_t step = (size_t)HF_SMALL_ROWS * 129;
    float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
    int k = sl;
    for (; k + 48 < nchunk; k += 64) {
        s0 += p[(size_t)k * step]; s1 += p[(size_t)(k + 16) * step]; s2 += p[(size_t)(k + 32) * step]; s3 += p[(size_t)(k + 48) * step];
    }
    for (; k < nchunk; k += 16) s0 += p[(size_t)k * step];
    out[((size_t)sl * HF_SMALL_ROWS + row) * 129 + c2] = (s0 + s1) + (s2 + s3);
}
__global__ __launch_bounds__(128) void head_fused_reduce_kernel(const HeadFusedRedK a) {
    const int head = blockIdx.y, ch = blockIdx.x, ci = threadIdx.x;
    if (ch >= hf_ch(head)) return;
    const float cs = a.chan_scale[a.chan_off[head] + ch];
    if (head < 5) {
        // 16 row slices of the per-chunk partials were summed by head_fused_small_reduce_kernel: [16][21][129]
        const float* p = a.small2 + (size_t)(hf_small_row0(head) + ch) * 129;
        for (int c2 = ci; c2 < 129; c2 += 128) {
            float s = 0.f;
#pragma unroll
            for (int k = 0; k < 16; ++k) s += p[(size_t)k * HF_SMALL_ROWS * 129 + c2];
            if (c2 < 128) a.dw[head][ch * 128 + c2] = s * cs; else a.db[head][ch] = s * cs;
        }
        return;
    }
    const int cpad = hf_tiles(head) * 32, row = hf_row_of_chan(head, ch);
    const float* p = a.partial[head] + (size_t)row * 128 + ci;
    float s0 = 0.f, s1 = 0.f;
    int k = 0;
    for (; k + 2 <= a.nsplit[head]; k += 2) { s0 += p[(size_t)k * cpad * 128]; s1 += p[(size_t)(k + 1) * cpad * 128]; }
    if (k < a.nsplit[head]) s0 += p[(size_t)k * cpad * 128];
    a.dw[head][ch * 128 + ci] = (s0 + s1) * cs;
    if (ci == 0) {
        float b = 0.f;
        for (int q = 0; q < a.nsplit[head]; ++q) b += a.rowsum[head][(size_t)q * cpad + row];
        a.db[head][ch] = b * cs;
    }
}

// conv2.weight.grad / conv2.bias.grad of all heads from the fused kernel's outputs (unet.py:70 under autograd):
// dW2[c][ci] = factor_c * sum_p dL[c][p] * act(feat[p][ci]); run after abc_loss_finalize (chan_scale)
extern "C" int abc_heads_fused_wgrad(const abc_heads_fused_desc* d, abc_stream_t stream) {
    const int HW = d->h * d->w, nchunk = d->B * HW / 128;
    if (HW % 128 || d->ld % 8 || (int64_t)d->B * HW * d->ld * 2 >= (int64_t(1) << 31))
        return abc_fail(ABC_EUNSUPPORTED, "heads_fused_wgrad: whole 128-pixel chunks, feature buffer below 2 GB");
    int ns[HF_NH];
    hf_splits(nchunk, ns);
    HeadWgBatch bt;
    HeadFusedRedK rk;
    float* ws = d->wgrad_work + (size_t)nchunk * HF_SMALL_ROWS * 129;
    rk.small2 = ws; ws += 16 * HF_SMALL_ROWS * 129;
    size_t row0 = 0;
    for (int i = 0; i < HF_NH; ++i) {
        const int cpad = hf_tiles(i) * 32;
        rk.dw[i] = d->dw2[i]; rk.db[i] = d->db2[i]; rk.nsplit[i] = ns[i]; rk.chan_off[i] = d->chan_off[i];
        rk.partial[i] = nullptr; rk.rowsum[i] = nullptr;
        if (i >= 5) {
            HeadK& k = bt.k[i - 5];
            k.dl = (const float*)((const bf16*)d->dl + row0 * (size_t)nchunk * 128);
            k.psc = k.psh = k.psl = nullptr;
            k.q = d->feat; k.qsc = d->scale; k.qsh = d->shift; k.qsl = d->slope;
            k.partial = ws; ws += (size_t)ns[i] * cpad * 128;
            k.rowsum = ws; ws += (size_t)ns[i] * cpad;
            k.HW = HW; k.hc = hf_ch(i); k.ldq = d->ld; k.cq_off = 128 * i; k.nchunks = nchunk; k.nsplit = ns[i];
            k.mtiles = hf_tiles(i); k.Ca_pad = cpad;
            k.drop_p = d->drop_p; k.drop_seed = d->drop_seed; k.drop_salt = d->drop_salt;
            k.bytesP = (unsigned)((size_t)nchunk * cpad * 128 * 2); k.bytesQ = (unsigned)((int64_t)d->B * HW * d->ld * 2);
            k.cpad_blk = cpad;
            k.keep = d->keep_mask != nullptr ? (const uint8_t*)d->keep_mask + (size_t)(i - 5) * nchunk * 2048 : nullptr;
            k.tiles = i == 5 ? d->dl_tiles : nullptr;   // (the bond types: the only head whose tiles the fused pass may leave unwritten)
            if ((size_t)nchunk * cpad * 128 * 2 >= (size_t(1) << 31)) return abc_fail(ABC_EUNSUPPORTED, "heads_fused_wgrad: d(logits) block above 2 GB");
            rk.partial[i] = k.partial; rk.rowsum[i] = k.rowsum;
        }
        row0 += cpad;
    }
    for (int i = 3; i < 8; ++i) bt.k[i] = bt.k[0];
    bt.first[0] = 0;
    for (int i = 0; i < 8; ++i) bt.first[i + 1] = bt.first[i] + (i < 3 ? bt.k[i].nsplit * abc_cdiv(bt.k[i].mtiles, 4) : 0);
    rk.chan_scale = d->chan_scale;
    static unsigned long long lds_ok = 0;
    if (int rc = abc_allow_lds((const void*)head_wgrad_blocked_kernel, 160 * 1024, &lds_ok)) return rc;
    hipLaunchKernelGGL(head_wgrad_blocked_kernel, dim3(bt.first[8]), dim3(512), HEAD_LDS, (hipStream_t)stream, bt);
    if (int rc = abc_check_launch("heads_fused_wgrad")) return rc;
    hipLaunchKernelGGL(head_fused_small_reduce_kernel, dim3(HF_SMALL_ROWS, 16), dim3(192), 0, (hipStream_t)stream, (const float*)d->wgrad_work, nchunk, (float*)rk.small2);
    hipLaunchKernelGGL(head_fused_reduce_kernel, dim3(360, HF_NH), dim3(128), 0, (hipStream_t)stream, rk);
    return abc_check_launch("heads_fused_wgrad_reduce");
}
