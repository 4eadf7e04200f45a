// Weight gradient of a tap-list convolution on the gfx950 matrix cores.
//
//   dW[t][a][b] = sum over pixels p of  P[p][a] * Q[stride*p + d_t][b]
//
// GEMM view per tap: M = a-channels, N = b-channels, K = pixels (split-K over 8x16 spatial
// patches across workgroups; every workgroup writes its own f32 slab and abc_wgrad_reduce sums
// the slabs in a fixed order -> bitwise reproducible, no atomics).
// Both operands have the reduction index (pixel) as the SLOW memory axis (NHWC), so the
// [pixel][channel] LDS images are read column-wise: in bf16 mode with the hardware-transposing
// ds_read_b64_tr_b16 (4 pixels x 16 channels per 16-lane group), in exact-f32 mode with plain
// ds_read_b32 (v_mfma_f32_32x32x2_f32 wants one value per lane).  One K-step = one 16-pixel row
// segment of the patch; the un-shifted operand's fragment is read once per K-step and reused by
// all taps.
//
// Workgroup = 8 waves (one per CU, two per SIMD) arranged AT x BT x RS: AT*BT 32x32 output tile
// pairs (every wave keeps all <= 9 taps of its pair: 144 accumulator VGPRs) and RS-way split of the
// patch rows (folded through LDS at the end).  Patches are double-buffered in LDS and the next patch's
// global loads are issued before / committed after the MFMA block (split-phase, T14), with the
// BatchNorm coefficients of both operands held in an LDS table.
//
// Reference ops covered: autograd of nn.Conv2d / nn.ConvTranspose2d weights
// (unet.py:12,15,44,66,70 under loss.backward(), train.py:140).
#include "wgrad_parts.hpp"
#include "capi_util.hpp"
#include "reduce_bn.hpp"
#include "conv_fast.hpp"
#include <stddef.h>
#include <stdlib.h>
#include <algorithm>

namespace {

constexpr int MAXT_FAST = 9;  // taps per workgroup (accumulator budget: 9 x 16 VGPRs)
constexpr int MAXT_SLOW = 5;  // the general loader needs the registers: fewer taps per workgroup, more tap groups
constexpr int WTHR_HOST = 512;  // 8 waves per workgroup

struct WgK {
    ActSrc p, q;
    float* partial;
    int B, Hg, Wg, Hq, Wq;
    int cp_off, Ca, cq_off, Cb, Ca_pad, Cb_pad;
    int ntaps, tgw, nsplit, npatch, tiles_x, tiles_y;
    int dy_min, dx_min, HH, HW, PSWP, PSWQ, sP_bytes, sQ_bytes, coef_off, cstrP, cstrQ, nta, ntb, fast_p, fast_q, nbuf;
    unsigned bytesP2;        // (here, not beside bytesP: this order keeps the argument offsets the kernels were tuned with -- a shift of
                             //  the fields below by four bytes changed their register allocation, and the 4 x 2 dual form spilled)
    int magicQ, k3;
    unsigned mg_tx, mg_ty;   // ceil(2^32 / tiles_x), ceil(2^32 / tiles_y): the patch index is split by two multiply-highs (scalar), not divisions
    int regP;                // P's patches are whole and P has no halo: its segment offsets are affine in the segment index
    int qtab_off;            // > 0: LDS byte offset of Q's segment table (HaloFetch::table_setup): whole patches, 3x3 halo, stride 1
    unsigned bytesP, bytesQ;
    const void* p2; void* p_out; int ld_p2, cp2_off, ld_pout;  // BN-backward correction fused into the load of P (DUAL)
    int8_t ty[ABC_MAX_TAPS], tx[ABC_MAX_TAPS];
};
static_assert(sizeof(WgK) == 448 && offsetof(WgK, bytesP2) == 284 && offsetof(WgK, k3) == 292 && offsetof(WgK, qtab_off) == 308 &&
              offsetof(WgK, p2) == 320 && offsetof(WgK, ty) == 348, "WgK: the argument offsets the kernels were tuned with");

// general (pool / dropout / planar / ragged-tail) loader kept out of line: inlined next to the accumulators and the
// prefetch registers it makes the register allocator spill inside the MFMA loop
template <typename T, typename CT, int CW>
__device__ inline void stage_slow(char* dst, int RS, int PS, int HH, int HW, int b, int iy0, int ix0, int Hin, int Win,
                                                     const ActSrc* s, int c0, int tid, int cvalid, int nthr) {
    stage_halo<T, CT, CW>(dst, RS, PS, HH, HW, b, iy0, ix0, Hin, Win, *s, c0, tid, nthr, cvalid);
}

// TS ("tap split", one 32x32 tile pair, more than 9 taps -- unet2's 5x5 convolutions): the 8 waves split the TAPS instead
// of the patch rows (wave w owns taps w, w + 8, w + 16, w + 24: <= 4 accumulators), every wave walks the whole patch, and
// ONE workgroup pass covers all taps.  With the row split 25 taps ran as 3 tap groups (grid.y) that each re-staged both
// operands: 596 MB fetched per launch against 302 MB algorithmic (profiles/r01_f_unet2_pmc_summary.json).
template <typename PT, typename QT, typename CT, int AT, int BT, int STRIDE, bool FAST, int PM, bool K3, bool DUAL = false, bool TS = false>
__global__ __launch_bounds__(WTHR_HOST, 2) void wgrad_kernel(const WgK a) {
    constexpr int WTHR = WTHR_HOST;
    static_assert(!TS || (AT == 1 && BT == 1 && FAST && !K3 && sizeof(CT) == 2), "tap split: one bf16 tile pair on the prefetch path");
    constexpr int MAXT = TS ? 4 : (FAST ? MAXT_FAST : MAXT_SLOW);
    constexpr int RSPLIT = TS ? 1 : (WTHR / 64) / (AT * BT);   // waves sharing one tile pair, splitting the patch rows
    constexpr int PROWS = 8 * PM;           // patch rows (x 16 columns)
    constexpr int ROWS = PROWS / RSPLIT;    // patch rows per wave
    constexpr int CWP = AT * 32, CWQ = BT * 32;
    constexpr int NPF_P = (PROWS * 16 * (CWP / Frag<CT>::NV) + WTHR - 1) / WTHR;
    constexpr int NPF_Q = (PM > 1 || STRIDE == 2) ? 5 : ((sizeof(CT) == 2) ? 4 : 6);  // (stride 2: 17 x 33 halo pixels)
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int buf_bytes = a.sP_bytes + a.sQ_bytes;
    float* sCoefP = (float*)(smem + a.coef_off);
    float* sCoefQ = sCoefP + 3 * a.cstrP;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 31, h = lane >> 5;

    // blocks with equal (blockIdx.x % 8) share an XCD and its L2: give each XCD a contiguous range of logical ids, so that
    // the nta x ntb workgroups of one split -- which re-read the same P / Q patches -- hit in L2 instead of going out again
    int id = abc_xcd_remap(blockIdx.x, gridDim.x);
    const int bt = id % a.ntb; id /= a.ntb;
    const int at = id % a.nta; id /= a.nta;
    const int split = id;
    const int t0 = blockIdx.y * a.tgw;
    const int tcnt = min(a.tgw, a.ntaps - t0);

    const int pair = TS ? 0 : wave / RSPLIT, rs = TS ? 0 : wave % RSPLIT;
    // tap owned by accumulator slot j (TS: wave-uniform, kept scalar)
    const int wave_u = __builtin_amdgcn_readfirstlane(wave);
    auto tap_of = [&](int j) { return TS ? wave_u + 8 * j : t0 + j; };
    auto tap_ok = [&](int j) { return TS ? (wave_u + 8 * j < a.ntaps) : (j < tcnt); };
    const int ai = pair / BT, bi = pair % BT;
    const int row_lo = rs * ROWS;
    const int PSWP = a.PSWP, PSWQ = a.PSWQ;
    const int ca0 = at * CWP, cb0 = bt * CWQ;          // first channel of the workgroup's a / b range
    const int cvalP = a.Ca - ca0, cvalQ = a.Cb - cb0;  // valid channels from there

    // ---- BatchNorm coefficient tables of both operands (relative channel index)
    // FAST: both operands are plain NHWC tensors -> split-phase prefetch; otherwise (pool / dropout / planar /
    // ragged channel tail on either operand) both are staged synchronously by the general loader.  Two separate
    // instantiations: inlining the general loader next to the prefetch registers makes the allocator spill.
    const bool coefP = FAST && a.p.scale != nullptr, coefQ = FAST && a.q.scale != nullptr;
    if (coefP)
        for (int i = tid; i < min(CWP, cvalP); i += WTHR) {
            sCoefP[i] = a.p.scale[a.cp_off + ca0 + i]; sCoefP[a.cstrP + i] = a.p.shift[a.cp_off + ca0 + i];
            sCoefP[2 * a.cstrP + i] = a.p.slope[a.cp_off + ca0 + i];
        }
    if (coefQ)
        for (int i = tid; i < min(CWQ, cvalQ); i += WTHR) {
            sCoefQ[i] = a.q.scale[a.cq_off + cb0 + i]; sCoefQ[a.cstrQ + i] = a.q.shift[a.cq_off + cb0 + i];
            sCoefQ[2 * a.cstrQ + i] = a.q.slope[a.cq_off + cb0 + i];
        }

    f32x16 acc[MAXT];
#pragma unroll
    for (int t = 0; t < MAXT; ++t)
#pragma unroll
        for (int k = 0; k < 16; ++k) acc[t][k] = 0.f;
    unsigned* const qtab = (unsigned*)(smem + a.qtab_off);

    int tapoff[MAXT];  // LDS byte offset of each tap inside the Q halo
#pragma unroll
    for (int t = 0; t < MAXT; ++t) tapoff[t] = tap_ok(t) ? (a.ty[tap_of(t)] * a.HW + a.tx[tap_of(t)]) * PSWQ : 0;

    // per-lane channel byte offsets inside a pixel
    int pch, qch;
    if constexpr (sizeof(CT) == 2) {
        const int sub = 16 * ((lane >> 4) & 1) + 4 * (lane & 3);
        pch = (ai * 32 + sub) * 2;
        qch = (bi * 32 + sub) * 2;
    } else {
        pch = (ai * 32 + r) * 4;
        qch = (bi * 32 + r) * 4;
    }

    HaloFetch<PT, CT, CWP, FAST ? NPF_P : 1, WTHR> pp;
    HaloFetch<QT, CT, CWQ, FAST ? NPF_Q : 1, WTHR> pq;
    const __amdgpu_buffer_rsrc_t rsP = abc_make_rsrc(a.p.x, a.bytesP), rsQ = abc_make_rsrc(a.q.x, a.bytesQ);
    // DUAL: P = ca * g + cb * y_raw + cc (the BatchNorm-backward correction, abc_bn_bwd_desc.ca/cb/cc), g and y_raw
    // fetched side by side; the corrected values go to LDS for the MFMAs and (from the b-tile-0 workgroups) to p_out
    // for the data-gradient conv: one pass over g and y instead of abc_bn_apply_bwd's read-modify-write plus a re-read
    HaloFetch<PT, CT, CWP, (FAST && DUAL) ? NPF_P : 1, WTHR> pp2;
    const __amdgpu_buffer_rsrc_t rsP2 = abc_make_rsrc(DUAL ? a.p2 : a.p.x, DUAL ? a.bytesP2 : a.bytesP);
    const HaloGeom gP2 = {PROWS, 16, 4097, a.Hg, a.Wg, a.Hg, a.Wg, a.ld_p2};
    const HaloGeom gP = {PROWS, 16, 4097, a.Hg, a.Wg, a.p.Hx, a.p.Wx, a.p.ldx};
    const HaloGeom gQ = {a.HH, a.HW, a.magicQ, a.Hq, a.Wq, a.q.Hx, a.q.Wx, a.q.ldx};

    // (patch < 2^16 and tiles <= 2^12: the multiply-high by ceil(2^32 / d) is the exact quotient; wave-uniform, stays on the scalar
    //  unit -- the two runtime divisions cost ~50 vector instructions per call, twice per patch)
    // Q's segment geometry once per kernel (FAST && the host found room for the table: a.qtab_off)
    // (compiled into the instantiations whose waves own a tile pair each: the narrow-layer forms are at their register limit)
    constexpr bool QTAB = FAST && K3 && STRIDE == 1 && !TS && sizeof(CT) == 2 && sizeof(QT) == 2 && AT * BT >= 4;
    unsigned qmask = 0;
    if constexpr (QTAB) {
        if (a.qtab_off) qmask = pq.table_setup(qtab, gQ, a.HW * PSWQ, PSWQ, tid, cvalQ, PROWS, a.dy_min, a.dx_min);
    }
    auto patch_origin = [&](int patch, int& b, int& gy0, int& gx0) {
        const unsigned pid = (unsigned)patch;
        // (a divisor of 1 has no 32-bit magic: ceil(2^32 / 1) = 2^32)
        const unsigned q1 = a.tiles_x == 1 ? pid : __umulhi(pid, a.mg_tx);
        const unsigned tx_i = pid - q1 * (unsigned)a.tiles_x;
        const unsigned q2 = a.tiles_y == 1 ? q1 : __umulhi(q1, a.mg_ty);
        const unsigned ty_i = q1 - q2 * (unsigned)a.tiles_y;
        b = (int)q2; gy0 = (int)ty_i * PROWS; gx0 = (int)tx_i * 16;
    };
    // SPREAD: the next patch's loads are not issued as one batch in front of the MFMA block but a few at a time between
    // its K-steps.  A CU's memory pipeline holds far less than a patch (55 .. 87 KB from 8 waves): the waves of a batch sat
    // in their load instructions until most of the data had come back, so loads and MFMAs never overlapped (ablations on the
    // eight heads' merged weight gradient: loads only 193 us, MFMAs only 214 us, both 329 us, with the commit 571 us).
    constexpr bool SPREAD = FAST && K3 && sizeof(CT) == 2 && !TS && ROWS >= 4;
    auto prepare = [&](int patch, bool live) {
        int b, gy0, gx0;
        patch_origin(patch, b, gy0, gx0);
        if constexpr (FAST) {
            // all address arithmetic first (see HaloFetch::prepare)
            if (live) {
                if (a.regP) pp.prepare_regular(gP, b, gy0, gx0, a.cp_off + ca0, tid, cvalP);
                else pp.prepare(gP, b, gy0, gx0, a.cp_off + ca0, tid, cvalP);
                if constexpr (DUAL) {
                    // (g and y_raw: same patch, same segments; with equal pixel strides the offsets differ by a constant)
                    if (a.ld_p2 == a.p.ldx && a.p.Hx == a.Hg && a.p.Wx == a.Wg)
                        pp2.prepare_like(pp, (unsigned)((a.cp2_off - a.cp_off) * (int)sizeof(PT)));
                    else
                        pp2.prepare(gP2, b, gy0, gx0, a.cp2_off + ca0, tid, cvalP);
                }
                if (QTAB && a.qtab_off) {
                    const unsigned sbase = (unsigned)(((b * a.q.Hx + gy0 + a.dy_min) * a.q.Wx + gx0 + a.dx_min) * a.q.ldx + a.cq_off + cb0) * (unsigned)sizeof(QT);
                    const unsigned border = (gy0 == 0 ? 0x1Fu << 5 : 0u) | (gy0 + PROWS == a.Hq ? 0x1Fu << 10 : 0u) | (gx0 == 0 ? 0x1Fu << 15 : 0u) |
                                            (gx0 + 16 == a.Wq ? 0x1Fu << 20 : 0u);
                    pq.prepare_tab(qtab, qmask, sbase, border, tid);
                } else {
                    pq.prepare(gQ, b, gy0 * STRIDE + a.dy_min, gx0 * STRIDE + a.dx_min, a.cq_off + cb0, tid, cvalQ);
                }
            } else {
                pp.prepare_none();
                if constexpr (DUAL) pp2.prepare_none();
                pq.prepare_none();
            }
        }
    };
    auto fire_all = [&]() {
        if constexpr (FAST) {
            __builtin_amdgcn_sched_barrier(0);
            pp.fire(rsP);
            if constexpr (DUAL) pp2.fire(rsP2);
            pq.fire(rsQ);
            __builtin_amdgcn_sched_barrier(0);
        }
    };
    // (over the FIRST half of the K-steps, so that the last load has the second half to come back in)
    constexpr int NPH = ROWS / 2;
    auto fire_slice = [&](int phase) {   // phase < NPH
        if constexpr (FAST) {
            pp.fire_slice(rsP, 0, phase, NPH);
            if constexpr (DUAL) pp2.fire_slice(rsP2, NPF_P, phase, NPH);
            pq.fire_slice(rsQ, DUAL ? 2 * NPF_P : NPF_P, phase, NPH);
        }
    };
    auto issue = [&](int patch) {
        prepare(patch, true);
        fire_all();
    };
    auto commit = [&](int patch, char* buf) {
        int b, gy0, gx0;
        patch_origin(patch, b, gy0, gx0);
        char* sP = buf;
        char* sQ = buf + a.sP_bytes;
        if constexpr (FAST) {
            if constexpr (DUAL) {
                constexpr int NV = Frag<CT>::NV;
                const int SEGS = pp.live_segs(cvalP);   // same thread -> segment mapping as HaloFetch::issue (a power of two)
                const int ssh = pp.live_shift(SEGS);
                const int lt = abc_launder(tid);
                const int part = lt & (SEGS - 1), cch = part * NV;
                const bool chan = cch < cvalP;
                float ka[NV], kb[NV], kc[NV];
                const float kzero[NV] = {};
#pragma unroll
                for (int j = 0; j < NV; ++j) { ka[j] = sCoefP[cch + j]; kc[j] = sCoefP[a.cstrP + cch + j]; kb[j] = sCoefP[2 * a.cstrP + cch + j]; }
                const bool store = (bt == 0) && (blockIdx.y == 0) && a.p_out != nullptr;
                // dY goes out through a buffer store with a 32-bit offset (an out-of-range offset drops it: no branch, no 64-bit
                // address arithmetic per segment; soffset 0 -- the store form LLVM's hazard recogniser covers)
                const __amdgpu_buffer_rsrc_t rsO = abc_make_rsrc(store ? a.p_out : a.p.x, store ? (unsigned)((size_t)a.B * a.Hg * a.Wg * a.ld_pout * sizeof(CT)) : 0u);
                const int obase = ((b * a.Hg + gy0) * a.Wg + gx0) * a.ld_pout + ca0 + cch;
#pragma unroll
                for (int i = 0; i < NPF_P; ++i) {
                    const int sidx = lt + i * WTHR;
                    if (sidx < PROWS * 16 * SEGS) {
                        const int pix = sidx >> ssh, hy = pix >> 4, hx = pix & 15;
                        float v1[NV], v2[NV];
                        pp.raw[i].get(v1); pp2.raw[i].get(v2);
                        const bool in = chan && ((pp.inb >> i) & 1u);
                        abc_fma2_n<NV>(v1, v2, ka, kb, kc);
                        typename Frag<CT>::type f = pack_frag<CT>(v1);
                        if (!in) f = pack_frag<CT>(kzero);      // (a select on the packed words: 4 instead of 8)
                        *(typename Frag<CT>::type*)(sP + (hy * 16 + hx) * PSWP + part * 16) = f;
                        static_assert(sizeof(f) == 16, "one 16-byte segment");
                        __builtin_amdgcn_raw_buffer_store_b128(*(u32x4*)&f, rsO,
                                                               (store && in) ? (unsigned)(obase + (hy * a.Wg + hx) * a.ld_pout) * (unsigned)sizeof(CT) : 0xFFFFFFF0u, 0, 0);
                    }
                }
            } else {
                pp.commit(sP, 16 * PSWP, PSWP, gP, coefP ? sCoefP : nullptr, a.cstrP, tid, cvalP);
            }
            if (QTAB && a.qtab_off) pq.commit_tab(sQ, qtab, qmask, coefQ ? sCoefQ : nullptr, a.cstrQ, tid, cvalQ);
            else pq.commit(sQ, a.HW * PSWQ, PSWQ, gQ, coefQ ? sCoefQ : nullptr, a.cstrQ, tid, cvalQ);
        } else {
            stage_slow<PT, CT, CWP>(sP, 16 * PSWP, PSWP, PROWS, 16, b, gy0, gx0, a.Hg, a.Wg, &a.p, a.cp_off + ca0, tid, cvalP, WTHR);
            stage_slow<QT, CT, CWQ>(sQ, a.HW * PSWQ, PSWQ, a.HH, a.HW, b, gy0 * STRIDE + a.dy_min, gx0 * STRIDE + a.dx_min, a.Hq, a.Wq,
                                    &a.q, a.cq_off + cb0, tid, cvalQ, WTHR);
        }
    };

    if constexpr (FAST) {
        // zero both patch buffers once: channel padding (Ca / Cb below the 32-wide tile) is never written again
        if (cvalP < CWP || cvalQ < CWQ) {
            const f32x4 z = {0.f, 0.f, 0.f, 0.f};
            for (int i = tid * 16; i < a.nbuf * buf_bytes; i += WTHR * 16) *(f32x4*)(smem + i) = z;
        }
    }
    __syncthreads();  // coefficient tables visible
    // it = -1 is the prologue (stage the first patch, no compute): one call site for issue / commit
    int patch = split - a.nsplit;
    for (int it = -1; it < 0 || patch < a.npatch; ++it, patch += a.nsplit) {
        const int next = patch + a.nsplit;
        const bool has_next = next < a.npatch;
        if constexpr (SPREAD) {
            prepare(has_next ? next : patch, has_next);
            if (it < 0) fire_all();     // prologue: nothing to hide behind
        } else {
            if (has_next) issue(next);
        }
        if (it >= 0) {
            const char* sP = smem + ((a.nbuf == 2) ? (it & 1) * buf_bytes : 0);
            const char* sQ = sP + a.sP_bytes;
            // ROT (stride 1, fully unrolled K-steps): tap (dy, dx) of patch row r reads the SAME fragment as tap (dy - 1, dx) of row
            // r + 1 (same halo pixels, same lanes), so only the three fragments of the NEW halo row are read per K-step and the
            // other six are carried in their registers: tap t of K-step rr lives in slot (t + 3 rr) mod 9.  4 instead of 10
            // transposing LDS reads per K-step (SQ_WAIT_INST_LDS 7.9 M -> 2.6 M wave-cycles per launch; the launch itself gains 4 %:
            // the LDS was not what bound the matrix phase -- profiles/r04_wgrad_pingpong.md).
            constexpr bool ROT = SPREAD && STRIDE == 1;
            bf16x8 fbr[9];
#pragma unroll(SPREAD ? ROWS : 1)
            for (int rr = 0; rr < ROWS; ++rr) {
                const int row = row_lo + rr;
                if constexpr (sizeof(CT) == 2 && FAST && K3 && ROT) {
                    constexpr int HW3 = 15 * STRIDE + 3;
                    constexpr int PQ = CWQ == 32 ? 64 : (CWQ == 64 ? 192 : 320);
                    constexpr int PP = CWP == 32 ? 64 : (CWP == 64 ? 192 : 320);
                    const int kq = 8 * h + ((lane & 15) >> 2);
                    const char* pa = sP + (row * 16 + kq) * PP + pch;
                    const char* qb = sQ + (row * HW3 + kq) * PQ + qch;
                    const bf16x8 fa = tr_read8(pa, pa + 4 * PP);
#pragma unroll
                    for (int t = 0; t < 9; ++t) {
                        if (rr == 0 || t >= 6) {
                            const int off = ((t / 3) * HW3 + (t % 3)) * PQ;
                            fbr[(t + 3 * rr) % 9] = tr_read8(qb + off, qb + off + 4 * PQ);
                        }
                    }
                    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                    for (int t = 0; t < 9; ++t) acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa, fbr[(t + 3 * rr) % 9], acc[t], 0, 0, 0);
                    __builtin_amdgcn_sched_barrier(0);
                    if (rr < NPH) fire_slice(rr);   // (unconditional: without a next patch the offsets are out of range)
                    __builtin_amdgcn_sched_barrier(0);
                } else if constexpr (sizeof(CT) == 2 && FAST && K3) {
                    {
                        // the usual case, a full 3x3 tap square: tap offsets are immediates, all 10 fragments of the
                        // K-step are read first (one wait), then 9 MFMAs back to back; the generic loop below pays a
                        // branch, two address adds and an exposed LDS round trip per tap
                        constexpr int HW3 = 15 * STRIDE + 3;
                        constexpr int PQ = CWQ == 32 ? 64 : (CWQ == 64 ? 192 : 320);
                        constexpr int PP = CWP == 32 ? 64 : (CWP == 64 ? 192 : 320);
                        const int kq = 8 * h + ((lane & 15) >> 2);
                        const char* pa = sP + (row * 16 + kq) * PP + pch;
                        const char* qb = sQ + ((row * STRIDE) * HW3 + kq * STRIDE) * PQ + qch;
                        const bf16x8 fa = tr_read8(pa, pa + 4 * PP);
                        bf16x8 fb[9];
#pragma unroll
                        for (int t = 0; t < 9; ++t) {
                            constexpr int dummy = 0; (void)dummy;
                            const int off = ((t / 3) * HW3 + (t % 3)) * PQ;
                            fb[t] = tr_read8(qb + off, qb + off + 4 * STRIDE * PQ);
                        }
                        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                        for (int t = 0; t < 9; ++t) acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa, fb[t], acc[t], 0, 0, 0);
                        __builtin_amdgcn_sched_barrier(0);
                        if constexpr (SPREAD) {
                            if (rr < NPH) fire_slice(rr);   // (unconditional: without a next patch the offsets are out of range)
                            __builtin_amdgcn_sched_barrier(0);
                        }
                    }
                } else if constexpr (sizeof(CT) == 2) {
                    // lane supplies the address of pixel k = 8h + 4q + ((lane&15)>>2), 4 channels
                    const int kq = 8 * h + ((lane & 15) >> 2);
                    const char* pa = sP + (row * 16 + kq) * PSWP + pch;
                    const bf16x8 fa = tr_read8(pa, pa + 4 * PSWP);
                    const char* qb = sQ + ((row * STRIDE) * a.HW + kq * STRIDE) * PSWQ + qch;
#pragma unroll
                    for (int t = 0; t < MAXT; ++t) {
                        if (tap_ok(t)) {
                            const bf16x8 fb = tr_read8(qb + tapoff[t], qb + tapoff[t] + 4 * STRIDE * PSWQ);
                            acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa, fb, acc[t], 0, 0, 0);
                        }
                    }
                } else {
#pragma unroll 2
                    for (int s = 0; s < 8; ++s) {
                        const int k = 2 * s + h;
                        const float fa = *(const float*)(sP + (row * 16 + k) * PSWP + pch);
                        const char* qb = sQ + ((row * STRIDE) * a.HW + k * STRIDE) * PSWQ + qch;
#pragma unroll
                        for (int t = 0; t < MAXT; ++t) {
                            if (t < tcnt) {
                                const float fb = *(const float*)(qb + tapoff[t]);
                                acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa, fb, acc[t], 0, 0, 0);
                            }
                        }
                    }
                }
            }
            if (a.nbuf == 1) __syncthreads();  // single buffer: everyone is done reading before it is refilled
        }
        if (has_next) commit(next, smem + ((a.nbuf == 2) ? ((it + 1) & 1) * buf_bytes : 0));
        __syncthreads();
    }

    if constexpr (RSPLIT > 1) {
        // the RSPLIT waves of a tile pair hold partial sums over different patch rows: fold into rs == 0
        float* red = (float*)smem;  // [8 waves][16][64] per tap round
#pragma unroll
        for (int t = 0; t < MAXT; ++t) {
            if (t < tcnt) {
                __syncthreads();
                if (rs > 0) {
#pragma unroll
                    for (int k = 0; k < 16; ++k) red[(wave * 16 + k) * 64 + lane] = acc[t][k];
                }
                __syncthreads();
                if (rs == 0) {
                    for (int w = 1; w < RSPLIT; ++w)
#pragma unroll
                        for (int k = 0; k < 16; ++k) acc[t][k] += red[((wave + w) * 16 + k) * 64 + lane];
                }
            }
        }
        if (rs != 0) return;
    }

#pragma unroll
    for (int t = 0; t < MAXT; ++t) {
        if (tap_ok(t)) {
            float* out = a.partial + ((size_t)(split * a.ntaps + tap_of(t)) * a.Ca_pad + ca0 + ai * 32) * a.Cb_pad + cb0 + bi * 32 + r;
#pragma unroll
            for (int k = 0; k < 16; ++k) {
                const int arow = (k & 3) + 8 * (k >> 2) + 4 * h;
                out[(size_t)arow * a.Cb_pad] = acc[t][k];
            }
        }
    }
}

// Sum the split-K slabs.  One thread per (tap, a, b) output element; consecutive threads walk
// b, so every slab read is a coalesced 4-byte stream and the whole reduction is one pass at
// HBM/L2 speed (slab order fixed -> bitwise reproducible).  Output = reference layout [a][b][tap].
__global__ __launch_bounds__(256) void wgrad_reduce_kernel(const abc_wgrad_reduce_desc d) { wgrad_reduce_body(d, blockIdx.x); }

__global__ __launch_bounds__(256) void wgrad_reduce_vec_kernel(const abc_wgrad_reduce_desc d) { wgrad_reduce_vec_body(d, blockIdx.x); }

// one launch: the slab reduction of one layer (blocks [0, nr)) beside the BatchNorm-backward finaliser of the next (reduce_bn.hpp)
struct ReduceBn { abc_wgrad_reduce_desc r; abc_bn_bwd_desc f; int nr, vec; };
__global__ __launch_bounds__(256) void wgrad_reduce_bn_kernel(const ReduceBn a) {
    if ((int)blockIdx.x < a.nr) {
        if (a.vec) wgrad_reduce_vec_body(a.r, blockIdx.x); else wgrad_reduce_body(a.r, blockIdx.x);
    } else {
        bn_finalize_bwd_body(a.f, a.f.C, (int)blockIdx.x - a.nr);
    }
}

// Few outputs, many slabs (the one-channel layer: 288 sums over 1024 slabs): one wave per output element, lanes stride
// the slabs, fixed shuffle tree -> still bitwise reproducible.
__global__ __launch_bounds__(64) void wgrad_reduce_wave_kernel(const abc_wgrad_reduce_desc d) {
    const int idx = blockIdx.x;
    const int bi = idx % d.Cb, ai = (idx / d.Cb) % d.Ca, t = idx / (d.Cb * d.Ca);
    const size_t slab = (size_t)d.Ca_pad * d.Cb_pad;
    const float* p = d.partial + (size_t)t * slab + (size_t)ai * d.Cb_pad + bi;
    const size_t step = (size_t)d.ntaps * slab;
    float s = 0.f;
    for (int k = threadIdx.x; k < d.nsplit; k += 64) s += p[(size_t)k * step];
    for (int m = 32; m >= 1; m >>= 1) s += __shfl_xor(s, m);
    if (threadIdx.x == 0) {
        float* o = d.dw + ((size_t)ai * d.Cb + bi) * d.ntaps + t;
        *o = d.accumulate ? (*o + s) : s;
    }
}

// Several small reductions (the heads' 8 weight gradients and 8 bias row sums) in ONE launch: blockIdx.y = item; an item
// whose output is small against its slab count goes wave-per-output (4 outputs per workgroup), the others thread-per-
// output; summation orders are those of the single-item kernels, so results are bit-identical to them.
constexpr int MAX_RB = 16;
struct ReduceBatch { abc_wgrad_reduce_desc d[MAX_RB]; };
__global__ __launch_bounds__(256) void wgrad_reduce_batch_kernel(const ReduceBatch bt) {
    const abc_wgrad_reduce_desc& d = bt.d[blockIdx.y];
    const int64_t n = (int64_t)d.ntaps * d.Ca * d.Cb;
    const size_t slab = (size_t)d.Ca_pad * d.Cb_pad;
    const size_t step = (size_t)d.ntaps * slab;
    if (n <= 4096 && d.nsplit >= 128) {
        const int64_t idx = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
        const int lane = threadIdx.x & 63;
        if (idx >= n) return;
        const int bi = (int)(idx % d.Cb), ai = (int)((idx / d.Cb) % d.Ca), t = (int)(idx / ((int64_t)d.Cb * d.Ca));
        const float* p = d.partial + (size_t)t * slab + (size_t)ai * d.Cb_pad + bi;
        float s = 0.f;
        for (int k = lane; k < d.nsplit; k += 64) s += p[(size_t)k * step];
        for (int m = 32; m >= 1; m >>= 1) s += __shfl_xor(s, m);
        if (lane == 0) {
            float* o = d.dw + ((size_t)ai * d.Cb + bi) * d.ntaps + t;
            *o = d.accumulate ? (*o + s) : s;
        }
        return;
    }
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= n) return;
    const int bi = (int)(idx % d.Cb);
    const int ai = (int)((idx / d.Cb) % d.Ca);
    const int t = (int)(idx / ((int64_t)d.Cb * d.Ca));
    const float* p = d.partial + (size_t)t * slab + (size_t)ai * d.Cb_pad + bi;
    float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
    int k = 0;
    for (; k + 4 <= d.nsplit; k += 4) {
        s0 += p[(size_t)k * step]; s1 += p[(size_t)(k + 1) * step]; s2 += p[(size_t)(k + 2) * step]; s3 += p[(size_t)(k + 3) * step];
    }
    for (; k < d.nsplit; ++k) s0 += p[(size_t)k * step];
    const float s = (s0 + s1) + (s2 + s3);
    float* o = d.dw + ((size_t)ai * d.Cb + bi) * d.ntaps + t;
    *o = d.accumulate ? (*o + s) : s;
}

struct WGeom {
    int AT, BT, dy_min, dx_min, HH, HW, PSWP, PSWQ, sP_bytes, sQ_bytes, coef_off, cstrP, cstrQ, lds, tgw, ngroups, nta, ntb, npatch,
        tiles_x, tiles_y, fast_p, fast_q, nbuf, PM, ts;
    int64_t bytesP, bytesQ;   // whole operand buffers
};

static int psw_for(int cw, int csz) {
    // bf16: the 64-byte column blocks of 4 consecutive pixels must fall on distinct quarters of the 256-byte bank row
    if (csz == 2) return cw == 32 ? 64 : (cw == 64 ? 192 : 320);
    return cw * 4;
}

static bool fast_ok(const abc_act_src& s, int csz_c, int cvalid_min, int64_t bytes) {
    const int nv = 16 / csz_c;
    return !s.pool && !s.planar && s.drop_p <= 0.f && (cvalid_min % nv) == 0 && bytes < (int64_t(1) << 31);
}

static int wgeom_pm(const abc_wgrad_desc* d, WGeom* g, int pm) {
    const int csz = d->dtype_c == ABC_BF16 ? 2 : 4;
    const int cwp = g->AT * 32, cwq = g->BT * 32;
    g->PM = pm;
    int dymin = 127, dymax = -127, dxmin = 127, dxmax = -127;
    for (int t = 0; t < d->ntaps; ++t) {
        dymin = d->tap_dy[t] < dymin ? d->tap_dy[t] : dymin; dymax = d->tap_dy[t] > dymax ? d->tap_dy[t] : dymax;
        dxmin = d->tap_dx[t] < dxmin ? d->tap_dx[t] : dxmin; dxmax = d->tap_dx[t] > dxmax ? d->tap_dx[t] : dxmax;
    }
    g->dy_min = dymin; g->dx_min = dxmin;
    g->HH = (8 * pm - 1) * d->stride + (dymax - dymin) + 1;
    g->HW = 15 * d->stride + (dxmax - dxmin) + 1;
    g->PSWP = psw_for(cwp, csz); g->PSWQ = psw_for(cwq, csz);
    g->sP_bytes = abc_roundup(128 * pm * g->PSWP, 256);
    g->sQ_bytes = abc_roundup(g->HH * g->HW * g->PSWQ, 256);
    g->cstrP = cwp; g->cstrQ = cwq;
    const int coef_bytes = 3 * (cwp + cwq) * 4 + 256;
    g->nbuf = (2 * (g->sP_bytes + g->sQ_bytes) + coef_bytes <= 160 * 1024) ? 2 : 1;
    g->coef_off = g->nbuf * (g->sP_bytes + g->sQ_bytes);
    g->lds = g->coef_off + coef_bytes;
    if (g->lds < 8 * 16 * 64 * 4) g->lds = 8 * 16 * 64 * 4;
    if (g->lds > 160 * 1024) return abc_fail(ABC_EUNSUPPORTED, "wgrad: LDS tile too large");
    g->nta = abc_cdiv(d->Ca, cwp); g->ntb = abc_cdiv(d->Cb, cwq);
    g->tiles_x = abc_cdiv(d->Wg, 16); g->tiles_y = abc_cdiv(d->Hg, 8 * pm);
    g->npatch = g->tiles_x * g->tiles_y * d->B;
    // prefetch fast path: plain NHWC source whose channel count in the LAST tile is a whole number of 16-byte segments
    const int lastP = d->Ca - (g->nta - 1) * cwp, lastQ = d->Cb - (g->ntb - 1) * cwq;
    const int segq = cwq / (16 / csz);
    g->bytesP = (int64_t)d->B * d->p.Hx * d->p.Wx * d->p.ldx * (d->dtype_p == ABC_BF16 ? 2 : 4);
    g->bytesQ = (int64_t)d->B * d->q.Hx * d->q.Wx * d->q.ldx * (d->dtype_q == ABC_BF16 ? 2 : 4);
    g->fast_p = (fast_ok(d->p, csz, lastP, g->bytesP) && g->HH * g->HW * g->HW < 65536) ? 1 : 0;
    g->fast_q = (fast_ok(d->q, csz, lastQ, g->bytesQ) && abc_cdiv(g->HH * g->HW * segq, WTHR_HOST) <= ((pm > 1 || (d->stride == 2 && csz == 2)) ? 5 : (csz == 2 ? 4 : 6))) ? 1 : 0;
    g->ngroups = abc_cdiv(d->ntaps, (g->fast_p && g->fast_q) ? MAXT_FAST : MAXT_SLOW);
    g->tgw = abc_cdiv(d->ntaps, g->ngroups);
    return ABC_OK;
}

static int wgeom(const abc_wgrad_desc* d, WGeom* g) {

    if (d->ntaps < 1 || d->ntaps > ABC_MAX_TAPS) return abc_fail(ABC_EINVAL, "wgrad: ntaps");
    if (d->stride != 1 && d->stride != 2) return abc_fail(ABC_EUNSUPPORTED, "wgrad: stride");
    const int csz = d->dtype_c == ABC_BF16 ? 2 : 4;
    const int ta = abc_cdiv(d->Ca, 32), tb = abc_cdiv(d->Cb, 32);
    // 32x32 tile pairs per workgroup (one pair per wave, the remaining waves split the patch rows).  Ragged channel
    // tails are fine (zero-filled): wide tiles are what keeps the operands from being re-staged per pair.
    // 4 x 2 pairs where a workgroup has patches to amortise its 295 KB slab over: with one round of <= 256 workgroups (the engine's
    // split rule: nsplit = min(patches / 2, 256 / tiles)) the 48 x 48 and smaller maps leave 2-5 patches per workgroup, the kernel is
    // prologue + slab store, and 2 x 2 pairs halve the slabs written here and re-read by the reduction (per layer: launch +0..5 us,
    // reduction -5..9 us; at 96 x 96 -- 9 patches per workgroup -- the wide tile wins by 10 us per launch)
    const int patches = d->B * abc_cdiv(d->Hg, 8) * abc_cdiv(d->Wg, 16);
    const int tiles42 = abc_cdiv(d->Ca, 128) * abc_cdiv(d->Cb, 64);
    const int ns42 = std::max(1, std::min(std::max(1, patches / 2), 256 / std::max(1, tiles42)));
    const bool few = patches < 6 * ns42;
    if (!few && d->stride == 1 && csz == 2 && ta >= 3 && tb >= 2) { g->AT = 4; g->BT = 2; }
    else if (d->stride == 1 && ta >= 2 && tb >= 2) { g->AT = 2; g->BT = 2; }
    else if (d->stride == 1 && csz == 2 && ta == 1 && tb >= 4) { g->AT = 1; g->BT = 4; }
    // ConvTranspose (stride 2): two P tiles share one staging of Q's 17 x 33-pixel halo (a 32-channel halo is what the prefetch path holds;
    // 64 x 64 pairs fall to the general loader: 150 us against 41).  41 -> 32 us per launch
    else if (d->stride == 2 && csz == 2 && d->dtype_p == ABC_BF16 && d->dtype_q == ABC_BF16 && ta >= 2) { g->AT = 2; g->BT = 1; }
    else { g->AT = 1; g->BT = 1; }
    // narrow layers (one tile pair, 8-way row split) take 32-row patches when both operands can be prefetched:
    // 4 K-steps per wave between barriers instead of 1
    g->ts = 0;
    if (g->AT == 1 && g->BT == 1 && d->stride == 1 && csz == 2 && d->Hg % 32 == 0) {
        int rc = wgeom_pm(d, g, 4);
        if (rc == ABC_OK && g->fast_p && g->fast_q) return ABC_OK;
    }
    // more than 9 taps on one tile pair (5x5): split the taps over the waves, one pass over the operands
    if (g->AT == 1 && g->BT == 1 && d->stride == 1 && csz == 2 && d->ntaps > MAXT_FAST && d->ntaps <= 32 &&
        d->dtype_p == ABC_BF16 && d->dtype_q == ABC_BF16) {
        for (int pm = (d->Hg % 16 == 0) ? 2 : 1; pm >= 1; --pm) {
            int rc = wgeom_pm(d, g, pm);
            if (rc == ABC_OK && g->fast_p && g->fast_q) { g->ts = 1; g->ngroups = 1; g->tgw = d->ntaps; return ABC_OK; }
        }
    }
    return wgeom_pm(d, g, 1);
}

template <typename PT, typename QT, typename CT, int AT, int BT, int STRIDE, bool FAST, int PM, bool K3, bool DUAL = false, bool TS = false>
static int wlaunch3(const WgK& k, const WGeom& g, int nsplit, hipStream_t st) {
    auto fn = wgrad_kernel<PT, QT, CT, AT, BT, STRIDE, FAST, PM, K3, DUAL, TS>;
    static unsigned long long lds_ok = 0;
    if (int rc = abc_allow_lds((const void*)fn, 160 * 1024, &lds_ok)) return rc;
    const int lds = k.qtab_off ? k.qtab_off + (PM > 1 ? 5 : 4) * WTHR_HOST * 4 : g.lds;     // (+ Q's segment table)
    hipLaunchKernelGGL(fn, dim3(g.nta * g.ntb * nsplit, g.ngroups), dim3(WTHR_HOST), lds, st, k);
    return abc_check_launch("wgrad");
}

template <typename PT, typename QT, typename CT, int AT, int BT, int STRIDE, bool FAST, int PM = 1>
static int wlaunch2(const WgK& k, const WGeom& g, int nsplit, hipStream_t st) {
    if constexpr (FAST && sizeof(CT) == 2) {
        if constexpr (sizeof(PT) == 2 && sizeof(QT) == 2 && STRIDE == 1) {
            if (k.k3 && k.p2 != nullptr) return wlaunch3<PT, QT, CT, AT, BT, STRIDE, FAST, PM, true, true>(k, g, nsplit, st);
        }
        if (k.k3) return wlaunch3<PT, QT, CT, AT, BT, STRIDE, FAST, PM, true>(k, g, nsplit, st);
    }
    if (k.p2 != nullptr) return abc_fail(ABC_EUNSUPPORTED, "wgrad: p_dual needs the prefetch path with 3x3 taps in bf16");
    return wlaunch3<PT, QT, CT, AT, BT, STRIDE, FAST, PM, false>(k, g, nsplit, st);
}

template <typename PT, typename QT, typename CT, int AT, int BT, int STRIDE>
static int wlaunch(const WgK& k, const WGeom& g, int nsplit, hipStream_t st) {
    return (g.fast_p && g.fast_q) ? wlaunch2<PT, QT, CT, AT, BT, STRIDE, true>(k, g, nsplit, st)
                                  : wlaunch2<PT, QT, CT, AT, BT, STRIDE, false>(k, g, nsplit, st);
}

template <typename PT, typename QT, typename CT>
static int wdispatch(const WgK& k, const WGeom& g, int stride, int nsplit, hipStream_t st) {
    if constexpr (sizeof(CT) == 2) {
        if (g.AT == 4) return wlaunch<PT, QT, CT, 4, 2, 1>(k, g, nsplit, st);
    }
    if constexpr (sizeof(CT) == 2 && sizeof(PT) == 2 && sizeof(QT) == 2) {
        if (g.AT == 2 && g.BT == 1 && stride == 2) return wlaunch<PT, QT, CT, 2, 1, 2>(k, g, nsplit, st);
    }
    if (g.AT == 2) return wlaunch<PT, QT, CT, 2, 2, 1>(k, g, nsplit, st);
    if constexpr (sizeof(CT) == 2) {
        if (g.BT == 4) return wlaunch<PT, QT, CT, 1, 4, 1>(k, g, nsplit, st);
        if constexpr (sizeof(PT) == 2 && sizeof(QT) == 2) {
            if (g.ts && k.p2 != nullptr) {
                if (g.PM == 2) return wlaunch3<PT, QT, CT, 1, 1, 1, true, 2, false, true, true>(k, g, nsplit, st);
                return wlaunch3<PT, QT, CT, 1, 1, 1, true, 1, false, true, true>(k, g, nsplit, st);
            }
            if (g.ts && g.PM == 2) return wlaunch3<PT, QT, CT, 1, 1, 1, true, 2, false, false, true>(k, g, nsplit, st);
            if (g.ts) return wlaunch3<PT, QT, CT, 1, 1, 1, true, 1, false, false, true>(k, g, nsplit, st);
        }
        if (g.PM == 4) return wlaunch2<PT, QT, CT, 1, 1, 1, true, 4>(k, g, nsplit, st);
    }
    if (stride == 1) return wlaunch<PT, QT, CT, 1, 1, 1>(k, g, nsplit, st);
    return wlaunch<PT, QT, CT, 1, 1, 2>(k, g, nsplit, st);
}


// the taps are the 3x3 square in row-major order, relative to (dy_min, dx_min)
static bool taps_square3(const abc_wgrad_desc* d, const WGeom& g) {
    if (d->ntaps != 9) return false;
    for (int t = 0; t < 9; ++t)
        if (d->tap_dy[t] - g.dy_min != t / 3 || d->tap_dx[t] - g.dx_min != t % 3) return false;
    return true;
}

// BN-backward correction on load of P: prefetch path for both operands, bf16 everywhere, stride 1, the static 3x3 K-step (k3)
static bool dual_ok(const abc_wgrad_desc* d, const WGeom& g, bool k3) {
    if (d->dtype_p != ABC_BF16 || d->dtype_q != ABC_BF16 || d->dtype_c != ABC_BF16) return false;
    if (d->p.scale == nullptr || d->p2 == nullptr || (d->ld_p2 % 8) || (d->cp2_off % 8) || (d->p_out && (d->ld_pout % 8))) return false;
    if ((int64_t)d->B * d->Hg * d->Wg * d->ld_p2 * 2 >= (int64_t(1) << 31)) return false;
    if (d->p_out && (int64_t)d->B * d->Hg * d->Wg * d->ld_pout * 2 >= (int64_t(1) << 31)) return false;   // (32-bit store offsets)
    // (the correction is applied where P is committed to LDS: independent of the taps, so the tap-split form of the 5x5
    //  layers takes it as well as the static 3x3 K-step)
    return g.fast_p && g.fast_q && d->stride == 1 && (g.ts || k3);
}

// Which kernel family serves a descriptor, and with which geometry: the ONE place that decides.  The queries the engine sizes its
// slabs and accounts its launches from, and the launch itself, all read this.
enum WgFamily { WG_HEAD, WG_C1, WG_NARROW16, WG_N32R2, WG_GENERAL };
struct WgRoute {
    WgFamily family;
    int ca_pad, cb_pad;      // slab extents
    int at, bt;              // abc_wgrad_tile: (0, 0) head, (0, 1) one-channel, (0, 2) 16-channel, (0, 3) 5x5 32-channel, else the general kernel's tile pairs
    int blocks;              // workgroups per K-split
    int fuses_apply;         // the BatchNorm-backward correction is applied on load of P (the general kernel: when p_dual asks; today's dual_ok)
    // WG_GENERAL only
    WGeom g;
    int k3;                  // the static 3x3 K-step: one tap group, the ordered 3x3 square
    int qtab_off;            // WgK::qtab_off
};

static int wgrad_route(const abc_wgrad_desc* d, WgRoute* r) {
    // {family, slab extents, tile code, workgroups per split, fuses_apply}
    if (abc_wgrad_head_ok(d)) { *r = WgRoute{WG_HEAD, abc_cdiv(d->Ca, 32) * 32, 128, 0, 0, abc_cdiv(abc_cdiv(d->Ca, 32), 4), 0}; return ABC_OK; }
    if (abc_wgrad_c1_ok(d)) { *r = WgRoute{WG_C1, d->Ca, 1, 0, 1, 1, (d->p_dual && d->p.scale) ? 1 : 0}; return ABC_OK; }   // (the one-channel kernel applies the correction on load too)
    if (abc_wgrad_narrow_ok(d)) { *r = WgRoute{WG_NARROW16, 16, 16, 0, 2, 1, d->p_dual ? 1 : 0}; return ABC_OK; }            // 16 x 16 channels, 3x3: wgrad_narrow.hip
    if (abc_wgrad_n32r2_ok(d)) { *r = WgRoute{WG_N32R2, 32, 32, 0, 3, 1, d->p_dual ? 1 : 0}; return ABC_OK; }                // 32 x 32 channels, 5x5: wgrad_narrow.hip
    *r = WgRoute{};
    WGeom& g = r->g;
    if (int rc = wgeom(d, &g)) return rc;
    r->family = WG_GENERAL;
    r->ca_pad = g.nta * g.AT * 32; r->cb_pad = g.ntb * g.BT * 32;
    r->at = g.AT; r->bt = g.BT;
    r->blocks = g.nta * g.ntb * g.ngroups;
    r->k3 = (g.ngroups == 1 && g.HW == 15 * d->stride + 3 && taps_square3(d, g)) ? 1 : 0;
    r->fuses_apply = dual_ok(d, g, r->k3) ? 1 : 0;
    // Q's segment table: the static 3x3 step of the 8-wave bf16 prefetch path over whole patches of a same-size image whose offsets
    // fit the entry (relative offset < 16 MB, LDS image < 64 KB), when the table (segments per thread x 512 x 4 bytes) fits the LDS
    if (r->k3 && d->stride == 1 && g.fast_p && g.fast_q && !g.ts && g.AT * g.BT >= 4 && d->dtype_c == ABC_BF16 && d->dtype_q == ABC_BF16 &&
        d->Hg % (8 * g.PM) == 0 && d->Wg % 16 == 0 && d->Hq == d->Hg && d->Wq == d->Wg && d->q.Hx == d->Hq && d->q.Wx == d->Wq &&
        (int64_t)(g.HH * d->q.Wx + g.HW) * d->q.ldx * 2 < (int64_t(1) << 24) && g.sQ_bytes < 65536) {
        const int npf_q = g.PM > 1 ? 5 : 4;
        const int off = abc_roundup(g.lds, 16);
        if (off + npf_q * WTHR_HOST * 4 <= 160 * 1024) r->qtab_off = off;
    }
    return ABC_OK;
}

enum ReduceKind { RED_WAVE, RED_VEC, RED_SCALAR };
struct ReduceForm { ReduceKind kind; int grid; };

// wave per output where few outputs face many slabs; else four outputs per thread where the slabs allow 16-byte reads (few outputs
// over many slabs: the scalar form walks them four at a time, 32 us for 4608 x 256); else one output per thread
static ReduceForm reduce_form(const abc_wgrad_reduce_desc& d) {
    const int64_t n = (int64_t)d.ntaps * d.Ca * d.Cb;
    if (n <= 4096 && d.nsplit >= 128) return {RED_WAVE, (int)n};
    if (d.Cb % 4 == 0 && d.Cb_pad % 4 == 0 && ((uintptr_t)d.partial & 15) == 0 && d.nsplit >= 16 && (n >= 16384 || d.nsplit >= 64))
        return {RED_VEC, (int)((n / 4 + 63) / 64)};
    return {RED_SCALAR, (int)((n + 255) / 256)};
}

}  // namespace

extern "C" int abc_wgrad_rowsum_ok(const abc_wgrad_desc* d) { return abc_wgrad_head_ok(d) ? 1 : 0; }

extern "C" int abc_wgrad_fuses_apply(const abc_wgrad_desc* d) {
    WgRoute r;
    return wgrad_route(d, &r) ? 0 : r.fuses_apply;
}

extern "C" int abc_wgrad_pads(const abc_wgrad_desc* d, int32_t* ca_pad, int32_t* cb_pad) {
    WgRoute r;
    if (int rc = wgrad_route(d, &r)) return rc;
    *ca_pad = r.ca_pad; *cb_pad = r.cb_pad;
    return ABC_OK;
}

extern "C" int abc_wgrad_tile(const abc_wgrad_desc* d, int32_t* at, int32_t* bt) {
    WgRoute r;
    if (int rc = wgrad_route(d, &r)) return rc;
    *at = r.at; *bt = r.bt;
    return ABC_OK;
}

// what the launch will take, for tests that must prove which path their case reaches (read-only: the same wgrad_route answer)
extern "C" int abc_wgrad_route_info(const abc_wgrad_desc* d, int32_t* info) {
    WgRoute r;
    if (int rc = wgrad_route(d, &r)) return rc;
    const bool gen = r.family == WG_GENERAL;
    info[0] = (int)r.family; info[1] = r.at; info[2] = r.bt;
    info[3] = gen ? r.g.PM : 0; info[4] = gen ? r.g.ts : 0; info[5] = (gen && r.g.fast_p && r.g.fast_q) ? 1 : 0;
    info[6] = gen ? r.k3 : 0; info[7] = (gen && r.qtab_off != 0) ? 1 : 0;
    return ABC_OK;
}

extern "C" int abc_wgrad_blocks(const abc_wgrad_desc* d) {
    WgRoute r;
    return wgrad_route(d, &r) ? -1 : r.blocks;
}

extern "C" int abc_wgrad(const abc_wgrad_desc* d, abc_stream_t stream) {
    if (d->nsplit < 1) return abc_fail(ABC_EINVAL, "wgrad: nsplit");
    if (d->ntaps < 1 || d->ntaps > ABC_MAX_TAPS) return abc_fail(ABC_EINVAL, "wgrad: ntaps");
    WgRoute r;
    if (int rc = wgrad_route(d, &r)) return rc;
    if (r.family == WG_HEAD) return abc_wgrad_head_launch(d, stream);
    // both operands at the resolution the taps index (after an on-load 2x2 pool)
    const int php = d->p.pool ? d->p.Hx / 2 : d->p.Hx, pwp = d->p.pool ? d->p.Wx / 2 : d->p.Wx;
    const int qhp = d->q.pool ? d->q.Hx / 2 : d->q.Hx, qwp = d->q.pool ? d->q.Wx / 2 : d->q.Wx;
    if (php != d->Hg || pwp != d->Wg || qhp != d->Hq || qwp != d->Wq) return abc_fail(ABC_EINVAL, "wgrad: dims mismatch");
    if (r.family == WG_C1) return abc_wgrad_c1_launch(d, stream);
    if (r.family == WG_NARROW16) return abc_wgrad_narrow_launch(d, stream);
    if (r.family == WG_N32R2) return abc_wgrad_n32r2_launch(d, stream);
    const WGeom& g = r.g;
    WgK k{};
    auto cp = [](ActSrc& o, const abc_act_src& i) {
        o.x = i.x; o.scale = i.scale; o.shift = i.shift; o.slope = i.slope; o.Hx = i.Hx; o.Wx = i.Wx; o.ldx = i.ldx;
        o.pool = i.pool; o.drop_p = i.drop_p; o.drop_seed = i.drop_seed; o.planar = i.planar; o.ctot = i.ctot; o.drop_salt = i.drop_salt;
    };
    cp(k.p, d->p); cp(k.q, d->q);
    k.partial = d->partial; k.B = d->B; k.Hg = d->Hg; k.Wg = d->Wg; k.Hq = d->Hq; k.Wq = d->Wq;
    k.cp_off = d->cp_off; k.Ca = d->Ca; k.cq_off = d->cq_off; k.Cb = d->Cb;
    k.Ca_pad = r.ca_pad; k.Cb_pad = r.cb_pad;
    k.ntaps = d->ntaps; k.tgw = g.tgw; k.nsplit = d->nsplit; k.npatch = g.npatch; k.tiles_x = g.tiles_x; k.tiles_y = g.tiles_y;
    k.dy_min = g.dy_min; k.dx_min = g.dx_min; k.HH = g.HH; k.HW = g.HW; k.PSWP = g.PSWP; k.PSWQ = g.PSWQ;
    k.sP_bytes = g.sP_bytes; k.sQ_bytes = g.sQ_bytes; k.coef_off = g.coef_off; k.cstrP = g.cstrP; k.cstrQ = g.cstrQ;
    k.nta = g.nta; k.ntb = g.ntb; k.fast_p = g.fast_p; k.fast_q = g.fast_q; k.nbuf = g.nbuf;
    k.magicQ = 65536 / g.HW + 1;
    if (g.npatch >= 65536 || g.tiles_x > 4096 || g.tiles_y > 4096) return abc_fail(ABC_EUNSUPPORTED, "wgrad: more than 65535 patches");
    k.mg_tx = (unsigned)((0x100000000ull + (unsigned)g.tiles_x - 1) / (unsigned)g.tiles_x);
    k.mg_ty = (unsigned)((0x100000000ull + (unsigned)g.tiles_y - 1) / (unsigned)g.tiles_y);
    k.regP = (d->Hg % (8 * g.PM) == 0 && d->Wg % 16 == 0 && d->p.Hx == d->Hg && d->p.Wx == d->Wg) ? 1 : 0;
    k.k3 = r.k3; k.qtab_off = r.qtab_off;
    if (d->p_dual) {
        if (!r.fuses_apply) return abc_fail(ABC_EUNSUPPORTED, "wgrad: p_dual is not served for this descriptor (abc_wgrad_fuses_apply)");
        k.p2 = d->p2; k.p_out = d->p_out; k.ld_p2 = d->ld_p2; k.cp2_off = d->cp2_off; k.ld_pout = d->ld_pout;
        k.bytesP2 = (unsigned)((int64_t)d->B * d->Hg * d->Wg * d->ld_p2 * 2);
    }
    k.bytesP = (unsigned)g.bytesP; k.bytesQ = (unsigned)g.bytesQ;
    for (int t = 0; t < d->ntaps; ++t) { k.ty[t] = (int8_t)(d->tap_dy[t] - g.dy_min); k.tx[t] = (int8_t)(d->tap_dx[t] - g.dx_min); }
    hipStream_t st = (hipStream_t)stream;
    if (d->dtype_c == ABC_F32) {
        if (d->dtype_p != ABC_F32 || d->dtype_q != ABC_F32) return abc_fail(ABC_EUNSUPPORTED, "wgrad: f32 compute needs f32 operands");
        return wdispatch<float, float, float>(k, g, d->stride, d->nsplit, st);
    }
    if (d->dtype_p == ABC_BF16 && d->dtype_q == ABC_BF16) return wdispatch<bf16, bf16, bf16>(k, g, d->stride, d->nsplit, st);
    if (d->dtype_p == ABC_F32 && d->dtype_q == ABC_BF16) return wdispatch<float, bf16, bf16>(k, g, d->stride, d->nsplit, st);
    if (d->dtype_p == ABC_BF16 && d->dtype_q == ABC_F32) return wdispatch<bf16, float, bf16>(k, g, d->stride, d->nsplit, st);
    return abc_fail(ABC_EUNSUPPORTED, "wgrad: dtype combination");
}

extern "C" int abc_wgrad_reduce(const abc_wgrad_reduce_desc* d, abc_stream_t stream) {
    const ReduceForm f = reduce_form(*d);
    if (f.kind == RED_WAVE) hipLaunchKernelGGL(wgrad_reduce_wave_kernel, dim3(f.grid), dim3(64), 0, (hipStream_t)stream, *d);
    else if (f.kind == RED_VEC) hipLaunchKernelGGL(wgrad_reduce_vec_kernel, dim3(f.grid), dim3(256), 0, (hipStream_t)stream, *d);
    else hipLaunchKernelGGL(wgrad_reduce_kernel, dim3(f.grid), dim3(256), 0, (hipStream_t)stream, *d);
    return abc_check_launch("wgrad_reduce");
}

// The slab reduction of one weight gradient and the BatchNorm-backward finaliser of ANOTHER layer (both inputs complete, neither
// reads the other's output) as one launch; the small-output reduction form (one wave per element) is launched on its own.
extern "C" int abc_wgrad_reduce_bn_bwd(const abc_wgrad_reduce_desc* d, const abc_bn_bwd_desc* f, abc_stream_t stream) {
    if (f->C < 1 || f->nblk < 1) return abc_fail(ABC_EINVAL, "wgrad_reduce_bn_bwd: empty finaliser");
    const ReduceForm rf = reduce_form(*d);
    if (rf.kind == RED_WAVE) {
        if (int rc = abc_wgrad_reduce(d, stream)) return rc;
        return abc_bn_finalize_bwd(f, stream);
    }
    ReduceBn a;
    a.r = *d; a.f = *f;
    a.vec = rf.kind == RED_VEC ? 1 : 0;
    a.nr = rf.grid;
    hipLaunchKernelGGL(wgrad_reduce_bn_kernel, dim3(a.nr + f->C), dim3(256), 0, (hipStream_t)stream, a);
    return abc_check_launch("wgrad_reduce_bn_bwd");
}

extern "C" int abc_wgrad_reduce_batch(const abc_wgrad_reduce_desc* descs, int32_t n, abc_stream_t stream) {
    if (n < 1 || n > MAX_RB) return abc_fail(ABC_EINVAL, "wgrad_reduce_batch: 1..16 items");
    ReduceBatch bt;
    int64_t gx = 1;
    for (int i = 0; i < n; ++i) {
        bt.d[i] = descs[i];
        // (the batch kernel packs four wave-form outputs into a workgroup)
        const int64_t cnt = (int64_t)descs[i].ntaps * descs[i].Ca * descs[i].Cb;
        const int64_t blocks = reduce_form(descs[i]).kind == RED_WAVE ? (cnt + 3) / 4 : (cnt + 255) / 256;
        gx = blocks > gx ? blocks : gx;
    }
    for (int i = n; i < MAX_RB; ++i) bt.d[i] = descs[0];
    hipLaunchKernelGGL(wgrad_reduce_batch_kernel, dim3((int)gx, n), dim3(256), 0, (hipStream_t)stream, bt);
    return abc_check_launch("wgrad_reduce_batch");
}
