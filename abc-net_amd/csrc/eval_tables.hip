// The evaluation tables of the reference's third driver (src/test_accuracy.py:105-298) on the device.
//
// The script judges a model by five (tp, tn, fp, fn) tables -- atom and bond detection by target class, atom type, charge and
// bond type -- and by 17 AverageMeters at the INFERENCE thresholds (raw logit > -1, img2smiles2.py:61-79), and pays about 190
// .sum().cpu() round trips per batch for them.  Everything they need is on the device when an inference step ends; this is the
// one reduction over it.
//
//   pass 0  clear    : zero the 301 counts of this call (a kernel, not a memset API call: the sequence stays capturable)
//   pass 1  tables   : one thread per quarter-resolution pixel.  It reads the TARGET planes of its pixel (all NCHW: adjacent
//                      lanes = adjacent pixels, coalesced) and a prediction only where a target gives it weight:
//                        3x3 neighbourhood of the target map  only at a predicted peak   (tp / fp, precision3)
//                        3x3 neighbourhood of the peak mask   only at a target centre    (fn, recall3)
//                        atom type / charge / hs logits       only where the target planes of that head are not all zero
//                        bond-type logits (or the arg-max byte), |rho| and the rho target of a bin
//                                                             only where that bin's six target planes are not all zero
//                        the omega-bin mask                   only at a bond target centre
//                      Each skipped read would have been multiplied by an exact zero, so the sums are the reference's own.
//                      Integer results go to a per-workgroup LDS table (ds_add_u32; at most 256 * 60 * 6 per entry) that is
//                      flushed with 64-bit vector atomics, non-zero entries only: exact whatever the order.  The 24 floating
//                      sums behind the meters leave as per-workgroup double partials.
//                      abc_eval_tables_update_sparse: the same pass under the rasteriser's group flags -- target planes are read
//                      only in the 32-pixel groups an atom / a bond was drawn into (eval_tables_body<true>).
//   pass 2  finalize : fixed-order reduction of the partials -> (num, den) of this call and the running totals; running
//                      counts += counts of this call.  Two runs on the same input agree bit for bit.
//
// Line 241-245's `temp` is (circular NMS of the 0/1 omega mask, > 0.25) * bond_targets; on a 0/1 map that NMS is the identity,
// so temp = omega_mask & Tb.
#include "common.hpp"
#include "../../include/abcnet_hip.h"
#include "capi_util.hpp"
#include "meter_sums.hpp"

namespace {

constexpr int NSUM = ABC_METER_NSUM, NCOUNT = ABC_EVAL_NCOUNT;
constexpr int O_ADET = 0, O_BDET = 42, O_TYPE = 60, O_CHARGE = 256, O_BTYPE = 265;   // offsets into counts[301]

__global__ __launch_bounds__(320) void eval_clear_kernel(const abc_eval_desc d) {
    if (threadIdx.x < NCOUNT) d.counts_last[threadIdx.x] = 0;
}

// K target planes of one pixel: their sum, the number that equal 1, their arg max (first index on ties; 0 when all are 0)
template <int K>
__device__ inline void target_class(const float* t, size_t stride, float* st, int* wgt, int* at) {
    float best = t[0], s = best;
    int a = 0, n = best == 1.f;
#pragma unroll
    for (int k = 1; k < K; ++k) {
        const float v = t[(size_t)k * stride];
        s += v;
        n += v == 1.f;
        if (v > best) { best = v; a = k; }
    }
    *st = s; *wgt = n; *at = a;
}

template <int K>
__device__ inline int argmax_plane(const float* z, size_t stride) {
    float best = z[0];
    int a = 0;
#pragma unroll
    for (int k = 1; k < K; ++k) {
        const float v = z[(size_t)k * stride];
        if (v > best) { best = v; a = k; }
    }
    return a;
}

// one atom head: accuracy sums (lines 204-215) and, with a table, its confusion matrix (lines 138-162); returns the target class
template <int K>
__device__ inline int class_head(const float* t, const float* z, size_t hw, double* num, double* den, unsigned* table) {
    float st; int wgt, at;
    target_class<K>(t, hw, &st, &wgt, &at);
    if (st != 0.f || wgt > 0) {
        const int az = argmax_plane<K>(z, hw);
        *den += (double)st;
        if (at == az) *num += (double)st;
        if (table != nullptr && wgt > 0) atomicAdd(&table[at * K + az], (unsigned)wgt);
    }
    return at;
}

// SPARSE: `flags` is abc_raster_desc.group_flags of the rasteriser that drew the target maps, one word per 32 pixels of the
// flattened batch -- half a wave, so every branch on a word is half-wave-uniform.  A group without bits 0-3 holds no atom-side
// target, one without bits 4-7 no bond-side target: what the dense form reads there is an exact zero and adds an exact zero,
// so the thread skips the loads and keeps the zeros its sums start with.  A 3x3 neighbour in another group is judged by that
// group's word.  The order of every per-thread sum and of the reductions is the dense form's.
template <bool SPARSE>
__device__ __forceinline__ bool target_is_centre(const float* T, const uint32_t* flags, uint32_t bits, size_t img0, int o) {
    if (SPARSE && !(flags[(img0 + o) / 32] & bits)) return false;
    return T[o] == 1.f;
}

template <bool SPARSE>
__device__ __forceinline__ void eval_tables_body(const abc_eval_desc& d, const uint32_t* flags) {
    __shared__ double sm[4][NSUM];
    __shared__ unsigned cnt[NCOUNT];
    for (int i = threadIdx.x; i < NCOUNT; i += 256) cnt[i] = 0;
    __syncthreads();
    const int hw = d.h * d.w;
    const int64_t npix = (int64_t)d.B * hw;
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int nv = d.n_valid != nullptr ? min(max(*d.n_valid, 0), d.B) : d.B;
    double s[NSUM];
#pragma unroll
    for (int i = 0; i < NSUM; ++i) s[i] = 0.0;
    if (p < npix && p / hw < nv) {
        const int b = (int)(p / hw), yx = (int)(p % hw);
        const int y = yx / d.w, x = yx % d.w;
        const size_t img0 = (size_t)b * hw;
        const uint32_t word = SPARSE ? flags[p / 32] : 0xFFu;
        const bool has_atom = (word & 0x0Fu) != 0, has_bond = (word & 0xF0u) != 0;
        // ---- centre maps: precision / precision3 / recall / recall3 (lines 188-202, 217-231) and the detection outcome
        bool pk[2], tc[2], t3[2], p3[2];
#pragma unroll
        for (int which = 0; which < 2; ++which) {
            const float* T = (which ? d.t_bond : d.t_atom) + (size_t)b * hw;
            const float* P = (which ? d.bond_mask : d.atom_mask) + (size_t)b * hw;
            const uint32_t bits = which ? 0xF0u : 0x0Fu;
            const bool t = (which ? has_bond : has_atom) && T[yx] == 1.f, k = P[yx] != 0.f;
            bool tn = false, pn = false;
            if (t || k)
                for (int dy = -1; dy <= 1; ++dy)
                    for (int dx = -1; dx <= 1; ++dx) {
                        const int yy = y + dy, xx = x + dx;
                        if (yy >= 0 && yy < d.h && xx >= 0 && xx < d.w) {
                            if (k) tn |= target_is_centre<SPARSE>(T, flags, bits, img0, yy * d.w + xx);
                            if (t) pn |= P[yy * d.w + xx] != 0.f;
                        }
                    }
            double* o = s + which * 5;
            o[0] = (k && t) ? 1.0 : 0.0;
            o[1] = (k && tn) ? 1.0 : 0.0;
            o[2] = k ? 1.0 : 0.0;
            o[3] = (t && pn) ? 1.0 : 0.0;
            o[4] = t ? 1.0 : 0.0;
            pk[which] = k; tc[which] = t; t3[which] = tn; p3[which] = pn;
        }
        // ---- atom heads
        int ca = 0;     // (all-zero target planes: class 0, and no weight for any of the three heads)
        if (has_atom) {
            ca = class_head<14>(d.t_types + (size_t)b * 14 * hw + yx, d.types + (size_t)b * 14 * hw + yx, hw, &s[10], &s[11], cnt + O_TYPE);
            class_head<3>(d.t_charges + (size_t)b * 3 * hw + yx, d.charges + (size_t)b * 3 * hw + yx, hw, &s[12], &s[13], cnt + O_CHARGE);
            class_head<2>(d.t_hs + (size_t)b * 2 * hw + yx, d.hs + (size_t)b * 2 * hw + yx, hw, &s[14], &s[15], nullptr);
        }
        if (pk[0]) atomicAdd(&cnt[O_ADET + ca * 3 + (t3[0] ? 0 : 1)], 1u);
        if (tc[0] && !p3[0]) atomicAdd(&cnt[O_ADET + ca * 3 + 2], 1u);
        // ---- per omega bin: bond types (6-way, channel = type * 60 + bin), rho MAE, omega mask / target bits
        unsigned long long temp = 0, tom = 0;
        float mass[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};     // sum over the bins of every type's target plane (line 166)
        const float* TB = d.t_btypes + (size_t)b * 360 * hw + yx;
        const size_t bin0 = (size_t)b * 60 * hw + yx;
        for (int o = 0; o < (has_bond ? 60 : 0); ++o) {     // (no bond-side target: mass, tom and temp stay 0)
            float st = 0.f, best = 0.f;
            int wgt = 0, at = 0;
#pragma unroll
            for (int k = 0; k < 6; ++k) {
                const float v = TB[(size_t)(k * 60 + o) * hw];
                st += v;
                wgt += v == 1.f;
                mass[k] += v;
                if (k == 0 || v > best) { best = v; at = k; }
            }
            const size_t q = bin0 + (size_t)o * hw;
            if (st != 0.f || wgt > 0) {
                const int az = d.btype_idx != nullptr ? (int)d.btype_idx[q]
                                                      : argmax_plane<6>(d.btypes + (size_t)b * 360 * hw + (size_t)o * hw + yx, (size_t)60 * hw);
                s[17] += (double)st;
                if (at == az) s[16] += (double)st;
                s[18] += fabs((double)fabsf(d.rho_abs[q]) - d.t_rho[q]) * (double)st;
                if (wgt > 0 && az < 6) atomicAdd(&cnt[O_BTYPE + at * 6 + az], (unsigned)wgt);
            }
            if (d.t_omega[q] == 1.0) tom |= 1ull << o;
            if (tc[1] && d.omega_mask[q] != 0.f) temp |= 1ull << o;
        }
        int cb = 0;
#pragma unroll
        for (int k = 1; k < 6; ++k)
            if (mass[k] > mass[cb]) cb = k;
        if (pk[1]) atomicAdd(&cnt[O_BDET + cb * 3 + (t3[1] ? 0 : 1)], 1u);
        if (tc[1] && !p3[1]) atomicAdd(&cnt[O_BDET + cb * 3 + 2], 1u);
        s[19] = (double)__popcll(tom & temp);
        s[20] = (double)__popcll(temp);
        s[21] = (double)__popcll(tom & abc_circ3(temp));
        s[22] = (double)__popcll(tom);
        s[23] = (double)__popcll(abc_circ3(tom) & temp);
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int i = 0; i < NSUM; ++i) {
        const double a = abc_wave_sum(s[i]);
        if (lane == 0) sm[wave][i] = a;
    }
    __syncthreads();
    if (threadIdx.x < NSUM)
        d.partial[(size_t)blockIdx.x * NSUM + threadIdx.x] = (sm[0][threadIdx.x] + sm[1][threadIdx.x]) + (sm[2][threadIdx.x] + sm[3][threadIdx.x]);
    for (int i = threadIdx.x; i < NCOUNT; i += 256) {
        const unsigned v = cnt[i];
        if (v != 0) atomicAdd((unsigned long long*)&d.counts_last[i], (unsigned long long)v);
    }
}

__global__ __launch_bounds__(256) void eval_tables_kernel(const abc_eval_desc d) { eval_tables_body<false>(d, nullptr); }
__global__ __launch_bounds__(256) void eval_tables_sparse_kernel(const abc_eval_desc d, const uint32_t* flags) { eval_tables_body<true>(d, flags); }

__global__ __launch_bounds__(1024) void eval_finalize_kernel(const abc_eval_desc d, int nblk) {
    __shared__ double red[32][NSUM];
    __shared__ double tot[NSUM];
    const int t = threadIdx.x;
    const int which = t % 32, part = t / 32;   // 32 lanes per sum slot (24 used), 32 parts, fixed order -> reproducible
    if (which < NSUM) {
        double a = 0.0;
        for (int k = part; k < nblk; k += 32) a += d.partial[(size_t)k * NSUM + which];
        red[part][which] = a;
    }
    __syncthreads();
    if (t < NSUM) {
        double a = 0.0;
        for (int q = 0; q < 32; ++q) a += red[q][t];
        tot[t] = a;
    }
    __syncthreads();
    if (t < ABC_METER_COUNT) {
        const double num = tot[abc_meter_num_slot(t)];
        const double den = tot[abc_meter_den_slot(t)] + (t == 6 ? 0.01 : 0.0);   // atom_hs: 0.01 + sum (lines 213-215)
        d.meters_last[2 * t] = num; d.meters_last[2 * t + 1] = den;
        d.meters_totals[2 * t] += num; d.meters_totals[2 * t + 1] += den;
    }
    if (t < NCOUNT) d.counts_totals[t] += d.counts_last[t];
}

}  // namespace

extern "C" int abc_eval_desc_size(void) { return (int)sizeof(abc_eval_desc); }

extern "C" int abc_eval_tables_blocks(const abc_eval_desc* d) {
    if (d->B < 1 || d->h < 1 || d->w < 1 || (int64_t)d->B * d->h * d->w > (int64_t)INT32_MAX) return abc_fail(ABC_EINVAL, "eval_tables: empty or oversized shape");
    return abc_cdiv(d->B * d->h * d->w, 256);
}

static int eval_tables_launch(const abc_eval_desc* d, const uint32_t* target_flags, bool sparse, abc_stream_t stream) {
    if (d->B < 1 || d->h < 1 || d->w < 1) return abc_fail(ABC_EINVAL, "eval_tables: empty");
    if ((int64_t)d->B * d->h * d->w > (int64_t)INT32_MAX) return abc_fail(ABC_EINVAL, "eval_tables: more than 2^31 - 1 pixels");
    if (!d->partial || !d->counts_last || !d->counts_totals || !d->meters_last || !d->meters_totals)
        return abc_fail(ABC_EINVAL, "eval_tables: null workspace");
    if (!d->atom_mask || !d->bond_mask || !d->omega_mask || !d->rho_abs || !d->types || !d->charges || !d->hs)
        return abc_fail(ABC_EINVAL, "eval_tables: null prediction map");
    if (!d->t_atom || !d->t_types || !d->t_charges || !d->t_hs || !d->t_bond || !d->t_btypes || !d->t_rho || !d->t_omega)
        return abc_fail(ABC_EINVAL, "eval_tables: null target map");
    if ((d->btypes != nullptr) == (d->btype_idx != nullptr))
        return abc_fail(ABC_EINVAL, "eval_tables: exactly one of btypes (raw planes) and btype_idx (arg-max map) must be given");
    if (sparse && !target_flags) return abc_fail(ABC_EINVAL, "eval_tables: null target_flags");
    if (sparse && ((int64_t)d->h * d->w) % 32) return abc_fail(ABC_EINVAL, "eval_tables: target_flags needs h * w a multiple of 32");
    const int nb = abc_eval_tables_blocks(d);
    hipLaunchKernelGGL(eval_clear_kernel, dim3(1), dim3(320), 0, (hipStream_t)stream, *d);
    if (sparse) hipLaunchKernelGGL(eval_tables_sparse_kernel, dim3(nb), dim3(256), 0, (hipStream_t)stream, *d, target_flags);
    else hipLaunchKernelGGL(eval_tables_kernel, dim3(nb), dim3(256), 0, (hipStream_t)stream, *d);
    hipLaunchKernelGGL(eval_finalize_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, *d, nb);
    return abc_check_launch("eval_tables_update");
}

extern "C" int abc_eval_tables_update(const abc_eval_desc* d, abc_stream_t stream) { return eval_tables_launch(d, nullptr, false, stream); }

extern "C" int abc_eval_tables_update_sparse(const abc_eval_desc* d, const uint32_t* target_flags, abc_stream_t stream) {
    return eval_tables_launch(d, target_flags, true, stream);
}
