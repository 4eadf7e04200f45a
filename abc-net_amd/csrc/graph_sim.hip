// The graded score after assembly: how NEAR is the molecule abc_assemble_graphs built to the annotated molecule, without reading a
// position?  (The reference's graded number is the Dice similarity of radius-3 Morgan fingerprints, cal_acc.py:38-43, through
// RDKit; this is the same idea on environments this file defines itself, exactly, in integers -- the contract is in
// include/abcnet_hip.h and DESIGN.md section 7.)
//
// One workgroup per image; integers only (uint64, wrapping), so every id is a pure function of the graph and the totals do not
// depend on the order of the workgroups.  Side 0 is the molecule, side 1 the record.
//
//   (A) degrees: one thread per bond row, a 64-bit integer LDS add per valid end (acc); the record's atoms with a bond (the set T of
//       graph_score.hip) are numbered in index order by a workgroup scan (remap); id_0 of every atom
//   (B) rounds r = 1 .. 3: one thread per bond row, acc[a] += mix(mix(id[j]) + order) for both ends -- the sum is commutative, so no
//       order of rows or atoms can change an id; then id_r[a] = mix(mix(id[a] + r) + acc[a]), kept as layer r of the fingerprint.
//       Bond rows are never held in LDS, so no bond capacity bounds the launch: row `tid` of each side stays in registers, the rows
//       past the workgroup's 256 threads are read from global memory again every round
//   (C) the multiset intersection of the two fingerprints by counting: a molecule element is common when fewer equal elements stand
//       before it in its own list than the record's list holds
//   (D) only when the atom and valid-bond counts are equal: the same recurrence on to T = min(n, 64) rounds and the same counting on
//       the two id_T lists (colour refinement)
//   (E) lane 0 writes the row and adds it to the totals (64-bit atomicAdd, non-zero columns only)
//
// Every index read from a row is range-checked before it addresses anything: hand-made rows may hold any int32.
#include "common.hpp"
#include "../../include/abcnet_hip.h"
#include "capi_util.hpp"
#include "block_scan.hpp"
#include "mol_rows.hpp"
#include "graph_ids.hpp"
#include "graph_refine.hpp"

namespace {

constexpr int GT = REFINE_GT;       // threads per workgroup (graph_refine.hpp)
constexpr int MAX_ATOMS = ABC_MAX_SIM_ATOMS;      // ids, sums and four fingerprint layers of both sides in 48 KB of LDS
constexpr int RADIUS = 3;            // fingerprint layers 0 .. 3
constexpr int MAX_ROUNDS = 64;       // refinement rounds of refine_equal
constexpr int FP = (RADIUS + 1) * MAX_ATOMS;
constexpr int NCOL = ABC_SIM_NCOL;
static_assert(FP == ABC_SIM_IDS, "ids_out holds one fingerprint per side");
static_assert(MAX_ATOMS == 2 * GT, "the record scan numbers two atoms per thread");

// this thread's share of the size of the multiset intersection of A and B (LDS lists; every read of the inner loops is a broadcast)
__device__ inline int common_share(const u64* A, int nA, const u64* Bv, int nB, int tid) {
    int c = 0;
    for (int k = tid; k < nA; k += GT) {
        const u64 e = A[k];
        int before = 0, there = 0;
        for (int i = 0; i < nA; ++i) before += (i < k) & (A[i] == e);
        for (int i = 0; i < nB; ++i) there += Bv[i] == e;
        c += before < there;
    }
    return c;
}

__global__ __launch_bounds__(GT) void graph_sim_kernel(const abc_graph_similarity_desc d) {
    __shared__ u64 cur[2][MAX_ATOMS];    // id_r of every atom
    __shared__ u64 acc[2][MAX_ATOMS];    // degree, then the neighbour sum of the round
    __shared__ u64 fp[2][FP];            // layer-major, atom-minor: id_r[a] at r * n + a
    __shared__ int remap[MAX_ATOMS];     // record atom -> its number in T, -1 outside T
    __shared__ unsigned wt[REFINE_NW + 1];
    __shared__ int cnt[4];               // valid molecule bonds, valid record bonds, envs_common, common id_T
    const int b = blockIdx.x, tid = threadIdx.x;
    ScoredImage im;
    if (!scored_image<NCOL>(d, b, tid, im)) return;
    const auto [nt, m, status, na, nb, empty, pa, pb, ra, rb] = im;

    // row `tid` of each side, kept through every round
    const BondRow none = {false, 0, 0, 0};
    const BondRow prow = tid < nb ? mol_row(pb, tid, na) : none;
    BondRow trow = tid < m ? rec_row(rb, tid, nt) : none;

    // ---- (A) degrees (in acc), T, id_0
    if (tid < 4) cnt[tid] = 0;
    for (int a = tid; a < MAX_ATOMS; a += GT) acc[0][a] = acc[1][a] = 0;
    __syncthreads();
    {
        const int valid_p = refine_degrees_mol(tid, pb, nb, na, prow, acc[0]), valid_t = refine_degrees_rec(tid, rb, m, nt, trow, acc[1]);
        if (valid_p) atomicAdd(cnt + 0, valid_p);
        if (valid_t) atomicAdd(cnt + 1, valid_t);
    }
    __syncthreads();
    refine_id0_mol(tid, pa, na, acc[0], cur[0], fp[0]);      // (id_0 is layer 0 of the fingerprint)
    for (int a = tid; a < na; a += GT) acc[0][a] = 0;        // (by the thread that read the degree)
    const int n_t = refine_number_rec(tid, ra, nt, acc[1], wt, remap, (int*)nullptr, cur[1], fp[1]);      // |T|
    __syncthreads();
    renumber(trow, remap);
    const int valid_p = cnt[0], valid_t = cnt[1];
    const bool size_equal = !empty && na == n_t && valid_p == valid_t;
    const int rounds_t = min(na, MAX_ROUNDS);
    const int rounds = size_equal ? max(rounds_t, RADIUS) : RADIUS;

    // ---- (B) and (D): the rounds, both sides between one pair of barriers; (C) after the third
    u64 *layer_p = fp[0], *layer_t = fp[1];      // layer r of the fingerprints while r <= RADIUS, then null
    for (int r = 1; r <= rounds; ++r) {
        layer_p = r <= RADIUS ? layer_p + na : nullptr, layer_t = r <= RADIUS ? layer_t + n_t : nullptr;
        refine_add_mol(tid, cur[0], acc[0], pb, nb, na, prow);
        refine_add_rec(tid, cur[1], acc[1], rb, m, nt, remap, trow);
        __syncthreads();
        refine_finish(tid, cur[0], acc[0], na, (u64)r, layer_p);
        refine_finish(tid, cur[1], acc[1], n_t, (u64)r, layer_t);
        __syncthreads();
        if (r == RADIUS) {
            const int c = common_share(fp[0], (RADIUS + 1) * na, fp[1], (RADIUS + 1) * n_t, tid);
            if (c) atomicAdd(cnt + 2, c);
        }
    }
    if (size_equal) {
        // id_T: a fingerprint layer while T <= 3 (na == n_t here), the current ids after that
        const u64* A = rounds_t <= RADIUS ? fp[0] + rounds_t * na : cur[0];
        const u64* Bv = rounds_t <= RADIUS ? fp[1] + rounds_t * na : cur[1];
        const int c = common_share(A, na, Bv, na, tid);
        if (c) atomicAdd(cnt + 3, c);
    }
    if (d.ids_out != nullptr) {
        u64* out = (u64*)d.ids_out + (size_t)b * 2 * FP;
        for (int k = tid; k < FP; k += GT) {
            out[k] = k < (RADIUS + 1) * na ? fp[0][k] : 0;
            out[FP + k] = k < (RADIUS + 1) * n_t ? fp[1][k] : 0;
        }
    }
    __syncthreads();

    // ---- (E)
    if (tid == 0) {
        int r[NCOL];
#pragma unroll
        for (int i = 0; i < NCOL; ++i) r[i] = 0;
        const int envs_p = (RADIUS + 1) * na, envs_t = (RADIUS + 1) * n_t, common = cnt[2];
        r[ABC_SIM_COUNTED] = 1;
        r[ABC_SIM_ENVS_TRUE] = envs_t;
        if (empty) {
            r[ABC_SIM_NONE] = 1;
        } else {
            r[ABC_SIM_TRUNCATED] = (status & ABC_MOL_TRUNCATED) ? 1 : 0;
            r[ABC_SIM_SIZE_EQUAL] = size_equal;
            r[ABC_SIM_REFINE_EQUAL] = size_equal && cnt[3] == na;
            r[ABC_SIM_DICE_ONE] = common > 0 && common == envs_p && common == envs_t;
            r[ABC_SIM_ATOMS_PRED] = na;
            r[ABC_SIM_ATOMS_TRUE] = n_t;
            r[ABC_SIM_ENVS_PRED] = envs_p;
            r[ABC_SIM_ENVS_COMMON] = common;
            r[ABC_SIM_DICE_Q20] = envs_p + envs_t ? (int)((((u64)common * 2) << 20) / (u64)(envs_p + envs_t)) : 0;
        }
        write_row_and_totals<NCOL>(d.rows + (size_t)b * NCOL, d.totals, r);
    }
}

}  // namespace

extern "C" int abc_graph_similarity_desc_size(void) { return (int)sizeof(abc_graph_similarity_desc); }

extern "C" int abc_graph_similarity_update(const abc_graph_similarity_desc* d, abc_stream_t stream) {
    if (d->B < 1) return abc_fail(ABC_EINVAL, "graph_similarity: empty");
    if (d->cap_atoms < 1 || d->cap_atoms > MAX_ATOMS) return abc_fail(ABC_EINVAL, "graph_similarity: cap_atoms must be 1..512");
    if (d->cap_mol_bonds < 1) return abc_fail(ABC_EINVAL, "graph_similarity: cap_mol_bonds must be >= 1");
    if (d->max_atoms < 1 || d->max_atoms > MAX_ATOMS) return abc_fail(ABC_EINVAL, "graph_similarity: max_atoms must be 1..512");
    if (d->max_bonds < 1) return abc_fail(ABC_EINVAL, "graph_similarity: max_bonds must be >= 1");
    if (!d->mol_counts || !d->mol_atoms || !d->mol_bonds) return abc_fail(ABC_EINVAL, "graph_similarity: null molecule buffer");
    if (!d->rec_atoms || !d->rec_bonds || !d->rec_counts) return abc_fail(ABC_EINVAL, "graph_similarity: null record buffer");
    if (!d->rows || !d->totals) return abc_fail(ABC_EINVAL, "graph_similarity: null output");
    hipLaunchKernelGGL(graph_sim_kernel, dim3(d->B), dim3(GT), 0, (hipStream_t)stream, *d);
    return abc_check_launch("graph_similarity_update");
}
