// The score after assembly: is the molecule abc_assemble_graphs built the annotated molecule?  (The reference answers offline,
// cal_acc.py through RDKit; this is the graph-level comparison on the head-map grid, accumulated like the evaluation tables.)
//
// One workgroup per image; integers only, so every count is exact and the totals do not depend on the order of the workgroups.
//
//   (A) the molecule's atom cells, the record's atom cells and the record's bonds (as pair keys) into LDS; an annotated atom is in
//       T when a record bond names it (integer atomicOr on an LDS flag)
//   (B) one THREAD per annotated atom of T, a loop over the molecule's atoms (LDS broadcasts): near_P, strict `<` in row order so
//       the lowest row wins a tie; one thread per molecule atom, a loop over T: near_T.  "Within radius^2" is the start value of
//       the running minimum (radius^2 + 1), not a second comparison.
//   (C) located = mutual nearest; matched = same symbol and charge (one thread per annotated atom)
//   (D) one thread per molecule bond: both ends located, then a scan of the record's pair keys (first listing wins)
//   (E) lane 0 writes the row and adds it to the totals (64-bit atomicAdd, non-zero columns only)
//
// Distances are 64-bit: hand-made rows may hold any int32 cell.
#include "common.hpp"
#include "../../include/abcnet_hip.h"
#include "capi_util.hpp"
#include "mol_rows.hpp"

namespace {

constexpr int GT = 256;              // threads per workgroup
constexpr int MAX_ATOMS = ABC_MAX_CAP_ATOMS;
constexpr int MAX_REC = ABC_MAX_SCORE_RECORD;      // pair key = lower index << 10 | higher index
static_assert(MAX_REC <= 1 << 10, "a record atom index fits the 10 bits of a pair key");
constexpr int MAX_RADIUS = 1 << 15;
constexpr int NCOL = ABC_GS_NCOL;

__global__ __launch_bounds__(GT) void graph_score_kernel(const abc_graph_score_desc d) {
    __shared__ int2 ppos[MAX_ATOMS];     // molecule atoms (x, y)
    __shared__ int near_t[MAX_ATOMS];    // per molecule atom: its nearest atom of T, or -1
    __shared__ int2 tpos[MAX_REC];       // annotated atoms (x, y)
    __shared__ int in_t[MAX_REC];        // annotated atom occurs in a record bond
    __shared__ int near_p[MAX_REC];      // per annotated atom of T: its nearest molecule atom, or -1
    __shared__ int rkey[MAX_REC];        // record bond: lower end << 10 | higher end, -1 for a row that names no pair
    __shared__ int acc[NCOL];
    const int b = blockIdx.x, tid = threadIdx.x;
    ScoredImage im;
    if (!scored_image<NCOL>(d, b, tid, im)) return;
    const auto [nt, m, status, na, nb, empty, pa, pb, ra, rb] = im;

    // ---- (A)
    if (tid < NCOL) acc[tid] = 0;
    for (int a = tid; a < nt; a += GT) {
        tpos[a] = make_int2(ra[a * REC_ATOM_W], ra[a * REC_ATOM_W + 1]);
        in_t[a] = 0;
    }
    for (int p = tid; p < na; p += GT) ppos[p] = make_int2(pa[p * ATOM_W], pa[p * ATOM_W + 1]);
    __syncthreads();
    for (int k = tid; k < m; k += GT) {
        int i, j, key = -1;
        if (rec_ends(rb, k, nt, i, j)) {
            key = (min(i, j) << 10) | max(i, j);
            atomicOr(in_t + i, 1);
            atomicOr(in_t + j, 1);
        }
        rkey[k] = key;
    }
    __syncthreads();

    // ---- (B) the two nearest searches
    const long long start = (long long)d.radius * d.radius + 1;
    int n_true = 0;
    for (int a = tid; a < nt; a += GT) {
        int best = -1;
        if (in_t[a]) {
            ++n_true;
            const int2 q = tpos[a];
            long long bd = start;
            for (int p = 0; p < na; ++p) {
                const int2 c = ppos[p];
                const long long dx = (long long)c.x - q.x, dy = (long long)c.y - q.y, dist = dx * dx + dy * dy;
                if (dist < bd) { bd = dist; best = p; }
            }
        }
        near_p[a] = best;
    }
    for (int p = tid; p < na; p += GT) {
        const int2 q = ppos[p];
        long long bd = start;
        int best = -1;
        for (int a = 0; a < nt; ++a) {
            if (!in_t[a]) continue;          // (the same `a` in every lane: uniform)
            const int2 c = tpos[a];
            const long long dx = (long long)c.x - q.x, dy = (long long)c.y - q.y, dist = dx * dx + dy * dy;
            if (dist < bd) { bd = dist; best = a; }
        }
        near_t[p] = best;
    }
    __syncthreads();

    // ---- (C) located and matched atoms
    int located = 0, matched = 0;
    for (int a = tid; a < nt; a += GT) {
        const int p = near_p[a];
        if (p < 0 || near_t[p] != a) continue;
        ++located;
        const int want = symbol_class(ra[a * REC_ATOM_W + 2]), got = symbol_class(pa[p * ATOM_W + 2]);
        if (want >= 0 && want == got && ra[a * REC_ATOM_W + 3] == pa[p * ATOM_W + 3]) ++matched;
    }
    // ---- (D) paired and matched bonds
    int paired = 0, bmatched = 0;
    for (int q = tid; q < nb; q += GT) {
        int e1, e2;
        if (!mol_ends(pb, q, na, e1, e2)) continue;
        const int a1 = near_t[e1], a2 = near_t[e2];
        if (a1 < 0 || a2 < 0 || near_p[a1] != e1 || near_p[a2] != e2) continue;
        const int key = (min(a1, a2) << 10) | max(a1, a2);
        for (int k = 0; k < m; ++k) {
            if (rkey[k] != key) continue;
            ++paired;
            if (rb[k * REC_BOND_W + 2] == pb[q * MOL_BOND_W + 2]) ++bmatched;
            break;
        }
    }
    if (n_true) atomicAdd(acc + ABC_GS_ATOMS_TRUE, n_true);
    if (located) atomicAdd(acc + ABC_GS_ATOMS_LOCATED, located);
    if (matched) atomicAdd(acc + ABC_GS_ATOMS_MATCHED, matched);
    if (paired) atomicAdd(acc + ABC_GS_BONDS_PAIRED, paired);
    if (bmatched) atomicAdd(acc + ABC_GS_BONDS_MATCHED, bmatched);
    __syncthreads();

    // ---- (E)
    if (tid == 0) {
        int r[NCOL];
#pragma unroll
        for (int i = 0; i < NCOL; ++i) r[i] = 0;
        r[ABC_GS_COUNTED] = 1;
        r[ABC_GS_ATOMS_TRUE] = acc[ABC_GS_ATOMS_TRUE];
        r[ABC_GS_BONDS_TRUE] = m;
        if (empty) {
            r[ABC_GS_NONE] = 1;
        } else {
            r[ABC_GS_TRUNCATED] = (status & ABC_MOL_TRUNCATED) ? 1 : 0;
            r[ABC_GS_ATOMS_PRED] = na;
            r[ABC_GS_BONDS_PRED] = nb;
            r[ABC_GS_ATOMS_LOCATED] = acc[ABC_GS_ATOMS_LOCATED];
            r[ABC_GS_ATOMS_MATCHED] = acc[ABC_GS_ATOMS_MATCHED];
            r[ABC_GS_BONDS_PAIRED] = acc[ABC_GS_BONDS_PAIRED];
            r[ABC_GS_BONDS_MATCHED] = acc[ABC_GS_BONDS_MATCHED];
            r[ABC_GS_ATOMS_EQUAL] = r[ABC_GS_ATOMS_MATCHED] == r[ABC_GS_ATOMS_TRUE] && r[ABC_GS_ATOMS_TRUE] == na;
            r[ABC_GS_BONDS_EQUAL] = r[ABC_GS_BONDS_MATCHED] == m && m == nb;
            r[ABC_GS_EXACT] = r[ABC_GS_ATOMS_EQUAL] && r[ABC_GS_BONDS_EQUAL];
        }
        write_row_and_totals<NCOL>(d.rows + (size_t)b * NCOL, d.totals, r);
    }
}

}  // namespace

extern "C" int abc_graph_score_desc_size(void) { return (int)sizeof(abc_graph_score_desc); }

extern "C" int abc_graph_score_update(const abc_graph_score_desc* d, abc_stream_t stream) {
    if (d->B < 1) return abc_fail(ABC_EINVAL, "graph_score: empty");
    if (d->cap_atoms < 1 || d->cap_atoms > MAX_ATOMS) return abc_fail(ABC_EINVAL, "graph_score: cap_atoms must be 1..2048");
    if (d->cap_mol_bonds < 1) return abc_fail(ABC_EINVAL, "graph_score: cap_mol_bonds must be >= 1");
    if (d->max_atoms < 1 || d->max_atoms > MAX_REC) return abc_fail(ABC_EINVAL, "graph_score: max_atoms must be 1..1024");
    if (d->max_bonds < 1 || d->max_bonds > MAX_REC) return abc_fail(ABC_EINVAL, "graph_score: max_bonds must be 1..1024");
    if (d->radius < 0 || d->radius > MAX_RADIUS) return abc_fail(ABC_EINVAL, "graph_score: radius must be 0..32768 cells");
    if (!d->mol_counts || !d->mol_atoms || !d->mol_bonds) return abc_fail(ABC_EINVAL, "graph_score: null molecule buffer");
    if (!d->rec_atoms || !d->rec_bonds || !d->rec_counts) return abc_fail(ABC_EINVAL, "graph_score: null record buffer");
    if (!d->rows || !d->totals) return abc_fail(ABC_EINVAL, "graph_score: null output");
    hipLaunchKernelGGL(graph_score_kernel, dim3(d->B), dim3(GT), 0, (hipStream_t)stream, *d);
    return abc_check_launch("graph_score_update");
}
