// The certain score after assembly: IS the molecule abc_assemble_graphs built the annotated molecule, without reading a position?
// (The reference's headline accuracy is the share of images whose canonical SMILES equal, cal_acc.py; graph_score.hip brackets it
// from below with positions, graph_sim.hip's refine_equal from above with colour refinement.  This is the middle column: an
// individualise-and-refine isomorphism test whose `same` is a VERIFIED bijection -- the contract is in include/abcnet_hip.h and
// DESIGN.md section 7, its executable form tests/graphident_oracle.py.)
//
// One workgroup per image; integers only (uint64, wrapping).  Side 0 is the molecule, side 1 the record.  The graphs, id_0 and the
// round id_r[a] = mix(mix(id[a] + r) + sum of mix(mix(id[j]) + order class)) are graph_sim.hip's (graph_ids.hpp, mol_rows.hpp).
//
//   (a) sizes: the atom counts and the valid-bond counts must be equal, else `different`
//   (b) the molecule walks ONE path to a discrete colouring.  Per level: rounds (r counts on through the levels) until one no longer
//       raises the number of distinct ids -- that round is counted, a level has at most n; the level's round count, the wrapping
//       sum of mix(id) and the class count are recorded; not discrete: the cell is the non-singleton class of the least id VALUE
//       (invariant under renumbering), its lowest-index member v is individualised, id[v] = indiv(id[v], level), one level down
//   (c) the record is searched depth first, doing exactly what (b) recorded: the same rounds per level, then the class count and
//       the sum must equal the record's -- a mismatch proves the branch wrong.  The candidates of a level are the record atoms
//       whose id is the recorded cell id, in index order.  A failed branch is a backtrack: the ids of the level above are rebuilt
//       by replaying the choices from level 0 (no id snapshots in LDS)
//   (d) at a leaf both colourings are discrete: map by equal id, VERIFY class and charge of every atom and, by counting, that the
//       multiset of (mapped end, mapped end, order class) of the molecule's valid rows is the record's.  Verified: `same`.  Not
//       verified (colliding hashes): the search goes on.  Search exhausted: `different`
//   (e) max_rounds is checked before every round of either side, max_tries before every individualisation of the record side;
//       running out gives `undecided`.  Every loop is bounded by n, by a budget or by a capacity
//   (f) every branch depends on values all threads hold alike (reductions read from LDS after a barrier, or descriptor fields)
//
// Bond rows are never held in LDS (row `tid` of each side stays in registers), so no bond capacity bounds the launch.  Every index
// read from a row is range-checked before it addresses anything: hand-made rows may hold any int32.
#include "common.hpp"
#include "../../include/abcnet_hip.h"
#include "capi_util.hpp"
#include "block_scan.hpp"
#include "mol_rows.hpp"
#include "graph_ids.hpp"
#include "graph_refine.hpp"

namespace {

constexpr int GT = REFINE_GT;         // threads per workgroup (graph_refine.hpp)
constexpr int MAX_ATOMS = ABC_MAX_SIM_ATOMS;      // ids of both sides, one sum, id_0 of the record, the level records, the class table: 46 KB of LDS
constexpr int NCOL = ABC_IDENT_NCOL;
constexpr int NW = GT / 64;
constexpr int SLOTS = 2 * MAX_ATOMS;  // of the class count's table: a power of two, at most half full
static_assert(MAX_ATOMS == 2 * GT, "two atoms per thread: the record scan, the class count");
enum { SAME = 1, DIFFERENT = 2, UNDECIDED = 3 };

__global__ __launch_bounds__(GT) void graph_ident_kernel(const abc_graph_identity_desc d) {
    __shared__ u64 cur[2][MAX_ATOMS];    // the ids of every atom
    __shared__ u64 acc[MAX_ATOMS];       // the neighbour sum of the round (one side runs at a time); the record's degrees in (A)
    __shared__ u64 init[MAX_ATOMS];      // id_0 of the record: where every replay starts
    __shared__ u64 lv_sum[MAX_ATOMS], lv_cell[MAX_ATOMS];      // per level: sum of mix(id), the id of the cell
    __shared__ int lv_rounds[MAX_ATOMS], lv_classes[MAX_ATOMS];
    __shared__ int choice[MAX_ATOMS], nxt[MAX_ATOMS + 1];      // the record's stack: the atom taken, the first index not yet tried
    __shared__ int remap[MAX_ATOMS];     // record atom -> its number in T, -1 outside T
    __shared__ int orig[MAX_ATOMS];      // number in T -> record atom
    __shared__ int mapv[MAX_ATOMS];      // molecule atom -> number in T, at a leaf
    __shared__ u64 table[SLOTS];         // the ids of one side, open-addressed: the class count
    __shared__ unsigned wt[NW + 1];
    __shared__ int wi[NW];
    __shared__ u64 wu[NW];
    __shared__ int cnt[2];               // valid molecule bonds, valid record bonds
    const int b = blockIdx.x, tid = threadIdx.x;
    int* const map_row = d.map_out != nullptr ? d.map_out + (size_t)b * d.cap_atoms : nullptr;
    ScoredImage im;
    if (!scored_image<NCOL>(d, b, tid, im)) {
        if (map_row != nullptr)
            for (int a = tid; a < d.cap_atoms; a += GT) map_row[a] = -1;
        return;
    }
    const int nt = im.nt, m = im.m, status = im.status, na = im.na, nb = im.nb;      // (plain locals: the lambdas below capture them)
    const bool empty = im.empty;
    const int *const pa = im.pa, *const pb = im.pb, *const ra = im.ra, *const rb = im.rb;
    const int max_tries = d.max_tries > 0 ? d.max_tries : ABC_IDENT_DEFAULT_TRIES;
    const int max_rounds = d.max_rounds > 0 ? d.max_rounds : ABC_IDENT_DEFAULT_ROUNDS;

    // row `tid` of each side, kept through every round
    const BondRow none = {false, 0, 0, 0};
    const BondRow prow = tid < nb ? mol_row(pb, tid, na) : none;
    BondRow trow = tid < m ? rec_row(rb, tid, nt) : none;

    // ---- (A) degrees, T, id_0 (graph_refine.hpp; the molecule's degrees in cur[1] to save LDS, the record's in acc)
    if (tid < 2) cnt[tid] = 0;
    for (int a = tid; a < MAX_ATOMS; a += GT) cur[1][a] = acc[a] = 0;
    __syncthreads();
    {
        const int valid_p = refine_degrees_mol(tid, pb, nb, na, prow, cur[1]), valid_t = refine_degrees_rec(tid, rb, m, nt, trow, acc);
        if (valid_p) atomicAdd(cnt + 0, valid_p);
        if (valid_t) atomicAdd(cnt + 1, valid_t);
    }
    __syncthreads();
    refine_id0_mol(tid, pa, na, cur[1], cur[0]);
    // (id_0 of the record goes into init alone: cur[1], the molecule's degrees until here, becomes the record's ids when the search
    // begins, by replay(0))
    const int n_t = refine_number_rec(tid, ra, nt, acc, wt, remap, orig, init);      // |T|
    __syncthreads();
    renumber(trow, remap);
    const int valid_p = cnt[0], valid_t = cnt[1];
    const bool size_equal = !empty && na == n_t && valid_p == valid_t;
    const int n = na;

    // one round of side `s` (uniform); acc is zero on entry and on exit
    auto round = [&](int s, u64 r) __attribute__((always_inline)) {
        if (s == 0) refine_add_mol(tid, cur[0], acc, pb, nb, na, prow);
        else refine_add_rec(tid, cur[1], acc, rb, m, nt, remap, trow);
        __syncthreads();
        refine_finish(tid, cur[s], acc, n, r);
        __syncthreads();
    };
    // the number of distinct ids, exactly; `shared` keeps this thread's least id two atoms share, `zeros` (uniform) the number of
    // ids that are 0, for the cell of the level
    u64 shared = ~0ull;
    int zeros = 0;
    auto classes = [&](const u64* id) __attribute__((always_inline)) { return refine_classes<SLOTS>(tid, id, n, table, wi, shared, zeros); };
    auto multiset_sum = [&](const u64* id) __attribute__((always_inline)) { return refine_multiset_sum(tid, id, n, wu); };

    int result = 0, levels = 0, tries = 0, backtracks = 0, rounds = 0;
    if (empty) {
        result = 0;
    } else if (!size_equal) {
        result = DIFFERENT;
    } else {
        // ---- (b) the molecule's path
        int level = 0, prev = classes(cur[0]);
        u64 r = 0;
        while (true) {
            int k = 0, c = 0;
            while (true) {
                if (rounds >= max_rounds) { result = UNDECIDED; break; }
                ++rounds, ++r, ++k;
                round(0, r);
                c = classes(cur[0]);
                if (c <= prev || k >= n) break;
                prev = c;
            }
            if (result) break;
            const u64 sum = multiset_sum(cur[0]);
            if (tid == 0) lv_rounds[level] = k, lv_sum[level] = sum, lv_classes[level] = c;
            if (c == n) break;
            // the cell: the least id that two atoms share, then its first atom
            const u64 least = block_reduce(shared, wu, [](u64 u, u64 v) { return min(u, v); });
            const u64 cell = zeros > 1 ? 0 : least;
            int first = MAX_ATOMS;
            for (int a = tid; a < n; a += GT)
                if (cur[0][a] == cell) first = min(first, a);
            const int v = block_reduce(first, wi, [](int u, int w) { return min(u, w); });
            if (level + 1 >= n || v >= n) { result = UNDECIDED; break; }      // (only colliding hashes get here)
            if (tid == 0) lv_cell[level] = cell, cur[0][v] = indiv(cur[0][v], level);
            __syncthreads();
            ++level;
            prev = c + 1;
        }
        levels = result ? 0 : level;
        __syncthreads();                 // (the level records are written)

        // ---- (c) the record's search
        u64 rt = 0;
        // the recorded rounds of level k on the record's ids; false: out of rounds
        auto refine = [&](int k) __attribute__((always_inline)) {
            const int todo = lv_rounds[k];
            for (int i = 0; i < todo; ++i) {
                if (rounds >= max_rounds) return false;
                ++rounds, ++rt;
                round(1, rt);
            }
            return true;
        };
        auto matches = [&](int k) __attribute__((always_inline)) {
            const int c = classes(cur[1]);
            const u64 s = multiset_sum(cur[1]);
            return c == lv_classes[k] && s == lv_sum[k];
        };
        // the ids after the rounds of level `upto` under choice[0 .. upto - 1]; false: out of rounds
        auto replay = [&](int upto) __attribute__((always_inline)) {
            for (int a = tid; a < n; a += GT) cur[1][a] = init[a];
            __syncthreads();
            rt = 0;
            for (int k = 0; k <= upto; ++k) {
                if (!refine(k)) return false;
                if (k < upto) {
                    if (tid == 0) cur[1][choice[k]] = indiv(cur[1][choice[k]], k);
                    __syncthreads();
                }
            }
            return true;
        };
        // (d) the leaf: true when mapping by equal id is an isomorphism
        auto verify = [&]() __attribute__((always_inline)) {
            int bad = 0;
            for (int a = tid; a < n; a += GT) {
                const u64 e = cur[0][a];
                int hits = 0, t = 0;
                for (int i = 0; i < n; ++i)
                    if (cur[1][i] == e) ++hits, t = i;
                mapv[a] = t;
                const int o = orig[t];
                bad += hits != 1 || atom_class(pa[a * ATOM_W + 2]) != atom_class(ra[o * REC_ATOM_W + 2]) ||
                       pa[a * ATOM_W + 3] != ra[o * REC_ATOM_W + 3];
            }
            if (block_reduce(bad, wi, [](int u, int v) { return u + v; })) return false;
            int common = 0;
            for (int q = tid; q < nb; q += GT) {
                const BondRow e = mol_row(pb, q, na);
                if (!e.v) continue;
                const int lo = min(mapv[e.i], mapv[e.j]), hi = max(mapv[e.i], mapv[e.j]);
                int before = 0, there = 0;
                for (int q2 = 0; q2 < q; ++q2) {
                    const BondRow e2 = mol_row(pb, q2, na);
                    if (!e2.v) continue;
                    before += min(mapv[e2.i], mapv[e2.j]) == lo && max(mapv[e2.i], mapv[e2.j]) == hi && e2.o == e.o;
                }
                for (int k = 0; k < m; ++k) {
                    const BondRow t = rec_row(rb, k, nt, remap);
                    if (!t.v) continue;
                    there += min(t.i, t.j) == lo && max(t.i, t.j) == hi && t.o == e.o;
                }
                common += before < there;
            }
            return block_reduce(common, wi, [](int u, int v) { return u + v; }) == valid_p;
        };

        if (!result) {
            int level = 0;
            bool ok = false;
            if (!replay(0)) result = UNDECIDED;
            else ok = matches(0);
            if (tid == 0) nxt[0] = 0;
            __syncthreads();
            while (!result) {
                if (ok && level == levels) {
                    if (verify()) { result = SAME; break; }
                    ok = false;
                }
                if (ok) {
                    const u64 cell = lv_cell[level];
                    const int from = nxt[level];
                    int first = MAX_ATOMS;
                    for (int a = tid; a < n; a += GT)
                        if (a >= from && cur[1][a] == cell) first = min(first, a);
                    const int v = block_reduce(first, wi, [](int u, int w) { return min(u, w); });
                    if (v < n) {
                        if (tries >= max_tries) { result = UNDECIDED; break; }
                        ++tries;
                        if (tid == 0) choice[level] = v, nxt[level] = v + 1, nxt[level + 1] = 0, cur[1][v] = indiv(cur[1][v], level);
                        __syncthreads();
                        ++level;
                        if (!refine(level)) { result = UNDECIDED; break; }
                        ok = matches(level);
                        continue;
                    }
                }
                if (level == 0) { result = DIFFERENT; break; }
                ++backtracks;
                --level;
                if (!replay(level)) { result = UNDECIDED; break; }
                ok = true;
            }
        }
    }
    __syncthreads();
    if (map_row != nullptr)
        for (int a = tid; a < d.cap_atoms; a += GT) map_row[a] = result == SAME && a < n ? orig[mapv[a]] : -1;

    if (tid == 0) {
        int r[NCOL];
#pragma unroll
        for (int i = 0; i < NCOL; ++i) r[i] = 0;
        r[ABC_IDENT_COUNTED] = 1;
        if (empty) {
            r[ABC_IDENT_NONE] = 1;
        } else {
            r[ABC_IDENT_TRUNCATED] = (status & ABC_MOL_TRUNCATED) ? 1 : 0;
            r[ABC_IDENT_SIZE_EQUAL] = size_equal;
            r[ABC_IDENT_SAME] = result == SAME;
            r[ABC_IDENT_DIFFERENT] = result == DIFFERENT;
            r[ABC_IDENT_UNDECIDED] = result == UNDECIDED;
            r[ABC_IDENT_LEVELS] = levels;
            r[ABC_IDENT_TRIES] = tries;
            r[ABC_IDENT_BACKTRACKS] = backtracks;
            r[ABC_IDENT_ROUNDS] = rounds;
        }
        write_row_and_totals<NCOL>(d.rows + (size_t)b * NCOL, d.totals, r);
    }
}

}  // namespace

extern "C" int abc_graph_identity_desc_size(void) { return (int)sizeof(abc_graph_identity_desc); }

extern "C" int abc_graph_identity_update(const abc_graph_identity_desc* d, abc_stream_t stream) {
    if (d->B < 1) return abc_fail(ABC_EINVAL, "graph_identity: empty");
    if (d->cap_atoms < 1 || d->cap_atoms > MAX_ATOMS) return abc_fail(ABC_EINVAL, "graph_identity: cap_atoms must be 1..512");
    if (d->cap_mol_bonds < 1) return abc_fail(ABC_EINVAL, "graph_identity: cap_mol_bonds must be >= 1");
    if (d->max_atoms < 1 || d->max_atoms > MAX_ATOMS) return abc_fail(ABC_EINVAL, "graph_identity: max_atoms must be 1..512");
    if (d->max_bonds < 1) return abc_fail(ABC_EINVAL, "graph_identity: max_bonds must be >= 1");
    if (d->max_tries < 0) return abc_fail(ABC_EINVAL, "graph_identity: max_tries must be >= 0 (0: the default)");
    if (d->max_rounds < 0) return abc_fail(ABC_EINVAL, "graph_identity: max_rounds must be >= 0 (0: the default)");
    if (!d->mol_counts || !d->mol_atoms || !d->mol_bonds) return abc_fail(ABC_EINVAL, "graph_identity: null molecule buffer");
    if (!d->rec_atoms || !d->rec_bonds || !d->rec_counts) return abc_fail(ABC_EINVAL, "graph_identity: null record buffer");
    if (!d->rows || !d->totals) return abc_fail(ABC_EINVAL, "graph_identity: null output");
    hipLaunchKernelGGL(graph_ident_kernel, dim3(d->B), dim3(GT), 0, (hipStream_t)stream, *d);
    return abc_check_launch("graph_identity_update");
}
