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

// What a thread holds of its pair in registers: the two images (mol_rows.hpp), the sizes of the graphs, row `tid` of each side
struct Pair {
    int tid, n;                      // n: the atoms of either graph, once the sizes are equal
    int na, nb, nt, m, valid_p;      // molecule atoms and rows, record atoms and rows, the molecule's valid rows
    const int *pa, *pb, *ra, *rb;
    BondRow prow, trow;              // kept through every round (the record row's ends are numbers in T)
};
// The outcome and the work counters (uniform), the budgets, and refine_classes' `shared` (this thread's) and `zeros`
struct Outcome {
    int max_tries, max_rounds;
    int result, levels, tries, backtracks, rounds;
    u64 shared;
    int zeros;
};

// 46 KB of LDS and the steps of the test on them.  Every step is inlined into the kernel; each says which barriers it places
struct Ident {
    u64 cur[2][MAX_ATOMS];           // the ids of every atom
    u64 acc[MAX_ATOMS];              // the neighbour sum of the round (one side runs at a time); the record's degrees in (A)
    u64 init[MAX_ATOMS];             // id_0 of the record: where every replay starts
    u64 lv_sum[MAX_ATOMS], lv_cell[MAX_ATOMS];      // per level: sum of mix(id), the id of the cell
    u64 table[SLOTS];                // the ids of one side, open-addressed: the class count
    u64 wu[NW];
    int lv_rounds[MAX_ATOMS], lv_classes[MAX_ATOMS];
    int choice[MAX_ATOMS], nxt[MAX_ATOMS + 1];      // the record's stack: the atom taken, the first index not yet tried
    int remap[MAX_ATOMS];            // record atom -> its number in T, -1 outside T
    int orig[MAX_ATOMS];             // number in T -> record atom
    int mapv[MAX_ATOMS];             // molecule atom -> number in T, at a leaf
    unsigned wt[NW + 1];
    int wi[NW];
    int cnt[2];                      // valid molecule bonds, valid record bonds

    // one round of side `s` (uniform); acc is zero on entry and on exit.  Barriers: between the halves, behind the new ids
    __device__ __forceinline__ void round(const Pair& p, int s, u64 r) {
        if (s == 0) refine_add_mol(p.tid, cur[0], acc, p.pb, p.nb, p.na, p.prow);
        else refine_add_rec(p.tid, cur[1], acc, p.rb, p.m, p.nt, remap, p.trow);
        __syncthreads();
        refine_finish(p.tid, cur[s], acc, p.n, r);
        __syncthreads();
    }
    // the number of distinct ids of side `s`, exactly; q.shared keeps this thread's least id two atoms share, q.zeros (uniform) the
    // number of ids that are 0, for the cell of the level
    __device__ __forceinline__ int classes(const Pair& p, Outcome& q, int s) { return refine_classes<SLOTS>(p.tid, cur[s], p.n, table, wi, q.shared, q.zeros); }

    // ---- (A) degrees, T, id_0 (graph_refine.hpp; the molecule's degrees in cur[1] to save LDS, the record's in acc); (a) true when
    // the sizes are equal.  Barriers: behind the clearing, behind the degrees, behind remap / orig / id_0
    __device__ __forceinline__ bool setup(const ScoredImage& im, Pair& p) {
        const int tid = p.tid = threadIdx.x;
        p.na = im.na, p.nb = im.nb, p.nt = im.nt, p.m = im.m, p.pa = im.pa, p.pb = im.pb, p.ra = im.ra, p.rb = im.rb;
        const BondRow none = {false, 0, 0, 0};
        p.prow = tid < p.nb ? mol_row(p.pb, tid, p.na) : none;
        p.trow = tid < p.m ? rec_row(p.rb, tid, p.nt) : none;
        if (tid < 2) cnt[tid] = 0;
        for (int a = tid; a < MAX_ATOMS; a += GT) cur[1][a] = acc[a] = 0;
        __syncthreads();
        {
            const int valid_p = refine_degrees_mol(tid, p.pb, p.nb, p.na, p.prow, cur[1]), valid_t = refine_degrees_rec(tid, p.rb, p.m, p.nt, p.trow, acc);
            if (valid_p) atomicAdd(cnt + 0, valid_p);
            if (valid_t) atomicAdd(cnt + 1, valid_t);
        }
        __syncthreads();
        refine_id0_mol(tid, p.pa, p.na, cur[1], cur[0]);
        // (id_0 of the record goes into init alone: cur[1], the molecule's degrees until here, becomes the record's ids when the search
        // begins, by the replay of level 0)
        const int n_t = refine_number_rec(tid, p.ra, p.nt, acc, wt, remap, orig, init);      // |T|
        __syncthreads();
        renumber(p.trow, remap);
        p.valid_p = cnt[0];
        p.n = p.na;
        return !im.empty && p.na == n_t && p.valid_p == cnt[1];
    }

    // ---- (b) the molecule's path: per level its rounds, the record of the level, then the cell's first atom individualised.  Sets
    // q.levels, or q.result = UNDECIDED.  Barriers of its own: behind every individualisation, behind the level records
    __device__ __forceinline__ void molecule_path(const Pair& p, Outcome& q) {
        const int tid = p.tid, n = p.n;
        int level = 0, prev = classes(p, q, 0);
        u64 r = 0;
        while (true) {
            const LevelRun lv = refine_level(n, prev, q.rounds, q.max_rounds, r, [&](u64 r_) __attribute__((always_inline)) { round(p, 0, r_); },
                                             [&]() __attribute__((always_inline)) { return classes(p, q, 0); });
            if (lv.out) { q.result = UNDECIDED; break; }
            const u64 sum = refine_multiset_sum(tid, cur[0], n, wu);
            if (tid == 0) lv_rounds[level] = lv.rounds, lv_sum[level] = sum, lv_classes[level] = lv.classes;
            if (lv.classes == n) break;
            // the cell: the least id that two atoms share, then its first atom
            const u64 cell = refine_cell(q.shared, q.zeros, wu);
            const int v = cell_member<false>(tid, cur[0], n, cell, 0, wi);
            if (level + 1 >= n || v >= n) { q.result = UNDECIDED; break; }      // (only colliding hashes get here)
            if (tid == 0) lv_cell[level] = cell, cur[0][v] = indiv(cur[0][v], level);
            __syncthreads();
            ++level;
            prev = lv.classes + 1;
        }
        q.levels = q.result ? 0 : level;
        __syncthreads();                 // (the level records are written)
    }

    // ---- (d) the leaf: true when mapping by equal id is an isomorphism -- every molecule atom has one record atom of its id (a scan:
    // the leaf is met once per image, see graph_refine.hpp), of its class and charge, and the multiset of the mapped rows is the
    // record's.  Barriers: the two reductions' (the first is behind mapv)
    __device__ __forceinline__ bool verify(const Pair& p) {
        const int tid = p.tid, n = p.n;
        int bad = 0;
        for (int a = tid; a < n; a += GT) {
            const u64 e = cur[0][a];
            int hits = 0, t = 0;
            for (int i = 0; i < n; ++i)
                if (cur[1][i] == e) ++hits, t = i;
            mapv[a] = t;
            const int o = orig[t];
            bad += hits != 1 || atom_class(p.pa[a * ATOM_W + 2]) != atom_class(p.ra[o * REC_ATOM_W + 2]) || p.pa[a * ATOM_W + 3] != p.ra[o * REC_ATOM_W + 3];
        }
        if (block_reduce(bad, wi, [](int u, int v) { return u + v; })) return false;
        // a molecule row is counted when fewer equal mapped rows stand before it than the record has rows equal to it (two loops:
        // the molecule's rows before q, then the record's; why this is not the canonical order's loop: graph_refine.hpp)
        int common = 0;
        for (int q = tid; q < p.nb; q += GT) {
            const BondRow e = mol_row(p.pb, q, p.na);
            if (!e.v) continue;
            const int lo = min(mapv[e.i], mapv[e.j]), hi = max(mapv[e.i], mapv[e.j]);
            int before = 0, there = 0;
            for (int q2 = 0; q2 < q; ++q2) {
                const BondRow e2 = mol_row(p.pb, q2, p.na);
                if (!e2.v) continue;
                before += min(mapv[e2.i], mapv[e2.j]) == lo && max(mapv[e2.i], mapv[e2.j]) == hi && e2.o == e.o;
            }
            for (int k = 0; k < p.m; ++k) {
                const BondRow t = rec_row(p.rb, k, p.nt, remap);
                if (!t.v) continue;
                there += min(t.i, t.j) == lo && max(t.i, t.j) == hi && t.o == e.o;
            }
            common += before < there;
        }
        return block_reduce(common, wi, [](int u, int v) { return u + v; }) == p.valid_p;
    }

    // ---- (c) the record's search, depth first, doing what (b) recorded.  Sets q.result.  Barriers of its own: behind nxt[0], behind
    // every individualisation with its stack entries
    __device__ __forceinline__ void record_search(const Pair& p, Outcome& q) {
        const int tid = p.tid, n = p.n;
        u64 rt = 0;
        auto round1 = [&](u64 r) __attribute__((always_inline)) { round(p, 1, r); };
        // the class count and the sum of the record's ids are those recorded for level k: else the branch is proved wrong
        auto matches = [&](int k) __attribute__((always_inline)) {
            const int c = classes(p, q, 1);
            const u64 s = refine_multiset_sum(tid, cur[1], n, wu);
            return c == lv_classes[k] && s == lv_sum[k];
        };
        auto replay = [&](int upto) __attribute__((always_inline)) {
            return refine_replay(tid, cur[1], init, n, upto, lv_rounds, choice, q.rounds, q.max_rounds, rt, round1);
        };
        int level = 0;
        bool ok = false;
        if (!replay(0)) q.result = UNDECIDED;
        else ok = matches(0);
        if (tid == 0) nxt[0] = 0;
        __syncthreads();
        while (!q.result) {
            if (ok && level == q.levels) {
                if (verify(p)) { q.result = SAME; break; }
                ok = false;
            }
            if (ok) {
                // the candidates of the level: the record atoms whose id is the recorded cell id, in index order
                const int v = cell_member<false>(tid, cur[1], n, lv_cell[level], nxt[level], wi);
                if (v < n) {
                    if (q.tries >= q.max_tries) { q.result = UNDECIDED; break; }
                    ++q.tries;
                    if (tid == 0) choice[level] = v, nxt[level] = v + 1, nxt[level + 1] = 0, cur[1][v] = indiv(cur[1][v], level);
                    __syncthreads();
                    ++level;
                    if (!refine_rounds(lv_rounds[level], q.rounds, q.max_rounds, rt, round1)) { q.result = UNDECIDED; break; }
                    ok = matches(level);
                    continue;
                }
            }
            if (level == 0) { q.result = DIFFERENT; break; }
            ++q.backtracks;
            --level;
            if (!replay(level)) { q.result = UNDECIDED; break; }      // a failed branch: the ids of the level above, rebuilt
            ok = true;
        }
    }

    // ---- the map of a verified pair (else -1 everywhere) and the stats row with its totals.  Barrier: in front (mapv, orig)
    __device__ __forceinline__ void write(const abc_graph_identity_desc& d, int b, const ScoredImage& im, const Pair& p, const Outcome& q, bool size_equal) {
        __syncthreads();
        if (d.map_out != nullptr) {
            int* const map_row = d.map_out + (size_t)b * d.cap_atoms;
            for (int a = p.tid; a < d.cap_atoms; a += GT) map_row[a] = q.result == SAME && a < p.n ? orig[mapv[a]] : -1;
        }
        if (p.tid != 0) return;
        int r[NCOL];
#pragma unroll
        for (int i = 0; i < NCOL; ++i) r[i] = 0;
        r[ABC_IDENT_COUNTED] = 1;
        if (im.empty) {
            r[ABC_IDENT_NONE] = 1;
        } else {
            r[ABC_IDENT_TRUNCATED] = (im.status & ABC_MOL_TRUNCATED) ? 1 : 0;
            r[ABC_IDENT_SIZE_EQUAL] = size_equal;
            r[ABC_IDENT_SAME] = q.result == SAME;
            r[ABC_IDENT_DIFFERENT] = q.result == DIFFERENT;
            r[ABC_IDENT_UNDECIDED] = q.result == UNDECIDED;
            r[ABC_IDENT_LEVELS] = q.levels;
            r[ABC_IDENT_TRIES] = q.tries;
            r[ABC_IDENT_BACKTRACKS] = q.backtracks;
            r[ABC_IDENT_ROUNDS] = q.rounds;
        }
        write_row_and_totals<NCOL>(d.rows + (size_t)b * NCOL, d.totals, r);
    }
};

__global__ __launch_bounds__(GT) void graph_ident_kernel(const abc_graph_identity_desc d) {
    __shared__ Ident s;
    const int b = blockIdx.x;
    ScoredImage im;
    if (!scored_image<NCOL>(d, b, threadIdx.x, im)) {
        if (d.map_out != nullptr)
            for (int a = threadIdx.x; a < d.cap_atoms; a += GT) d.map_out[(size_t)b * d.cap_atoms + a] = -1;
        return;
    }
    Pair p;
    Outcome q = {};
    q.max_tries = d.max_tries > 0 ? d.max_tries : ABC_IDENT_DEFAULT_TRIES;
    q.max_rounds = d.max_rounds > 0 ? d.max_rounds : ABC_IDENT_DEFAULT_ROUNDS;
    q.shared = ~0ull;
    const bool size_equal = s.setup(im, p);
    if (im.empty) {
        q.result = 0;
    } else if (!size_equal) {
        q.result = DIFFERENT;
    } else {
        s.molecule_path(p, q);
        if (!q.result) s.record_search(p, q);
    }
    s.write(d, b, im, p, q, size_equal);
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
