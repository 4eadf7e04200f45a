// Individualise-and-refine on the graphs of graph_ids.hpp, for one workgroup of 256 threads per image: what the environment similarity
// (graph_sim.hip), the identity test (graph_ident.hip) and the canonical order (graph_canon.hip) share, so that the three cannot drift
// apart -- a bond row as a thread holds it, stage (A) (degrees, the numbering of a record's bonded atoms, id_0), the round in its two
// halves, the id of an individualised atom, the workgroup reduction, the exact class count through an LDS table, and the pieces of the
// SEARCH that the identity and the canonical order both run: the rounds of a level, the replay of a path, the cell and its members.
//
// Every piece is a function that works on the caller's LDS arrays; none branches on which kernel calls it.  Stage (A) and the halves of
// the round do not synchronise: the callers place the barriers, and say why there.  The pieces that do synchronise say so in their
// comment: block_reduce, refine_number_rec (its scan), refine_classes and refine_multiset_sum (their reductions), and of the search
// refine_replay, refine_cell and cell_member; refine_level and refine_rounds hold only the barriers of the `round` and `classes` they
// are given.
//
// STILL WRITTEN IN BOTH SEARCH KERNELS, and why:
//   - "the multiset of the mapped rows equals the multiset of the rows, by counting" (Ident::verify, Canon::map_onto_best).  The
//     canonical order maps a graph onto ITSELF, so one loop reads every row once for both counts; the identity has two sides and reads
//     the molecule's rows before q, then the record's.  One function over two row readers and a map (one loop, the second side first,
//     the first side's row under `q2 < q`) was measured: the identity's reads stay, but the canonical order's row reader branches on
//     its side, the two reads of a row are not merged, and the launch on the trained fixture took 55.1 us for 49.2 (plain, `raw`),
//     63.4 for 57.9 (`peaks`), 170 propanes at capacity 31.5 ms for 29.5 (profiles/r29_graph_search.md).  The identity's two-loop form
//     for both would read every row of the canonical order 1.5 times.  So each kernel keeps its loop; they state the same test.
//   - the map of a leaf onto the other colouring by equal id.  The identity scans (quadratic, no table: its leaf is met once per image),
//     the canonical order looks the ids up in the class table (one leaf per automorphism).  Two algorithms with two costs, not one
//     piece written twice; id_table_put / id_table_find below are the table's only insert and lookup.
//   - what a level records and what is done with it: the identity records the molecule's trace and demands it of the record, the
//     canonical order compares the trace of the path with the best leaf's.  The order of the search (one path and a depth-first match
//     against all the tree with orbit pruning) is what makes them two kernels.
#pragma once
#include "block_scan.hpp"
#include "mol_rows.hpp"
#include "graph_ids.hpp"

constexpr int REFINE_GT = 256;       // threads per workgroup
constexpr int REFINE_NW = REFINE_GT / 64;

// the id of the atom individualised at `level`
__device__ inline u64 indiv(u64 id, int level) { return mix(mix(id) + 0x9E3779B97F4A7C15ull * (u64)(level + 1)); }

// f over the workgroup's values; wt = LDS scratch [REFINE_NW].  Every thread must call it (it synchronises, before and after)
template <class T, class F>
__device__ inline T block_reduce(T v, T* wt, F f) {
#pragma unroll
    for (int o = 32; o; o >>= 1) v = f(v, (T)__shfl_xor(v, o));
    __syncthreads();                 // wt may still be read from the previous call; what the callers wrote before is visible after
    if ((threadIdx.x & 63) == 0) wt[threadIdx.x >> 6] = v;
    __syncthreads();
    return f(f(wt[0], wt[1]), f(wt[2], wt[3]));
}
static_assert(REFINE_NW == 4, "block_reduce folds four waves");

// ---- a bond row: v, it names a pair of atoms of its side; its ends i and j as atom numbers; its order class.  A thread keeps row `tid`
// of a side in registers through every round (tens of bonds per drawing: most launches read no bond row twice); the rows past the
// workgroup's 256 threads are read from global memory again, by the same readers.  The bond code is read with the ends, whatever
// they hold (the row is there): one load per row, not a second one that waits for the first
struct BondRow {
    bool v;
    int i, j, o;
};
__device__ inline BondRow mol_row(const int* pb, int q, int na) {
    BondRow e = {false, 0, 0, bond_class(pb[q * MOL_BOND_W + 2])};
    e.v = mol_ends(pb, q, na, e.i, e.j);
    return e;
}
// (ends in the record's own numbering: what the degrees are counted in)
__device__ inline BondRow rec_row(const int* rb, int k, int nt) {
    BondRow e = {false, 0, 0, bond_class(rb[k * REC_BOND_W + 2])};
    e.v = rec_ends(rb, k, nt, e.i, e.j);
    return e;
}
// the ends of a record row as numbers in T (remap: record atom -> its number in T; both ends of a valid row are in T: the row is one
// of those that put them there)
__device__ inline void renumber(BondRow& e, const int* remap) {
    if (e.v) e.i = remap[e.i], e.j = remap[e.j];
}
__device__ inline BondRow rec_row(const int* rb, int k, int nt, const int* remap) {
    BondRow e = rec_row(rb, k, nt);
    renumber(e, remap);
    return e;
}

// ---- stage (A), in the steps between the callers' barriers.  First the degrees of one side into deg (zero on entry) by 64-bit LDS
// adds, one per valid end; `own` is the caller's row `tid`.  Returns the number of valid rows this thread met
__device__ inline void count_ends(u64* deg, const BondRow& e) {
    atomicAdd(&deg[e.i], 1ull);
    atomicAdd(&deg[e.j], 1ull);
}
__device__ __forceinline__ int refine_degrees_mol(int tid, const int* pb, int nb, int na, const BondRow& own, u64* deg) {
    int valid = own.v;
    if (own.v) count_ends(deg, own);
    for (int q = tid + REFINE_GT; q < nb; q += REFINE_GT) {
        const BondRow e = mol_row(pb, q, na);
        if (!e.v) continue;
        ++valid;
        count_ends(deg, e);
    }
    return valid;
}
__device__ __forceinline__ int refine_degrees_rec(int tid, const int* rb, int m, int nt, const BondRow& own, u64* deg) {
    int valid = own.v;
    if (own.v) count_ends(deg, own);
    for (int k = tid + REFINE_GT; k < m; k += REFINE_GT) {
        const BondRow e = rec_row(rb, k, nt);
        if (!e.v) continue;
        ++valid;
        count_ends(deg, e);
    }
    return valid;
}
// Then, the degrees complete (a barrier of the caller): id_0 of every molecule atom into id and, where given, into layer as well.
// deg is read only
__device__ __forceinline__ void refine_id0_mol(int tid, const int* pa, int na, const u64* deg, u64* id, u64* layer = nullptr) {
    for (int a = tid; a < na; a += REFINE_GT) {
        const u64 e = id0(atom_class(pa[a * ATOM_W + 2]), pa[a * ATOM_W + 3], deg[a]);
        id[a] = e;
        if (layer != nullptr) layer[a] = e;
    }
}
// The record side: its atoms with a bond (the set T) are numbered in index order by a workgroup scan, two atoms per thread, their
// degrees in registers across it.  Writes remap (all of it: -1 outside T), orig (number in T -> record atom; may be null) and id_0 in
// T numbering into id (and into layer, where given), and leaves deg zero again: each degree is read, before the scan's barriers, and
// cleared by the one thread that numbers its atom.  Returns |T|; the caller's next barrier makes remap, orig and id visible (then
// renumber() the kept row).  wt = LDS scratch [REFINE_NW + 1]
template <class O>
__device__ __forceinline__ int refine_number_rec(int tid, const int* ra, int nt, u64* deg, unsigned* wt, int* remap, O* orig, u64* id,
                                                 u64* layer = nullptr) {
    const int a0 = 2 * tid, a1 = 2 * tid + 1;
    const u64 deg0 = a0 < nt ? deg[a0] : 0, deg1 = a1 < nt ? deg[a1] : 0;
    const unsigned f0 = deg0 != 0, f1 = deg1 != 0;
    unsigned total;
    const unsigned r0 = block_excl_scan<REFINE_GT>(f0 + f1, wt, &total), r1 = r0 + f0;
    remap[a0] = f0 ? (int)r0 : -1;
    remap[a1] = f1 ? (int)r1 : -1;
    auto number = [&](int a, unsigned t, u64 degree) __attribute__((always_inline)) {
        const u64 e = id0(atom_class(ra[a * REC_ATOM_W + 2]), ra[a * REC_ATOM_W + 3], degree);
        id[t] = e;
        if (layer != nullptr) layer[t] = e;
        if (orig != nullptr) orig[t] = (O)a;
    };
    if (f0) number(a0, r0, deg0);
    if (f1) number(a1, r1, deg1);
    deg[a0] = deg[a1] = 0;
    return (int)total;
}

// ---- one round, id_r[a] = mix(mix(id[a] + r) + sum over the rows at a of mix(mix(id[other end]) + order class)), in two halves with
// a barrier of the caller between them.  First the sums of one side's rows into acc (zero on entry): commutative, so no order of rows
// or atoms can change an id.  `own` is the caller's row `tid` (a record's: renumbered)
__device__ inline void add_terms(u64* acc, const u64* id, const BondRow& e) {
    const u64 at_i = id[e.i], at_j = id[e.j];      // (both read before either add: the two hash chains overlap)
    atomicAdd(&acc[e.i], mix(mix(at_j) + (u64)e.o));
    atomicAdd(&acc[e.j], mix(mix(at_i) + (u64)e.o));
}
__device__ __forceinline__ void refine_add_mol(int tid, const u64* id, u64* acc, const int* pb, int nb, int na, const BondRow& own) {
    if (own.v) add_terms(acc, id, own);
    for (int q = tid + REFINE_GT; q < nb; q += REFINE_GT) {
        const BondRow e = mol_row(pb, q, na);
        if (e.v) add_terms(acc, id, e);
    }
}
__device__ __forceinline__ void refine_add_rec(int tid, const u64* id, u64* acc, const int* rb, int m, int nt, const int* remap, const BondRow& own) {
    if (own.v) add_terms(acc, id, own);
    for (int k = tid + REFINE_GT; k < m; k += REFINE_GT) {
        const BondRow e = rec_row(rb, k, nt, remap);
        if (e.v) add_terms(acc, id, e);
    }
}
// Then the new ids of the side's n atoms, acc zero again; layer (may be null): the new ids are stored there as well
__device__ __forceinline__ void refine_finish(int tid, u64* id, u64* acc, int n, u64 r, u64* layer = nullptr) {
    for (int a = tid; a < n; a += REFINE_GT) {
        const u64 e = mix(mix(id[a] + r) + acc[a]);
        id[a] = e;
        acc[a] = 0;
        if (layer != nullptr) layer[a] = e;
    }
}

// ---- An open-addressed table of ids in LDS: SLOTS (a power of two) 64-bit words, 0 marks a free slot, so an id that IS 0 is never
// put (the callers count it apart).  id_table_put inserts e by compare-and-swap, in any order of the threads: slot >= 0 and fresh when
// e took a free slot, slot >= 0 and not fresh when e was there already (two atoms share it), slot < 0 when no slot was free (a table at
// most half full always has one).  id_table_find, after a barrier behind the puts: the slot that holds e, or -1.  Neither synchronises.
// The probe loops are not unrolled: the first probe nearly always ends them, and unrolled (the compiler's choice for a loop that
// returns) they add 2 KB of cold code per kernel and 1 % to a launch of the canonical order (profiles/r29_graph_search.md)
struct TableSlot {
    int slot;
    bool fresh;
};
template <int SLOTS>
__device__ __forceinline__ TableSlot id_table_put(u64* table, u64 e) {
    unsigned slot = (unsigned)(e >> 32) & (SLOTS - 1);
#pragma unroll 1
    for (int probe = 0; probe < SLOTS; ++probe) {
        const u64 old = atomicCAS(&table[slot], 0ull, e);
        if (old == 0 || old == e) return {(int)slot, old == 0};
        slot = (slot + 1) & (SLOTS - 1);
    }
    return {-1, false};
}
template <int SLOTS>
__device__ __forceinline__ int id_table_find(const u64* table, u64 e) {
    unsigned slot = (unsigned)(e >> 32) & (SLOTS - 1);
#pragma unroll 1
    for (int probe = 0; probe < SLOTS; ++probe) {
        const u64 at = table[slot];
        if (at == e) return (int)slot;
        if (at == 0) break;
        slot = (slot + 1) & (SLOTS - 1);
    }
    return -1;
}

// ---- The number of distinct ids, exactly: every id goes into the table of SLOTS >= 2 n slots (the ids that ARE 0 are counted apart),
// and the ids that found a free slot are counted -- as many as there are distinct values, in any order of the threads.  An id that
// finds itself there is shared by two atoms: `shared` keeps this thread's least such id, `zeros` (uniform) the number of ids that are
// 0, for the cell of the level (refine_cell).  wi = LDS scratch [REFINE_NW].  Barriers: one behind the clearing of the table, and the
// reduction's two (the first of them is behind every put)
template <int SLOTS>
__device__ __forceinline__ int refine_classes(int tid, const u64* id, int n, u64* table, int* wi, u64& shared, int& zeros) {
    for (int k = tid; k < SLOTS; k += REFINE_GT) table[k] = 0;
    __syncthreads();
    int fresh = 0, zero = 0;
    shared = ~0ull;
    for (int a = tid; a < n; a += REFINE_GT) {
        const u64 e = id[a];
        if (e == 0) {
            ++zero;
            continue;
        }
        const TableSlot at = id_table_put<SLOTS>(table, e);      // (n <= SLOTS / 2 ids: a free slot is always found)
        if (at.slot < 0) continue;
        if (at.fresh) ++fresh;
        else shared = min(shared, e);
    }
    const int both = block_reduce(fresh + (zero << 16), wi, [](int u, int v) { return u + v; });
    zeros = both >> 16;
    return (both & 0xFFFF) + (zeros > 0);
}
// the wrapping sum of mix(id) over the atoms; wu = LDS scratch [REFINE_NW]
__device__ __forceinline__ u64 refine_multiset_sum(int tid, const u64* id, int n, u64* wu) {
    u64 s = 0;
    for (int a = tid; a < n; a += REFINE_GT) s += mix(id[a]);
    return block_reduce(s, wu, [](u64 u, u64 v) { return u + v; });
}

// ---- The search of graph_ident.hip and graph_canon.hip.  `round(r)` runs round r on the caller's ids, both halves and their two
// barriers; `classes()` is the caller's refine_classes.  rounds / max_rounds: the image's count of rounds and its budget, checked BEFORE
// every round, replays included; r: the number of the round, which counts on through the levels of a path.
//
// The rounds of one level: until one no longer raises the class count (that round is counted), at most n.  prev: the class count the
// first round has to beat.  out: the budget ran out before round `rounds + 1` of the level; classes is then the count after the last
// round that ran (0: none ran)
struct LevelRun {
    int rounds, classes;
    bool out;
};
template <class Round, class Classes>
__device__ __forceinline__ LevelRun refine_level(int n, int prev, int& rounds, int max_rounds, u64& r, Round round, Classes classes) {
    int k = 0, c = 0;
    while (true) {
        if (rounds >= max_rounds) return {k, c, true};
        ++rounds, ++r, ++k;
        round(r);
        c = classes();
        if (c <= prev || k >= n) break;
        prev = c;
    }
    return {k, c, false};
}
// `todo` recorded rounds, no class count between them; false: out of rounds
template <class Round>
__device__ __forceinline__ bool refine_rounds(int todo, int& rounds, int max_rounds, u64& r, Round round) {
    for (int i = 0; i < todo; ++i) {
        if (rounds >= max_rounds) return false;
        ++rounds, ++r;
        round(r);
    }
    return true;
}
// Replay: the ids after the rounds of level `upto` under choice[0 .. upto) -- id from init, r from 0, then for every level its
// recorded rounds lv_rounds[k] and, below `upto`, its choice individualised (no id snapshots in LDS).  false: out of rounds.
// Barriers: one behind the copy of init (the first round reads every id), one behind every individualisation (tid 0 writes it, the
// next round reads it)
template <class K, class C, class Round>
__device__ __forceinline__ bool refine_replay(int tid, u64* id, const u64* init, int n, int upto, const K* lv_rounds, const C* choice, int& rounds,
                                              int max_rounds, u64& r, Round round) {
    for (int a = tid; a < n; a += REFINE_GT) id[a] = init[a];
    __syncthreads();
    r = 0;
    for (int k = 0; k <= upto; ++k) {
        if (!refine_rounds(lv_rounds[k], rounds, max_rounds, r, round)) return false;
        if (k < upto) {
            if (tid == 0) id[choice[k]] = indiv(id[choice[k]], k);
            __syncthreads();
        }
    }
    return true;
}

// The cell of a level that is not discrete: the non-singleton class of the least id VALUE (invariant under renumbering) -- the least id
// two atoms share, 0 when more than one id is 0.  shared, zeros: of the refine_classes that counted this colouring.  Uniform.
// wu = LDS scratch [REFINE_NW].  Barriers: the reduction's two
__device__ __forceinline__ u64 refine_cell(u64 shared, int zeros, u64* wu) {
    const u64 least = block_reduce(shared, wu, [](u64 u, u64 v) { return min(u, v); });
    return zeros > 1 ? 0 : least;
}
// The first (LAST: the last) atom at or past `from` whose id is `cell` and for which pred(atom) holds; none: n (LAST: -1).  Uniform.
// wi = LDS scratch [REFINE_NW].  Barriers: the reduction's two, so an id written before the call is read by every thread
template <bool LAST, class P>
__device__ __forceinline__ int cell_member(int tid, const u64* id, int n, u64 cell, int from, int* wi, P pred) {
    int at = LAST ? -1 : n;
    for (int a = tid; a < n; a += REFINE_GT)
        if (a >= from && id[a] == cell && pred(a)) at = LAST ? max(at, a) : min(at, a);
    return block_reduce(at, wi, [](int u, int v) { return LAST ? max(u, v) : min(u, v); });
}
template <bool LAST>
__device__ __forceinline__ int cell_member(int tid, const u64* id, int n, u64 cell, int from, int* wi) {
    return cell_member<LAST>(tid, id, n, cell, from, wi, [](int) { return true; });
}
