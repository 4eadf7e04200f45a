// A canonical atom order per image: the least leaf of an individualise-and-refine search over EVERY branch (graph_ident.hip walks one
// path of one side and matches the other against it; this visits the whole tree of one side and keeps the least leaf).  With it the
// text rules of smiles.hip and molblock.hip -- pure functions of atom order, graph and implicit-H list -- write equal strings if and
// only if the graphs are equal.  The contract is in include/abcnet_hip.h (abc_canon_desc) and DESIGN.md section 7, its host form
// decode.canonical_labelling, its oracle tests/graphcanon_oracle.py.
//
// One workgroup per image; integers only (uint64, wrapping).  The graph is ONE side of the identity's, built by the same code: the bond
// rows, stage (A) with id_0, the round, the class count and indiv are graph_refine.hpp's.
//
//   (a) a node is the sequence choice[0 .. level); REFINE runs the level's rounds (r counts on) until one no longer raises the class
//       count, records the trace (rounds, classes, sum of mix(id)) and compares it with the best leaf's while the path has equalled it:
//       greater drops the branch, less makes the path strictly better (less_from)
//   (b) a discrete colouring is a leaf: rank = the number of smaller ids, h = the hash of the relabelled graph.  The first leaf, a leaf
//       of a strictly better path and a leaf with a smaller h become the best (ids, ranks, traces, choices kept in LDS).  An equal key:
//       atoms are mapped onto the best's by equal id through the class table and the map is VERIFIED (class, charge, tag, the multiset
//       of mapped rows by counting) -- an automorphism, merged into the orbit tables of the levels whose prefix it fixes, and the search
//       returns to the level where the path left the best's; not verified: colliding sums, the search stops (COLLISION)
//   (c) CHILD takes the next atom of the node's cell (the non-singleton class of the least id value) at or past nxt[level] that is the
//       least of its orbit (levels <= ABC_CANON_ORBIT_LEVELS; the tables are kept flat, the root is the least atom) and individualises it
//   (d) BACK goes to the nearest level at or above its target that still has an atom of its cell to try (nxt <= cell_max) and rebuilds
//       its ids by replaying the recorded rounds and the choices from id_0 (no id snapshots)
//   (e) max_rounds is checked before every round (replays included), max_tries before every individualisation: UNDECIDED, the order
//       of the best leaf so far, or the identity order.  Every loop is bounded by n, a budget or a capacity
//   (f) every branch depends on values all threads hold alike (reductions read from LDS after a barrier, or descriptor fields)
//   (g) <STEREO>, the second instantiation (abc_canonical_order_stereo, the molecule side alone): at a leaf every thread computes the
//       stereo word of its atoms from the element table of stereo.hip and the ranks, one byte per canonical position; the leaves are
//       ordered by (traces, h, word), the word compared exactly.  At an equal h the map is verified as in (b); words equal: an
//       automorphism of the STEREO graph, merged and jumped as in (b); word smaller: the leaf becomes the best, nothing is merged;
//       greater: a normal backtrack.  Orbit pruning so uses only automorphisms that keep the stereo
//
// Bond rows are never held in LDS (row `tid` stays in registers); the sorts of the certificate and of the canonical rows count, for
// every row, the rows before it (quadratic in the rows of ONE image, no scratch).  Every index read from a row is range-checked before
// it addresses anything: hand-made rows may hold any int32.
#include "common.hpp"
#include "../../include/abcnet_hip.h"
#include "capi_util.hpp"
#include "block_scan.hpp"
#include "mol_rows.hpp"
#include "graph_ids.hpp"
#include "graph_refine.hpp"
#include <type_traits>

namespace {

constexpr int GT = REFINE_GT;
constexpr int MAX_ATOMS = ABC_MAX_SIM_ATOMS;
constexpr int MAX_ROW_BONDS = 4096;  // cap_mol_bonds when the canonical rows are requested
constexpr int NCOL = ABC_CANON_NCOL;
constexpr int NW = REFINE_NW;
constexpr int SLOTS = 2 * MAX_ATOMS;
constexpr int ORBITS = ABC_CANON_ORBIT_LEVELS + 1;      // the levels 0 .. ABC_CANON_ORBIT_LEVELS have an orbit table
constexpr int NONE = 1 << 30;        // less_from: the path has equalled the best so far
constexpr u64 TAG_K = 0xD6E8FEB86659FD93ull, BOND_K = 0xC2B2AE3D27D4EB4Full;
static_assert(MAX_ATOMS == 2 * GT, "two atoms per thread: the record scan");
typedef unsigned short u16;

// <STEREO> abc_canonical_order_stereo: the stereo word of abc_canon_stereo_desc as a third key of the leaves (every line of it is
// compiled out of the plain instantiation)
template <bool STEREO> struct CanonDescOf { typedef abc_canon_desc type; };
template <> struct CanonDescOf<true> { typedef abc_canon_stereo_desc type; };

// What a thread holds of its image in registers: the side that was given (mol_rows.hpp), the graph built from it, the thread's own row
struct Image {
    int tid;
    bool mol, empty;
    int na, nt, nrows, nlisted;      // molecule atoms; record atoms; bond rows of the side; entries of the implicit-H list
    int n, nvalid;                   // atoms of the graph, its valid rows
    const int *pa, *pb, *ph, *ra, *rb, *elements;
    BondRow own;                     // row `tid`, kept through every round (a record row's ends are numbers in T)
};

// The state of the search, uniform over the workgroup but `shared`: budgets, where the search stands, the best leaf's scalars, counters
enum Mode { REFINE, CHILD, BACK, STOP };
struct Search {
    int max_tries, max_rounds;
    Mode mode;
    int level, target, less_from;    // target: the level BACK returns to; less_from: the level from which the path is strictly better
    int prev;                        // the class count the level's first round has to beat
    u64 r, best_h, shared;           // the round number of the path; h of the best leaf; refine_classes' least shared id of this thread
    int zeros;
    bool have_best;
    int best_levels, status;
    int leaves, tries, rounds, levels_max, pruned_trace, pruned_orbit, autos, improved;
    int s_unequal, s_improved, s_autos;      // <STEREO> the stereo_search row
};

// The LDS of the two instantiations apart: the records side needs remap and the scan's scratch and is refused with <STEREO> (so the
// plain kernel holds neither word nor element, the stereo kernel no remap: what the separate arrays were sized to before)
struct RecordSide {
    int remap[MAX_ATOMS];            // record atom -> its number in T, -1 outside T
    unsigned wt[NW + 1];
};
// <STEREO> 2.5 KB: the word of the leaf and of the best leaf, by position, and per atom its checked centre code and the lower-index end
// of the marked double bond it is an end of
struct StereoSide {
    unsigned char sword[MAX_ATOMS], bword[MAX_ATOMS];
    signed char scode[MAX_ATOMS];
    short dsrc[MAX_ATOMS];
};

// 71 KB of LDS: the ids (current, best, id_0), the round's sums, the class table with the atom of every slot, the traces of the current
// path and of the best leaf, the stack, 9 orbit tables -- and the steps of the search on them.  Every step is inlined into the kernel;
// each says which barriers it places
template <bool STEREO>
struct Canon : std::conditional_t<STEREO, StereoSide, RecordSide> {
    u64 cur[MAX_ATOMS], acc[MAX_ATOMS], init[MAX_ATOMS], best_ids[MAX_ATOMS];
    u64 table[SLOTS];
    u64 cur_sum[MAX_ATOMS], best_sum[MAX_ATOMS], cell[MAX_ATOMS];       // per level: the trace's sum; the id of the cell
    u64 wu[NW];
    int orbit[ORBITS][MAX_ATOMS];
    int wi[NW];
    int cnt[1], zero_at;
    u16 cur_k[MAX_ATOMS], cur_c[MAX_ATOMS], best_k[MAX_ATOMS], best_c[MAX_ATOMS];      // per level: rounds, classes
    u16 choice[MAX_ATOMS], best_choice[MAX_ATOMS], nxt[MAX_ATOMS], cell_max[MAX_ATOMS];    // the stack
    u16 tidx[SLOTS];                 // the best leaf's atom of every table slot
    u16 orig[MAX_ATOMS];             // atom of the graph -> its row
    u16 rk[MAX_ATOMS], brank[MAX_ATOMS], gam[MAX_ATOMS];      // ranks of the leaf, of the best leaf; the map onto the best
    unsigned char tag[MAX_ATOMS];

    // ---- class, charge of an atom of the graph; a bond row of the graph; the reductions
    __device__ __forceinline__ int cls_of(const Image& im, int a) const {
        return atom_class(im.mol ? im.pa[a * ATOM_W + 2] : im.ra[orig[a] * REC_ATOM_W + 2]);
    }
    __device__ __forceinline__ int chg_of(const Image& im, int a) const { return im.mol ? im.pa[a * ATOM_W + 3] : im.ra[orig[a] * REC_ATOM_W + 3]; }
    __device__ __forceinline__ BondRow row(const Image& im, int q) const {
        if constexpr (!STEREO)
            if (!im.mol) return rec_row(im.rb, q, im.nt, this->remap);
        return mol_row(im.pb, q, im.na);
    }
    __device__ __forceinline__ int sum_int(int v) { return block_reduce(v, wi, [](int u, int w) { return u + w; }); }
    __device__ __forceinline__ int min_int(int v) { return block_reduce(v, wi, [](int u, int w) { return min(u, w); }); }
    // one round on cur: the sums, a barrier, the new ids (acc zero again), a barrier
    __device__ __forceinline__ void round(const Image& im, u64 r) {
        if (im.mol) refine_add_mol(im.tid, cur, acc, im.pb, im.nrows, im.na, im.own);
        else if constexpr (!STEREO) refine_add_rec(im.tid, cur, acc, im.rb, im.nrows, im.nt, this->remap, im.own);
        __syncthreads();
        refine_finish(im.tid, cur, acc, im.n, r);
        __syncthreads();
    }
    __device__ __forceinline__ int classes(const Image& im, Search& q) { return refine_classes<SLOTS>(im.tid, cur, im.n, table, wi, q.shared, q.zeros); }

    // ---- the image (mol_rows.hpp) of the side that was given, and stage (A): degrees (in acc), the atoms of the graph, tags, id_0
    // (graph_refine.hpp), cur = id_0.  Returns the status bits of the image.  Barriers: behind the clearing, behind the degrees and
    // tags, behind remap / orig / id_0, behind cur
    template <class Desc>
    __device__ __forceinline__ int setup(const Desc& d, int b, Image& im) {
        const int tid = im.tid = threadIdx.x;
        const bool mol = im.mol = STEREO || d.mol_counts != nullptr;      // (the launcher refuses the records side with <STEREO>)
        int status = 0;
        im.na = im.nt = im.nrows = im.nlisted = 0;
        im.pa = im.pb = im.ph = im.ra = im.rb = im.elements = nullptr;
        if (mol) {
            const MolImage m = mol_image(d, b);
            status = m.status, im.na = m.na, im.nrows = m.nb, im.nlisted = m.nh, im.pa = m.pa, im.pb = m.pb, im.ph = m.ph;
        } else {
            const RecImage m = rec_image(d, b);
            im.nt = m.nt, im.nrows = m.m, im.ra = m.ra, im.rb = m.rb;
        }
        im.empty = (status & ABC_CANON_EMPTY) != 0;
        static_assert((int)ABC_CANON_EMPTY == (int)ABC_MOL_EMPTY && (int)ABC_CANON_TRUNCATED == (int)ABC_MOL_TRUNCATED, "the two bits are copied");
        im.own = {false, 0, 0, 0};
        if (tid < im.nrows) im.own = mol ? mol_row(im.pb, tid, im.na) : rec_row(im.rb, tid, im.nt);

        if (tid == 0) cnt[0] = 0, zero_at = -1;
        for (int a = tid; a < MAX_ATOMS; a += GT) acc[a] = 0, tag[a] = 0;
        __syncthreads();
        {
            const int valid = mol ? refine_degrees_mol(tid, im.pb, im.nrows, im.na, im.own, acc) : refine_degrees_rec(tid, im.rb, im.nrows, im.nt, im.own, acc);
            if (valid) atomicAdd(cnt, valid);
            for (int k = tid; k < im.nlisted; k += GT) {
                const int e = im.ph[k];
                if (e >= 1 && e <= im.na) tag[e - 1] = 1;
            }
        }
        __syncthreads();
        im.nvalid = cnt[0];
        im.n = im.na;
        if (mol) {
            refine_id0_mol(tid, im.pa, im.na, acc, init);
            for (int a = tid; a < im.na; a += GT) {      // (by the thread that wrote id_0 and read the degree: acc becomes the round's sums)
                if (tag[a]) init[a] = mix(init[a] + TAG_K);
                orig[a] = (u16)a;
                acc[a] = 0;
            }
        } else if constexpr (!STEREO) {
            im.n = refine_number_rec(tid, im.ra, im.nt, acc, this->wt, this->remap, orig, init);
        }
        __syncthreads();                     // (remap, orig and id_0 are written)
        if constexpr (!STEREO)
            if (!mol) renumber(im.own, this->remap);
        for (int a = tid; a < im.n; a += GT) cur[a] = init[a];
        __syncthreads();
        return status;
    }
    // <STEREO> the elements of the image, checked once: an index that is no atom of the image makes its element none.  Barriers: behind
    // scode and the clearing of dsrc, behind dsrc
    template <class Desc>
    __device__ __forceinline__ void check_elements(const Desc& d, int b, Image& im) {
        const int tid = im.tid, n = im.n;
        const int* elements = im.elements = d.elements + (size_t)b * d.cap_atoms * STEREO_W;
        auto atom = [&](int v, int least) __attribute__((always_inline)) { return v >= least && v < n; };
        for (int a = tid; a < n; a += GT) {
            const int* el = elements + a * STEREO_W;
            const int c = el[0];
            this->scode[a] = (signed char)((c == 1 || c == -1) && atom(el[1], 0) && atom(el[2], 0) && atom(el[3], 0) && atom(el[4], -1) ? c : 0);
            this->dsrc[a] = -1;
        }
        __syncthreads();
        for (int a = tid; a < n; a += GT) {
            const int* el = elements + a * STEREO_W;
            const int c = el[5], other = el[7];
            if ((c == 1 || c == -1) && atom(other, 0) && other != a && atom(el[8], 0) && atom(el[9], -1) && atom(el[10], 0) && atom(el[11], -1))
                this->dsrc[a] = this->dsrc[other] = (short)a;
        }
        __syncthreads();
    }

    // ---- (b) the leaf.  rank = the number of smaller ids, into rk.  Barrier: behind the ranks (and tid 0's trace of this level)
    __device__ __forceinline__ void leaf_ranks(const Image& im) {
        for (int a = im.tid; a < im.n; a += GT) {
            const u64 e = cur[a];
            int below = 0;
            for (int x = 0; x < im.n; ++x) below += cur[x] < e;
            rk[a] = (u16)below;
        }
        __syncthreads();
    }
    // h of the relabelled graph under the ranks `rank` (uniform).  Barriers: the reduction's two
    __device__ __forceinline__ u64 leaf_hash(const Image& im, const u16* rank) {
        u64 h = 0;
        for (int a = im.tid; a < im.n; a += GT)
            h += mix(mix(mix(mix((u64)rank[a] + 1) + (u64)(cls_of(im, a) + 1)) + (u64)(long long)chg_of(im, a)) + (u64)tag[a]);
        for (int q = im.tid; q < im.nrows; q += GT) {
            const BondRow e = row(im, q);
            if (!e.v) continue;
            const u64 lo = min((int)rank[e.i], (int)rank[e.j]), hi = max((int)rank[e.i], (int)rank[e.j]);
            h += mix(mix(((lo << 32) | hi) + BOND_K) + (u64)e.o);
        }
        return block_reduce(h, wu, [](u64 u, u64 v) { return u + v; });
    }
    // <STEREO> the stereo word of the leaf whose ranks are in rk, by position (every position is written: the ranks are a
    // permutation).  Barrier: behind the word
    __device__ __forceinline__ void leaf_word(const Image& im) {
        for (int a = im.tid; a < im.n; a += GT) {
            int byte = 0;
            const int sc = this->scode[a], a0 = this->dsrc[a];
            if (sc != 0) {
                const int* el = im.elements + a * STEREO_W;
                const int last = el[4];
                const int r0 = rk[el[1]], r1 = rk[el[2]], r2 = rk[el[3]], r3 = last >= 0 ? (int)rk[last] : MAX_ATOMS;      // (the hydrogen stays last)
                const int swaps = (r0 > r1) + (r0 > r2) + (r0 > r3) + (r1 > r2) + (r1 > r3) + (r2 > r3);
                byte = ((swaps & 1) ? -sc : sc) > 0 ? 1 : 2;
            }
            if (a0 >= 0) {
                const int* el = im.elements + a0 * STEREO_W;
                const int other = a == a0 ? el[7] : a0;
                if (rk[a] < rk[other]) {      // the lower-rank end bears the bond's part
                    int v = el[5];
                    if (el[9] >= 0 && rk[el[8]] > rk[el[9]]) v = -v;
                    if (el[11] >= 0 && rk[el[10]] > rk[el[11]]) v = -v;
                    byte |= (v > 0 ? 1 : 2) << 2;
                }
            }
            this->sword[rk[a]] = (unsigned char)byte;
        }
        __syncthreads();
    }
    // the leaf becomes the best: ids, ranks, <STEREO> word, the choices of the path and, with `traces`, the traces of the levels 0 ..
    // level (without: they equal the best's).  Barrier: behind the copies
    __device__ __forceinline__ void keep_best(const Image& im, int level, bool traces) {
        for (int a = im.tid; a < im.n; a += GT) {
            best_ids[a] = cur[a], brank[a] = rk[a];
            if constexpr (STEREO) this->bword[a] = this->sword[a];
        }
        for (int l = im.tid; l <= level; l += GT) {
            if (traces) best_k[l] = cur_k[l], best_c[l] = cur_c[l], best_sum[l] = cur_sum[l];
            if (l < level) best_choice[l] = choice[l];
        }
        __syncthreads();
    }
    // the map onto the best leaf by equal id, through the class table, into gam, VERIFIED: class, charge and tag of every atom, and the
    // multiset of the mapped rows is the multiset of the rows.  Uniform.  Barriers: behind the clearing of the table, behind the puts,
    // the two reductions' (the first is behind gam)
    __device__ __forceinline__ bool map_onto_best(const Image& im) {
        const int tid = im.tid, n = im.n;
        for (int k = tid; k < SLOTS; k += GT) table[k] = 0;
        if (tid == 0) zero_at = -1;
        __syncthreads();
        for (int a = tid; a < n; a += GT) {
            const u64 e = best_ids[a];
            if (e == 0) {
                zero_at = a;
                continue;
            }
            const TableSlot at = id_table_put<SLOTS>(table, e);
            if (at.slot >= 0 && at.fresh) tidx[at.slot] = (u16)a;
        }
        __syncthreads();
        int bad = 0;
        for (int a = tid; a < n; a += GT) {
            const u64 e = cur[a];
            int t = zero_at;
            if (e != 0) {
                const int slot = id_table_find<SLOTS>(table, e);
                t = slot >= 0 ? (int)tidx[slot] : -1;
            }
            const int y = t < 0 || t >= n ? a : t;
            gam[a] = (u16)y;
            bad += t < 0 || t >= n || cls_of(im, a) != cls_of(im, y) || chg_of(im, a) != chg_of(im, y) || tag[a] != tag[y];
        }
        if (sum_int(bad) != 0) return false;      // (gam is written: the reduction synchronises)
        // the multiset of the mapped rows is the multiset of the rows, by counting (one loop: the graph is mapped onto itself, so
        // every row is read once for both counts; why this is not the identity's loop: graph_refine.hpp)
        int common = 0;
        for (int q = tid; q < im.nrows; q += GT) {
            const BondRow e = row(im, q);
            if (!e.v) continue;
            const int gi = gam[e.i], gj = gam[e.j], lo = min(gi, gj), hi = max(gi, gj);
            int before = 0, there = 0;
            for (int q2 = 0; q2 < im.nrows; ++q2) {
                const BondRow e2 = row(im, q2);
                if (!e2.v || e2.o != e.o) continue;
                const int gi2 = gam[e2.i], gj2 = gam[e2.j];
                before += q2 < q && min(gi2, gj2) == lo && max(gi2, gj2) == hi;
                there += min(e2.i, e2.j) == lo && max(e2.i, e2.j) == hi;
            }
            common += before < there;
        }
        return sum_int(common) == im.nvalid;
    }
    // x ~ gam(x) in the orbit tables of the levels 0 .. upto, whose prefix the map fixes: the greater root is hung under the less.
    // Barrier: behind the unions
    __device__ __forceinline__ void merge_orbits(const Image& im, int upto) {
        const int n = im.n;
        for (int l = 0; l <= upto; ++l) {
            int* p = orbit[l];
            for (int a = im.tid; a < n; a += GT) {
                int x = a, y = gam[a];
                for (int it = 0; it < n; ++it) {
                    for (int w = 0; w < n; ++w) {
                        const int up = __hip_atomic_load(&p[x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                        if (up == x) break;
                        x = up;
                    }
                    for (int w = 0; w < n; ++w) {
                        const int up = __hip_atomic_load(&p[y], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                        if (up == y) break;
                        y = up;
                    }
                    if (x == y) break;
                    if (x < y) { const int t = x; x = y; y = t; }
                    if (atomicCAS(&p[x], x, y) == x) break;
                }
            }
        }
        __syncthreads();
    }
    // the tables 0 .. upto flat again: every atom under its root, the least of its orbit.  Barriers: per table between the reading of
    // the roots and the writing, and behind the last table
    __device__ __forceinline__ void flatten_orbits(const Image& im, int upto) {
        const int tid = im.tid, n = im.n;
        for (int l = 0; l <= upto; ++l) {
            int* p = orbit[l];
            int root[MAX_ATOMS / GT];
#pragma unroll
            for (int u = 0; u < MAX_ATOMS / GT; ++u) {
                int x = min(tid + u * GT, MAX_ATOMS - 1);
                for (int w = 0; w < n; ++w) {
                    const int up = p[x];
                    if (up == x) break;
                    x = up;
                }
                root[u] = x;
            }
            __syncthreads();
#pragma unroll
            for (int u = 0; u < MAX_ATOMS / GT; ++u)
                if (tid + u * GT < n) p[tid + u * GT] = root[u];
        }
        __syncthreads();
    }
    // (b) a discrete colouring: ranks, h, <STEREO> word; the first leaf, a leaf of a strictly better path and a leaf with a smaller h
    // become the best; an equal h is mapped onto the best and verified -- an automorphism is merged into the orbits and the search
    // returns to the level where the path left the best's
    __device__ __forceinline__ Mode leaf(const Image& im, Search& q) {
        const int tid = im.tid, n = im.n, level = q.level;
        ++q.leaves;
        leaf_ranks(im);
        const u64 h = leaf_hash(im, rk);
        if constexpr (STEREO) leaf_word(im);
        if (!q.have_best || q.less_from != NONE || h < q.best_h) {
            q.improved += q.have_best;
            keep_best(im, level, true);
            q.have_best = true, q.best_levels = level, q.best_h = h, q.less_from = NONE;
            return BACK;
        }
        if (h != q.best_h) return BACK;
        if (!map_onto_best(im)) {
            q.status |= ABC_CANON_COLLISION;
            return STOP;
        }
        if constexpr (STEREO) {
            // the third key, compared exactly: the first position at which the words differ
            int differs = NONE;
            for (int k = tid; k < n; k += GT)
                if (this->sword[k] != this->bword[k]) differs = min(differs, k);
            differs = min_int(differs);
            if (differs != NONE) {      // a map that does not keep the stereo: no orbit merge, no jump
                ++q.s_unequal;
                const bool less = this->sword[differs] < this->bword[differs];
                __syncthreads();         // (read before the best leaf's word is replaced)
                if (less) {
                    ++q.s_improved, ++q.improved;
                    keep_best(im, level, false);      // (the traces are equal)
                }
                return BACK;
            }
            ++q.s_autos;
        }
        ++q.autos;
        int first = NONE;
        for (int l = tid; l < level; l += GT)
            if (choice[l] != best_choice[l]) first = min(first, l);
        q.target = min(min_int(first), level - 1);      // the level where the path left the best's
        const int upto = min(q.target, ORBITS - 1);
        merge_orbits(im, upto);
        flatten_orbits(im, upto);
        return BACK;
    }

    // ---- (a) REFINE: the level's rounds, the trace and its comparison with the best leaf's, then the leaf or the cell of the node.
    // Barrier of its own: behind the cell, cell_max, nxt and the fresh orbit table of the level
    __device__ __forceinline__ Mode refine(const Image& im, Search& q) {
        const int tid = im.tid, n = im.n, level = q.level;
        const LevelRun lv = refine_level(n, q.prev, q.rounds, q.max_rounds, q.r, [&](u64 r) __attribute__((always_inline)) { round(im, r); },
                                         [&]() __attribute__((always_inline)) { return classes(im, q); });
        if (lv.out) {
            q.status |= ABC_CANON_UNDECIDED;
            return STOP;
        }
        const int k = lv.rounds, c = lv.classes;
        const u64 s = refine_multiset_sum(tid, cur, n, wu);
        if (tid == 0) cur_k[level] = (u16)k, cur_c[level] = (u16)c, cur_sum[level] = s;
        q.levels_max = max(q.levels_max, level);
        q.target = level - 1;
        if (q.have_best && q.less_from == NONE) {
            const int bk = best_k[level], bc = best_c[level];
            const u64 bs = best_sum[level];
            const int cmp = k != bk ? (k < bk ? -1 : 1) : (c != bc ? (c < bc ? -1 : 1) : (s != bs ? (s < bs ? -1 : 1) : 0));
            if (cmp > 0) {
                ++q.pruned_trace;
                return BACK;
            }
            if (cmp < 0) q.less_from = level;
        }
        if (c == n) return leaf(im, q);
        if (level + 1 >= n) {            // (only colliding hashes get here)
            q.status |= ABC_CANON_COLLISION;
            return STOP;
        }
        // the cell: the least id that two atoms share; its last atom
        const u64 cellv = refine_cell(q.shared, q.zeros, wu);
        const int last = cell_member<true>(tid, cur, n, cellv, 0, wi);
        if (last < 0) {
            q.status |= ABC_CANON_COLLISION;
            return STOP;
        }
        if (tid == 0) cell[level] = cellv, cell_max[level] = (u16)last, nxt[level] = 0;
        if (level < ORBITS)
            for (int a = tid; a < MAX_ATOMS; a += GT) orbit[level][a] = a;
        __syncthreads();
        return CHILD;
    }
    // ---- (c) CHILD: the next atom of the cell that is the least of its orbit, individualised.  Barrier of its own: behind the stack
    // and the individualised id
    __device__ __forceinline__ Mode next_child(const Image& im, Search& q) {
        const int tid = im.tid, n = im.n, level = q.level;
        const u64 cellv = cell[level];
        const int from = nxt[level];
        const bool orbits = level < ORBITS;
        const int* least_of = orbit[min(level, ORBITS - 1)];
        const int v = cell_member<false>(tid, cur, n, cellv, from, wi, [&](int a) __attribute__((always_inline)) { return !orbits || least_of[a] == a; });
        if (orbits) {
            int skipped = 0;
            for (int a = tid; a < n; a += GT) skipped += a >= from && a < v && cur[a] == cellv;
            q.pruned_orbit += sum_int(skipped);
        }
        if (v >= n) {
            q.target = level - 1;
            return BACK;
        }
        if (q.tries >= q.max_tries) {
            q.status |= ABC_CANON_UNDECIDED;
            return STOP;
        }
        ++q.tries;
        q.prev = cur_c[level] + 1;
        if (tid == 0) choice[level] = (u16)v, nxt[level] = (u16)(v + 1), cur[v] = indiv(cur[v], level);
        __syncthreads();
        ++q.level;
        return REFINE;
    }
    // ---- (d) BACK: the nearest level at or above the target that still has an atom of its cell to try; its ids by replay.  Barrier
    // of its own: in front (nxt and cell_max of the levels are tid 0's writes)
    __device__ __forceinline__ Mode back(const Image& im, Search& q) {
        __syncthreads();
        for (int it = 0; it < im.n && q.target >= 0 && nxt[q.target] > cell_max[q.target]; ++it) --q.target;
        if (q.target < 0) return STOP;
        q.level = q.target;
        if (q.less_from != NONE && q.less_from > q.level) q.less_from = NONE;
        if (!refine_replay(im.tid, cur, init, im.n, q.level, cur_k, choice, q.rounds, q.max_rounds, q.r, [&](u64 r) __attribute__((always_inline)) { round(im, r); })) {
            q.status |= ABC_CANON_UNDECIDED;
            return STOP;
        }
        return CHILD;
    }

    // ---- the outputs: every word of every buffer.  The order of the best leaf (none: the identity order), the two keys, the stats row
    // and <STEREO> the stereo_search row.  Barriers: in front (the search's last writes), behind the identity order, the reductions'
    template <class Desc>
    __device__ __forceinline__ void write_order_key_stats(const Desc& d, int b, const Image& im, const Search& q, int cap) {
        const int tid = im.tid, n = im.n;
        int* const order = d.order + (size_t)b * cap;
        __syncthreads();
        if (!q.have_best)
            for (int a = tid; a < n; a += GT) brank[a] = (u16)a;
        __syncthreads();
        const bool none = im.empty || n == 0;
        for (int k = tid; k < cap; k += GT)
            if (k >= n) order[k] = -1;
        for (int a = tid; a < n; a += GT) order[brank[a]] = orig[a];
        const u64 key0 = none ? 0 : leaf_hash(im, brank);
        u64 t = 0;
        if (q.have_best)
            for (int l = tid; l <= q.best_levels; l += GT) t += mix(mix(mix(mix((u64)l + 1) + (u64)best_k[l]) + (u64)best_c[l]) + best_sum[l]);
        t = block_reduce(t, wu, [](u64 u, u64 v) { return u + v; });
        if (tid != 0) return;
        int* st = d.stats + (size_t)b * NCOL;
        st[ABC_CANON_STATUS] = q.status;
        st[ABC_CANON_LEAVES] = q.leaves, st[ABC_CANON_TRIES] = q.tries, st[ABC_CANON_ROUNDS] = q.rounds, st[ABC_CANON_LEVELS_MAX] = q.levels_max;
        st[ABC_CANON_PRUNED_TRACE] = q.pruned_trace, st[ABC_CANON_PRUNED_ORBIT] = q.pruned_orbit;
        st[ABC_CANON_AUTOMORPHISMS] = q.autos, st[ABC_CANON_IMPROVED] = q.improved;
        d.key[(size_t)b * 2] = (long long)key0;
        d.key[(size_t)b * 2 + 1] = im.empty ? 0 : (long long)mix(mix(mix((u64)n) + (u64)im.nvalid) + t);
        if constexpr (STEREO) {
            int* ss = d.stereo_search + (size_t)b * 4;
            ss[0] = q.s_unequal, ss[1] = q.s_improved, ss[2] = q.s_autos, ss[3] = 0;
        }
    }
    // the certificate but its triples: the padding, the two counts, a word per atom at its canonical position
    __device__ __forceinline__ void write_certificate(int* cert, const Image& im, int cap, int cap_bonds) {
        const int tid = im.tid, n = im.n, used = 2 + n + 3 * im.nvalid;
        for (int k = tid; k < 2 + cap + 3 * cap_bonds; k += GT)
            if (k >= used) cert[k] = -1;
        if (tid == 0) cert[0] = n, cert[1] = im.nvalid;
        for (int a = tid; a < n; a += GT)
            cert[2 + brank[a]] = (int)(((unsigned)chg_of(im, a) << 5) | ((unsigned)tag[a] << 4) | (unsigned)cls_of(im, a));
    }
    // the canonical rows but the bond rows' places: the counts, the atom rows at their positions, the padding of atoms and bonds
    template <class Desc>
    __device__ __forceinline__ void write_canonical_rows(const Desc& d, int b, const Image& im, int* oa, int* ob) {
        const int tid = im.tid, n = im.n;
        int* const oc = d.out_counts + (size_t)b * 4;
        if (tid < 4) oc[tid] = d.mol_counts[(size_t)b * 4 + tid];
        for (int k = tid; k < (d.cap_atoms - n) * ATOM_W; k += GT) oa[n * ATOM_W + k] = 0;
        for (int k = tid; k < n * ATOM_W; k += GT) oa[brank[k / ATOM_W] * ATOM_W + k % ATOM_W] = im.pa[k];
        for (int k = tid; k < (d.cap_mol_bonds - im.nrows) * MOL_BOND_W; k += GT) ob[im.nrows * MOL_BOND_W + k] = 0;
    }
    // the implicit-H list: the entries in 1..n renumbered and ascending, the others after them verbatim
    __device__ __forceinline__ void write_implicit_h(int* oh, const Image& im, int cap_atoms) {
        const int n = im.n, nlisted = im.nlisted;
        const int* ph = im.ph;
        for (int k = im.tid; k < cap_atoms; k += GT) {
            if (k >= nlisted) {
                oh[k] = 0;
                continue;
            }
            const int e = ph[k];
            const bool in = e >= 1 && e <= n;
            const int val = in ? brank[e - 1] + 1 : 0;
            int less = 0, in_all = 0, out_before = 0;
            for (int k2 = 0; k2 < nlisted; ++k2) {
                const int e2 = ph[k2];
                const bool in2 = e2 >= 1 && e2 <= n;
                in_all += in2;
                out_before += !in2 && k2 < k;
                if (in && in2) {
                    const int val2 = brank[e2 - 1] + 1;
                    less += val2 < val || (val2 == val && k2 < k);
                }
            }
            oh[in ? less : in_all + out_before] = in ? val : e;
        }
    }
    // the bond rows, by counting: the place of a row among the certificate's triples (cert, may be null) and among the canonical
    // rows (ob, may be null)
    __device__ __forceinline__ void write_bond_rows(int* cert, int* ob, const Image& im) {
        const int n = im.n, nrows = im.nrows;
        for (int q = im.tid; q < nrows; q += GT) {
            const BondRow e = row(im, q);
            const bool valid = e.v;
            const int bi = valid ? brank[e.i] : 0, bj = valid ? brank[e.j] : 0, lo = min(bi, bj), hi = max(bi, bj);
            const int pair = lo * MAX_ATOMS + hi;
            int at_cert = 0, at_rows = 0, valid_before = 0;
            for (int q2 = 0; q2 < nrows; ++q2) {
                const BondRow e2 = row(im, q2);
                if (!e2.v) continue;
                valid_before += q2 < q;
                const int bi2 = brank[e2.i], bj2 = brank[e2.j], pair2 = min(bi2, bj2) * MAX_ATOMS + max(bi2, bj2);
                at_rows += pair2 < pair || (pair2 == pair && q2 < q);
                at_cert += pair2 < pair || (pair2 == pair && (e2.o < e.o || (e2.o == e.o && q2 < q)));
            }
            if (cert != nullptr && valid) {
                int* tr = cert + 2 + n + 3 * at_cert;
                tr[0] = lo, tr[1] = hi, tr[2] = e.o;
            }
            if (ob != nullptr) {
                const int* src = im.pb + q * MOL_BOND_W;
                int* dst = ob + (valid ? at_rows : im.nvalid + q - valid_before) * MOL_BOND_W;
                dst[0] = valid ? bi + 1 : src[0], dst[1] = valid ? bj + 1 : src[1], dst[2] = src[2], dst[3] = src[3];
            }
        }
    }
};

// The search as a loop of modes: REFINE -> the leaf (then BACK) or CHILD; CHILD -> REFINE one level down, or BACK; BACK -> CHILD at a
// level that has a candidate left, or the end.  A budget or a collision stops it where it stands.  One turn of the loop runs the modes
// in that order, so REFINE falls through to CHILD and either to BACK
template <bool STEREO>
__global__ __launch_bounds__(GT) void graph_canon_kernel(const typename CanonDescOf<STEREO>::type d) {
    __shared__ Canon<STEREO> s;
    const int b = blockIdx.x;
    Image im;
    Search q = {};
    q.status = s.setup(d, b, im);
    if constexpr (STEREO) s.check_elements(d, b, im);
    q.max_tries = d.max_tries > 0 ? d.max_tries : ABC_CANON_DEFAULT_TRIES;
    q.max_rounds = d.max_rounds > 0 ? d.max_rounds : ABC_CANON_DEFAULT_ROUNDS;
    q.mode = REFINE, q.target = -1, q.less_from = NONE, q.shared = ~0ull;
    if (!im.empty && im.n > 0) {
        q.prev = s.classes(im, q);
        while (q.mode != STOP) {
            if (q.mode == REFINE) q.mode = s.refine(im, q);
            if (q.mode == CHILD) q.mode = s.next_child(im, q);
            if (q.mode == BACK) q.mode = s.back(im, q);
        }
    }

    const int cap = im.mol ? d.cap_atoms : d.max_atoms, cap_bonds = im.mol ? d.cap_mol_bonds : d.max_bonds;
    s.write_order_key_stats(d, b, im, q, cap);
    int* const cert = d.cert_out != nullptr ? d.cert_out + (size_t)b * (2 + cap + 3 * (size_t)cap_bonds) : nullptr;
    const bool want_rows = im.mol && d.out_counts != nullptr;
    if (cert == nullptr && !want_rows) return;
    int* const ob = want_rows ? d.out_bonds + (size_t)b * d.cap_mol_bonds * MOL_BOND_W : nullptr;
    if (cert != nullptr) s.write_certificate(cert, im, cap, cap_bonds);
    if (want_rows) {
        s.write_canonical_rows(d, b, im, d.out_atoms + (size_t)b * d.cap_atoms * ATOM_W, ob);
        s.write_implicit_h(d.out_implh + (size_t)b * d.cap_atoms, im, d.cap_atoms);
    }
    s.write_bond_rows(cert, ob, im);
}

// the guards of both entry points, and the launch
template <bool STEREO>
int canonical_order(const typename CanonDescOf<STEREO>::type* d, abc_stream_t stream, const char* entry) {
    bool mol;
    if (const int rc = abc_one_side(entry, d, mol)) return rc;
    if constexpr (STEREO) {
        if (!mol) return abc_fail_in(ABC_EINVAL, entry, "the stereo elements are the molecule side's: records are refused");
        if (!d->elements || !d->stereo_search) return abc_fail_in(ABC_EINVAL, entry, "null elements or stereo_search");
    }
    if (d->max_tries < 0) return abc_fail_in(ABC_EINVAL, entry, "max_tries must be >= 0 (0: the default)");
    if (d->max_rounds < 0) return abc_fail_in(ABC_EINVAL, entry, "max_rounds must be >= 0 (0: the default)");
    if (!d->order || !d->stats || !d->key) return abc_fail_in(ABC_EINVAL, entry, "null output (order, stats, key)");
    const int rows_given = (d->out_counts != nullptr) + (d->out_atoms != nullptr) + (d->out_bonds != nullptr) + (d->out_implh != nullptr);
    if (rows_given != 0 && rows_given != 4) return abc_fail_in(ABC_EINVAL, entry, "the canonical rows are four buffers, or none");
    if (const int rc = abc_one_side_buffers(entry, d, mol)) return rc;
    if (const int rc = abc_one_side_capacities(entry, d, mol)) return rc;
    if (mol && rows_given && d->cap_mol_bonds > MAX_ROW_BONDS)
        return abc_fail_in(ABC_EUNSUPPORTED, entry, "cap_mol_bonds must be <= 4096 when the canonical rows are requested");
    if (!mol && rows_given) return abc_fail_in(ABC_EINVAL, entry, "the canonical rows are the molecule side's");
    const size_t B = (size_t)d->B, cap = (size_t)(mol ? d->cap_atoms : d->max_atoms), cb = (size_t)(mol ? d->cap_mol_bonds : d->max_bonds);
    abc_extent out[9] = {{d->order, B * cap * 4}, {d->stats, B * NCOL * 4}, {d->key, B * 16}, {d->cert_out, B * (2 + cap + 3 * cb) * 4},
                         {d->out_counts, B * 16}, {d->out_atoms, B * cap * ATOM_W * 4}, {d->out_bonds, B * cb * MOL_BOND_W * 4}, {d->out_implh, B * cap * 4},
                         {nullptr, 0}};
    if constexpr (STEREO) {
        out[8] = {d->stereo_search, B * 16};
        for (const abc_extent& o : out)
            if (overlap(o.p, o.bytes, d->elements, B * cap * STEREO_W * 4)) return abc_fail_in(ABC_EINVAL, entry, "an output overlaps an input");
    }
    if (const int rc = abc_one_side_overlap(entry, d, mol, out)) return rc;
    hipLaunchKernelGGL(graph_canon_kernel<STEREO>, dim3(d->B), dim3(GT), 0, (hipStream_t)stream, *d);
    return abc_check_launch(entry);
}

}  // namespace

extern "C" int abc_canon_desc_size(void) { return (int)sizeof(abc_canon_desc); }

extern "C" int abc_canonical_order(const abc_canon_desc* d, abc_stream_t stream) { return canonical_order<false>(d, stream, "canonical_order"); }

extern "C" int abc_canon_stereo_desc_size(void) { return (int)sizeof(abc_canon_stereo_desc); }

extern "C" int abc_canonical_order_stereo(const abc_canon_stereo_desc* d, abc_stream_t stream) {
    return canonical_order<true>(d, stream, "canonical_order_stereo");
}
