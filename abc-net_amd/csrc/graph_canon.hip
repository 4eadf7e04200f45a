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
// compiled out of the plain instantiation, which keeps its instructions)
template <bool STEREO> struct CanonDescOf { typedef abc_canon_desc type; };
template <> struct CanonDescOf<true> { typedef abc_canon_stereo_desc type; };

// 71 KB of LDS: the ids (current, best, id_0), the round's sums, the class table with the atom of every slot, the traces of the current
// path and of the best leaf, the stack, 9 orbit tables; <STEREO> 2.5 KB more: the word of the leaf and of the best leaf, by position, and
// per atom its checked centre code and the lower-index end of the marked double bond it is an end of
template <bool STEREO>
__global__ __launch_bounds__(GT) void graph_canon_kernel(const typename CanonDescOf<STEREO>::type d) {
    __shared__ unsigned char sword[STEREO ? MAX_ATOMS : 1], bword[STEREO ? MAX_ATOMS : 1];
    __shared__ signed char scode[STEREO ? MAX_ATOMS : 1];
    __shared__ short dsrc[STEREO ? MAX_ATOMS : 1];
    __shared__ u64 cur[MAX_ATOMS], acc[MAX_ATOMS], init[MAX_ATOMS], best_ids[MAX_ATOMS];
    __shared__ u64 table[SLOTS];
    __shared__ u64 cur_sum[MAX_ATOMS], best_sum[MAX_ATOMS], cell[MAX_ATOMS];       // per level: the trace's sum; the id of the cell
    __shared__ u16 cur_k[MAX_ATOMS], cur_c[MAX_ATOMS], best_k[MAX_ATOMS], best_c[MAX_ATOMS];      // per level: rounds, classes
    __shared__ u16 choice[MAX_ATOMS], best_choice[MAX_ATOMS], nxt[MAX_ATOMS], cell_max[MAX_ATOMS];    // the stack
    __shared__ u16 tidx[SLOTS];          // the best leaf's atom of every table slot
    __shared__ int remap[MAX_ATOMS];     // record atom -> its number in T, -1 outside T
    __shared__ u16 orig[MAX_ATOMS];      // atom of the graph -> its row
    __shared__ u16 rk[MAX_ATOMS], brank[MAX_ATOMS], gam[MAX_ATOMS];      // ranks of the leaf, of the best leaf; the map onto the best
    __shared__ unsigned char tag[MAX_ATOMS];
    __shared__ int orbit[ORBITS][MAX_ATOMS];
    __shared__ unsigned wt[NW + 1];
    __shared__ int wi[NW];
    __shared__ u64 wu[NW];
    __shared__ int cnt[1], zero_at;
    const int b = blockIdx.x, tid = threadIdx.x;
    const bool mol = STEREO || d.mol_counts != nullptr;      // (the launcher refuses the records side with <STEREO>)
    const int cap = mol ? d.cap_atoms : d.max_atoms, cap_bonds = mol ? d.cap_mol_bonds : d.max_bonds;
    int* const order = d.order + (size_t)b * cap;
    int* const cert = d.cert_out != nullptr ? d.cert_out + (size_t)b * (2 + cap + 3 * (size_t)cap_bonds) : nullptr;
    const bool want_rows = mol && d.out_counts != nullptr;
    const int max_tries = d.max_tries > 0 ? d.max_tries : ABC_CANON_DEFAULT_TRIES;
    const int max_rounds = d.max_rounds > 0 ? d.max_rounds : ABC_CANON_DEFAULT_ROUNDS;

    // ---- the image (mol_rows.hpp), of the side that was given
    int status = 0, na = 0, nrows = 0, nt = 0, nlisted = 0;      // na: molecule atoms; nt: record atoms; nrows: bond rows of the side
    const int *pa = nullptr, *pb = nullptr, *ph = nullptr, *ra = nullptr, *rb = nullptr;
    if (mol) {
        const MolImage im = mol_image(d, b);
        status = im.status, na = im.na, nrows = im.nb, nlisted = im.nh, pa = im.pa, pb = im.pb, ph = im.ph;
    } else {
        const RecImage im = rec_image(d, b);
        nt = im.nt, nrows = im.m, ra = im.ra, rb = im.rb;
    }
    const bool empty = (status & ABC_CANON_EMPTY) != 0;
    static_assert((int)ABC_CANON_EMPTY == (int)ABC_MOL_EMPTY && (int)ABC_CANON_TRUNCATED == (int)ABC_MOL_TRUNCATED, "the two bits are copied");

    // row `tid`, kept through every round (a record row's ends become numbers in T below)
    BondRow own = {false, 0, 0, 0};
    if (tid < nrows) own = mol ? mol_row(pb, tid, na) : rec_row(rb, tid, nt);

    // ---- (A) degrees (in acc), the atoms of the graph, tags, id_0 (graph_refine.hpp, for the side that was given)
    if (tid == 0) cnt[0] = 0, zero_at = -1;
    for (int a = tid; a < MAX_ATOMS; a += GT) acc[a] = 0, tag[a] = 0;
    __syncthreads();
    {
        const int valid = mol ? refine_degrees_mol(tid, pb, nrows, na, own, acc) : refine_degrees_rec(tid, rb, nrows, nt, own, acc);
        if (valid) atomicAdd(cnt, valid);
        for (int k = tid; k < nlisted; k += GT) {
            const int e = ph[k];
            if (e >= 1 && e <= na) tag[e - 1] = 1;
        }
    }
    __syncthreads();
    const int nvalid = cnt[0];
    int n = na;
    if (mol) {
        refine_id0_mol(tid, pa, na, acc, init);
        for (int a = tid; a < na; a += GT) {      // (by the thread that wrote id_0 and read the degree: acc becomes the round's sums)
            if (tag[a]) init[a] = mix(init[a] + TAG_K);
            orig[a] = (u16)a;
            acc[a] = 0;
        }
    } else {
        n = refine_number_rec(tid, ra, nt, acc, wt, remap, orig, init);
    }
    __syncthreads();                     // (remap, orig and id_0 are written)
    if (!mol) renumber(own, remap);
    for (int a = tid; a < n; a += GT) cur[a] = init[a];
    __syncthreads();

    // class, charge of an atom of the graph; a bond row of the graph
    auto cls_of = [&](int a) __attribute__((always_inline)) { return atom_class(mol ? pa[a * ATOM_W + 2] : ra[orig[a] * REC_ATOM_W + 2]); };
    auto chg_of = [&](int a) __attribute__((always_inline)) { return mol ? pa[a * ATOM_W + 3] : ra[orig[a] * REC_ATOM_W + 3]; };
    auto row = [&](int q) __attribute__((always_inline)) { return mol ? mol_row(pb, q, na) : rec_row(rb, q, nt, remap); };
    auto round = [&](u64 r) __attribute__((always_inline)) {
        if (mol) refine_add_mol(tid, cur, acc, pb, nrows, na, own);
        else refine_add_rec(tid, cur, acc, rb, nrows, nt, remap, own);
        __syncthreads();
        refine_finish(tid, cur, acc, n, r);
        __syncthreads();
    };
    u64 shared = ~0ull;
    int zeros = 0;
    auto classes = [&]() __attribute__((always_inline)) { return refine_classes<SLOTS>(tid, cur, n, table, wi, shared, zeros); };
    auto sum_int = [&](int v) __attribute__((always_inline)) { return block_reduce(v, wi, [](int u, int w) { return u + w; }); };
    auto min_int = [&](int v) __attribute__((always_inline)) { return block_reduce(v, wi, [](int u, int w) { return min(u, w); }); };
    // h of the relabelled graph under the ranks `rank` (uniform)
    auto leaf_hash = [&](const u16* rank) __attribute__((always_inline)) {
        u64 h = 0;
        for (int a = tid; a < n; a += GT)
            h += mix(mix(mix(mix((u64)rank[a] + 1) + (u64)(cls_of(a) + 1)) + (u64)(long long)chg_of(a)) + (u64)tag[a]);
        for (int q = tid; q < nrows; q += GT) {
            const BondRow e = row(q);
            if (!e.v) continue;
            const u64 lo = min((int)rank[e.i], (int)rank[e.j]), hi = max((int)rank[e.i], (int)rank[e.j]);
            h += mix(mix(((lo << 32) | hi) + BOND_K) + (u64)e.o);
        }
        return block_reduce(h, wu, [](u64 u, u64 v) { return u + v; });
    };

    // <STEREO> the elements of the image, checked once: an index that is no atom of the image makes its element none
    const int* elements = nullptr;
    int s_unequal = 0, s_improved = 0, s_autos = 0;
    if constexpr (STEREO) {
        elements = d.elements + (size_t)b * d.cap_atoms * STEREO_W;
        auto atom = [&](int v, int least) __attribute__((always_inline)) { return v >= least && v < n; };
        for (int a = tid; a < n; a += GT) {
            const int* el = elements + a * STEREO_W;
            const int c = el[0];
            scode[a] = (signed char)((c == 1 || c == -1) && atom(el[1], 0) && atom(el[2], 0) && atom(el[3], 0) && atom(el[4], -1) ? c : 0);
            dsrc[a] = -1;
        }
        __syncthreads();
        for (int a = tid; a < n; a += GT) {
            const int* el = elements + a * STEREO_W;
            const int c = el[5], other = el[7];
            if ((c == 1 || c == -1) && atom(other, 0) && other != a && atom(el[8], 0) && atom(el[9], -1) && atom(el[10], 0) && atom(el[11], -1))
                dsrc[a] = dsrc[other] = (short)a;
        }
        __syncthreads();
    }
    // the stereo word of the leaf whose ranks are in rk, by position (every position is written: the ranks are a permutation)
    auto leaf_word = [&]() __attribute__((always_inline)) {
        for (int a = tid; a < n; a += GT) {
            int byte = 0;
            const int sc = scode[a], a0 = dsrc[a];
            if (sc != 0) {
                const int* el = elements + a * STEREO_W;
                const int last = el[4];
                const int r0 = rk[el[1]], r1 = rk[el[2]], r2 = rk[el[3]], r3 = last >= 0 ? (int)rk[last] : MAX_ATOMS;      // (the hydrogen stays last)
                const int swaps = (r0 > r1) + (r0 > r2) + (r0 > r3) + (r1 > r2) + (r1 > r3) + (r2 > r3);
                byte = ((swaps & 1) ? -sc : sc) > 0 ? 1 : 2;
            }
            if (a0 >= 0) {
                const int* el = elements + a0 * STEREO_W;
                const int other = a == a0 ? el[7] : a0;
                if (rk[a] < rk[other]) {      // the lower-rank end bears the bond's part
                    int v = el[5];
                    if (el[9] >= 0 && rk[el[8]] > rk[el[9]]) v = -v;
                    if (el[11] >= 0 && rk[el[10]] > rk[el[11]]) v = -v;
                    byte |= (v > 0 ? 1 : 2) << 2;
                }
            }
            sword[rk[a]] = (unsigned char)byte;
        }
        __syncthreads();
    };

    int leaves = 0, tries = 0, rounds = 0, levels_max = 0, pruned_trace = 0, pruned_orbit = 0, autos = 0, improved = 0;
    bool have_best = false;
    int best_levels = 0;
    if (!empty && n > 0) {
        enum { REFINE, CHILD, BACK };
        int mode = REFINE, target = -1, level = 0, less_from = NONE;
        u64 r = 0, best_h = 0;
        int prev = classes();
        while (true) {
            if (mode == REFINE) {
                int k = 0, c = 0;
                bool out = false;
                while (true) {
                    if (rounds >= max_rounds) { out = true; break; }
                    ++rounds, ++r, ++k;
                    round(r);
                    c = classes();
                    if (c <= prev || k >= n) break;
                    prev = c;
                }
                if (out) { status |= ABC_CANON_UNDECIDED; break; }
                const u64 s = refine_multiset_sum(tid, cur, n, wu);
                if (tid == 0) cur_k[level] = (u16)k, cur_c[level] = (u16)c, cur_sum[level] = s;
                levels_max = max(levels_max, level);
                mode = BACK, target = level - 1;
                if (have_best && less_from == NONE) {
                    const int bk = best_k[level], bc = best_c[level];
                    const u64 bs = best_sum[level];
                    const int cmp = k != bk ? (k < bk ? -1 : 1) : (c != bc ? (c < bc ? -1 : 1) : (s != bs ? (s < bs ? -1 : 1) : 0));
                    if (cmp > 0) {
                        ++pruned_trace;
                        continue;
                    }
                    if (cmp < 0) less_from = level;
                }
                if (c == n) {
                    // ---- (b) the leaf
                    ++leaves;
                    for (int a = tid; a < n; a += GT) {
                        const u64 e = cur[a];
                        int below = 0;
                        for (int x = 0; x < n; ++x) below += cur[x] < e;
                        rk[a] = (u16)below;
                    }
                    __syncthreads();     // (the ranks and tid 0's trace of this level are written)
                    const u64 h = leaf_hash(rk);
                    if constexpr (STEREO) leaf_word();
                    if (!have_best || less_from != NONE || h < best_h) {
                        improved += have_best;
                        for (int a = tid; a < n; a += GT) best_ids[a] = cur[a], brank[a] = rk[a];
                        if constexpr (STEREO)
                            for (int a = tid; a < n; a += GT) bword[a] = sword[a];
                        for (int l = tid; l <= level; l += GT) {
                            best_k[l] = cur_k[l], best_c[l] = cur_c[l], best_sum[l] = cur_sum[l];
                            if (l < level) best_choice[l] = choice[l];
                        }
                        have_best = true, best_levels = level, best_h = h, less_from = NONE;
                        __syncthreads();
                    } else if (h == best_h) {
                        // the map onto the best leaf by equal id, through the table
                        for (int k2 = tid; k2 < SLOTS; k2 += GT) table[k2] = 0;
                        if (tid == 0) zero_at = -1;
                        __syncthreads();
                        for (int a = tid; a < n; a += GT) {
                            const u64 e = best_ids[a];
                            if (e == 0) {
                                zero_at = a;
                                continue;
                            }
                            unsigned slot = (unsigned)(e >> 32) & (SLOTS - 1);
                            for (int probe = 0; probe < SLOTS; ++probe) {
                                const u64 old = atomicCAS(&table[slot], 0ull, e);
                                if (old == 0) {
                                    tidx[slot] = (u16)a;
                                    break;
                                }
                                if (old == e) break;
                                slot = (slot + 1) & (SLOTS - 1);
                            }
                        }
                        __syncthreads();
                        int bad = 0;
                        for (int a = tid; a < n; a += GT) {
                            const u64 e = cur[a];
                            int t = -1;
                            if (e == 0) {
                                t = zero_at;
                            } else {
                                unsigned slot = (unsigned)(e >> 32) & (SLOTS - 1);
                                for (int probe = 0; probe < SLOTS; ++probe) {
                                    const u64 at = table[slot];
                                    if (at == e) t = tidx[slot];
                                    if (at == e || at == 0) break;
                                    slot = (slot + 1) & (SLOTS - 1);
                                }
                            }
                            const int y = t < 0 || t >= n ? a : t;
                            gam[a] = (u16)y;
                            bad += t < 0 || t >= n || cls_of(a) != cls_of(y) || chg_of(a) != chg_of(y) || tag[a] != tag[y];
                        }
                        bool ok = sum_int(bad) == 0;      // (gam is written: the reduction synchronises)
                        if (ok) {
                            // the multiset of the mapped rows is the multiset of the rows, by counting
                            int common = 0;
                            for (int q = tid; q < nrows; q += GT) {
                                const BondRow e = row(q);
                                if (!e.v) continue;
                                const int gi = gam[e.i], gj = gam[e.j], lo = min(gi, gj), hi = max(gi, gj);
                                int before = 0, there = 0;
                                for (int q2 = 0; q2 < nrows; ++q2) {
                                    const BondRow e2 = row(q2);
                                    if (!e2.v || e2.o != e.o) continue;
                                    const int gi2 = gam[e2.i], gj2 = gam[e2.j];
                                    before += q2 < q && min(gi2, gj2) == lo && max(gi2, gj2) == hi;
                                    there += min(e2.i, e2.j) == lo && max(e2.i, e2.j) == hi;
                                }
                                common += before < there;
                            }
                            ok = sum_int(common) == nvalid;
                        }
                        if (!ok) { status |= ABC_CANON_COLLISION; break; }
                        if constexpr (STEREO) {
                            // the third key, compared exactly: the first position at which the words differ
                            int differs = NONE;
                            for (int k2 = tid; k2 < n; k2 += GT)
                                if (sword[k2] != bword[k2]) differs = min(differs, k2);
                            differs = min_int(differs);
                            if (differs != NONE) {      // a map that does not keep the stereo: no orbit merge, no jump
                                ++s_unequal;
                                const bool less = sword[differs] < bword[differs];
                                __syncthreads();         // (read before the best leaf's word is replaced)
                                if (less) {
                                    ++s_improved, ++improved;
                                    for (int a = tid; a < n; a += GT) best_ids[a] = cur[a], brank[a] = rk[a], bword[a] = sword[a];
                                    for (int l = tid; l < level; l += GT) best_choice[l] = choice[l];      // (the traces are equal)
                                    __syncthreads();
                                }
                                continue;
                            }
                            ++s_autos;
                        }
                        ++autos;
                        int first = NONE;
                        for (int l = tid; l < level; l += GT)
                            if (choice[l] != best_choice[l]) first = min(first, l);
                        target = min(min_int(first), level - 1);      // the level where the path left the best's
                        // x ~ gamma(x) in the orbit tables of the levels whose prefix gamma fixes: the greater root is hung under the less
                        const int upto = min(target, ORBITS - 1);
                        for (int l = 0; l <= upto; ++l) {
                            int* p = orbit[l];
                            for (int a = tid; a < n; a += GT) {
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
                        for (int l = 0; l <= upto; ++l) {     // flat again: every atom under its root, the least of its orbit
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
                    continue;
                }
                if (level + 1 >= n) { status |= ABC_CANON_COLLISION; break; }      // (only colliding hashes get here)
                // the cell: the least id that two atoms share; its last atom
                const u64 least = block_reduce(shared, wu, [](u64 u, u64 v) { return min(u, v); });
                const u64 cellv = zeros > 1 ? 0 : least;
                int last = -1;
                for (int a = tid; a < n; a += GT)
                    if (cur[a] == cellv) last = max(last, a);
                last = block_reduce(last, wi, [](int u, int w) { return max(u, w); });
                if (last < 0) { status |= ABC_CANON_COLLISION; break; }
                if (tid == 0) cell[level] = cellv, cell_max[level] = (u16)last, nxt[level] = 0;
                if (level < ORBITS)
                    for (int a = tid; a < MAX_ATOMS; a += GT) orbit[level][a] = a;
                __syncthreads();
                mode = CHILD;
            }
            if (mode == CHILD) {
                // ---- (c) the next atom of the cell that is the least of its orbit
                const u64 cellv = cell[level];
                const int from = nxt[level];
                const bool orbits = level < ORBITS;
                int first = MAX_ATOMS;
                for (int a = tid; a < n; a += GT)
                    if (a >= from && cur[a] == cellv && (!orbits || orbit[level][a] == a)) first = min(first, a);
                const int v = min_int(first);
                if (orbits) {
                    int skipped = 0;
                    for (int a = tid; a < n; a += GT) skipped += a >= from && a < v && cur[a] == cellv;
                    pruned_orbit += sum_int(skipped);
                }
                if (v >= n) {
                    mode = BACK, target = level - 1;
                    continue;
                }
                if (tries >= max_tries) { status |= ABC_CANON_UNDECIDED; break; }
                ++tries;
                prev = cur_c[level] + 1;
                if (tid == 0) choice[level] = (u16)v, nxt[level] = (u16)(v + 1), cur[v] = indiv(cur[v], level);
                __syncthreads();
                ++level;
                mode = REFINE;
                continue;
            }
            // ---- (d) back
            __syncthreads();
            for (int it = 0; it < n && target >= 0 && nxt[target] > cell_max[target]; ++it) --target;
            if (target < 0) break;
            level = target;
            if (less_from != NONE && less_from > level) less_from = NONE;
            for (int a = tid; a < n; a += GT) cur[a] = init[a];
            __syncthreads();
            r = 0;
            bool out = false;
            for (int k = 0; k <= level && !out; ++k) {
                const int todo = cur_k[k];
                for (int i = 0; i < todo; ++i) {
                    if (rounds >= max_rounds) { out = true; break; }
                    ++rounds, ++r;
                    round(r);
                }
                if (!out && k < level) {
                    if (tid == 0) cur[choice[k]] = indiv(cur[choice[k]], k);
                    __syncthreads();
                }
            }
            if (out) { status |= ABC_CANON_UNDECIDED; break; }
            mode = CHILD;
        }
    }
    __syncthreads();

    // ---- the outputs: every word of every buffer
    if (!have_best)
        for (int a = tid; a < n; a += GT) brank[a] = (u16)a;
    __syncthreads();
    const bool none = empty || n == 0;
    for (int k = tid; k < cap; k += GT)
        if (k >= n) order[k] = -1;
    for (int a = tid; a < n; a += GT) order[brank[a]] = orig[a];
    const u64 key0 = none ? 0 : leaf_hash(brank);
    u64 t = 0;
    if (have_best)
        for (int l = tid; l <= best_levels; l += GT) t += mix(mix(mix(mix((u64)l + 1) + (u64)best_k[l]) + (u64)best_c[l]) + best_sum[l]);
    t = block_reduce(t, wu, [](u64 u, u64 v) { return u + v; });
    if (tid == 0) {
        int* st = d.stats + (size_t)b * NCOL;
        st[ABC_CANON_STATUS] = status;
        st[ABC_CANON_LEAVES] = leaves, st[ABC_CANON_TRIES] = tries, st[ABC_CANON_ROUNDS] = rounds, st[ABC_CANON_LEVELS_MAX] = levels_max;
        st[ABC_CANON_PRUNED_TRACE] = pruned_trace, st[ABC_CANON_PRUNED_ORBIT] = pruned_orbit;
        st[ABC_CANON_AUTOMORPHISMS] = autos, st[ABC_CANON_IMPROVED] = improved;
        d.key[(size_t)b * 2] = (long long)key0;
        d.key[(size_t)b * 2 + 1] = empty ? 0 : (long long)mix(mix(mix((u64)n) + (u64)nvalid) + t);
        if constexpr (STEREO) {
            int* ss = d.stereo_search + (size_t)b * 4;
            ss[0] = s_unequal, ss[1] = s_improved, ss[2] = s_autos, ss[3] = 0;
        }
    }
    if (cert == nullptr && !want_rows) return;

    int* const oc = want_rows ? d.out_counts + (size_t)b * 4 : nullptr;
    int* const oa = want_rows ? d.out_atoms + (size_t)b * d.cap_atoms * ATOM_W : nullptr;
    int* const ob = want_rows ? d.out_bonds + (size_t)b * d.cap_mol_bonds * MOL_BOND_W : nullptr;
    int* const oh = want_rows ? d.out_implh + (size_t)b * d.cap_atoms : nullptr;
    if (cert != nullptr) {
        const int used = 2 + n + 3 * nvalid;
        for (int k = tid; k < 2 + cap + 3 * cap_bonds; k += GT)
            if (k >= used) cert[k] = -1;
        if (tid == 0) cert[0] = n, cert[1] = nvalid;
        for (int a = tid; a < n; a += GT)
            cert[2 + brank[a]] = (int)(((unsigned)chg_of(a) << 5) | ((unsigned)tag[a] << 4) | (unsigned)cls_of(a));
    }
    if (want_rows) {
        if (tid < 4) oc[tid] = d.mol_counts[(size_t)b * 4 + tid];
        for (int k = tid; k < (d.cap_atoms - n) * ATOM_W; k += GT) oa[n * ATOM_W + k] = 0;
        for (int k = tid; k < n * ATOM_W; k += GT) oa[brank[k / ATOM_W] * ATOM_W + k % ATOM_W] = pa[k];
        for (int k = tid; k < (d.cap_mol_bonds - nrows) * MOL_BOND_W; k += GT) ob[nrows * MOL_BOND_W + k] = 0;
        // the implicit-H list: the entries in 1..n renumbered and ascending, the others after them verbatim
        for (int k = tid; k < d.cap_atoms; k += GT) {
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
    // the bond rows, by counting: the place of a row among the certificate's triples and among the canonical rows
    for (int q = tid; q < nrows; q += GT) {
        const BondRow e = row(q);
        const bool valid = e.v;
        const int bi = valid ? brank[e.i] : 0, bj = valid ? brank[e.j] : 0, lo = min(bi, bj), hi = max(bi, bj);
        const int pair = lo * MAX_ATOMS + hi;
        int at_cert = 0, at_rows = 0, valid_before = 0;
        for (int q2 = 0; q2 < nrows; ++q2) {
            const BondRow e2 = row(q2);
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
        if (want_rows) {
            const int* src = pb + q * MOL_BOND_W;
            int* dst = ob + (valid ? at_rows : nvalid + q - valid_before) * MOL_BOND_W;
            dst[0] = valid ? bi + 1 : src[0], dst[1] = valid ? bj + 1 : src[1], dst[2] = src[2], dst[3] = src[3];
        }
    }
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
