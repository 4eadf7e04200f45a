// A SMILES string for every assembled molecule, written on the device from the rows of abc_assemble_graphs, read in place
// (decode.Molecule.smiles() is the host form and the oracle).  The contract -- text rule, statuses, prefix rule -- is in
// include/abcnet_hip.h and DESIGN.md section 7.  Integers only.
//
//   smiles_compose_kernel  one workgroup per image.  The walk is done ONCE, here, and what is kept of it is the text itself: the
//                          image's bytes go to its own slice of `work`, its length to work[b] (-1: a refused row, -2: the ring limit)
//     1  validate every row; count degrees by LDS atomics, scan them, fill a CSR adjacency of (neighbour << 3 | order class)
//     2  order every atom's list by neighbour index (a rank sort, one slot per thread at a time: position = how many of the list
//        are smaller); equal neighbours side by side are a pair listed twice
//     3  per atom: aromatic flag and hydrogen count; <stereo> the centre's code from its wedge slots, its neighbours' positions and
//        an int64 determinant (one byte per atom), after which a wedge slot is a class-1 slot like any other
//     4  ONE lane walks the graph (depth first, the parent pointers are the stack: no restart of a cursor, 2 m + n steps): preorder
//        rank, parent, the class of the bond to the parent, which atoms open a branch and how many ")" follow each position
//     5  order every list again, by the RANK of the neighbour: a neighbour that is neither the parent nor a child is the other end of
//        a ring bond, the lower ranks (closings) now come first and both kinds in the order the rule writes them; every slot
//        finds its twin in the neighbour's list (binary search)
//     6  ONE lane hands out the ring numbers in preorder (the free numbers are two 64-bit masks), O(n + m)
//     7  all threads: the byte length of every preorder position, a workgroup scan, and every thread writes its positions;
//        <stereo> a centre's mark is its code times the sign of the permutation from index order to the order the text names
//   smiles_pack_kernel     one workgroup per image: the prefix rule over work[0 .. b] (text_pack.hpp), then a copy of the image's bytes
// Lengths and bytes come from ONE emitter run over two sinks, so they cannot disagree; every store of either kernel is checked
// against the end of the image's own bytes.
// Both kernels are templates over a mode of two bits: <stereo> the tetrahedral rule (abc_write_smiles_stereo), <ez> the double-bond
// rule (abc_write_smiles_ez), both of DESIGN.md section 7; a line of a rule the mode does not hold is compiled out.  <ez> adds:
//     3  per atom: is it a possible end (C or N, degree 2 or 3, one class-2 bond, class 1 besides); then one thread per candidate
//        (two such ends naming each other): twin, the sides of its substituents from the positions (int64), its code
//     4  the walk keeps a lowpoint per atom (of the atom it stands on: in a register); behind it a tree bond to c is a bridge iff
//        low[c] == rank[c]: any other candidate is RING
//     5  the rank sort stores a class-1 slot at a marked end as class 5, a parallel pass does the same for the tree bonds: from here
//        on a bond that bears a symbol is told from bits that are loaded anyway
//     6  the same lane, in the same pass over the preorder, fixes the orientation of every group at the first symbol it meets (a
//        stack over the group's double bonds, which form a tree: every one is pushed once)
//     7  the symbol of a class-5 bond comes from the marked end's side bits and orientation
#include "common.hpp"
#include "../../include/abcnet_hip.h"
#include "capi_util.hpp"
#include "block_scan.hpp"
#include "mol_rows.hpp"
#include "graph_ids.hpp"
#include "text_pack.hpp"
#include "text_hydrogens.hpp"
#include "stereo_rules.hpp"      // ST, MAX_ATOMS, MAX_BONDS, the codes, the rank sort and both stereo rules: shared with stereo.hip

namespace {

constexpr int MAX_NUMBER = 99;
constexpr int LEN_BAD_ROW = -1, LEN_RING_LIMIT = -2;

// decode.ATOM_SYMBOLS, two columns each
__device__ const char SYMBOL2[N_SYMBOLS * 2 + 1] = "C C N O P F ClS BrB SeI H Si";
constexpr unsigned BARE_SET = 0x3FFFu & ~(1u << 10 | 1u << 12 | 1u << 13);                                  // all but Se, H, Si
// (AROMATIC_SET, the valence lists and hydrogens(): text_hydrogens.hpp, shared with aromatic.hip)

// two sinks for one emitter: Count adds up, Write stores below `end`
struct Count {
    int n;
    __device__ inline void put(int) { ++n; }
};
struct Write {
    uint8_t* at;
    const uint8_t* end;
    __device__ inline void put(int c) {
        if (at < end) *at = (uint8_t)c;
        ++at;
    }
};

template <class Sink>
__device__ inline void put_number(Sink& o, int k) {
    if (k >= 10) o.put('%'), o.put('0' + k / 10);
    o.put('0' + (k >= 10 ? k % 10 : k));
}
// class 1: nothing, but '-' between two aromatic atoms; 2 '='; 3 '#'; 4: nothing between two aromatic atoms, else ':'
template <class Sink>
__device__ inline void put_bond(Sink& o, int cls, bool both_aromatic) {
    if (cls == 1) { if (both_aromatic) o.put('-'); }
    else if (cls == 2) o.put('=');
    else if (cls == 3) o.put('#');
    else if (!both_aromatic) o.put(':');
}
// marks: 0 none, 1 "@", 2 "@@" (a marked atom is never bare)
template <class Sink>
__device__ inline void put_token(Sink& o, int sym, int charge, int h, bool aromatic, bool listed, int marks = 0) {
    const int lower = aromatic ? 0x20 : 0;
    const bool bare = charge == 0 && !listed && (BARE_SET >> sym & 1u) && marks == 0;
    if (!bare) o.put('[');
    o.put(SYMBOL2[sym * 2] | lower);
    if (SYMBOL2[sym * 2 + 1] != ' ') o.put(SYMBOL2[sym * 2 + 1]);
    if (bare) return;
    if (marks >= 1) o.put('@');
    if (marks >= 2) o.put('@');
    if (h >= 1) o.put('H');
    if (h >= 2) o.put('0' + h);            // (h <= 6: the largest valence)
    if (charge != 0) {
        o.put(charge > 0 ? '+' : '-');
        const int m = charge > 0 ? charge : -charge;      // (1 .. 15)
        if (m >= 10) o.put('1');
        if (m >= 2) o.put('0' + m % 10);
    }
    o.put(']');
}

// everything the emitter reads, in LDS
struct Walk {
    unsigned short adj[2][MAX_SLOTS];      // [0]: the lists as filled, then ordered by rank; [1]: ordered by index, then the twins
    unsigned char number[MAX_SLOTS];       // the ring number of a ring bond's slot, at both ends
    int deg[MAX_ATOMS];                    // degree, then the fill cursor
    unsigned short start[MAX_ATOMS + 1];
    short rank[MAX_ATOMS], parent[MAX_ATOMS], last_child[MAX_ATOMS];
    unsigned short order[MAX_ATOMS], cursor[MAX_ATOMS], closes[MAX_ATOMS];
    unsigned char sym[MAX_ATOMS], hcount[MAX_ATOMS], aromatic[MAX_ATOMS], listed[MAX_ATOMS], opens[MAX_ATOMS], parent_cls[MAX_ATOMS];
    signed char charge[MAX_ATOMS];
};

// The mark of a centre at preorder position p: 1 "@", 2 "@@".  The text names its four neighbours as parent, hydrogen, closings,
// openings, children (the lists are in rank order: each kind stands in the order it is written); the local order is ascending
// index with the hydrogen last, so the permutation's sign is the parity of the pairs out of order.
__device__ inline int stereo_marks(const Walk& w, int a, int p, int code) {
    const int par = w.parent[a], lo = w.start[a], hi = w.start[a + 1];
    unsigned long long named = 0;          // 16 bits per neighbour, the first in the highest place used
    if (par >= 0) named = (unsigned)par;
    if (hi - lo == 3) named = named << 16 | 0xFFFFu;
    for (int s = lo; s < hi; ++s) {        // closings, then openings
        const int y = w.adj[0][s] >> 3;
        if (y != par && w.parent[y] != a) named = named << 16 | (unsigned)y;
    }
    for (int s = lo; s < hi; ++s) {
        const int y = w.adj[0][s] >> 3;
        if (y != par && w.parent[y] == a) named = named << 16 | (unsigned)y;
    }
    const int k0 = (int)(named >> 48 & 0xFFFFu), k1 = (int)(named >> 32 & 0xFFFFu), k2 = (int)(named >> 16 & 0xFFFFu), k3 = (int)(named & 0xFFFFu);
    const int swaps = (k0 > k1) + (k0 > k2) + (k0 > k3) + (k1 > k2) + (k1 > k3) + (k2 > k3);
    return ((swaps & 1) ? -code : code) > 0 ? 1 : 2;
}

// ez: what is kept per atom of the double bond it is an end of (an atom is an end of at most one candidate)
constexpr unsigned EZ_UP = 4, EZ_FIXED = 8;      // (beside EZ_SIDE0, EZ_SIDE1 of the rule)
template <bool EZ>
struct Ends {
    short partner[EZ ? MAX_ATOMS : 1];          // after step 3: the other end of this atom's one class-2 bond if the atom may be an end, else -1
    short sub0[EZ ? MAX_ATOMS : 1];             // the lower of its substituents
    short low[EZ ? MAX_ATOMS : 1];              // the least rank its subtree reaches by one ring bond
    signed char code[EZ ? MAX_ATOMS : 1];       // the code of its candidate, 0 without one
    unsigned char bits[EZ ? MAX_ATOMS : 1];     // side > 0 of sub0 and of the other substituent, the orientation u > 0, u is fixed
};
template <bool EZ> struct WalkRegs { int low, parent; };      // the lowpoint and the parent of the atom the walk stands on
template <> struct WalkRegs<false> {};
template <bool EZ>
__device__ inline bool ez_marked(const Ends<EZ>& z, int e) { return z.code[e] == 1 || z.code[e] == -1; }
template <bool EZ>
__device__ inline int ez_side(const Ends<EZ>& z, int e, int s) { return (z.bits[e] & (s == z.sub0[e] ? EZ_SIDE0 : EZ_SIDE1)) ? 1 : -1; }
template <bool EZ>
__device__ inline int ez_u(const Ends<EZ>& z, int e) { return (z.bits[e] & EZ_UP) ? 1 : -1; }

// One lane, in text order: the directed bond read first -> second (an end of it is marked).  The first symbol met of a group fixes
// the group: it is "/".  `stack` holds one end of every double bond whose neighbours are still to be tied (each once).
__device__ inline void ez_fix(const Walk& w, Ends<true>& z, unsigned short* stack, int first, int second) {
    int e, s, sign;
    if (ez_marked(z, first)) e = first, s = second, sign = 1;
    else e = second, s = first, sign = -1;
    if (z.bits[e] & EZ_FIXED) return;
    const unsigned up = sign * ez_side(z, e, s) > 0 ? EZ_UP : 0;
    z.bits[e] |= EZ_FIXED | up, z.bits[z.partner[e]] |= EZ_FIXED | up;
    int top = 0;
    stack[top++] = (unsigned short)e;
    while (top > 0) {
        const int x0 = stack[--top];
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const int x = k ? (int)z.partner[x0] : x0;
            for (int q = w.start[x], hi = w.start[x + 1]; q < hi; ++q) {
                const int t = w.adj[0][q] >> 3;
                if (t == z.partner[x] || !ez_marked(z, t) || (z.bits[t] & EZ_FIXED)) continue;
                // the bond x -> t read from both ends: u(x) side(x, t) = -u(t) side(t, x)
                const unsigned ut = -ez_u(z, x) * ez_side(z, x, t) * ez_side(z, t, x) > 0 ? EZ_UP : 0;
                z.bits[t] |= EZ_FIXED | ut, z.bits[z.partner[t]] |= EZ_FIXED | ut;
                if (top < MAX_ATOMS) stack[top++] = (unsigned short)t;      // (at most one entry per double bond: never full)
            }
        }
    }
}

// the symbol of the directed bond read first -> second
template <bool EZ>
__device__ inline int ez_symbol(const Ends<EZ>& z, int first, int second) {
    if (ez_marked(z, first)) return ez_u(z, first) * ez_side(z, first, second) > 0 ? '/' : '\\';
    return ez_u(z, second) * ez_side(z, second, first) < 0 ? '/' : '\\';
}

// position p of the preorder: what stands in front of the atom, its token, its ring digits, the brackets behind it
template <int MODE, class Sink>
__device__ inline void put_position(Sink& o, const Walk& w, const signed char* centre, const Ends<(MODE & 2) != 0>& z, int p) {
    constexpr bool STEREO = (MODE & 1) != 0, EZ = (MODE & 2) != 0;
    const int a = w.order[p], par = w.parent[a];
    const bool arom = w.aromatic[a] != 0;
    if (par < 0) {
        if (p > 0) o.put('.');
    } else {
        if (w.opens[a]) o.put('(');
        if (EZ && w.parent_cls[a] == CLS_DIRECTED) o.put(ez_symbol(z, par, a));
        else put_bond(o, w.parent_cls[a], arom && w.aromatic[par]);
    }
    int marks = 0;
    if (STEREO) {
        const int code = centre[a];
        if (code == 1 || code == -1) marks = stereo_marks(w, a, p, code);
    }
    put_token(o, w.sym[a], w.charge[a], w.hcount[a], arom, w.listed[a] != 0, marks);
    for (int s = w.start[a], hi = w.start[a + 1]; s < hi; ++s) {
        const int e = w.adj[0][s], y = e >> 3;
        if (y == par || w.parent[y] == a) continue;
        if (w.rank[y] < p) {                                               // a closing: the symbol, then the number
            if (EZ && (e & 7) == CLS_DIRECTED) o.put(ez_symbol(z, a, y));
            else put_bond(o, e & 7, arom && w.aromatic[y]);
        }
        put_number(o, w.number[s]);
    }
    for (int i = w.closes[p]; i > 0; --i) o.put(')');
}

// the modes: bit 0 tetrahedral, bit 1 double bonds
template <int MODE> struct DescOf { typedef abc_smiles_ez_desc type; };
template <> struct DescOf<0> { typedef abc_smiles_desc type; };
template <> struct DescOf<1> { typedef abc_smiles_stereo_desc type; };

// bytes one image may take at these capacities (abc_smiles_text_bytes, abc_smiles_stereo_text_bytes: a marked token is two bytes
// longer and never bare): also the stride of the slices of `work`
template <bool STEREO>
__host__ __device__ inline int64_t image_bytes(int64_t cap_atoms, int64_t cap_mol_bonds) { return (STEREO ? 14 : 12) * cap_atoms + 7 * cap_mol_bonds; }
template <int MODE>
__device__ inline uint8_t* slice_of(const typename DescOf<MODE>::type& d, int b) {
    return (uint8_t*)(d.work + d.B) + (size_t)b * (size_t)image_bytes<(MODE & 1) != 0>(d.cap_atoms, d.cap_mol_bonds);
}

// stereo / ez, an image without text (EMPTY, refused): a row of zeros, and every word of its slice of stereo_out / ez_out
template <int MODE>
__device__ inline void no_centres(const typename DescOf<MODE>::type& d, int b, int tid) {
    if constexpr ((MODE & 1) != 0) {
        if (tid < 4) d.stereo_stats[(size_t)b * 4 + tid] = 0;
        if (d.stereo_out != nullptr)
            for (int i = tid; i < d.cap_atoms; i += ST) d.stereo_out[(size_t)b * d.cap_atoms + i] = 0;
    }
    if constexpr ((MODE & 2) != 0) {
        if (tid < 4) d.ez_stats[(size_t)b * 4 + tid] = 0;
        if (d.ez_out != nullptr)
            for (int q = tid; q < d.cap_mol_bonds; q += ST) d.ez_out[(size_t)b * d.cap_mol_bonds + q] = 0;
    }
}

template <int MODE>
__global__ __launch_bounds__(ST) void smiles_compose_kernel(const typename DescOf<MODE>::type d) {
    constexpr bool STEREO = (MODE & 1) != 0, EZ = (MODE & 2) != 0;
    __shared__ Walk w;
    __shared__ Ends<EZ> z;                                      // <ez>
    __shared__ int ez_tally[4];                                 // <ez> marked, flat, ring, twin
    __shared__ unsigned wt[ST / 64 + 1];
    __shared__ int refused;                // 0, LEN_BAD_ROW or LEN_RING_LIMIT
    __shared__ signed char centre[STEREO ? MAX_ATOMS : 1];      // <stereo> the code of every atom
    __shared__ int tally[4];                                    // <stereo> marked, flat, unqualified, wedge rows
    const int b = blockIdx.x, tid = threadIdx.x;
    const MolCounts c = mol_counts_row(d, b);
    const int na = c.na, nb = c.nb, slots = 2 * nb;
    if ((c.status & ABC_MOL_EMPTY) || na == 0) {      // (uniform.  Bonds without an atom cannot be: their ends are outside 1..0)
        if (tid == 0) d.work[b] = (c.status & ABC_MOL_EMPTY) || nb == 0 ? 0 : LEN_BAD_ROW;
        if constexpr (MODE != 0) no_centres<MODE>(d, b, tid);
        return;
    }
    const int* pa = d.mol_atoms + (size_t)b * d.cap_atoms * ATOM_W;
    const int* pb = d.mol_bonds + (size_t)b * d.cap_mol_bonds * MOL_BOND_W;
    const int* ph = d.mol_implh + (size_t)b * d.cap_atoms;

    // ---- 1: rows
    if (tid == 0) refused = 0;
    if (STEREO && tid < 4) tally[tid] = 0;
    if (EZ && tid < 4) ez_tally[tid] = 0;
    for (int i = tid; i < na; i += ST) {
        w.deg[i] = 0;
        w.rank[i] = w.parent[i] = w.last_child[i] = -1;
        w.closes[i] = 0;
        w.listed[i] = w.opens[i] = w.parent_cls[i] = 0;
    }
    __syncthreads();
    bool bad = false;
    for (int i = tid; i < na; i += ST) {
        const int t = pa[i * ATOM_W + 2], q = pa[i * ATOM_W + 3];
        bad |= t < 0 || t >= N_SYMBOLS || q < -15 || q > 15;
        w.sym[i] = (unsigned char)clampi(t, 0, N_SYMBOLS - 1);
        w.charge[i] = (signed char)clampi(q, -15, 15);
    }
    for (int q = tid; q < nb; q += ST) {
        int e1, e2;
        if (mol_ends(pb, q, na, e1, e2) && bond_class(pb[q * MOL_BOND_W + 2]) != 0) {
            atomicAdd(&w.deg[e1], 1);
            atomicAdd(&w.deg[e2], 1);
        } else {
            bad = true;
        }
    }
    for (int k = tid; k < c.nh; k += ST) {
        const int a = ph[k];
        if (a >= 1 && a <= na) w.listed[a - 1] = 1;      // (several entries may name one atom: they store the same byte)
    }
    if (bad) atomicOr(&refused, LEN_BAD_ROW);
    __syncthreads();
    if (refused) {                         // (uniform: read behind the barrier)
        if (tid == 0) d.work[b] = LEN_BAD_ROW;
        if constexpr (MODE != 0) no_centres<MODE>(d, b, tid);
        return;
    }
    {   // every thread takes atoms 2 tid and 2 tid + 1
        const int i0 = 2 * tid, d0 = i0 < na ? w.deg[i0] : 0, d1 = i0 + 1 < na ? w.deg[i0 + 1] : 0;
        unsigned total;
        const unsigned first = block_excl_scan<ST>((unsigned)(d0 + d1), wt, &total);      // (total == slots)
        if (i0 < na) w.start[i0] = (unsigned short)first, w.deg[i0] = 0;
        if (i0 + 1 < na) w.start[i0 + 1] = (unsigned short)(first + d0), w.deg[i0 + 1] = 0;
        if (tid == 0) w.start[na] = (unsigned short)total;
    }
    __syncthreads();
    for (int q = tid; q < nb; q += ST) {
        int e1, e2;
        mol_ends(pb, q, na, e1, e2);       // (true for every row: checked above)
        const int order = pb[q * MOL_BOND_W + 2], cls = bond_class(order);
        // <stereo> a wedge speaks for its end 1 alone: that end's slot keeps the order, 5 or 6, in the three class bits until step 3
        const bool wedge = STEREO && order >= 5;
        w.adj[0][w.start[e1] + atomicAdd(&w.deg[e1], 1)] = (unsigned short)(e2 << 3 | (wedge ? order : cls));
        w.adj[0][w.start[e2] + atomicAdd(&w.deg[e2], 1)] = (unsigned short)(e1 << 3 | cls);
        if (wedge) atomicAdd(&tally[3], 1);
    }
    __syncthreads();

    // ---- 2: by neighbour index (into adj[1]); a pair listed twice
    order_lists<false>(w, na, slots, 0, tid);
    __syncthreads();
    bad = false;
    for (int i = tid; i < na; i += ST)
        for (int s = w.start[i] + 1, hi = w.start[i + 1]; s < hi; ++s) bad |= w.adj[1][s] >> 3 == w.adj[1][s - 1] >> 3;
    if (bad) atomicOr(&refused, LEN_BAD_ROW);

    // ---- 3: classes
    for (int i = tid; i < na; i += ST) {
        int s2 = 0, any4 = 0;
        unsigned zbits = 0;
        int doubles = 0, others = 0, partner = -1;      // <ez>
        const int lo = w.start[i], deg = w.start[i + 1] - lo;
        for (int s = lo, hi = lo + deg; s < hi; ++s) {
            int cls = w.adj[1][s] & 7;
            if (STEREO && cls >= 5) {      // this atom's own wedge: from here on a class-1 slot (no other thread reads this list now)
                if (s - lo < 4) zbits |= (unsigned)(cls - 4) << (2 * (s - lo));
                zbits |= 1u << 8;
                cls = 1;
                w.adj[1][s] = (unsigned short)((w.adj[1][s] & ~7) | 1);
            }
            s2 += bond_s2(cls);
            any4 |= cls == 4;
            if constexpr (EZ) {
                if (cls == 2) ++doubles, partner = w.adj[1][s] >> 3;
                else others |= cls != 1;
            }
        }
        if constexpr (EZ) {
            z.partner[i] = (short)possible_end(w, i, deg, doubles, others, partner);
            z.code[i] = EZ_NONE;
            z.bits[i] = 0;
        }
        w.aromatic[i] = (unsigned char)(any4 && (AROMATIC_SET >> w.sym[i] & 1u));
        w.hcount[i] = (unsigned char)(w.listed[i] ? 1 : hydrogens(w.sym[i], w.charge[i], s2));
        w.cursor[i] = w.start[i];
        if constexpr (STEREO) {
            int code = ST_NONE;
            if (zbits) {
                code = stereo_code(w, pa, i, lo, deg, zbits & 0xFFu, s2 == 2 * deg, w.hcount[i]);
                atomicAdd(&tally[code == ST_FLAT ? 1 : (code == ST_UNQUALIFIED ? 2 : 0)], 1);
            }
            centre[i] = (signed char)code;
        }
    }
    __syncthreads();
    if (refused) {
        if (tid == 0) d.work[b] = LEN_BAD_ROW;
        if constexpr (MODE != 0) no_centres<MODE>(d, b, tid);
        return;
    }
    if constexpr (EZ) {                    // one thread per candidate, the one of its lower end (it alone writes both ends)
        for (int i = tid; i < na; i += ST) {
            const int j = z.partner[i];
            if (j > i && z.partner[j] == i) ez_classify<true>(w, z, pa, i, j);
        }
    }

    // ---- 4: the walk
    if (tid == 0) {
        int next = 0, steps = slots + 2 * na;      // (every slot is passed once, every atom is left once)
        for (int root = 0; root < na; ++root) {
            if (w.rank[root] >= 0) continue;
            w.rank[root] = (short)next;
            w.order[next++] = (unsigned short)root;
            int cur = root;
            WalkRegs<EZ> reg;                  // <ez> of the atom the walk stands on, in registers: a slot passed costs no LDS access
            if constexpr (EZ) reg.low = next - 1, reg.parent = -1;
            while (cur >= 0 && steps-- > 0) {
                const int at = w.cursor[cur];
                if (at == w.start[cur + 1]) {
                    if constexpr (EZ) {            // the atom's lowpoint is final; the parent's, kept when the walk went down, takes it in
                        z.low[cur] = (short)reg.low;
                        cur = reg.parent;
                        if (cur >= 0) reg.low = min((int)z.low[cur], reg.low), reg.parent = w.parent[cur];
                    } else {
                        cur = w.parent[cur];
                    }
                    continue;
                }
                w.cursor[cur] = (unsigned short)(at + 1);
                const int e = w.adj[1][at], y = e >> 3;
                if (w.rank[y] >= 0) {              // the parent, or the other end of a ring bond
                    if constexpr (EZ)
                        if (y != reg.parent) reg.low = min(reg.low, (int)w.rank[y]);
                    continue;
                }
                const int before = w.last_child[cur];
                if (before >= 0) {                 // that child was not the last: it stands in a branch, which ends behind the
                    w.opens[before] = 1;           // atom visited last
                    w.closes[next - 1] += 1;
                }
                w.last_child[cur] = (short)y;
                w.parent[y] = (short)cur;
                w.parent_cls[y] = (unsigned char)(e & 7);
                w.rank[y] = (short)next;
                if constexpr (EZ) z.low[cur] = (short)reg.low, reg.parent = cur, reg.low = next;
                w.order[next++] = (unsigned short)y;
                cur = y;
            }
        }
    }
    __syncthreads();

    if constexpr (EZ) {                    // a candidate that is no bridge is RING, whatever else it is; the counters
        for (int i = tid; i < na; i += ST) {
            const int j = z.partner[i];
            if (j <= i || z.code[i] == EZ_NONE) continue;      // (a code: the two ends name each other)
            const bool bridge = is_bridge(w, z.low, i, j);      // (ahead of the code's load: the order that moves this kernel least, r27_stereo_rules.md)
            int code = z.code[i];
            if (!bridge) z.code[i] = z.code[j] = (signed char)(code = EZ_RING);
            atomicAdd(&ez_tally[code == EZ_FLAT ? 1 : (code == EZ_RING ? 2 : (code == EZ_TWIN ? 3 : 0))], 1);
        }
        __syncthreads();                   // (the codes are final: step 5 tags the slots, and here the tree bonds, that bear a symbol)
        for (int i = tid; i < na; i += ST) {
            const int par = w.parent[i];
            if (par >= 0 && w.parent_cls[i] == 1 && (ez_marked(z, i) || ez_marked(z, par))) w.parent_cls[i] = CLS_DIRECTED;
        }
    }

    // ---- 5: by rank (back into adj[0]), then the twin of every slot (over adj[1])
    order_lists<true, EZ>(w, na, slots, 1, tid, z.code);
    __syncthreads();
    for (int s = tid; s < slots; s += ST) {
        const int a = owner_of(w, na, s), y = w.adj[0][s] >> 3, want = w.rank[a];
        int lo = w.start[y], hi = w.start[y + 1] - 1;
        while (lo < hi) {                  // (the list of y holds a, once, and is ascending in rank)
            const int mid = (lo + hi) >> 1;
            if ((int)w.rank[w.adj[0][mid] >> 3] < want) lo = mid + 1;
            else hi = mid;
        }
        w.adj[1][s] = (unsigned short)lo;
    }
    __syncthreads();

    // ---- 6: ring numbers
    if (tid == 0) {
        typedef unsigned long long u64;
        u64 free_lo = ~1ull, free_hi = (1ull << (MAX_NUMBER - 63)) - 1;      // bit k of lo: number k (1 .. 63); bit j of hi: 64 + j
        bool limit = false;
        for (int p = 0; p < na && !limit; ++p) {
            const int a = w.order[p], par = w.parent[a];
            u64 closed_lo = 0, closed_hi = 0;
            if constexpr (EZ)                  // (w.cursor is free behind the walk: the stack)
                if (par >= 0 && w.parent_cls[a] == CLS_DIRECTED) ez_fix(w, z, w.cursor, par, a);
            for (int s = w.start[a], hi = w.start[a + 1]; s < hi; ++s) {
                const int y = w.adj[0][s] >> 3;
                if (y == par || w.parent[y] == a) continue;
                if (w.rank[y] < p) {
                    if constexpr (EZ)
                        if ((w.adj[0][s] & 7) == CLS_DIRECTED) ez_fix(w, z, w.cursor, a, y);
                    const int k = w.number[s];
                    if (k < 64) closed_lo |= 1ull << k;
                    else closed_hi |= 1ull << (k - 64);
                    continue;
                }
                int k;
                if (free_lo) k = __ffsll((long long)free_lo) - 1, free_lo &= free_lo - 1;
                else if (free_hi) k = 64 + __ffsll((long long)free_hi) - 1, free_hi &= free_hi - 1;
                else {
                    limit = true;
                    break;
                }
                w.number[s] = (unsigned char)k;
                w.number[w.adj[1][s]] = (unsigned char)k;
            }
            free_lo |= closed_lo, free_hi |= closed_hi;
        }
        if (limit) refused = LEN_RING_LIMIT;
    }
    __syncthreads();
    if (refused) {
        if (tid == 0) d.work[b] = LEN_RING_LIMIT;
        if constexpr (MODE != 0) no_centres<MODE>(d, b, tid);
        return;
    }

    // ---- 7: the bytes
    int lo, hi;
    text_pack::my_range<ST>(na, tid, lo, hi);
    Count n = {0};
    for (int p = lo; p < hi; ++p) put_position<MODE>(n, w, centre, z, p);
    unsigned total;
    const unsigned first = block_excl_scan<ST>((unsigned)n.n, wt, &total);
    uint8_t* slice = slice_of<MODE>(d, b);
    Write o = {slice + first, slice + image_bytes<STEREO>(d.cap_atoms, d.cap_mol_bonds)};
    for (int p = lo; p < hi; ++p) put_position<MODE>(o, w, centre, z, p);
    if (tid == 0) d.work[b] = (int)total;
    if constexpr (STEREO) {
        if (tid < 4) d.stereo_stats[(size_t)b * 4 + tid] = tally[tid];
        if (d.stereo_out != nullptr)
            for (int i = tid; i < d.cap_atoms; i += ST) d.stereo_out[(size_t)b * d.cap_atoms + i] = i < na ? (int)centre[i] : 0;
    }
    if constexpr (EZ) {
        if (tid < 4) d.ez_stats[(size_t)b * 4 + tid] = ez_tally[tid];
        if (d.ez_out != nullptr)
            for (int q = tid; q < d.cap_mol_bonds; q += ST) {      // the code of a candidate's row stands on both its ends
                int code = 0, e1, e2;
                if (q < nb && mol_ends(pb, q, na, e1, e2) && bond_class(pb[q * MOL_BOND_W + 2]) == 2 && z.partner[e1] == e2
                    && z.partner[e2] == e1)
                    code = z.code[e1];
                d.ez_out[(size_t)b * d.cap_mol_bonds + q] = code;
            }
    }
}

template <int MODE>
__global__ __launch_bounds__(ST) void smiles_pack_kernel(const typename DescOf<MODE>::type d) {
    constexpr bool STEREO = (MODE & 1) != 0;
    const int b = blockIdx.x, tid = threadIdx.x;
    int* offsets = d.index;
    int* status_out = d.index + d.B + 1;
    const text_pack::Span span = text_pack::prefix_rule<ST>(d.work, b, d.cap_text);
    const int len = d.work[b];
    const bool overflow = span.through > (unsigned long long)d.cap_text;
    if (tid == 0) {
        if (b == 0) offsets[0] = 0;
        offsets[b + 1] = (int)span.fits;      // (fits <= cap_text <= INT32_MAX; == through unless this image overflows)
        status_out[b] = mol_counts_row(d, b).status | (len == LEN_BAD_ROW ? ABC_TEXT_BAD_ROW : 0) | (len == LEN_RING_LIMIT ? ABC_TEXT_RING_LIMIT : 0)
                        | (overflow ? ABC_TEXT_OVERFLOW : 0);
    }
    if (overflow || len <= 0) return;
    // (through - before == len, and through <= cap_text: every store is inside the image's own bytes; the slice holds len of them)
    const uint8_t* slice = slice_of<MODE>(d, b);
    const int n = (int)min((long long)len, (long long)image_bytes<STEREO>(d.cap_atoms, d.cap_mol_bonds));
    for (int i = tid; i < n; i += ST) d.text[span.before + i] = slice[i];
}

// the guards of both entry points, and the two launches
template <int MODE>
int write_smiles(const typename DescOf<MODE>::type* d, abc_stream_t stream, const char* what) {
    char msg[160];
#define REFUSE(code, text) return (snprintf(msg, sizeof msg, "%s: %s", what, text), abc_fail(code, msg))
    if (!d) REFUSE(ABC_EINVAL, "null descriptor");
    if (d->B < 1) REFUSE(ABC_EINVAL, "empty");
    if (d->cap_atoms < 1 || d->cap_mol_bonds < 1) REFUSE(ABC_EINVAL, "cap_atoms and cap_mol_bonds must be >= 1");
    if (d->cap_atoms > MAX_ATOMS) REFUSE(ABC_EUNSUPPORTED, "cap_atoms must be <= 512 (ABC_MAX_SMILES_ATOMS)");
    if (d->cap_mol_bonds > MAX_BONDS) REFUSE(ABC_EUNSUPPORTED, "cap_mol_bonds must be <= 4096");
    if (d->cap_text < 1 || d->cap_text > INT32_MAX) REFUSE(ABC_EINVAL, "cap_text must be 1..2^31-1");
    if (!d->mol_counts || !d->mol_atoms || !d->mol_bonds || !d->mol_implh) REFUSE(ABC_EINVAL, "null molecule buffer");
    if (!d->text || !d->index || !d->work) REFUSE(ABC_EINVAL, "null output");
    if constexpr ((MODE & 1) != 0)
        if (!d->stereo_stats) REFUSE(ABC_EINVAL, "null stereo_stats");
    if constexpr ((MODE & 2) != 0)
        if (!d->ez_stats) REFUSE(ABC_EINVAL, "null ez_stats");
#undef REFUSE
    hipLaunchKernelGGL(smiles_compose_kernel<MODE>, dim3(d->B), dim3(ST), 0, (hipStream_t)stream, *d);
    hipLaunchKernelGGL(smiles_pack_kernel<MODE>, dim3(d->B), dim3(ST), 0, (hipStream_t)stream, *d);
    return abc_check_launch(what);
}

}  // namespace

extern "C" int abc_smiles_desc_size(void) { return (int)sizeof(abc_smiles_desc); }

extern "C" int64_t abc_smiles_text_bytes(const abc_smiles_desc* d) {
    if (!d || d->cap_atoms < 1 || d->cap_mol_bonds < 1) return 0;
    return image_bytes<false>(d->cap_atoms, d->cap_mol_bonds);
}

extern "C" int64_t abc_smiles_work_ints(const abc_smiles_desc* d) {
    if (!d || d->B < 1 || d->cap_atoms < 1 || d->cap_mol_bonds < 1) return 0;
    return d->B + (d->B * image_bytes<false>(d->cap_atoms, d->cap_mol_bonds) + 3) / 4;
}

extern "C" int abc_write_smiles(const abc_smiles_desc* d, abc_stream_t stream) { return write_smiles<0>(d, stream, "write_smiles"); }

extern "C" int abc_smiles_stereo_desc_size(void) { return (int)sizeof(abc_smiles_stereo_desc); }

extern "C" int64_t abc_smiles_stereo_text_bytes(const abc_smiles_stereo_desc* d) {
    if (!d || d->cap_atoms < 1 || d->cap_mol_bonds < 1) return 0;
    return image_bytes<true>(d->cap_atoms, d->cap_mol_bonds);
}

extern "C" int64_t abc_smiles_stereo_work_ints(const abc_smiles_stereo_desc* d) {
    if (!d || d->B < 1 || d->cap_atoms < 1 || d->cap_mol_bonds < 1) return 0;
    return d->B + (d->B * image_bytes<true>(d->cap_atoms, d->cap_mol_bonds) + 3) / 4;
}

extern "C" int abc_write_smiles_stereo(const abc_smiles_stereo_desc* d, abc_stream_t stream) {
    return write_smiles<1>(d, stream, "write_smiles_stereo");
}

extern "C" int abc_smiles_ez_desc_size(void) { return (int)sizeof(abc_smiles_ez_desc); }

extern "C" int64_t abc_smiles_ez_text_bytes(const abc_smiles_ez_desc* d) {
    if (!d || d->cap_atoms < 1 || d->cap_mol_bonds < 1) return 0;
    return d->tetrahedral ? image_bytes<true>(d->cap_atoms, d->cap_mol_bonds) : image_bytes<false>(d->cap_atoms, d->cap_mol_bonds);
}

extern "C" int64_t abc_smiles_ez_work_ints(const abc_smiles_ez_desc* d) {
    if (!d || d->B < 1 || d->cap_atoms < 1 || d->cap_mol_bonds < 1) return 0;
    return d->B + (d->B * abc_smiles_ez_text_bytes(d) + 3) / 4;
}

extern "C" int abc_write_smiles_ez(const abc_smiles_ez_desc* d, abc_stream_t stream) {
    if (d && d->tetrahedral) return write_smiles<3>(d, stream, "write_smiles_ez");
    return write_smiles<2>(d, stream, "write_smiles_ez");
}
