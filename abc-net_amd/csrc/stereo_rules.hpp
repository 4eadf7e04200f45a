// The two stereo rules of DESIGN.md section 7, stated ONCE for the two kernels that apply them: smiles_compose_kernel (smiles.hip: the
// codes decide the marks of the text) and stereo_perceive_kernel (stereo.hip: the codes go into the element table).  Both kernels keep
// the molecule in LDS as lists of (neighbour << 3 | class) slots, filled by the same steps; here are
//   - the codes, the shapes both kernels are built for, owner_of and the rank sort of the lists (order_lists)
//   - the tetrahedral rule: stereo_code
//   - the double-bond rule: possible_end, substituents, ez_classify, and is_bridge, which makes a candidate RING behind either walk
// Every function is a template over the kernel's LDS struct (Walk of smiles.hip, Lists of stereo.hip), which name the members read here
// alike: adj, start, sym, charge, listed, rank, parent.  The structs themselves stay apart: an LDS offset is an immediate, and the
// writer's instructions are held line for line wherever a shared form allows it (profiles/r27_stereo_rules.md).
//
// STILL WRITTEN IN BOTH FILES, and why:
//   - Step 1 (row validation with the degree count, the scan into start[], the fill with the wedge order kept in the class bits), the
//     "pair listed twice" test of step 2 and the slot loop of step 3 (s2, wedge bits, doubles / others / partner).  They are loops in
//     the kernel's own body.  As functions (tried one at a time, with and without forced inlining) each leaves every instantiation of
//     the writer, the two without a rule included, with other instructions than it had: the same blocks in another order, and
//     another value in an immediate that the compiler numbers by the scope exits in front of it.
//     Neither copy decides anything about stereo: what the rules need of them is the layout of a slot, which is stated above.
//   - The depth-first walks: the writer's records the text's structure and keeps the lowpoint in registers, the perceiver's only
//     numbers the atoms.  A bridge is a property of the graph, so is_bridge reads either.
//   - The initial values of the per-atom arrays, the tallies (different columns), the exits of an image without elements, every output.
#pragma once
#include <hip/hip_runtime.h>
#include "../../include/abcnet_hip.h"
#include "mol_rows.hpp"

constexpr int ST = 256;                              // threads per workgroup
constexpr int MAX_ATOMS = ABC_MAX_SMILES_ATOMS;      // LDS arrays per atom
constexpr int MAX_BONDS = 4096, MAX_SLOTS = 2 * MAX_BONDS;
static_assert(MAX_ATOMS == 2 * ST, "the degree scan gives every thread two atoms");
static_assert(MAX_ATOMS <= 1 << 13 && MAX_SLOTS <= 1 << 16, "a slot holds neighbour << 3 | class in 16 bits, an index of a slot too");

// the code of an atom (abc_smiles_stereo_desc.stereo_out, column 0 of the element table); +1 / -1: the local parity of a marked centre
constexpr int ST_NONE = 0, ST_FLAT = 2, ST_UNQUALIFIED = 3;
// the code of a candidate double bond (abc_smiles_ez_desc.ez_out, column 5); +1 / -1: a marked double bond, together / opposite
constexpr int EZ_NONE = 0, EZ_FLAT = 2, EZ_RING = 3, EZ_TWIN = 4;
// the writer's alone, behind its walk: a class-1 bond that bears "/" or "\\" (1 | 4: the wedge orders are gone by then)
constexpr int CLS_DIRECTED = 5;

// the atom whose list holds slot s: start[a] <= s < start[a + 1]
template <class T>
__device__ inline int owner_of(const T& w, int na, int s) {
    int lo = 0, hi = na - 1;
    while (lo < hi) {                      // (at most 10 rounds)
        const int mid = (lo + hi + 1) >> 1;
        if ((int)w.start[mid] <= s) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// Order every atom's list: slot s of `src` goes to the position that counts the slots of its list with a smaller key (ties by
// slot: a permutation whatever the keys).  by_rank: the key is the neighbour's preorder rank, else the slot's own 16 bits.
// TAG, code: the code byte of every atom; a class-1 slot at a marked end (code +1 / -1) is stored as class 5, a slot with a direction.
// (by_rank and TAG are the writer's step 5; the order by index is step 2 of both kernels)
template <bool by_rank, bool TAG = false, class T>
__device__ inline void order_lists(T& w, int na, int slots, int src, int tid, const signed char* code = nullptr) {
    for (int s = tid; s < slots; s += ST) {
        const int a = owner_of(w, na, s), lo = w.start[a], hi = w.start[a + 1];
        const int e = w.adj[src][s];
        const int key = by_rank ? (int)w.rank[e >> 3] : e;
        int pos = 0;
        for (int t = lo; t < hi; ++t) {
            const int f = w.adj[src][t];
            const int other = by_rank ? (int)w.rank[f >> 3] : f;
            pos += other < key || (other == key && t < s);
        }
        if constexpr (TAG) {
            const int ca = code[a], cy = code[e >> 3];
            const bool directed = (e & 7) == 1 && (ca == 1 || ca == -1 || cy == 1 || cy == -1);
            w.adj[src ^ 1][lo + pos] = (unsigned short)(directed ? e | CLS_DIRECTED : e);
        } else {
            w.adj[src ^ 1][lo + pos] = (unsigned short)e;
        }
    }
}

// Atom i of degree deg, with `doubles` class-2 slots, the neighbour of the last being `partner`, and `others` set by a slot that is neither
// class 1 nor class 2: the other end of its double bond if the atom may be an end of a candidate (C or N, degree 2 or 3, one class-2
// bond, class 1 besides), else -1.  (The symbol is read here, behind the other tests: handed over as a value it is loaded for every atom.)
template <class T>
__device__ inline int possible_end(const T& w, int i, int deg, int doubles, int others, int partner) {
    return doubles == 1 && !others && (deg == 2 || deg == 3) && w.sym[i] <= 2 ? partner : -1;      // (0, 1: C; 2: N)
}

// The tetrahedral rule: the code of atom i, a candidate (end 1 of a wedge row): deg slots from lo in ascending neighbour index, zbits
// two bits per slot, single = every bond has class 1, h the text rule's hydrogen count.
template <class T>
__device__ inline int stereo_code(const T& w, const int* pa, int i, int lo, int deg, unsigned zbits, bool single, int h) {
    if (w.sym[i] == 12 || !single || !((deg == 4 && h == 0) || (deg == 3 && h == 1))) return ST_UNQUALIFIED;
    const int xa = pa[i * ATOM_W], ya = pa[i * ATOM_W + 1];
    bool flat = xa < 0 || xa > MAX_POSITION || ya < 0 || ya > MAX_POSITION;
    long long px[4], py[4], pz[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        px[k] = py[k] = pz[k] = 0;         // (the hydrogen of deg == 3 stands on the centre)
        if (k < deg) {
            const int j = w.adj[1][lo + k] >> 3;      // (< na: the row's ends were checked in step 1)
            const int x = pa[j * ATOM_W], y = pa[j * ATOM_W + 1];
            flat |= x < 0 || x > MAX_POSITION || y < 0 || y > MAX_POSITION || (x == xa && y == ya);
            const unsigned z = zbits >> (2 * k) & 3u;
            px[k] = (long long)x - xa, py[k] = (long long)y - ya, pz[k] = z == 1 ? 1 : (z == 2 ? -1 : 0);
        }
    }
    if (flat) return ST_FLAT;
    const long long a1 = px[0] - px[3], a2 = py[0] - py[3], a3 = pz[0] - pz[3];
    const long long b1 = px[1] - px[3], b2 = py[1] - py[3], b3 = pz[1] - pz[3];
    const long long c1 = px[2] - px[3], c2 = py[2] - py[3], c3 = pz[2] - pz[3];
    const long long t = a1 * (b2 * c3 - b3 * c2) - a2 * (b1 * c3 - b3 * c1) + a3 * (b1 * c2 - b2 * c1);
    return t == 0 ? ST_FLAT : (t > 0 ? 1 : -1);
}

// the substituents of end e besides `other`, ascending (the lists are in index order), `none` where there is none; cnt, 0 on entry,
// counts them: 0 .. 2
template <class T>
__device__ inline void substituents(const T& w, int e, int other, int none, int (&sub)[2], int& cnt) {
    sub[0] = sub[1] = none;
    for (int s = w.start[e], hi = w.start[e + 1]; s < hi; ++s) {      // (degree 2 or 3: one or two besides the partner)
        const int y = w.adj[1][s] >> 3;
        if (y != other && cnt < 2) sub[cnt++] = y;
    }
}

// The double-bond rule: the code of the candidate between a < b (both possible ends naming each other), a bridge supposed; lists by
// index in adj[1].  The code goes to z.code of both ends.  SIDES, for the writer's symbols: z.sub0 of an end is the lower of its
// substituents, z.bits its SIDE0 / SIDE1, set where sub0 / the other substituent lies on the positive side of a -> b.
constexpr unsigned EZ_SIDE0 = 1, EZ_SIDE1 = 2;
template <bool SIDES, class T, class Z>
__device__ inline void ez_classify(const T& w, Z& z, const int* pa, int a, int b) {
    int sub[2][2], cnt[2] = {0, 0};
    bool twin = false;
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const int e = k ? b : a, other = k ? a : b;
        substituents(w, e, other, e, sub[k], cnt[k]);
        if (cnt[k] == 1) sub[k][1] = sub[k][0];
        const int s0 = sub[k][0], s1 = sub[k][1];
        twin |= cnt[k] == 2 && w.start[s0 + 1] - w.start[s0] == 1 && w.start[s1 + 1] - w.start[s1] == 1
                && atom_class(w.sym[s0]) == atom_class(w.sym[s1]) && w.charge[s0] == w.charge[s1] && w.listed[s0] == w.listed[s1];
    }
    int code = EZ_TWIN;
    unsigned bits[2] = {0, 0};
    if (!twin) {
        const long long ax = pa[a * ATOM_W], ay = pa[a * ATOM_W + 1], bx = pa[b * ATOM_W], by = pa[b * ATOM_W + 1];
        const long long dx = bx - ax, dy = by - ay;
        bool flat = ax < 0 || ax > MAX_POSITION || ay < 0 || ay > MAX_POSITION || bx < 0 || bx > MAX_POSITION || by < 0 || by > MAX_POSITION;
        int side[2][2];
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const long long ex = k ? bx : ax, ey = k ? by : ay;
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                const long long x = pa[sub[k][t] * ATOM_W], y = pa[sub[k][t] * ATOM_W + 1];
                flat |= x < 0 || x > MAX_POSITION || y < 0 || y > MAX_POSITION;
                const long long c = dx * (y - ey) - dy * (x - ex);      // (in range: below 2^40)
                side[k][t] = (c > 0) - (c < 0);
                flat |= c == 0;
            }
            flat |= cnt[k] == 2 && side[k][0] == side[k][1];
            bits[k] = (side[k][0] > 0 ? EZ_SIDE0 : 0) | (side[k][1] > 0 ? EZ_SIDE1 : 0);
        }
        code = flat ? EZ_FLAT : (side[0][0] == side[1][0] ? 1 : -1);
    }
    z.code[a] = z.code[b] = (signed char)code;
    if constexpr (SIDES) {
        z.sub0[a] = (short)sub[0][0], z.sub0[b] = (short)sub[1][0];
        z.bits[a] = (unsigned char)bits[0], z.bits[b] = (unsigned char)bits[1];
    }
}

// Behind a depth-first walk that left preorder ranks, parents and, in low[], the least rank every subtree reaches by one ring bond: is
// the bond between i and j a bridge?  (A tree bond to a child that reaches nothing above itself.)  A candidate that is none is RING.
template <class T>
__device__ inline bool is_bridge(const T& w, const short* low, int i, int j) {
    const int child = w.parent[j] == i ? j : (w.parent[i] == j ? i : -1);
    return child >= 0 && low[child] == w.rank[child];
}
