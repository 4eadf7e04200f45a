// The rows the decoder's stages hand to each other (extract -> assemble -> mol block / graph score / graph similarity), for the
// device side; the host side is abc-net_amd/contract.py, the table of every row and count DESIGN.md section 7.
#pragma once
#include <hip/hip_runtime.h>
#include "../../include/abcnet_hip.h"

// int32 words per row: atoms of both layouts, bond candidates, molecule bonds, record atoms, record bonds
constexpr int ATOM_W = 5, CAND_W = 4, MOL_BOND_W = 4, REC_ATOM_W = 4, REC_BOND_W = 3;
// the element table of stereo.hip, int32 [B][cap_atoms][STEREO_W] (include/abcnet_hip.h, abc_stereo_desc): [0] centre code; [1..4] a
// marked centre's neighbours ascending, the hydrogen -1 last; [5] at the lower-index end of a candidate double bond its code; [6..11] of
// a marked one the bond row, the partner, this end's substituents ascending, the partner's; "none" is 0 in [0] and [5], -1 elsewhere
constexpr int STEREO_W = ABC_STEREO_W;
constexpr int N_SYMBOLS = 14;        // the atom vocabulary of utils.py:12-13: indices 0 .. 13
// x and y of an atom row, 0 .. 199999: what the mol block can print (|px - 60| * 500 * 2 + 3 stays far inside int32), and the range of
// the stereo rules (stereo_rules.hpp), where every product of two differences stays under 2^40
constexpr int MAX_POSITION = 199999;

__device__ inline int clampi(int v, int lo, int hi) { return min(max(v, lo), hi); }

// The class of a vocabulary index: 0 (the reference's unknown) decodes to carbon, img2smiles2.py:24-25.  The two differ ON PURPOSE:
// in graph_score.hip's an unknown matches nothing (-1), in graph_sim.hip's an unknown equals an unknown (class 0 equals only itself).
__device__ inline int symbol_class(int t) { return t < 0 || t >= N_SYMBOLS ? -1 : (t == 0 ? 1 : t); }
__device__ inline int atom_class(int t) { return t < 0 || t >= N_SYMBOLS ? 0 : (t == 0 ? 1 : t); }

// the ends of molecule row q / record row k as atom indices of their side, false for a row that names no pair
__device__ inline bool mol_ends(const int* pb, int q, int na, int& e1, int& e2) {
    const int r1 = pb[q * MOL_BOND_W], r2 = pb[q * MOL_BOND_W + 1];      // 1-based
    if (r1 < 1 || r2 < 1 || r1 > na || r2 > na || r1 == r2) return false;
    e1 = r1 - 1, e2 = r2 - 1;
    return true;
}
__device__ inline bool rec_ends(const int* rb, int k, int nt, int& i, int& j) {
    i = rb[k * REC_BOND_W], j = rb[k * REC_BOND_W + 1];
    return i >= 0 && j >= 0 && i < nt && j < nt && i != j;
}

// ---- the one reader of an image per side: counts clamped to their capacities, no rows when EMPTY (MolCounts below: the text kernels')
// the molecule side of image b (every descriptor names these fields alike).  status: the two bits the assembler set; nh = 0 and ph null
// for a descriptor whose mol_implh is null or that has no such field
struct MolImage {
    int status, na, nb, nh;            // EMPTY | TRUNCATED of abc_mol_status, atoms, bonds, implicit-H entries
    bool empty;
    const int *pa, *pb, *ph;           // mol_atoms, mol_bonds, mol_implh of the image
};
// the counts row of image b alone, clamped to the capacities but NOT zeroed when EMPTY, and the two status bits: what mol_image starts
// from, and the whole reader of the text kernels (molblock.hip, smiles.hip), which test EMPTY first, always have mol_implh and measured
// slower through mol_image (profiles/r24_image_reader.md).  The four words are read before anything is decided: one load of the row
struct MolCounts { int na, nb, nh, status; };
template <class Desc>
__device__ inline MolCounts mol_counts_row(const Desc& d, int b) {
    const int* mc = d.mol_counts + (size_t)b * 4;
    MolCounts c;
    c.na = clampi(mc[0], 0, d.cap_atoms);
    c.nb = clampi(mc[1], 0, d.cap_mol_bonds);
    c.nh = clampi(mc[2], 0, d.cap_atoms);
    c.status = mc[3] & (ABC_MOL_EMPTY | ABC_MOL_TRUNCATED);
    return c;
}
// d.mol_implh, or null for a descriptor without the field (the scoring descriptors: scored_image goes through mol_image too).  The
// int / long parameter only ranks the overloads: the first is taken wherever it compiles
template <class Desc> __device__ inline auto implh_of(const Desc& d, int) -> decltype(d.mol_implh) { return d.mol_implh; }
template <class Desc> __device__ inline const int* implh_of(const Desc&, long) { return nullptr; }
template <class Desc>
__device__ inline MolImage mol_image(const Desc& d, int b) {
    const MolCounts c = mol_counts_row(d, b);
    const int* implh = implh_of(d, 0);
    MolImage s;
    s.status = c.status;
    s.empty = (s.status & ABC_MOL_EMPTY) != 0;
    s.na = s.empty ? 0 : c.na, s.nb = s.empty ? 0 : c.nb;
    s.nh = s.empty || implh == nullptr ? 0 : c.nh;
    s.pa = d.mol_atoms + (size_t)b * d.cap_atoms * ATOM_W;
    s.pb = d.mol_bonds + (size_t)b * d.cap_mol_bonds * MOL_BOND_W;
    s.ph = implh != nullptr ? implh + (size_t)b * d.cap_atoms : nullptr;
    return s;
}
// the record side of image b
struct RecImage {
    int nt, m;                         // record atoms and bonds
    const int *ra, *rb;                // rec_atoms, rec_bonds of the image
};
template <class Desc>
__device__ inline RecImage rec_image(const Desc& d, int b) {
    RecImage s;
    s.nt = clampi(d.rec_counts[b], 0, d.max_atoms), s.m = clampi(d.rec_counts[d.B + b], 0, d.max_bonds);
    s.ra = d.rec_atoms + (size_t)b * d.max_atoms * REC_ATOM_W;
    s.rb = d.rec_bonds + (size_t)b * d.max_bonds * REC_BOND_W;
    return s;
}

// image b of a scoring kernel: both sides (the scoring kernels read no status bit beyond MolImage's two)
struct ScoredImage {
    int nt, m, status, na, nb;
    bool empty;
    const int *pa, *pb, *ra, *rb;
};
// false for an image at or past n_valid: its row is zeroed and the workgroup has nothing more to do (uniform)
template <int NCOL, class Desc>
__device__ inline bool scored_image(const Desc& d, int b, int tid, ScoredImage& s) {
    const int nv = d.n_valid != nullptr ? clampi(*d.n_valid, 0, d.B) : d.B;
    if (b >= nv) {
        if (tid < NCOL) d.rows[(size_t)b * NCOL + tid] = 0;
        return false;
    }
    const RecImage r = rec_image(d, b);
    const MolImage m = mol_image(d, b);
    s = {r.nt, r.m, m.status, m.na, m.nb, m.empty, m.pa, m.pb, r.ra, r.rb};
    return true;
}

// the end of a scoring kernel, one lane: the row of the image, its non-zero columns added to the totals (64-bit atomicAdd)
template <int NCOL>
__device__ inline void write_row_and_totals(int* row, uint64_t* totals, const int (&r)[NCOL]) {
#pragma unroll
    for (int i = 0; i < NCOL; ++i) {
        row[i] = r[i];
        if (r[i] != 0) atomicAdd((unsigned long long*)&totals[i], (unsigned long long)r[i]);
    }
}
