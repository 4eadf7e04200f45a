// Aromaticity perception per image: the rows of abc_assemble_graphs (or the bond rows of a graph record) copied with the bonds of every
// aromatic cycle set to order 4, so that a ring drawn with alternating orders 1 / 2 and the same ring drawn with order 4 are ONE graph
// for everything downstream (graph_canon.hip, smiles.hip, graph_score.hip, graph_sim.hip, graph_ident.hip).  The rule is this project's
// own -- a function of the graph alone, integers only -- and stands in include/abcnet_hip.h (abc_aromatic_desc) and DESIGN.md section 7;
// its host form is decode.perceive_aromatic, its oracle tests/aromatic_oracle.py.
//
// One workgroup per image.  The graph is one side of graph_refine.hpp's (mol_row / rec_row: the valid rows, the order class).
//   1  degrees by LDS atomics and up to three (neighbour, class, row) slots per atom; a fourth row leaves no slot and no candidate
//   2  the candidate flag of every atom
//   3  every thread takes start atoms and walks the simple paths of candidates above the start (a candidate has at most three rows:
//      3 * 2^5 paths of seven atoms at the most; the path is seven registers, one function per depth); a path that closes on its start
//      with 5, 6 or 7 atoms and its second atom below its last is a candidate cycle, met exactly once: RING is OR-ed into its slots
//   4  the electrons e of every candidate, from the input classes and the RING marks
//   5  the same walk: a cycle without NONE whose e sum to 6 is aromatic, AROMATIC is OR-ed into its slots
//   6  one thread per bond row writes the output row; its mark is in the slots of its lower end
//   7  (molecule side) one thread per two atoms compares the text rule's hydrogen count before and after; the atoms that would lose
//      their hydrogen are appended to the implicit-H list, ascending, by a workgroup scan
// The slot ORDER of an atom depends on the order the LDS atomics are served in; nothing that is written does: marks are OR-ed, the
// counters are sums, and a candidate's slots hold all of its rows whatever their order.  One pass: no step reads an order it wrote.
// Every barrier stands outside divergent code; every index read from a row is range-checked by mol_ends / rec_ends first.
#include "common.hpp"
#include "../../include/abcnet_hip.h"
#include "capi_util.hpp"
#include "block_scan.hpp"
#include "mol_rows.hpp"
#include "graph_ids.hpp"
#include "graph_refine.hpp"
#include "text_hydrogens.hpp"

namespace {

constexpr int GT = REFINE_GT;
constexpr int MAX_ATOMS = ABC_MAX_SIM_ATOMS;
constexpr int NCOL = ABC_AROM_NCOL;
constexpr int SLOTS = 3;             // rows of a candidate at the most
constexpr int MAX_RING = 7;
constexpr unsigned NB_MASK = 1023u, CLS_SHIFT = 10, RING = 1u << 13, AROMATIC = 1u << 14;     // a slot: neighbour | class << 10 | marks
constexpr int NOT_CANDIDATE = ABC_AROM_NOT_CANDIDATE, NONE = ABC_AROM_NONE;
static_assert(MAX_ATOMS == 2 * GT && MAX_ATOMS <= (int)NB_MASK + 1, "two atoms per thread in the scan; a neighbour fits its slot bits");
// vocabulary indices (decode.ATOM_SYMBOLS): the sets the rule names
constexpr unsigned SET_C = 1u << 0 | 1u << 1, SET_N_P = 1u << 2 | 1u << 4, SET_O_S_SE = 1u << 3 | 1u << 7 | 1u << 10, SET_B = 1u << 9;
constexpr unsigned SET_N_O_S_SE = 1u << 2 | SET_O_S_SE;
__device__ inline bool in_set(unsigned set, int sym) { return sym >= 0 && sym < N_SYMBOLS && (set >> sym & 1u); }

// what the walk reads, in LDS
struct Rings {
    unsigned slot[MAX_ATOMS * SLOTS];
    int slot_row[MAX_ATOMS * SLOTS];
    int deg[MAX_ATOMS];
    signed char code[MAX_ATOMS];     // NOT_CANDIDATE, NONE or e
    signed char sym[MAX_ATOMS], chg[MAX_ATOMS];      // vocabulary index (-1: none), charge clamped to -2..2: read once, in step 1
    unsigned char cand[MAX_ATOMS], listed[MAX_ATOMS];
};

// OR `bit` into the slot of u that names v, and into the slot of v that names u (candidates: each names the other once)
__device__ inline void mark_bond(Rings& g, int u, int v, unsigned bit) {
#pragma unroll
    for (int k = 0; k < SLOTS; ++k) {
        if (k < g.deg[u] && (int)(g.slot[u * SLOTS + k] & NB_MASK) == v) atomicOr(&g.slot[u * SLOTS + k], bit);
        if (k < g.deg[v] && (int)(g.slot[v * SLOTS + k] & NB_MASK) == u) atomicOr(&g.slot[v * SLOTS + k], bit);
    }
}

// a cycle of D atoms was met: pass 3 marks it RING; pass 5 marks it AROMATIC if no atom is NONE and the electrons sum to 6
template <bool ELECTRONS>
struct Hit {
    int found;
    template <int D>
    __device__ inline void cycle(Rings& g, const int (&path)[MAX_RING]) {
        if (ELECTRONS) {
            int sum = 0;
            bool none = false;
#pragma unroll
            for (int i = 0; i < D; ++i) {
                const int e = g.code[path[i]];
                none |= e < 0;
                sum += e;
            }
            if (none || sum != 6) return;
        }
        ++found;
#pragma unroll
        for (int i = 0; i < D; ++i) mark_bond(g, path[i], path[i + 1 < D ? i + 1 : 0], ELECTRONS ? AROMATIC : RING);
    }
};

// path[0 .. D) is a simple path of candidates, path[0] its least atom: every way on from path[D - 1]
template <int D, bool ELECTRONS>
__device__ __forceinline__ void walk(Rings& g, int (&path)[MAX_RING], Hit<ELECTRONS>& hit) {
    const int u = path[D - 1], du = g.deg[u];
#pragma unroll 1
    for (int k = 0; k < SLOTS; ++k) {
        if (k >= du) break;
        const int v = (int)(g.slot[u * SLOTS + k] & NB_MASK);
        if (v == path[0]) {
            if (D >= 5 && path[1] < path[D - 1]) hit.template cycle<D>(g, path);
            continue;
        }
        if (v < path[0] || !g.cand[v]) continue;
        if constexpr (D < MAX_RING) {
            bool seen = false;
#pragma unroll
            for (int i = 1; i < D; ++i) seen |= path[i] == v;
            if (seen) continue;
            path[D] = v;
            walk<D + 1, ELECTRONS>(g, path, hit);
        }
    }
}

template <bool ELECTRONS>
__device__ inline int walk_all(Rings& g, int n, int tid) {
    Hit<ELECTRONS> hit = {0};
    for (int s = tid; s < n; s += GT) {
        if (!g.cand[s]) continue;
        int path[MAX_RING] = {s, 0, 0, 0, 0, 0, 0};
        walk<1, ELECTRONS>(g, path, hit);
    }
    return hit.found;
}

// 17 KB of LDS, 51 VGPRs, no scratch
__global__ __launch_bounds__(GT) void aromatic_kernel(const abc_aromatic_desc d) {
    __shared__ Rings g;
    __shared__ unsigned wt[REFINE_NW + 1];
    __shared__ int tally[4];             // candidates, candidate cycles, aromatic cycles, rows changed
    const int b = blockIdx.x, tid = threadIdx.x;
    const bool mol = d.mol_counts != nullptr;
    const int cap = mol ? d.cap_atoms : d.max_atoms, cap_bonds = mol ? d.cap_mol_bonds : d.max_bonds;

    // ---- the image (mol_rows.hpp), of the side that was given
    int status = 0, n = 0, nrows = 0, nlisted = 0;
    const int *pa = nullptr, *pb = nullptr, *ph = nullptr, *ra = nullptr, *rb = nullptr;
    if (mol) {
        const MolImage im = mol_image(d, b);
        status = im.status, n = im.na, nrows = im.nb, nlisted = im.nh, pa = im.pa, pb = im.pb, ph = im.ph;
    } else {
        const RecImage im = rec_image(d, b);
        n = im.nt, nrows = im.m, ra = im.ra, rb = im.rb;
    }
    auto row = [&](int q) __attribute__((always_inline)) { return mol ? mol_row(pb, q, n) : rec_row(rb, q, n); };
    auto sym_of = [&](int a) __attribute__((always_inline)) { return (int)g.sym[a]; };
    auto chg_of = [&](int a) __attribute__((always_inline)) { return (int)g.chg[a]; };

    // ---- 1: degrees and slots; symbol and charge of every atom (a charge outside -1..1 only has to stay outside)
    if (tid < 4) tally[tid] = 0;
    for (int a = tid; a < MAX_ATOMS; a += GT) {
        if (a < n) {
            const int t = mol ? pa[a * ATOM_W + 2] : ra[a * REC_ATOM_W + 2], q = mol ? pa[a * ATOM_W + 3] : ra[a * REC_ATOM_W + 3];
            g.sym[a] = (signed char)(t < 0 || t >= N_SYMBOLS ? -1 : t);
            g.chg[a] = (signed char)clampi(q, -2, 2);
        }
        g.deg[a] = 0;
        g.cand[a] = g.listed[a] = 0;
        g.code[a] = (signed char)NOT_CANDIDATE;
#pragma unroll
        for (int k = 0; k < SLOTS; ++k) g.slot[a * SLOTS + k] = 0, g.slot_row[a * SLOTS + k] = -1;
    }
    __syncthreads();
    for (int q = tid; q < nrows; q += GT) {
        const BondRow e = row(q);
        if (!e.v) continue;
        const int ki = atomicAdd(&g.deg[e.i], 1), kj = atomicAdd(&g.deg[e.j], 1);
        if (ki < SLOTS) g.slot[e.i * SLOTS + ki] = (unsigned)e.j | (unsigned)e.o << CLS_SHIFT, g.slot_row[e.i * SLOTS + ki] = q;
        if (kj < SLOTS) g.slot[e.j * SLOTS + kj] = (unsigned)e.i | (unsigned)e.o << CLS_SHIFT, g.slot_row[e.j * SLOTS + kj] = q;
    }
    for (int k = tid; k < nlisted; k += GT) {
        const int a = ph[k];
        if (a >= 1 && a <= n) g.listed[a - 1] = 1;       // (several entries may name one atom: they store the same byte)
    }
    __syncthreads();

    // ---- 2: candidates
    {
        int mine = 0;
        for (int a = tid; a < n; a += GT) {
            const int deg = g.deg[a], chg = chg_of(a);
            bool ok = in_set(AROMATIC_SET, sym_of(a)) && chg >= -1 && chg <= 1 && (deg == 2 || deg == 3);
            if (ok) {
                int doubles = 0, nb[SLOTS];
#pragma unroll
                for (int k = 0; k < SLOTS; ++k) {
                    const unsigned s = g.slot[a * SLOTS + k];
                    const int cls = (int)(s >> CLS_SHIFT & 7u);
                    nb[k] = k < deg ? (int)(s & NB_MASK) : -1 - k;
                    if (k < deg) ok &= cls != 0 && cls != 3, doubles += cls == 2;
                }
                ok &= doubles <= 1 && nb[0] != nb[1] && nb[0] != nb[2] && nb[1] != nb[2];
            }
            g.cand[a] = ok;
            mine += ok;
        }
        if (mine) atomicAdd(&tally[0], mine);
    }
    __syncthreads();

    // ---- 3: the ring bonds
    {
        const int found = walk_all<false>(g, n, tid);
        if (found) atomicAdd(&tally[1], found);
    }
    __syncthreads();

    // ---- 4: electrons
    for (int a = tid; a < n; a += GT) {
        if (!g.cand[a]) continue;
        const int deg = g.deg[a], sym = sym_of(a), chg = chg_of(a);
        int e = NONE;
        bool has2 = false, has4 = false;
#pragma unroll
        for (int k = 0; k < SLOTS; ++k) {
            if (k >= deg) continue;
            const unsigned s = g.slot[a * SLOTS + k];
            const int cls = (int)(s >> CLS_SHIFT & 7u);
            has4 |= cls == 4;
            if (cls == 2) {
                has2 = true;
                e = (s & RING) ? 1 : (in_set(SET_N_O_S_SE, sym_of((int)(s & NB_MASK))) ? 0 : NONE);
            }
        }
        if (!has2) {
            if (in_set(SET_C, sym)) e = chg == 0 ? (has4 ? 1 : NONE) : (chg < 0 ? 2 : 0);
            else if (in_set(SET_B, sym)) e = chg == 0 ? 0 : NONE;
            else if (in_set(SET_N_P, sym)) e = chg < 0 ? 2 : (chg > 0 ? (has4 ? 1 : NONE) : (has4 ? (deg == 3 ? 2 : 1) : 2));
            else e = chg == 0 ? 2 : NONE;      // O, S, Se
        }
        g.code[a] = (signed char)e;
    }
    __syncthreads();

    // ---- 5: the aromatic cycles
    {
        const int found = walk_all<true>(g, n, tid);
        if (found) atomicAdd(&tally[2], found);
    }
    __syncthreads();

    // ---- 6: the bond rows, every word up to the capacity
    {
        int changed = 0;
        int* const ob = mol ? d.out_bonds + (size_t)b * d.cap_mol_bonds * MOL_BOND_W : d.out_rec_bonds + (size_t)b * d.max_bonds * REC_BOND_W;
        const int width = mol ? MOL_BOND_W : REC_BOND_W;
        const int* const src = mol ? pb : rb;
        for (int q = tid; q < cap_bonds; q += GT) {
            int* dst = ob + (size_t)q * width;
            if (q >= nrows) {
                for (int w = 0; w < width; ++w) dst[w] = 0;
                continue;
            }
            const BondRow e = row(q);
            bool marked = false;
            if (e.v) {
                const int lo = min(e.i, e.j);
                if (g.cand[lo]) {
#pragma unroll
                    for (int k = 0; k < SLOTS; ++k) marked |= g.slot_row[lo * SLOTS + k] == q && (g.slot[lo * SLOTS + k] & AROMATIC) != 0;
                }
            }
            const int order = src[q * width + 2];
            changed += marked && order != 4;
            dst[0] = src[q * width], dst[1] = src[q * width + 1], dst[2] = marked ? 4 : order;
            if (mol) dst[3] = src[q * width + 3];
        }
        if (changed) atomicAdd(&tally[3], changed);
    }

    // ---- 7: atoms, counts and the implicit-H list (molecule side)
    int added = 0;
    if (mol) {
        int* const oc = d.out_counts + (size_t)b * 4;
        int* const oa = d.out_atoms + (size_t)b * d.cap_atoms * ATOM_W;
        int* const oh = d.out_implh + (size_t)b * d.cap_atoms;
        for (int k = tid; k < d.cap_atoms * ATOM_W; k += GT) oa[k] = k < n * ATOM_W ? pa[k] : 0;
        // the atoms whose hydrogen count by the text rule is 1 on the input rows and 0 on the output rows (only a candidate's rows change)
        auto loses_h = [&](int a) __attribute__((always_inline)) {
            if (a >= n || !g.cand[a] || g.listed[a]) return 0u;
            int before = 0, after = 0;
#pragma unroll
            for (int k = 0; k < SLOTS; ++k) {
                if (k >= g.deg[a]) continue;
                const unsigned s = g.slot[a * SLOTS + k];
                const int cls = (int)(s >> CLS_SHIFT & 7u);
                before += bond_s2(cls), after += bond_s2((s & AROMATIC) ? 4 : cls);
            }
            const int sym = sym_of(a), chg = chg_of(a);
            return (unsigned)(hydrogens(sym, chg, before) == 1 && hydrogens(sym, chg, after) == 0);
        };
        const unsigned f0 = loses_h(2 * tid), f1 = loses_h(2 * tid + 1);
        unsigned total;
        const unsigned first = block_excl_scan<GT>(f0 + f1, wt, &total);       // (every thread: the scan synchronises)
        const int room = d.cap_atoms - nlisted;                                // (a list that names an atom twice may leave too little)
        added = min((int)total, room);
        if (f0 && (int)first < room) oh[nlisted + first] = 2 * tid + 1;
        if (f1 && (int)(first + f0) < room) oh[nlisted + first + f0] = 2 * tid + 2;
        for (int k = tid; k < d.cap_atoms; k += GT) {
            if (k < nlisted) oh[k] = ph[k];
            else if (k >= nlisted + added) oh[k] = 0;
        }
        if (tid < 4) {
            const int v = d.mol_counts[(size_t)b * 4 + tid];
            oc[tid] = tid == 2 && !(status & ABC_MOL_EMPTY) ? nlisted + added : v;
        }
    }
    if (d.code_out != nullptr)
        for (int k = tid; k < cap; k += GT) d.code_out[(size_t)b * cap + k] = k < n ? (int)g.code[k] : NOT_CANDIDATE;
    __syncthreads();                     // (tally[3] is complete)
    if (tid == 0) {
        int* st = d.stats + (size_t)b * NCOL;
        st[ABC_AROM_STATUS] = status;
        st[ABC_AROM_CANDIDATES] = tally[0], st[ABC_AROM_CYCLES] = tally[1], st[ABC_AROM_AROMATIC] = tally[2];
        st[ABC_AROM_ROWS_CHANGED] = tally[3], st[ABC_AROM_LISTED] = added;
    }
}

}  // namespace

extern "C" int abc_aromatic_desc_size(void) { return (int)sizeof(abc_aromatic_desc); }

extern "C" int abc_perceive_aromatic(const abc_aromatic_desc* d, abc_stream_t stream) {
    const char* const entry = "perceive_aromatic";
    bool mol;
    if (const int rc = abc_one_side(entry, d, mol)) return rc;
    if (!d->stats) return abc_fail(ABC_EINVAL, "perceive_aromatic: null output (stats)");
    const int rows_given = (d->out_counts != nullptr) + (d->out_atoms != nullptr) + (d->out_bonds != nullptr) + (d->out_implh != nullptr);
    if (const int rc = abc_one_side_buffers(entry, d, mol)) return rc;
    if (mol && (rows_given != 4 || d->out_rec_bonds))
        return abc_fail(ABC_EINVAL, "perceive_aromatic: the molecule side writes out_counts, out_atoms, out_bonds and out_implh, all four");
    if (!mol && (rows_given != 0 || !d->out_rec_bonds)) return abc_fail(ABC_EINVAL, "perceive_aromatic: the records side writes out_rec_bonds alone");
    if (const int rc = abc_one_side_capacities(entry, d, mol)) return rc;
    const size_t B = (size_t)d->B, cap = (size_t)(mol ? d->cap_atoms : d->max_atoms), cb = (size_t)(mol ? d->cap_mol_bonds : d->max_bonds);
    const abc_extent out[7] = {{d->stats, B * NCOL * 4}, {d->code_out, B * cap * 4}, {d->out_counts, B * 16}, {d->out_atoms, B * cap * ATOM_W * 4},
                               {d->out_bonds, B * cb * MOL_BOND_W * 4}, {d->out_implh, B * cap * 4}, {d->out_rec_bonds, B * cb * REC_BOND_W * 4}};
    if (const int rc = abc_one_side_overlap(entry, d, mol, out)) return rc;
    hipLaunchKernelGGL(aromatic_kernel, dim3(d->B), dim3(GT), 0, (hipStream_t)stream, *d);
    return abc_check_launch(entry);
}
