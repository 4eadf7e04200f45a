// The stereo elements of every assembled molecule, perceived as a stage of its own: what the two stereo rules of the SMILES writer
// decide (smiles.hip: the tetrahedral rule of abc_write_smiles_stereo, the double-bond rule of abc_write_smiles_ez), written as an
// ELEMENT TABLE per image that the canonical search reads (graph_canon.hip, abc_canonical_order_stereo).  The contract is in
// include/abcnet_hip.h (abc_stereo_desc) and DESIGN.md section 7, the host form decode.stereo_elements.  Integers only.
//
// One workgroup per image, the molecule side only; the rows are read in place, nothing but the table and the stats row is written.
//   1  validate every row as the writer does; count degrees by LDS atomics, scan them, fill a CSR adjacency of (neighbour << 3 | class)
//   2  order every atom's list by neighbour index; equal neighbours side by side are a pair listed twice (BAD_ROW)
//   3  per atom: the hydrogen count (text_hydrogens.hpp), the centre's code from its wedge slots and an int64 determinant, whether it may
//      be an end of a candidate double bond; then one thread per candidate: twin, the sides of its substituents, its code
//   4  ONE lane walks every component depth first with a lowpoint per atom: a candidate whose bond is no bridge is RING.  (A bridge is
//      a property of the graph: the walk need not be the writer's.)
//   5  the table, every word of the image's cap_atoms rows
// Both rules are the writer's, from the one header both files include (stereo_rules.hpp: the codes, the rank sort, stereo_code,
// possible_end, ez_classify, is_bridge), so a rule changes in one place.  Written here again, as that header explains, are the row
// checks and the fill of step 1, the duplicate test of step 2 and the slot loop of step 3; its own are the LDS struct, the walk of
// step 4, the tally (three columns, FLAT of both kinds in one), the exits without elements and the table.  tests/
// test_gpu_stereo_perceive.py holds the two kernels to one answer on every case of both rules.  Every index read from a row is
// range-checked before it addresses anything.
#include "common.hpp"
#include "../../include/abcnet_hip.h"
#include "capi_util.hpp"
#include "block_scan.hpp"
#include "mol_rows.hpp"
#include "graph_ids.hpp"
#include "text_hydrogens.hpp"
#include "stereo_rules.hpp"      // ST, MAX_ATOMS, MAX_BONDS, the codes, the rank sort and both stereo rules: shared with smiles.hip

namespace {

constexpr int W = ABC_STEREO_W;
static_assert(W == 12, "the layout of mol_rows.hpp");

struct Lists {
    unsigned short adj[2][MAX_SLOTS];      // [0]: the lists as filled; [1]: ordered by neighbour index
    int deg[MAX_ATOMS];                    // degree, then the fill cursor
    unsigned short start[MAX_ATOMS + 1];
    short rank[MAX_ATOMS], parent[MAX_ATOMS], low[MAX_ATOMS];
    unsigned short cursor[MAX_ATOMS];
    short partner[MAX_ATOMS];              // the other end of this atom's one class-2 bond if the atom may be an end, else -1
    short row_of[MAX_ATOMS];               // the bond row of the candidate this atom is the lower end of
    unsigned char sym[MAX_ATOMS], listed[MAX_ATOMS];
    signed char charge[MAX_ATOMS], centre[MAX_ATOMS], code[MAX_ATOMS];
};

// an image without elements (EMPTY, refused): every row of the table is "none"
__device__ inline void none_row(int* el) {
#pragma unroll
    for (int k = 0; k < W; ++k) el[k] = k == 0 || k == 5 ? 0 : -1;
}
__device__ inline void no_elements(const abc_stereo_desc& d, int b, int tid, int status) {
    int* el = d.elements + (size_t)b * d.cap_atoms * W;
    for (int i = tid; i < d.cap_atoms; i += ST) none_row(el + i * W);
    if (tid < 4) d.stats[(size_t)b * 4 + tid] = tid == 3 ? status : 0;
}

__global__ __launch_bounds__(ST) void stereo_perceive_kernel(const abc_stereo_desc d) {
    __shared__ Lists w;
    __shared__ unsigned wt[ST / 64 + 1];
    __shared__ int refused;
    __shared__ int tally[3];               // marked centres, marked double bonds, flat (both kinds)
    const int b = blockIdx.x, tid = threadIdx.x;
    const MolCounts c = mol_counts_row(d, b);
    const int na = c.na, nb = c.nb, slots = 2 * nb;
    if ((c.status & ABC_MOL_EMPTY) || na == 0) {      // (uniform.  Bonds without an atom cannot be: their ends are outside 1..0)
        no_elements(d, b, tid, c.status | ((c.status & ABC_MOL_EMPTY) || nb == 0 ? 0 : ABC_TEXT_BAD_ROW));
        return;
    }
    const int* pa = d.mol_atoms + (size_t)b * d.cap_atoms * ATOM_W;
    const int* pb = d.mol_bonds + (size_t)b * d.cap_mol_bonds * MOL_BOND_W;
    const int* ph = d.mol_implh + (size_t)b * d.cap_atoms;

    // ---- 1: rows
    if (tid == 0) refused = 0;
    if (tid < 3) tally[tid] = 0;
    for (int i = tid; i < na; i += ST) {
        w.deg[i] = 0;
        w.rank[i] = w.parent[i] = w.row_of[i] = -1;
        w.listed[i] = 0;
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
        if (a >= 1 && a <= na) w.listed[a - 1] = 1;
    }
    if (bad) atomicOr(&refused, 1);
    __syncthreads();
    if (refused) {                         // (uniform: read behind the barrier)
        no_elements(d, b, tid, c.status | ABC_TEXT_BAD_ROW);
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
        // a wedge speaks for its end 1 alone: that end's slot keeps the order, 5 or 6, in the three class bits until step 3
        w.adj[0][w.start[e1] + atomicAdd(&w.deg[e1], 1)] = (unsigned short)(e2 << 3 | (order >= 5 ? order : cls));
        w.adj[0][w.start[e2] + atomicAdd(&w.deg[e2], 1)] = (unsigned short)(e1 << 3 | cls);
    }
    __syncthreads();

    // ---- 2: by neighbour index (into adj[1]); a pair listed twice
    order_lists<false>(w, na, slots, 0, tid);
    __syncthreads();
    bad = false;
    for (int i = tid; i < na; i += ST)
        for (int s = w.start[i] + 1, hi = w.start[i + 1]; s < hi; ++s) bad |= w.adj[1][s] >> 3 == w.adj[1][s - 1] >> 3;
    if (bad) atomicOr(&refused, 1);

    // ---- 3: the centres, the possible ends
    for (int i = tid; i < na; i += ST) {
        int s2 = 0, doubles = 0, others = 0, partner = -1;
        unsigned zbits = 0;
        const int lo = w.start[i], deg = w.start[i + 1] - lo;
        for (int s = lo, hi = lo + deg; s < hi; ++s) {
            int cls = w.adj[1][s] & 7;
            if (cls >= 5) {                // this atom's own wedge: from here on a class-1 slot (no other thread reads this list now)
                if (s - lo < 4) zbits |= (unsigned)(cls - 4) << (2 * (s - lo));
                zbits |= 1u << 8;
                cls = 1;
                w.adj[1][s] = (unsigned short)((w.adj[1][s] & ~7) | 1);
            }
            s2 += bond_s2(cls);
            if (cls == 2) ++doubles, partner = w.adj[1][s] >> 3;
            else others |= cls != 1;
        }
        w.partner[i] = (short)possible_end(w, i, deg, doubles, others, partner);
        w.code[i] = EZ_NONE;
        w.cursor[i] = w.start[i];
        int code = ST_NONE;
        if (zbits) {
            const int h = w.listed[i] ? 1 : hydrogens(w.sym[i], w.charge[i], s2);
            code = stereo_code(w, pa, i, lo, deg, zbits & 0xFFu, s2 == 2 * deg, h);
            if (code != ST_UNQUALIFIED) atomicAdd(&tally[code == ST_FLAT ? 2 : 0], 1);
        }
        w.centre[i] = (signed char)code;
    }
    __syncthreads();
    if (refused) {
        no_elements(d, b, tid, c.status | ABC_TEXT_BAD_ROW);
        return;
    }
    for (int i = tid; i < na; i += ST) {   // one thread per candidate, the one of its lower end (it alone writes both ends)
        const int j = w.partner[i];
        if (j > i && w.partner[j] == i) ez_classify<false>(w, w, pa, i, j);      // (the code alone, at both ends)
    }

    // ---- 4: the bridges
    if (tid == 0) {
        int next = 0, steps = slots + 2 * na;      // (every slot is passed once, every atom is left once)
        for (int root = 0; root < na; ++root) {
            if (w.rank[root] >= 0) continue;
            w.rank[root] = w.low[root] = (short)next++;
            int cur = root;
            while (cur >= 0 && steps-- > 0) {
                const int at = w.cursor[cur], par = w.parent[cur];
                if (at == w.start[cur + 1]) {
                    if (par >= 0) w.low[par] = min(w.low[par], w.low[cur]);
                    cur = par;
                    continue;
                }
                w.cursor[cur] = (unsigned short)(at + 1);
                const int y = w.adj[1][at] >> 3;
                if (w.rank[y] >= 0) {              // the parent, or the other end of a ring bond
                    if (y != par) w.low[cur] = min(w.low[cur], w.rank[y]);
                    continue;
                }
                w.parent[y] = (short)cur;
                w.rank[y] = w.low[y] = (short)next++;
                cur = y;
            }
        }
    }
    __syncthreads();
    for (int i = tid; i < na; i += ST) {   // a candidate that is no bridge is RING, whatever else it is; the counters
        const int j = w.partner[i];
        if (j <= i || w.code[i] == EZ_NONE) continue;      // (a code: the two ends name each other)
        int code = w.code[i];
        if (!is_bridge(w, w.low, i, j)) w.code[i] = w.code[j] = (signed char)(code = EZ_RING);
        if (code == 1 || code == -1) atomicAdd(&tally[1], 1);
        if (code == EZ_FLAT) atomicAdd(&tally[2], 1);
    }
    for (int q = tid; q < nb; q += ST) {   // the row of every candidate, kept at its lower end (pairs are unique: one writer)
        int e1, e2;
        if (mol_ends(pb, q, na, e1, e2) && bond_class(pb[q * MOL_BOND_W + 2]) == 2 && w.partner[e1] == e2 && w.partner[e2] == e1)
            w.row_of[min(e1, e2)] = (short)q;
    }
    __syncthreads();

    // ---- 5: the table
    int* const el = d.elements + (size_t)b * d.cap_atoms * W;
    for (int i = tid; i < d.cap_atoms; i += ST) {
        int* r = el + i * W;
        none_row(r);
        if (i >= na) continue;
        const int centre = w.centre[i], lo = w.start[i], deg = w.start[i + 1] - lo;
        r[0] = centre;
        if (centre == 1 || centre == -1)
            for (int k = 0; k < deg && k < 4; ++k) r[1 + k] = w.adj[1][lo + k] >> 3;      // (deg 3: the hydrogen, -1, stays last)
        const int j = w.partner[i], q = w.row_of[i];
        if (q < 0 || j <= i) continue;
        const int code = w.code[i];
        r[5] = code;
        if (code != 1 && code != -1) continue;
        int sa[2], sb[2], ca = 0, cb = 0;      // (the counts are not needed: -1 stands where there is none)
        substituents(w, i, j, -1, sa, ca);
        substituents(w, j, i, -1, sb, cb);
        r[6] = q, r[7] = j, r[8] = sa[0], r[9] = sa[1], r[10] = sb[0], r[11] = sb[1];
    }
    if (tid < 4) d.stats[(size_t)b * 4 + tid] = tid == 3 ? c.status : tally[tid];
}

}  // namespace

extern "C" int abc_stereo_desc_size(void) { return (int)sizeof(abc_stereo_desc); }

extern "C" int abc_perceive_stereo(const abc_stereo_desc* d, abc_stream_t stream) {
    const char* const entry = "perceive_stereo";
    if (!d) return abc_fail_in(ABC_EINVAL, entry, "null descriptor");
    if (d->B < 1) return abc_fail_in(ABC_EINVAL, entry, "empty");
    if (d->cap_atoms < 1 || d->cap_mol_bonds < 1) return abc_fail_in(ABC_EINVAL, entry, "cap_atoms and cap_mol_bonds must be >= 1");
    if (d->cap_atoms > MAX_ATOMS) return abc_fail_in(ABC_EUNSUPPORTED, entry, "cap_atoms must be <= 512 (ABC_MAX_SMILES_ATOMS)");
    if (d->cap_mol_bonds > MAX_BONDS) return abc_fail_in(ABC_EUNSUPPORTED, entry, "cap_mol_bonds must be <= 4096");
    if (!d->mol_counts || !d->mol_atoms || !d->mol_bonds || !d->mol_implh) return abc_fail_in(ABC_EINVAL, entry, "null molecule buffer");
    if (!d->elements || !d->stats) return abc_fail_in(ABC_EINVAL, entry, "null output (elements, stats)");
    hipLaunchKernelGGL(stereo_perceive_kernel, dim3(d->B), dim3(ST), 0, (hipStream_t)stream, *d);
    return abc_check_launch(entry);
}
