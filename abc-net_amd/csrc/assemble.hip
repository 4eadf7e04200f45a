// Graph assembly for the SMILES decoder: img2smiles2.py:193-311 on the device.
//
// Input: the ordered candidate lists extract.hip leaves (read in place).  Output: the molecule the reference hands to its
// mol-block writer -- atoms (position, repaired type, charge, hs) numbered from 1, bonds (end 1, end 2, order) and the
// implicit-hydrogen list.  One workgroup per image; the reference's sequential loops become order-preserving parallel forms:
//
//   (A) atoms into LDS, the image's pair table cleared
//   (B) one THREAD per candidate, a loop over the accepted atoms (positions are LDS broadcasts): the two arg-mins of :204-210
//       with a strict `<` in atom order, so the first minimum wins as in np.argmin.  (A wave per candidate with lanes over the
//       atoms needs a cross-lane (value, index) reduction and repeats the candidate's division and square root in 64 lanes; with
//       the tens of atoms of a drawing the thread form does less work and needs no reduction.)  A candidate whose ends differ
//       lowers the pair table's entry of its unordered atom pair to its own index (integer atomicMin in an open-addressing table).
//   (C) the candidates whose index IS their pair's entry are the reference's kept bonds (:217-234: "first of each pair, list order");
//       ordered compaction by block scans; valence counts and the touched flags by integer LDS atomics
//   (D) valence repair (:247-271)   (E) atom compaction and numbering (:273-287)
//   (F) first appearance of every atom at an aromatic bond (integer atomicMin)   (G) bond renumbering (:291-297) and the
//       implicit-hydrogen list (:299-311) in order of first appearance, again by block scans
//
// The decisions of (B) are float64 comparisons with near-ties as the normal case (atoms sit on an integer grid): every multiply,
// add, divide and square root below is rounded on its own, in the reference's order.  The file is compiled without contraction
// (a fused multiply-add in a distance moves arg-mins); cos / sin come from a table the host computed with numpy.
#include "common.hpp"
#include "../../include/abcnet_hip.h"
#include "capi_util.hpp"
#include "block_scan.hpp"
#include "mol_rows.hpp"

#include <climits>

namespace {

constexpr int AT = 1024;            // threads per workgroup
constexpr int MAX_ATOMS = ABC_MAX_CAP_ATOMS;
constexpr int EXTRACT_MAX_BPEAKS = ABC_MAX_BOND_PEAKS;      // (more: the extractor's lists are truncated)
static_assert(MAX_ATOMS <= 1 << 11, "an atom index fits the 11 bits of a pair key");
constexpr int MAX_CAP_BONDS = 1 << 24;

// img2smiles2.py:32-34 restricted to the vocabulary of utils.py:12-13 (index 0 decodes to 'C', img2smiles2.py:25)
//                                  ?  C  N  O  P  F  Cl S  Br B  Se I  H  Si
__constant__ int MAX_VALENCE[N_SYMBOLS] = {4, 4, 3, 2, 5, 1, 1, 6, 1, 3, 6, 1, 1, 4};
//                               count: 2 -> O, 3 -> N, 4 -> C, 5 -> P, 6 -> S, 7 -> Cl   (vocabulary indices)
__constant__ int REPAIR_TYPE[8] = {0, 0, 3, 2, 1, 4, 7, 6};

// slots of an open-addressing table that holds `distinct` keys at a load of at most 1/2 (a power of two, >= 2)
__host__ __device__ inline int table_slots(long long distinct) {
    int h = 2;
    while ((long long)h < 2 * distinct) h <<= 1;
    return h;
}
// distinct unordered atom pairs `bonds` candidates over `atoms` atoms can name
__host__ __device__ inline long long max_pairs(long long atoms, long long bonds) {
    const long long p = atoms * (atoms - 1) / 2;
    return p < bonds ? p : bonds;
}

__device__ inline int load_relaxed(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__device__ inline unsigned slot_of(int key, int mask) {
    unsigned h = (unsigned)key * 0x9E3779B1u;
    return (h ^ (h >> 15)) & (unsigned)mask;
}

__global__ __launch_bounds__(AT) void assemble_kernel(const abc_assemble_desc d, int slots_max) {
#pragma clang fp contract(off)
    __shared__ double2 apos[MAX_ATOMS];   // accepted atoms (x, y) as float64
    __shared__ int ainfo[MAX_ATOMS];      // vocabulary index | (hs != 0) << 8
    __shared__ int acount[MAX_ATOMS];     // valence count (C, D), then first appearance at an aromatic bond (F, G)
    __shared__ int anew[MAX_ATOMS];       // touched flag (C), then the 1-based final index (E)
    __shared__ double trig[120];
    __shared__ unsigned wt[AT / 64 + 1];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int* cin = d.counts + (size_t)b * 4;
    const int c0 = cin[0], c1 = cin[1], c2 = cin[2], c3 = cin[3];
    int status = (c0 > d.cap_atoms || c1 > d.cap_atoms || c2 > EXTRACT_MAX_BPEAKS || c3 > d.cap_bonds) ? ABC_MOL_TRUNCATED : 0;
    int* mc = d.mol_counts + (size_t)b * 4;
    if (c0 <= 0 || c2 <= 0) {             // img2smiles2.py:126-129
        if (tid == 0) { mc[0] = 0; mc[1] = 0; mc[2] = 0; mc[3] = status | ABC_MOL_EMPTY; }
        return;
    }
    const int na = max(min(c1, d.cap_atoms), 0), nc = max(min(c3, d.cap_bonds), 0);
    const int* atoms = d.atoms + (size_t)b * d.cap_atoms * ATOM_W;
    const int* bonds = d.bonds + (size_t)b * d.cap_bonds * CAND_W;
    const float* rhos = d.bond_rho + (size_t)b * d.cap_bonds;
    int* pair = d.work + (size_t)b * ((size_t)d.cap_bonds + 2 * (size_t)slots_max);   // per candidate: end 1 << 16 | end 2, or -1
    int* keys = pair + d.cap_bonds;       // pair table: key = lower end << 11 | higher end, -1 = free
    int* first = keys + slots_max;        //             the lowest candidate index that named the pair
    const int slots = table_slots(max_pairs(na, nc)), mask = slots - 1;      // (<= slots_max: na <= cap_atoms, nc <= cap_bonds)

    // ---- (A)
    for (int a = tid; a < na; a += AT) {
        const int* r = atoms + (size_t)a * ATOM_W;
        apos[a] = make_double2((double)r[0], (double)r[1]);
        ainfo[a] = (r[2] & 0xFF) | (r[4] != 0 ? 0x100 : 0);
        acount[a] = r[3] == 1 ? -1 : (r[3] == 2 ? 1 : 0);        // -charge (charge_vocab: 0 -> 0, 1 -> +1, 2 -> -1)
        anew[a] = 0;
    }
    if (tid < 120) trig[tid] = d.trig[tid];
    for (int s = tid; s < slots; s += AT) {
        __hip_atomic_store(keys + s, -1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(first + s, INT_MAX, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __syncthreads();

    // ---- (B) bond ends (:193-210) and the pair table
    for (int i = tid; i < nc; i += AT) {
        const int* c = bonds + (size_t)i * CAND_W;
        const int k = c[2];
        const double rho = (double)rhos[i];
        int pr = -1;
        // rho == 0 gives 0 / 0 in the reference: NaN rows, both arg-mins 0, the candidate dropped (the same for a rho that is not finite)
        if (na > 0 && k >= 0 && k < 60 && rho > 0.0 && rho < __builtin_huge_val()) {
            const double dx = rho * trig[k], dy = rho * trig[60 + k];
            const double n = __dsqrt_rn(dx * dx + dy * dy);
            const double e1x = dx / n, e1y = dy / n;
            const double e2x = -e1y, e2y = e1x;
            const double p1x = (double)c[0] + dx, p1y = (double)c[1] + dy;
            const double p2x = (double)c[0] - dx, p2y = (double)c[1] - dy;
            double best1 = 0.0, best2 = 0.0;
            int i1 = 0, i2 = 0;
            for (int j = 0; j < na; ++j) {
                const double2 a = apos[j];
                const double u1 = p1x - a.x, v1 = p1y - a.y;
                const double s1 = u1 * e1x + v1 * e1y;
                const double dist1 = fabs(fmax(s1, 0.5 * s1)) + fabs((2.0 * u1) * e2x + (2.0 * v1) * e2y);
                const double u2 = p2x - a.x, v2 = p2y - a.y;
                const double s2 = -(u2 * e1x + v2 * e1y);
                const double dist2 = fabs(fmax(s2, 0.5 * s2)) + fabs((2.0 * u2) * e2x + (2.0 * v2) * e2y);
                if (j == 0 || dist1 < best1) { best1 = dist1; i2 = j; }     // atom_index2 = distance1.argmin
                if (j == 0 || dist2 < best2) { best2 = dist2; i1 = j; }     // atom_index1 = distance2.argmin
            }
            if (i1 != i2) {
                pr = (i1 << 16) | i2;
                const int key = (min(i1, i2) << 11) | max(i1, i2);
                unsigned s = slot_of(key, mask);
                for (int probe = 0; probe < slots; ++probe, s = (s + 1) & (unsigned)mask) {
                    const int prev = atomicCAS(keys + s, -1, key);
                    if (prev == -1 || prev == key) { atomicMin(first + s, i); break; }
                }
            }
        }
        pair[i] = pr;        // (read back by this very thread)
    }
    __syncthreads();

    // ---- (C) the first candidate of every pair, in list order (:212-234); valence counts (:247-255), touched atoms (:236-245)
    int* mb = d.mol_bonds + (size_t)b * d.cap_mol_bonds * MOL_BOND_W;
    int kept = 0;
    for (int base = 0; base < nc; base += AT) {
        const int i = base + tid;
        const int pr = i < nc ? pair[i] : -1;
        bool keep = false;
        if (pr >= 0) {
            const int i1 = pr >> 16, i2 = pr & 0xFFFF;
            const int key = (min(i1, i2) << 11) | max(i1, i2);
            unsigned s = slot_of(key, mask);
            for (int probe = 0; probe < slots; ++probe, s = (s + 1) & (unsigned)mask) {
                if (load_relaxed(keys + s) == key) { keep = load_relaxed(first + s) == i; break; }
            }
        }
        unsigned tot;
        const int pos = kept + (int)block_excl_scan<AT>(keep ? 1u : 0u, wt, &tot);
        if (keep && pos < d.cap_mol_bonds) {
            const int i1 = pr >> 16, i2 = pr & 0xFFFF;
            const int order = bonds[(size_t)i * CAND_W + 3] + 1;          // bond_type_devocab
            int* o = mb + (size_t)pos * MOL_BOND_W;
            o[0] = i1; o[1] = i2; o[2] = order; o[3] = i;             // (ends renumbered in (G))
            const int v = order >= 4 ? 1 : order;
            atomicAdd(acount + i1, v); atomicAdd(acount + i2, v);
            atomicOr(anew + i1, 1); atomicOr(anew + i2, 1);
        }
        kept += (int)tot;
    }
    if (kept > d.cap_mol_bonds) status |= ABC_MOL_TRUNCATED;
    const int nk = min(kept, d.cap_mol_bonds);
    __syncthreads();
    __threadfence_block();      // mol_bonds rows are read back by other threads of this workgroup below

    // ---- (D) valence repair (:256-271)
    for (int a = tid; a < na; a += AT) {
        const int count = acount[a], info = ainfo[a], type = info & 0xFF;
        const int maxv = type < N_SYMBOLS ? MAX_VALENCE[type] : 4;
        if (maxv < count && count >= 2 && count <= 7) ainfo[a] = (info & ~0xFF) | REPAIR_TYPE[count];
        acount[a] = INT_MAX;
    }
    // ---- (E) atoms some kept bond touches, numbered from 1 in list order (:273-287)
    int* ma = d.mol_atoms + (size_t)b * d.cap_atoms * ATOM_W;
    int natoms = 0;
    for (int base = 0; base < na; base += AT) {       // (the scan's barriers also order (D) before the reads of ainfo below)
        const int a = base + tid;
        const bool shown = a < na && anew[a] != 0;
        unsigned tot;
        const int idx = natoms + (int)block_excl_scan<AT>(shown ? 1u : 0u, wt, &tot);
        if (shown) {
            const int* r = atoms + (size_t)a * ATOM_W;
            int* o = ma + (size_t)idx * ATOM_W;
            o[0] = r[0]; o[1] = r[1]; o[2] = ainfo[a] & 0xFF; o[3] = r[3] == 1 ? 1 : (r[3] == 2 ? -1 : 0); o[4] = r[4];
            anew[a] = idx + 1;
        }
        natoms += (int)tot;
    }
    __syncthreads();

    // ---- (F) first appearance (bond position, end) of every hetero atom with hs != 0 at an aromatic bond (:299-311)
    for (int p = tid; p < nk; p += AT) {
        const int* o = mb + (size_t)p * MOL_BOND_W;
        if (o[2] != 4) continue;
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            const int a = o[e], info = ainfo[a];
            if ((info & 0xFF) > 1 && (info & 0x100)) atomicMin(acount + a, 2 * p + e);     // (vocabulary 0 and 1 are both 'C')
        }
    }
    __syncthreads();
    // ---- (G) bond ends renumbered (:291-297); the implicit-hydrogen list in order of first appearance
    int* mh = d.mol_implh + (size_t)b * d.cap_atoms;
    int nimpl = 0;
    for (int base = 0; base < nk; base += AT) {
        const int p = base + tid;
        int f0 = 0, f1 = 0, n0 = 0, n1 = 0;
        if (p < nk) {
            int* o = mb + (size_t)p * MOL_BOND_W;
            const int a0 = o[0], a1 = o[1];
            n0 = anew[a0]; n1 = anew[a1];
            if (o[2] == 4) { f0 = acount[a0] == 2 * p; f1 = acount[a1] == 2 * p + 1; }
            o[0] = n0; o[1] = n1;
        }
        unsigned tot;
        int at = nimpl + (int)block_excl_scan<AT>((unsigned)(f0 + f1), wt, &tot);
        if (f0) mh[at++] = n0;
        if (f1) mh[at] = n1;
        nimpl += (int)tot;
    }
    if (tid == 0) { mc[0] = natoms; mc[1] = nk; mc[2] = nimpl; mc[3] = status; }
}

}  // namespace

extern "C" int64_t abc_assemble_work_ints(const abc_assemble_desc* d) {
    if (d->B < 1 || d->cap_atoms < 1 || d->cap_atoms > MAX_ATOMS || d->cap_bonds < 1 || d->cap_bonds > MAX_CAP_BONDS) return 0;
    return (int64_t)d->B * ((int64_t)d->cap_bonds + 2 * (int64_t)table_slots(max_pairs(d->cap_atoms, d->cap_bonds)));
}

extern "C" int abc_assemble_graphs(const abc_assemble_desc* d, abc_stream_t stream) {
    if (d->B < 1) return abc_fail(ABC_EINVAL, "assemble: empty");
    if (d->cap_atoms < 1 || d->cap_atoms > MAX_ATOMS) return abc_fail(ABC_EINVAL, "assemble: cap_atoms must be 1..2048");
    if (d->cap_bonds < 1 || d->cap_bonds > MAX_CAP_BONDS) return abc_fail(ABC_EINVAL, "assemble: cap_bonds must be 1..2^24");
    if (d->cap_mol_bonds < 1) return abc_fail(ABC_EINVAL, "assemble: cap_mol_bonds must be >= 1");
    if (!d->trig) return abc_fail(ABC_EINVAL, "assemble: null cos / sin table");
    if (!d->counts || !d->atoms || !d->bonds || !d->bond_rho || !d->mol_counts || !d->mol_atoms || !d->mol_bonds || !d->mol_implh || !d->work)
        return abc_fail(ABC_EINVAL, "assemble: null buffer");
    const int slots_max = table_slots(max_pairs(d->cap_atoms, d->cap_bonds));
    hipLaunchKernelGGL(assemble_kernel, dim3(d->B), dim3(AT), 0, (hipStream_t)stream, *d, slots_max);
    return abc_check_launch("assemble_graphs");
}
