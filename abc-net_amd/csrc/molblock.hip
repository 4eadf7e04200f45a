// The V2000 mol block of every assembled molecule (generate_smiles.py:18-105; decode.Molecule.molblock() is the host form and the
// oracle), written on the device from the rows of abc_assemble_graphs, read in place.  The contract -- byte rule, statuses, prefix
// rule -- is in include/abcnet_hip.h and DESIGN.md section 7.
//
// The text of an image is a sequence of ITEMS whose lengths depend on their rows alone:
//   head    "\n     RDKit\n\n" and the counts line                                    (thread 0)
//   atoms   one line per atom row: two coordinates, the symbol, the fixed tail
//   bonds   one line per bond row: four numbers
//   CHG     "M  CHG" and the count (thread 0), one "%4d%4d" entry per atom row with a charge, the line end
//   implicit H (only with entries): the STY and the SLB line, whose entry k depends on k alone -- its offset is a closed form of
//           the digit counts of 1 .. k -- then four lines per entry
//   end     "M  END\n$$$$"
// Integers only; no floating point runs here (the coordinate rule is coord_q below).
//
//   molblock_size_kernel   one workgroup per image: every thread adds up the lengths of its items, one workgroup sum -> lens[b]
//                          (-1: a row the writer refuses)
//   molblock_write_kernel  one workgroup per image: the running totals of lens[0 .. b] by a 64-bit workgroup scan (the prefix rule of
//                          text_pack.hpp needs the largest total that still fits), then per item class every thread takes a CONTIGUOUS range of
//                          rows, a workgroup scan of the ranges' lengths gives its first byte, and it writes its rows one after
//                          the other
// Both kernels compute lengths with the same functions the writer advances by (every put_* returns the position after it), and
// every byte store is checked against the end of the image's own text: a store can never leave text[offsets[b] .. offsets[b+1]).
#include "common.hpp"
#include "../../include/abcnet_hip.h"
#include "capi_util.hpp"
#include "block_scan.hpp"
#include "mol_rows.hpp"
#include "text_pack.hpp"

namespace {

typedef unsigned long long u64;

constexpr int MT = 256;                  // threads per workgroup

// utils.py:12-13 inverted, index 0 decoded as carbon (decode.ATOM_SYMBOLS), each padded to the 4 columns of the atom line
__device__ const char SYMBOLS[N_SYMBOLS * 4 + 1] = "C   C   N   O   P   F   Cl  S   Br  B   Se  I   H   Si  ";

#define LIT_LEN(s) ((int)sizeof(s) - 1)
#define HEAD_TEXT "\n     RDKit\n\n"
#define COUNTS_TAIL "  0  0  0  0  0  0  0  0999 V2000\n"
#define ATOM_Z "    0.0000 "
#define ATOM_TAIL "0  0  0  0  0  0  0  0  0  0  0  0\n"
#define CHG_HEAD "M  CHG"
#define STY_HEAD "M  STY  "
#define SLB_HEAD "M  SLB  "
#define SAL_HEAD "M  SAL   "
#define SAL_MID "  1  "
#define SAL_TAIL "  \n"
#define SDT_HEAD "M  SDT   "
#define SDT_TAIL " MRV_IMPLICIT_H    \n"
#define SDD_HEAD "M  SDD   "
#define SDD_TAIL "     0.0000    0.0000    DA    ALL  1       1    \n"
#define SED_HEAD "M  SED   "
#define SED_TAIL " IMPL_H1\n"
#define END_TEXT "M  END\n$$$$"

// decimal digits of u
__device__ inline int ndig(unsigned u) {
    int n = 1;
    if (u >= 10u) n = 2;
    if (u >= 100u) n = 3;
    if (u >= 1000u) n = 4;
    if (u >= 10000u) n = 5;
    if (u >= 100000u) n = 6;
    if (u >= 1000000u) n = 7;
    if (u >= 10000000u) n = 8;
    if (u >= 100000000u) n = 9;
    if (u >= 1000000000u) n = 10;
    return n;
}
__device__ inline unsigned absu(int v) { return v < 0 ? 0u - (unsigned)v : (unsigned)v; }
// the length of "%<w>d" % v: w is a MINIMUM width
__device__ inline int int_len(int v, int w) { return max(ndig(absu(v)) + (v < 0), w); }
// ndig(1) + ... + ndig(k), k >= 0
__device__ inline int digits_upto(int k) {
    const int n = ndig((unsigned)k);
    int ones = 0;      // 1, 11, 111, ...: (10^n - 1) / 9
    for (int i = 0; i < n; ++i) ones = ones * 10 + 1;
    return (k + 1) * n - ones;
}

// the text of one image: every store is bounds-checked against the image's end
struct Out {
    uint8_t* text;
    int64_t end;
    __device__ inline void put(int64_t pos, int c) const { if (pos < end) text[pos] = (uint8_t)c; }
};

template <int N>
__device__ inline int64_t put_lit(const Out& o, int64_t pos, const char (&s)[N]) {
#pragma unroll
    for (int i = 0; i < N - 1; ++i) o.put(pos + i, s[i]);
    return pos + (N - 1);
}
__device__ inline int64_t put_digits(const Out& o, int64_t pos, unsigned u, int n) {      // exactly n digits, zero-padded
    for (int i = n - 1; i >= 0; --i) {
        o.put(pos + i, '0' + (int)(u % 10u));
        u /= 10u;
    }
    return pos + n;
}
__device__ inline int64_t put_int(const Out& o, int64_t pos, int v, int w) {              // "%<w>d"
    const unsigned u = absu(v);
    const int n = ndig(u), len = n + (v < 0);
    for (int i = len; i < w; ++i) o.put(pos++, ' ');
    if (v < 0) o.put(pos++, '-');
    return put_digits(o, pos, u, n);
}

// px / 60 - 1 to four decimals: q = round(|px - 60| * 10000 / 60) = floor((2 a + 3) / 6), a = |px - 60| * 500 (a third never
// lands on a half, so there is no tie); negative exactly when px < 60
__device__ inline unsigned coord_q(int px) { return (2u * (absu(px - 60) * 500u) + 3u) / 6u; }
// a negative value follows three blanks, any other four: either way 4 + the digits of the integer part + ".dddd"
__device__ inline int coord_len(int px) { return 4 + ndig(coord_q(px) / 10000u) + 5; }
__device__ inline int64_t put_coord(const Out& o, int64_t pos, int px) {
    const unsigned q = coord_q(px), ip = q / 10000u;
    o.put(pos, ' '); o.put(pos + 1, ' '); o.put(pos + 2, ' '); o.put(pos + 3, px < 60 ? '-' : ' ');
    pos = put_digits(o, pos + 4, ip, ndig(ip));
    o.put(pos, '.');
    return put_digits(o, pos + 1, q % 10000u, 4);
}

__device__ inline bool atom_ok(const int* a) {
    return a[0] >= 0 && a[0] <= MAX_POSITION && a[1] >= 0 && a[1] <= MAX_POSITION && a[2] >= 0 && a[2] < N_SYMBOLS;
}
__device__ inline int atom_len(const int* a) { return coord_len(a[0]) + coord_len(a[1]) + LIT_LEN(ATOM_Z) + 4 + LIT_LEN(ATOM_TAIL); }
__device__ inline int64_t put_atom(const Out& o, int64_t pos, const int* a) {
    pos = put_coord(o, pos, a[0]);
    pos = put_coord(o, pos, a[1]);
    pos = put_lit(o, pos, ATOM_Z);
    const int t = clampi(a[2], 0, N_SYMBOLS - 1);      // (atom_ok has refused the image otherwise)
#pragma unroll
    for (int i = 0; i < 4; ++i) o.put(pos + i, SYMBOLS[t * 4 + i]);
    return put_lit(o, pos + 4, ATOM_TAIL);
}

// order <= 4: (order, 0); 5: (1, 1); anything else: (1, 6)
__device__ inline void bond_kind(int order, int& kind, int& stereo) {
    kind = order <= 4 ? order : 1;
    stereo = order <= 4 ? 0 : (order == 5 ? 1 : 6);
}
__device__ inline int bond_len(const int* r) {
    int kind, stereo;
    bond_kind(r[2], kind, stereo);
    return int_len(r[0], 3) + int_len(r[1], 3) + int_len(kind, 3) + int_len(stereo, 3) + 1;
}
__device__ inline int64_t put_bond(const Out& o, int64_t pos, const int* r) {
    int kind, stereo;
    bond_kind(r[2], kind, stereo);
    pos = put_int(o, pos, r[0], 3);
    pos = put_int(o, pos, r[1], 3);
    pos = put_int(o, pos, kind, 3);
    pos = put_int(o, pos, stereo, 3);
    o.put(pos, '\n');
    return pos + 1;
}

// the "%4d%4d" entry of atom i (0-based) on the charge line: nothing for a charge of 0
__device__ inline int chg_len(int i, int c) { return c != 0 ? int_len(i + 1, 4) + int_len(c, 4) : 0; }
__device__ inline int64_t put_chg(const Out& o, int64_t pos, int i, int c) {
    if (c == 0) return pos;
    pos = put_int(o, pos, i + 1, 4);
    return put_int(o, pos, c, 4);
}

// the four lines of implicit-H entry k (0-based) naming atom a
__device__ inline int implh_len(int k, int a) {
    return 4 * ndig((unsigned)(k + 1)) + int_len(a, 0) + LIT_LEN(SAL_HEAD) + LIT_LEN(SAL_MID) + LIT_LEN(SAL_TAIL) + LIT_LEN(SDT_HEAD)
           + LIT_LEN(SDT_TAIL) + LIT_LEN(SDD_HEAD) + LIT_LEN(SDD_TAIL) + LIT_LEN(SED_HEAD) + LIT_LEN(SED_TAIL);
}
__device__ inline int64_t put_implh(const Out& o, int64_t pos, int k, int a) {
    pos = put_lit(o, pos, SAL_HEAD); pos = put_int(o, pos, k + 1, 0); pos = put_lit(o, pos, SAL_MID);
    pos = put_int(o, pos, a, 0); pos = put_lit(o, pos, SAL_TAIL);
    pos = put_lit(o, pos, SDT_HEAD); pos = put_int(o, pos, k + 1, 0); pos = put_lit(o, pos, SDT_TAIL);
    pos = put_lit(o, pos, SDD_HEAD); pos = put_int(o, pos, k + 1, 0); pos = put_lit(o, pos, SDD_TAIL);
    pos = put_lit(o, pos, SED_HEAD); pos = put_int(o, pos, k + 1, 0); return put_lit(o, pos, SED_TAIL);
}
// "M  STY  %d" + "   %d DAT" * n + "\n" and "M  SLB  %d" + "   %d   %d" * n + "\n": entry k (0-based) of either starts a closed
// form behind the line's head
__device__ inline int sty_entry_off(int k) { return 7 * k + digits_upto(k); }
__device__ inline int slb_entry_off(int k) { return 6 * k + 2 * digits_upto(k); }
__device__ inline int sty_len(int n) { return LIT_LEN(STY_HEAD) + ndig((unsigned)n) + sty_entry_off(n) + 1; }
__device__ inline int slb_len(int n) { return LIT_LEN(SLB_HEAD) + ndig((unsigned)n) + slb_entry_off(n) + 1; }

__device__ inline int head_len(int na, int nb) { return LIT_LEN(HEAD_TEXT) + int_len(na, 3) + int_len(nb, 3) + LIT_LEN(COUNTS_TAIL); }

// rows [lo, hi) of thread tid when n rows are dealt out in contiguous ranges
__device__ inline void my_range(int n, int tid, int& lo, int& hi) { text_pack::my_range<MT>(n, tid, lo, hi); }

__global__ __launch_bounds__(MT) void molblock_size_kernel(const abc_molblock_desc d) {
    __shared__ unsigned wt[MT / 64 + 1];
    __shared__ int flags[2];             // charged atoms, a refused row
    const int b = blockIdx.x, tid = threadIdx.x;
    const MolCounts c = mol_counts_row(d, b);
    if (c.status & ABC_MOL_EMPTY) {
        if (tid == 0) d.work[b] = 0;
        return;
    }
    const int* pa = d.mol_atoms + (size_t)b * d.cap_atoms * ATOM_W;
    const int* pb = d.mol_bonds + (size_t)b * d.cap_mol_bonds * MOL_BOND_W;
    const int* ph = d.mol_implh + (size_t)b * d.cap_atoms;
    if (tid < 2) flags[tid] = 0;
    __syncthreads();
    unsigned len = 0;
    int charged = 0, bad = 0;
    for (int i = tid; i < c.na; i += MT) {
        const int* a = pa + i * ATOM_W;
        bad |= !atom_ok(a);
        len += atom_len(a) + chg_len(i, a[3]);
        charged += a[3] != 0;
    }
    for (int q = tid; q < c.nb; q += MT) len += bond_len(pb + q * MOL_BOND_W);
    for (int k = tid; k < c.nh; k += MT) len += implh_len(k, ph[k]);
    if (charged) atomicAdd(&flags[0], charged);
    if (bad) atomicOr(&flags[1], 1);
    unsigned total;
    block_excl_scan<MT>(len, wt, &total);      // (its barriers also publish flags)
    if (tid == 0) {
        total += head_len(c.na, c.nb) + LIT_LEN(CHG_HEAD) + int_len(flags[0], 3) + 1 + LIT_LEN(END_TEXT);
        if (c.nh > 0) total += sty_len(c.nh) + slb_len(c.nh);
        d.work[b] = flags[1] ? -1 : (int)total;
    }
}

__global__ __launch_bounds__(MT) void molblock_write_kernel(const abc_molblock_desc d) {
    __shared__ unsigned wt[MT / 64 + 1];
    __shared__ int charged_all;
    const int b = blockIdx.x, tid = threadIdx.x;
    int* offsets = d.index;
    int* status_out = d.index + d.B + 1;
    const MolCounts c = mol_counts_row(d, b);

    // ---- the prefix rule (text_pack.hpp): the running total in front of image b and through it, and the largest that still fits
    if (tid == 0) charged_all = 0;       // (published by the rule's barriers)
    const text_pack::Span span = text_pack::prefix_rule<MT>(d.work, b, d.cap_text);
    int lo, hi;
    const int my_len = d.work[b];
    const bool overflow = span.through > (u64)d.cap_text;
    const bool bad = my_len < 0;
    const bool written = !overflow && my_len > 0;
    if (tid == 0) {
        if (b == 0) offsets[0] = 0;
        offsets[b + 1] = (int)span.fits;      // (fits <= cap_text <= INT32_MAX; == through unless this image overflows)
        status_out[b] = c.status | (bad ? ABC_TEXT_BAD_ROW : 0) | (overflow ? ABC_TEXT_OVERFLOW : 0);
    }
    if (!written) return;                // (uniform over the workgroup)

    Out o;
    o.text = d.text;
    o.end = (int64_t)span.through;
    int64_t pos = (int64_t)span.before;
    const int* pa = d.mol_atoms + (size_t)b * d.cap_atoms * ATOM_W;
    const int* pb = d.mol_bonds + (size_t)b * d.cap_mol_bonds * MOL_BOND_W;
    const int* ph = d.mol_implh + (size_t)b * d.cap_atoms;
    unsigned total;

    // ---- head
    if (tid == 0) {
        int64_t p = put_lit(o, pos, HEAD_TEXT);
        p = put_int(o, p, c.na, 3);
        p = put_int(o, p, c.nb, 3);
        put_lit(o, p, COUNTS_TAIL);
    }
    pos += head_len(c.na, c.nb);

    // ---- atom lines (and this thread's share of the charge line, for the scan after the next)
    my_range(c.na, tid, lo, hi);
    unsigned len = 0, chg = 0;
    int charged = 0;
    for (int i = lo; i < hi; ++i) {
        const int* a = pa + i * ATOM_W;
        len += atom_len(a);
        chg += chg_len(i, a[3]);
        charged += a[3] != 0;
    }
    if (charged) atomicAdd(&charged_all, charged);
    {
        int64_t p = pos + block_excl_scan<MT>(len, wt, &total);
        for (int i = lo; i < hi; ++i) p = put_atom(o, p, pa + i * ATOM_W);
    }
    pos += total;

    // ---- bond lines
    {
        int blo, bhi;
        my_range(c.nb, tid, blo, bhi);
        len = 0;
        for (int q = blo; q < bhi; ++q) len += bond_len(pb + q * MOL_BOND_W);
        int64_t p = pos + block_excl_scan<MT>(len, wt, &total);
        for (int q = blo; q < bhi; ++q) p = put_bond(o, p, pb + q * MOL_BOND_W);
        pos += total;
    }

    // ---- the charge line (charged_all: every add came before the barriers of the two scans above)
    {
        const int n_chg = charged_all;
        if (tid == 0) put_int(o, put_lit(o, pos, CHG_HEAD), n_chg, 3);
        pos += LIT_LEN(CHG_HEAD) + int_len(n_chg, 3);
        int64_t p = pos + block_excl_scan<MT>(chg, wt, &total);
        for (int i = lo; i < hi; ++i) p = put_chg(o, p, i, pa[i * ATOM_W + 3]);
        pos += total;
        if (tid == 0) o.put(pos, '\n');
        pos += 1;
    }

    // ---- the implicit-H block
    if (c.nh > 0) {
        const int n = c.nh;
        int64_t sty = pos, slb = pos + sty_len(n);
        if (tid == 0) {
            put_int(o, put_lit(o, sty, STY_HEAD), n, 0);
            put_int(o, put_lit(o, slb, SLB_HEAD), n, 0);
            o.put(sty + sty_len(n) - 1, '\n');
            o.put(slb + slb_len(n) - 1, '\n');
        }
        sty += LIT_LEN(STY_HEAD) + ndig((unsigned)n);
        slb += LIT_LEN(SLB_HEAD) + ndig((unsigned)n);
        pos += sty_len(n) + slb_len(n);
        int hlo, hhi;
        my_range(n, tid, hlo, hhi);
        len = 0;
        for (int k = hlo; k < hhi; ++k) len += implh_len(k, ph[k]);
        int64_t p = pos + block_excl_scan<MT>(len, wt, &total);
        for (int k = hlo; k < hhi; ++k) {
            int64_t s = sty + sty_entry_off(k);
            o.put(s, ' '); o.put(s + 1, ' '); o.put(s + 2, ' ');
            s = put_int(o, s + 3, k + 1, 0);
            o.put(s, ' '); o.put(s + 1, 'D'); o.put(s + 2, 'A'); o.put(s + 3, 'T');
            s = slb + slb_entry_off(k);
            o.put(s, ' '); o.put(s + 1, ' '); o.put(s + 2, ' ');
            s = put_int(o, s + 3, k + 1, 0);
            o.put(s, ' '); o.put(s + 1, ' '); o.put(s + 2, ' ');
            put_int(o, s + 3, k + 1, 0);
            p = put_implh(o, p, k, ph[k]);
        }
        pos += total;
    }

    // ---- end
    if (tid == 0) put_lit(o, pos, END_TEXT);
}

// host: decimal digits of v >= 0
inline int64_t host_ndig(int64_t v) {
    int64_t n = 1;
    while (v >= 10) v /= 10, ++n;
    return n;
}

}  // namespace

extern "C" int abc_molblock_desc_size(void) { return (int)sizeof(abc_molblock_desc); }

extern "C" int64_t abc_molblock_text_bytes(const abc_molblock_desc* d) {
    if (!d || d->cap_atoms < 1 || d->cap_mol_bonds < 1) return 0;
    const int64_t na = d->cap_atoms, nb = d->cap_mol_bonds;
    const int64_t da = host_ndig(na), db = host_ndig(nb);
    const int64_t INT_W = 11;      // "-2147483648": the widest a stored int32 prints
    const int64_t w3a = da > 3 ? da : 3, w3b = db > 3 ? db : 3, w4a = da > 4 ? da : 4;
    // a coordinate: four leading columns, at most four integer digits (199999 / 60 - 1 < 10000), ".dddd"
    const int64_t coord = 4 + 4 + 5;
    int64_t n = LIT_LEN(HEAD_TEXT) + w3a + w3b + LIT_LEN(COUNTS_TAIL);
    n += na * (2 * coord + LIT_LEN(ATOM_Z) + 4 + LIT_LEN(ATOM_TAIL));
    n += nb * (4 * INT_W + 1);
    n += LIT_LEN(CHG_HEAD) + w3a + na * (w4a + INT_W) + 1;
    n += LIT_LEN(STY_HEAD) + da + na * (3 + da + 4) + 1;
    n += LIT_LEN(SLB_HEAD) + da + na * (3 + da + 3 + da) + 1;
    n += na * (4 * da + INT_W + LIT_LEN(SAL_HEAD) + LIT_LEN(SAL_MID) + LIT_LEN(SAL_TAIL) + LIT_LEN(SDT_HEAD) + LIT_LEN(SDT_TAIL)
               + LIT_LEN(SDD_HEAD) + LIT_LEN(SDD_TAIL) + LIT_LEN(SED_HEAD) + LIT_LEN(SED_TAIL));
    n += LIT_LEN(END_TEXT);
    return n;
}

extern "C" int abc_write_molblocks(const abc_molblock_desc* d, abc_stream_t stream) {
    if (!d) return abc_fail(ABC_EINVAL, "write_molblocks: null descriptor");
    if (d->B < 1) return abc_fail(ABC_EINVAL, "write_molblocks: empty");
    if (d->cap_atoms < 1 || d->cap_mol_bonds < 1) return abc_fail(ABC_EINVAL, "write_molblocks: cap_atoms and cap_mol_bonds must be >= 1");
    if (d->cap_text < 1 || d->cap_text > INT32_MAX) return abc_fail(ABC_EINVAL, "write_molblocks: cap_text must be 1..2^31-1");
    if (!d->mol_counts || !d->mol_atoms || !d->mol_bonds || !d->mol_implh) return abc_fail(ABC_EINVAL, "write_molblocks: null molecule buffer");
    if (!d->text || !d->index || !d->work) return abc_fail(ABC_EINVAL, "write_molblocks: null output");
    // (one image's length is an int32 in work[])
    if (abc_molblock_text_bytes(d) > INT32_MAX) return abc_fail(ABC_EINVAL, "write_molblocks: one image's text may pass 2^31-1 bytes at these capacities");
    hipLaunchKernelGGL(molblock_size_kernel, dim3(d->B), dim3(MT), 0, (hipStream_t)stream, *d);
    hipLaunchKernelGGL(molblock_write_kernel, dim3(d->B), dim3(MT), 0, (hipStream_t)stream, *d);
    return abc_check_launch("write_molblocks");
}
