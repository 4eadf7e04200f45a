// Graph records read from a batch of SMILES strings on the device: the writer's inverse (decode.parse_smiles is the host form and the
// reference).  The contract -- reading rule, statuses, record layout -- is in include/abcnet_hip.h and DESIGN.md section 7; every
// decision of the grammar is a function of smiles_tokens.hpp, which a plain C++ build reads too.  Integers only.
//
//   smiles_read_kernel     one workgroup per string, its bytes in LDS.  Every thread owns a run of consecutive bytes, later of tokens
//     1  bytes: `[` and `]` counted and scanned -- a byte is inside a bracket atom iff one more `[` than `]` stands in front of it --
//        then every byte outside says whether a token starts at it (one or two bytes back decide); a scan of the starts is the token
//        index, and the thread of a start classifies its token (the thread of a `[` reads the whole bracket atom)
//     2  tokens: may this class follow the two in front (smiles_tokens.hpp: follows); scans give the atom index, the nesting depth
//        (opened minus closed brackets: never below zero, zero at a dot and at the end) and the places in the lists of `(` `)` and
//        of ring numbers; every token keeps the index of the nearest atom in front of it
//     3  ONE lane per ring number 0..99 walks the list of ring tokens (their numbers stand in list order, sixteen to a load) and pairs
//        those that bear its number: opened, closed, free again; a closing token keeps the opener's atom and the order.  Beside them
//        ONE lane walks the list of `(` and `)` with a stack (an entry says which of the two it is and, for `(`, the atom in front):
//        `(` keeps the atom it branches from, `)` the atom it returns to -- so the atom in front of ANY token is one load away, and
//        the predecessor of an atom is that of the token in front of it (none behind a dot)
//     4  tokens: an atom with a predecessor and a closing number each complete a bond; their scan is the row index.  All bonds whose
//        higher end is atom b are completed by b's own token and the ring numbers behind it, side by side: the duplicate test
//        compares a closing number with those in front of it on the same atom and with the atom's predecessor
//     5  status by priority; rows and counts only for a string that was read
// Every count that bounds a loop is clamped, every store is checked against the image's own rows.
#include "common.hpp"
#include "../../include/abcnet_hip.h"
#include "capi_util.hpp"
#include "block_scan.hpp"
#include "mol_rows.hpp"
#include "text_pack.hpp"
#include "smiles_tokens.hpp"

namespace {

using namespace smiles_read;

constexpr int RT = 256;                                  // threads per workgroup
constexpr int MAXB = ABC_MAX_SMILES_READ_BYTES;          // bytes, and so tokens, atoms and bonds, of one string
constexpr int MAX_NUMBER = 99;
constexpr int NO_ATOM = 0xFFFF;
constexpr unsigned PAREN_CLOSE = 0x8000u;
constexpr int PAREN_LANE = 128;                          // the first lane of the wave behind the ring lanes
static_assert(MAXB <= 1 << 12, "a closing token packs an atom index in 12 bits beside the order");
static_assert(MAX_NUMBER < PAREN_LANE && PAREN_LANE < RT, "one lane per ring number, one more for the brackets");

struct Read {
    alignas(16) uint8_t number[MAXB];     // per ring token, in the order of the list: its number (the ring lanes read sixteen at a time)
    uint8_t text[MAXB];
    uint8_t mark[MAXB];                   // step 1: a token starts at this byte; from step 2: atom a is written aromatic
    uint8_t cls[MAXB];                    // per token: the class
    int8_t val[MAXB], charge[MAXB];       // per token: Token.val, Token.charge
    unsigned short atom[MAXB];            // per token: an atom its own index; a number, a symbol, a dot the atom in front of it in the bytes;
                                          // `(` the atom it branches from, `)` the atom it returns to (step 3)
    unsigned short closing[MAXB];         // per ring token: NO_ATOM at an opening, else the opener's atom | order << 12
    unsigned list[MAXB];                  // from the front `(` and `)`: token | PAREN_CLOSE | the atom in front of it in the bytes << 16; behind
                                          // them the ring tokens
    unsigned short stack[MAXB / 2];       // the atoms of the open branches (every level takes two bytes at least)
};

__device__ inline int symbol_at(const Read& r, int t) { return t > 0 && r.cls[t - 1] == T_BOND ? r.val[t - 1] : 0; }

// atom token t: its predecessor (-1: none) and the order of the symbol in front of it (0: none)
__device__ inline int predecessor(const Read& r, int t, int& symbol) {
    symbol = symbol_at(r, t);
    const int q = t - (symbol ? 2 : 1);
    if (q < 0 || r.cls[q] == T_DOT) return -1;
    const int a = r.atom[q];
    return a == NO_ATOM ? -1 : a;
}

__device__ inline void finish(const abc_smiles_read_desc& d, int b, int status, int bytes, int atoms, int bonds, int rings) {
    const bool ok = status == ABC_READ_OK;
    d.status[b] = status;
    d.rec_counts[b] = ok ? atoms : 0;
    d.rec_counts[d.B + b] = ok ? bonds : 0;
    if (d.stats != nullptr) {
        int* st = d.stats + (size_t)b * 4;
        st[0] = bytes, st[1] = ok ? atoms : 0, st[2] = ok ? bonds : 0, st[3] = ok ? rings : 0;
    }
}

__global__ __launch_bounds__(RT) void smiles_read_kernel(const abc_smiles_read_desc d) {
    __shared__ Read r;
    __shared__ unsigned wt[RT / 64 + 1];
    __shared__ int bad, twice;
    const int b = blockIdx.x, tid = threadIdx.x;
    const int from = d.offsets[b], to = d.offsets[b + 1];
    if (from < 0 || to < from || to > d.cap_text || to == from || to - from > MAXB) {      // (uniform)
        if (tid == 0) {
            const bool range = from < 0 || to < from || to > d.cap_text;
            finish(d, b, range ? ABC_READ_SYNTAX : (to == from ? ABC_READ_EMPTY : ABC_READ_TOO_LONG), range ? 0 : to - from, 0, 0, 0);
        }
        return;
    }
    const int n = to - from;               // 1 .. MAXB
    for (int i = tid; i < n; i += RT) r.text[i] = d.text[(size_t)from + i];
    if (tid == 0) bad = twice = 0;
    __syncthreads();

    // ---- 1: bytes -> tokens
    bool wrong = false;
    unsigned total;
    int lo, hi;
    text_pack::my_range<RT>(n, tid, lo, hi);
    int opened = 0, closed = 0;
    for (int i = lo; i < hi; ++i) opened += r.text[i] == '[', closed += r.text[i] == ']';
    const unsigned before = block_excl_scan<RT>((unsigned)(opened | closed << 16), wt, &total);
    wrong |= (total & 0xFFFFu) != total >> 16;                     // a `[` is left open
    int inside = (int)(before & 0xFFFFu) - (int)(before >> 16), starts = 0;
    for (int i = lo; i < hi; ++i) {
        const int c = r.text[i];
        bool start = false;
        if (c == '[') wrong |= inside != 0, ++inside, start = true;
        else if (c == ']') wrong |= inside != 1, --inside;
        else if (inside == 0) start = is_start(r.text, n, i);
        r.mark[i] = start;
        starts += start;
    }
    int t = (int)block_excl_scan<RT>((unsigned)starts, wt, &total);
    const int nt = min((int)total, n);      // tokens: 1 .. n (the first byte starts one, or is a stray `]`: wrong)
    for (int i = lo; i < hi; ++i) {
        if (!r.mark[i]) continue;
        const Token k = classify(r.text, n, i);
        wrong |= k.cls == T_BAD;
        if (t < MAXB) r.cls[t] = (uint8_t)(k.cls | (k.aromatic ? 8 : 0)), r.val[t] = (int8_t)k.val, r.charge[t] = (int8_t)k.charge;
        ++t;
    }
    if (wrong) atomicOr(&bad, 1);
    __syncthreads();
    if (bad || nt < 1) {                   // (uniform: read behind the barrier)
        if (tid == 0) finish(d, b, ABC_READ_SYNTAX, n, 0, 0, 0);
        return;
    }

    // ---- 2: tokens -> atom index, depth, the two lists
    text_pack::my_range<RT>(nt, tid, lo, hi);
    int atoms = 0, rings = 0;
    opened = closed = 0;
    for (int q = lo; q < hi; ++q) {
        const int c = r.cls[q] & 7;
        atoms += c == T_ATOM, rings += c == T_RING, opened += c == T_OPEN, closed += c == T_CLOSE;
    }
    const unsigned ar = block_excl_scan<RT>((unsigned)(atoms | rings << 16), wt, &total);
    const int na = (int)(total & 0xFFFFu), nr = (int)(total >> 16);
    const unsigned oc = block_excl_scan<RT>((unsigned)(opened | closed << 16), wt, &total);
    const int np = (int)(total & 0xFFFFu) + (int)(total >> 16);      // (na + nr + np <= nt <= MAXB)
    wrong |= (total & 0xFFFFu) != total >> 16;                       // a branch is left open
    {                                      // (mark: every thread is through with the starts, the scans' barriers lie between)
        int a = (int)(ar & 0xFFFFu), ring = (int)(ar >> 16), o = (int)(oc & 0xFFFFu), c2 = (int)(oc >> 16);
        for (int q = lo; q < hi; ++q) {
            const int c = r.cls[q] & 7, p = q > 0 ? r.cls[q - 1] & 7 : T_NONE, p2 = q > 1 ? r.cls[q - 2] & 7 : T_NONE;
            wrong |= !follows(p2, p, c);
            if (q == nt - 1) wrong |= !follows(p, c, T_END);
            if (c == T_ATOM) {
                r.mark[a] = (r.cls[q] & 8) != 0;
                r.atom[q] = (unsigned short)a++;
                continue;
            }
            const unsigned front = a > 0 ? a - 1 : NO_ATOM;      // the atom in front of this token in the bytes
            r.atom[q] = (unsigned short)front;
            if (c == T_RING) {
                r.list[min(np + ring, MAXB - 1)] = (unsigned)q;
                r.number[min(ring, MAXB - 1)] = (uint8_t)r.val[q], ++ring;
            } else if (c == T_OPEN) {
                r.list[min(o + c2, MAXB - 1)] = (unsigned)q | front << 16, ++o;
            } else if (c == T_CLOSE) {
                wrong |= o - c2 < 1;
                r.list[min(o + c2, MAXB - 1)] = (unsigned)q | PAREN_CLOSE, ++c2;
            } else if (c == T_DOT) {
                wrong |= o != c2;
            }
        }
    }
    if (wrong) atomicOr(&bad, 1);
    __syncthreads();
    if (bad) {
        if (tid == 0) finish(d, b, ABC_READ_SYNTAX, n, 0, 0, 0);
        return;
    }

    // ---- 3: one lane per ring number; one lane for the brackets (the grammar holds from here on: a token stands in front of every
    //         `(`, no `)` without its `(`, an atom in front of every ring number)
    if (tid <= MAX_NUMBER) {
        int open = -1;
        for (int k0 = 0; k0 < nr; k0 += 16) {      // (k0 + 15 < MAXB; the numbers past nr are not looked at)
            const uint4 w = *reinterpret_cast<const uint4*>(&r.number[k0]);
            const unsigned word[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                if (k0 + j >= nr || (word[j >> 2] >> (8 * (j & 3)) & 0xFFu) != (unsigned)tid) continue;
                const int q = (int)r.list[np + k0 + j];
                if (open < 0) {
                    open = q;
                    r.closing[q] = NO_ATOM;
                    continue;
                }
                const int a = r.atom[open], a2 = r.atom[q];
                const int order = ring_order(symbol_at(r, open), symbol_at(r, q), r.mark[a & (MAXB - 1)] != 0, r.mark[a2 & (MAXB - 1)] != 0);
                wrong |= a == a2 || order == 0;
                r.closing[q] = (unsigned short)((a & (MAXB - 1)) | order << 12);
                open = -1;
            }
        }
        wrong |= open >= 0;
        if (wrong) atomicOr(&bad, 1);
    } else if (tid == PAREN_LANE) {
        int top = 0, closed_at = -2;
        unsigned short back = NO_ATOM;     // the atom the last `)` returned to, at token closed_at
        for (int k = 0; k < np; ++k) {
            const unsigned e = r.list[k];
            const int q = (int)(e & (PAREN_CLOSE - 1));
            if (!(e & PAREN_CLOSE)) {      // in front of `(` stands an atom or a number -- the entry holds their atom -- or the last `)`
                const unsigned short owner = closed_at == q - 1 ? back : (unsigned short)(e >> 16);
                r.atom[q] = owner;
                if (top < MAXB / 2) r.stack[top] = owner;
                ++top;
            } else {
                top = max(top - 1, 0);
                back = top < MAXB / 2 ? r.stack[top] : (unsigned short)NO_ATOM;
                r.atom[q] = back, closed_at = q;
            }
        }
    }
    __syncthreads();
    if (bad) {
        if (tid == 0) finish(d, b, ABC_READ_SYNTAX, n, 0, 0, 0);
        return;
    }

    // ---- 4: the bonds: rows, and a pair bonded twice
    int rows = 0, ring_rows = 0;
    bool again = false;
    for (int q = lo; q < hi; ++q) {
        const int c = r.cls[q] & 7;
        int symbol;
        if (c == T_ATOM) {
            rows += predecessor(r, q, symbol) >= 0;
        } else if (c == T_RING && r.closing[q] != NO_ATOM) {
            ++rows, ++ring_rows;
            const int a = r.closing[q] & (MAXB - 1);
            for (int f = q - 1; f >= 0; --f) {      // back over this atom's numbers and symbols to its own token
                const int cf = r.cls[f] & 7;
                if (cf == T_RING) again |= r.closing[f] != NO_ATOM && (r.closing[f] & (MAXB - 1)) == a;
                else if (cf == T_ATOM) { again |= predecessor(r, f, symbol) == a; break; }
                else if (cf != T_BOND) break;
            }
        }
    }
    if (again) atomicOr(&twice, 1);
    int row = (int)(block_excl_scan<RT>((unsigned)(rows | ring_rows << 16), wt, &total) & 0xFFFFu);      // (its barriers publish `twice`)
    const int m = (int)(total & 0xFFFFu), ring_bonds = (int)(total >> 16);

    // ---- 5: status, and the rows of a string that was read
    const int status = na > d.max_atoms || m > d.max_bonds ? ABC_READ_TRUNCATED : (twice ? ABC_READ_DUPLICATE : ABC_READ_OK);
    if (tid == 0) finish(d, b, status, n, na, m, ring_bonds);
    if (status != ABC_READ_OK) return;
    int* ra = d.rec_atoms + (size_t)b * d.max_atoms * REC_ATOM_W;
    int* rb = d.rec_bonds + (size_t)b * d.max_bonds * REC_BOND_W;
    for (int q = lo; q < hi; ++q) {
        const int c = r.cls[q] & 7;
        int i = -1, j = -1, order = 0;
        if (c == T_ATOM) {
            j = r.atom[q];
            if (j < d.max_atoms) {
                int* row_a = ra + (size_t)j * REC_ATOM_W;
                row_a[0] = 0, row_a[1] = 0, row_a[2] = r.val[q], row_a[3] = r.charge[q];
            }
            int symbol;
            i = predecessor(r, q, symbol);
            if (i >= 0) order = symbol ? symbol : implicit_order(r.mark[i] != 0, (r.cls[q] & 8) != 0);
        } else if (c == T_RING && r.closing[q] != NO_ATOM) {
            i = r.closing[q] & (MAXB - 1), j = r.atom[q], order = r.closing[q] >> 12;
        }
        if (i < 0) continue;
        if (row < d.max_bonds) {
            int* row_b = rb + (size_t)row * REC_BOND_W;
            row_b[0] = i, row_b[1] = j, row_b[2] = order;
        }
        ++row;
    }
}

}  // namespace

extern "C" int abc_smiles_read_desc_size(void) { return (int)sizeof(abc_smiles_read_desc); }

extern "C" int abc_read_smiles(const abc_smiles_read_desc* d, abc_stream_t stream) {
    const char* entry = "read_smiles";
    if (!d) return abc_fail_in(ABC_EINVAL, entry, "null descriptor");
    if (d->B < 1) return abc_fail_in(ABC_EINVAL, entry, "empty");
    if (d->max_atoms < 1 || d->max_bonds < 1) return abc_fail_in(ABC_EINVAL, entry, "max_atoms and max_bonds must be >= 1");
    if (d->cap_text < 1) return abc_fail_in(ABC_EINVAL, entry, "cap_text must be >= 1");
    if (!d->text || !d->offsets) return abc_fail_in(ABC_EINVAL, entry, "null text or offsets");
    if (!d->rec_atoms || !d->rec_bonds || !d->rec_counts) return abc_fail_in(ABC_EINVAL, entry, "null record buffer");
    if (!d->status) return abc_fail_in(ABC_EINVAL, entry, "null status");
    hipLaunchKernelGGL(smiles_read_kernel, dim3(d->B), dim3(RT), 0, (hipStream_t)stream, *d);
    return abc_check_launch(entry);
}
