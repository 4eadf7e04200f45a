// Host-side helpers for the C-ABI launchers: error text + launch check.
#pragma once
#include <cstdio>
#include <hip/hip_runtime.h>
#include "../../include/abcnet_hip.h"

int abc_fail(int code, const char* msg);     // records msg, returns code
int abc_check_launch(const char* what);      // hipGetLastError -> ABC_ELAUNCH
// hipFuncAttributeMaxDynamicSharedMemorySize is a PER-DEVICE attribute of a kernel: set it once per (kernel, device) --
// `done` is the caller's per-kernel bitmask over device ordinals -- and report a refusal instead of failing later at launch
int abc_allow_lds(const void* fn, int bytes, unsigned long long* done);
// bytes per element of an abc_dtype
inline int abc_dsize(int dtype) { return dtype == ABC_F32 ? 4 : (dtype == ABC_BF16 ? 2 : 1); }

// ---- the launchers that read the molecule rows OR the graph records (abc_canon_desc, abc_aromatic_desc: the same mol_* / rec_* fields)
#include "mol_rows.hpp"              // (the words per row)
struct abc_extent { const void* p; size_t bytes; };
inline int abc_fail_in(int code, const char* entry, const char* what) {      // "<entry>: <what>"
    char msg[256];
    snprintf(msg, sizeof(msg), "%s: %s", entry, what);
    return abc_fail(code, msg);
}
inline bool overlap(const void* p, size_t np, const void* q, size_t nq) {
    const char *a = (const char*)p, *c = (const char*)q;
    return p != nullptr && q != nullptr && a < c + nq && c < a + np;
}
// the first refusals of such a launcher: a descriptor, a batch, one side -- `mol` says which
template <class Desc>
inline int abc_one_side(const char* entry, const Desc* d, bool& mol) {
    if (!d) return abc_fail_in(ABC_EINVAL, entry, "null descriptor");
    mol = d->mol_counts != nullptr;
    if (d->B < 1) return abc_fail_in(ABC_EINVAL, entry, "empty");
    if (mol == (d->rec_counts != nullptr)) return abc_fail_in(ABC_EINVAL, entry, "give the molecule rows or the graph records, one side");
    return ABC_OK;
}
// the side that was given: its buffers, then its capacities (two calls: abc_perceive_aromatic has a refusal of its own between them)
template <class Desc>
inline int abc_one_side_buffers(const char* entry, const Desc* d, bool mol) {
    if (mol ? !d->mol_atoms || !d->mol_bonds : !d->rec_atoms || !d->rec_bonds)
        return abc_fail_in(ABC_EINVAL, entry, mol ? "null molecule buffer" : "null record buffer");
    return ABC_OK;
}
template <class Desc>
inline int abc_one_side_capacities(const char* entry, const Desc* d, bool mol) {
    static_assert(ABC_MAX_SIM_ATOMS == 512, "the two refusals below say 512");
    if (mol ? d->cap_atoms < 1 || d->cap_mol_bonds < 1 : d->max_atoms < 1 || d->max_bonds < 1)
        return abc_fail_in(ABC_EINVAL, entry, mol ? "cap_atoms and cap_mol_bonds must be >= 1" : "max_atoms and max_bonds must be >= 1");
    if ((mol ? d->cap_atoms : d->max_atoms) > ABC_MAX_SIM_ATOMS)
        return abc_fail_in(ABC_EUNSUPPORTED, entry, mol ? "cap_atoms must be <= 512" : "max_atoms must be <= 512");
    return ABC_OK;
}
// no output may overlap an input or another output: (pointer, bytes) of the seven inputs at the capacities of the side that was given
// against the caller's table of outputs
template <class Desc, int NOUT>
inline int abc_one_side_overlap(const char* entry, const Desc* d, bool mol, const abc_extent (&out)[NOUT]) {
    const size_t B = (size_t)d->B, cap = (size_t)(mol ? d->cap_atoms : d->max_atoms), cb = (size_t)(mol ? d->cap_mol_bonds : d->max_bonds);
    const abc_extent in[7] = {{d->mol_counts, B * 16}, {d->mol_atoms, B * cap * ATOM_W * 4}, {d->mol_bonds, B * cb * MOL_BOND_W * 4}, {d->mol_implh, B * cap * 4},
                              {d->rec_atoms, B * cap * REC_ATOM_W * 4}, {d->rec_bonds, B * cb * REC_BOND_W * 4}, {d->rec_counts, B * 8}};
    for (int o = 0; o < NOUT; ++o) {
        for (int i = 0; i < 7; ++i)
            if (overlap(out[o].p, out[o].bytes, in[i].p, in[i].bytes)) return abc_fail_in(ABC_EINVAL, entry, "an output overlaps an input");
        for (int o2 = 0; o2 < o; ++o2)
            if (overlap(out[o].p, out[o].bytes, out[o2].p, out[o2].bytes)) return abc_fail_in(ABC_EINVAL, entry, "two outputs overlap");
    }
    return ABC_OK;
}
