// The hydrogen count `h` of the SMILES text rule ("Hydrogen count"): ONE definition for the writer (smiles.hip)
// and for the aromaticity perception (aromatic.hip), which lists an atom exactly where this count would drop from 1 to 0.
#pragma once
#include <hip/hip_runtime.h>
#include "mol_rows.hpp"

constexpr unsigned AROMATIC_SET = 1u << 0 | 1u << 1 | 1u << 2 | 1u << 3 | 1u << 4 | 1u << 7 | 1u << 9 | 1u << 10;      // B C N O P S Se
// the valence lists by vocabulary index and charge -1 | 0 | +1: up to three values, four bits each, lowest first, 0 = no more
#define V1(a) (a)
#define V2(a, b) ((a) | (b) << 4)
#define V3(a, b, c) ((a) | (b) << 4 | (c) << 8)
__device__ const unsigned short VALENCES[N_SYMBOLS][3] = {
    {V1(3), V1(4), V1(3)}, {V1(3), V1(4), V1(3)},                     // C, C
    {V1(2), V1(3), V1(4)}, {V1(1), V1(2), V1(3)},                     // N, O
    {V3(2, 4, 6), V2(3, 5), V1(4)}, {0, V1(1), V1(2)},                // P, F
    {0, V1(1), V3(2, 4, 6)}, {V1(1), V3(2, 4, 6), V2(3, 5)},          // Cl, S
    {0, V1(1), V3(2, 4, 6)}, {V1(4), V1(3), V1(2)},                   // Br, B
    {V1(1), V3(2, 4, 6), V2(3, 5)}, {0, V1(1), V3(2, 4, 6)},          // Se, I
    {0, 0, 0}, {V2(3, 5), V1(4), V1(3)}};                             // H, Si
#undef V1
#undef V2
#undef V3

// the contribution of a bond of order class `cls` to s2: 3 for class 4 and 2 * class otherwise
__device__ inline int bond_s2(int cls) { return cls == 4 ? 3 : 2 * cls; }

// h of an unlisted atom: s2 = the sum of bond_s2 over its bonds
__device__ inline int hydrogens(int sym, int charge, int s2) {
    if (sym == 12 || charge < -1 || charge > 1) return 0;
    const int v = s2 >> 1;
    for (unsigned list = VALENCES[sym][charge + 1]; list != 0; list >>= 4) {
        const int t = (int)(list & 15u);
        if (t >= v) return t - v;
    }
    return 0;
}
