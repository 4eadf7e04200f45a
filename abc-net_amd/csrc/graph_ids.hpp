// The atom ids of the position-free graph kernels (graph_sim.hip, graph_ident.hip, graph_canon.hip): one definition of the hash, of the
// order class of a bond code and of id_0, so that the three kernels cannot drift apart (the contract: include/abcnet_hip.h,
// abc_graph_similarity_desc).
#pragma once
#include <hip/hip_runtime.h>

typedef unsigned long long u64;

// the splitmix64 finaliser
__device__ inline u64 mix(u64 x) {
    x ^= x >> 30; x *= 0xBF58476D1CE4E5B9ull;
    x ^= x >> 27; x *= 0x94D049BB133111EBull;
    x ^= x >> 31;
    return x;
}

// a wedge is a single bond (generate_smiles.py:58-68)
__device__ inline int bond_class(int c) { return c == 5 || c == 6 ? 1 : (c >= 1 && c <= 4 ? c : 0); }
__device__ inline u64 id0(int cls, int charge, u64 degree) { return mix(mix(mix((u64)(cls + 1)) + (u64)(long long)charge) + degree); }
