// Individualise-and-refine on the graphs of graph_ids.hpp, for one workgroup of 256 threads per image: what the identity test
// (graph_ident.hip) and the canonical order (graph_canon.hip) share, so that the two cannot drift apart -- the id of an individualised
// atom, the workgroup reduction, one round over the rows of either side, and the exact class count through an LDS table.
//
// The round and the class count are stated once as statement macros, REFINE_*, and wrapped in functions below.  graph_ident.hip expands
// the macros inside the lambdas it always had: through the functions its kernel computes the same but is laid out differently, and that
// kernel is held to the instructions it had.  New code calls the functions.
#pragma once
#include "mol_rows.hpp"
#include "graph_ids.hpp"

constexpr int REFINE_GT = 256;       // threads per workgroup
constexpr int REFINE_NW = REFINE_GT / 64;

// the id of the atom individualised at `level`
__device__ inline u64 indiv(u64 id, int level) { return mix(mix(id) + 0x9E3779B97F4A7C15ull * (u64)(level + 1)); }

// f over the workgroup's values; wt = LDS scratch [REFINE_NW].  Every thread must call it (it synchronises, before and after)
template <class T, class F>
__device__ inline T block_reduce(T v, T* wt, F f) {
#pragma unroll
    for (int o = 32; o; o >>= 1) v = f(v, (T)__shfl_xor(v, o));
    __syncthreads();                 // wt may still be read from the previous call; what the callers wrote before is visible after
    if ((threadIdx.x & 63) == 0) wt[threadIdx.x >> 6] = v;
    __syncthreads();
    return f(f(wt[0], wt[1]), f(wt[2], wt[3]));
}
static_assert(REFINE_NW == 4, "block_reduce folds four waves");

// The sums of one round over molecule rows into acc (zero on entry).  Row `tid` is held by the caller (pv: it is valid, its ends pi and
// pj, its order class po); the rows past the workgroup are read again.  i, j: two int lvalues of the caller
#define REFINE_ROUND_MOL(id, acc, pb, nb, na, tid, pv, pi, pj, po, i, j)              \
    if (pv) {                                                                         \
        atomicAdd(&acc[pi], mix(mix(id[pj]) + po));                                   \
        atomicAdd(&acc[pj], mix(mix(id[pi]) + po));                                   \
    }                                                                                 \
    for (int q = tid + REFINE_GT; q < nb; q += REFINE_GT) {                           \
        if (!mol_ends(pb, q, na, i, j)) continue;                                     \
        const u64 o = (u64)bond_class(pb[q * MOL_BOND_W + 2]);                        \
        atomicAdd(&acc[i], mix(mix(id[j]) + o));                                      \
        atomicAdd(&acc[j], mix(mix(id[i]) + o));                                      \
    }
// The same over record rows: ti and tj are already numbers in T, the rows past the workgroup go through remap (record atom -> its
// number in T; both ends of a valid row are in T)
#define REFINE_ROUND_REC(id, acc, rb, m, nt, remap, tid, tv, ti, tj, to, i, j)        \
    if (tv) {                                                                         \
        atomicAdd(&acc[ti], mix(mix(id[tj]) + to));                                   \
        atomicAdd(&acc[tj], mix(mix(id[ti]) + to));                                   \
    }                                                                                 \
    for (int k = tid + REFINE_GT; k < m; k += REFINE_GT) {                            \
        if (!rec_ends(rb, k, nt, i, j)) continue;                                     \
        const u64 o = (u64)bond_class(rb[k * REC_BOND_W + 2]);                        \
        i = remap[i], j = remap[j];                                                   \
        atomicAdd(&acc[i], mix(mix(id[j]) + o));                                      \
        atomicAdd(&acc[j], mix(mix(id[i]) + o));                                      \
    }
// the end of a round: id[a] = mix(mix(id[a] + r) + acc[a]), acc zeroed again
#define REFINE_ROUND_END(id, acc, n, r, tid)                                          \
    __syncthreads();                                                                  \
    for (int a = tid; a < n; a += REFINE_GT) {                                        \
        id[a] = mix(mix(id[a] + r) + acc[a]);                                         \
        acc[a] = 0;                                                                   \
    }                                                                                 \
    __syncthreads();
// The number of distinct ids, exactly (the body of a function that returns it): every id goes into an open-addressed table of SLOTS >=
// 2 n slots (64-bit LDS compare-and-swap; 0 marks a free slot, so the ids that ARE 0 are counted apart), and the ids that found a free
// slot are counted -- as many as there are distinct values, in any order of the threads.  An id that finds itself there is shared by
// two atoms: `shared` keeps this thread's least such id, `zeros` (uniform) the number of ids that are 0, for the cell of the level.
// wi = LDS scratch [REFINE_NW]
#define REFINE_CLASSES(id, n, table, SLOTS, wi, tid, shared, zeros)                                   \
    for (int k = tid; k < SLOTS; k += REFINE_GT) table[k] = 0;                                        \
    __syncthreads();                                                                                  \
    int fresh = 0, zero = 0;                                                                          \
    shared = ~0ull;                                                                                   \
    for (int a = tid; a < n; a += REFINE_GT) {                                                        \
        const u64 e = id[a];                                                                          \
        if (e == 0) {                                                                                 \
            ++zero;                                                                                   \
            continue;                                                                                 \
        }                                                                                             \
        unsigned slot = (unsigned)(e >> 32) & (SLOTS - 1);                                            \
        for (int probe = 0; probe < SLOTS; ++probe) { /* (n <= SLOTS / 2 ids: a free slot is always found) */ \
            const u64 old = atomicCAS(&table[slot], 0ull, e);                                         \
            if (old == 0) {                                                                           \
                ++fresh;                                                                              \
                break;                                                                                \
            }                                                                                         \
            if (old == e) {                                                                           \
                shared = min(shared, e);                                                              \
                break;                                                                                \
            }                                                                                         \
            slot = (slot + 1) & (SLOTS - 1);                                                          \
        }                                                                                             \
    }                                                                                                 \
    const int both = block_reduce(fresh + (zero << 16), wi, [](int u, int v) { return u + v; });      \
    zeros = both >> 16;                                                                               \
    return (both & 0xFFFF) + (zeros > 0);
// the wrapping sum of mix(id) over the atoms (the body of a function that returns it); wu = LDS scratch [REFINE_NW]
#define REFINE_MULTISET_SUM(id, n, wu, tid)                                           \
    u64 s = 0;                                                                        \
    for (int a = tid; a < n; a += REFINE_GT) s += mix(id[a]);                         \
    return block_reduce(s, wu, [](u64 u, u64 v) { return u + v; });

// ---- the same as functions (uniform; acc is zero on entry and on exit of a round)
__device__ __forceinline__ void refine_round_mol(int tid, u64* id, u64* acc, const int* pb, int nb, int na, int n, u64 r, bool pv, int pi, int pj,
                                                 u64 po) {
    int i, j;
    REFINE_ROUND_MOL(id, acc, pb, nb, na, tid, pv, pi, pj, po, i, j)
    REFINE_ROUND_END(id, acc, n, r, tid)
}
__device__ __forceinline__ void refine_round_rec(int tid, u64* id, u64* acc, const int* rb, int m, int nt, const int* remap, int n, u64 r, bool tv,
                                                 int ti, int tj, u64 to) {
    int i, j;
    REFINE_ROUND_REC(id, acc, rb, m, nt, remap, tid, tv, ti, tj, to, i, j)
    REFINE_ROUND_END(id, acc, n, r, tid)
}
template <int SLOTS>
__device__ __forceinline__ int refine_classes(int tid, const u64* id, int n, u64* table, int* wi, u64& shared, int& zeros) {
    REFINE_CLASSES(id, n, table, SLOTS, wi, tid, shared, zeros)
}
__device__ __forceinline__ u64 refine_multiset_sum(int tid, const u64* id, int n, u64* wu) {
    REFINE_MULTISET_SUM(id, n, wu, tid)
}
