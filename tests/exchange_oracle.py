"""numpy mirror of the bf16 gradient exchange (GradReducer(mode="direct", wire_dtype="bf16")): the rounding
rule on the f32 bit pattern and steps 1 to 5 of the exchange of one bucket over W ranks, written independently of the kernels
(csrc/exchange.hip) and of the torch ops of the CPU path (distributed.py)."""
import numpy as np


def bf16_rne(x):
    """f32 array -> uint16 array of bf16 bit patterns: round-to-nearest-even on the bit pattern u,
    (u + 0x7FFF + ((u >> 16) & 1)) >> 16; a NaN keeps its sign and gets the quiet bit (never Inf)"""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    r = (u + 0x7FFF + ((u >> 16) & 1)) >> 16
    nan = (u & 0x7FFFFFFF) > 0x7F800000
    return np.where(nan, (u >> 16) | 0x40, r).astype(np.uint16)


def bf16_to_f32(h):
    """uint16 array of bf16 bit patterns -> f32 array (exact)"""
    return (np.ascontiguousarray(h, dtype=np.uint16).astype(np.uint32) << 16).view(np.float32)


def round_bf16(x):
    """f32 -> the nearest bf16, as f32"""
    return bf16_to_f32(bf16_rne(x))


def reduce_rows(rows):
    """rows: uint16 [W][n] of bf16 bit patterns -> uint16 [n]: ((row 0 + row 1) + row 2) + ... in f32, rounded to bf16"""
    rows = np.asarray(rows, dtype=np.uint16)
    with np.errstate(invalid="ignore", over="ignore"):
        acc = bf16_to_f32(rows[0]).copy()
        for q in range(1, rows.shape[0]):
            acc = (acc + bf16_to_f32(rows[q])).astype(np.float32)
    return bf16_rne(acc)


def exchange(per_rank):
    """per_rank: list of W f32 arrays of W * n elements, rank q's bucket g_q[lo:hi].  Returns the f32 array of W * n elements
    every rank holds afterwards: send_q = bf16(g_q); rank r receives row q = send_q[r*n:(r+1)*n]; shard_r = bf16(rank-ordered
    f32 sum of its rows); the gathered shards, widened to f32."""
    w = len(per_rank)
    total = per_rank[0].size
    assert total % w == 0 and all(g.size == total for g in per_rank)
    n = total // w
    send = [bf16_rne(g) for g in per_rank]
    shards = [reduce_rows(np.stack([send[q][r * n:(r + 1) * n] for q in range(w)])) for r in range(w)]
    return bf16_to_f32(np.concatenate(shards))


def same_bits(a, b):
    """f32 / uint16 arrays equal bit for bit, except that a NaN matches any NaN"""
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype == np.uint16:
        a, b = bf16_to_f32(a), bf16_to_f32(b)
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and bool(np.array_equal(na, nb)) and bool(np.array_equal(a.view(np.uint32)[~na], b.view(np.uint32)[~nb]))


# f32 bit patterns the rounding rule must get right (test_exchange_bf16_host.py, test_gpu_exchange_bf16.py)
EDGE_BITS = [
    0x00000000, 0x80000000,                          # +-0
    0x00000001, 0x80000001, 0x00007FFF, 0x00008000, 0x00008001, 0x00018000, 0x007FFFFF, 0x807F8000,   # f32 subnormals (rounded, not flushed)
    0x3F808000, 0x3F818000,                          # exact ties: kept bit even (stays), odd (goes up)
    0x3F807FFF, 0x3F808001, 0x3F817FFF, 0x3F818001,  # one ulp either side of those ties
    0xBF808000, 0xBF818000, 0xBF808001,              # the same, negative
    0x3F7FFFFF, 0x3FFF8000,                          # carries into the exponent
    0x7F7F0000, 0x7F7F7FFF, 0x7F7F8000, 0x7F7FFFFF, 0xFF7FFFFF,   # largest bf16 stays, above it (from the tie on) -> Inf
    0x7F800000, 0xFF800000,                          # +-Inf
]
NAN_BITS = [0x7FC00000, 0xFFC00000, 0x7F800001, 0x7FBFFFFF, 0xFF800001, 0x7FFFFFFF]   # quiet, signalling, low payload only


def edge_values(nan=True):
    return np.array(EDGE_BITS + (NAN_BITS if nan else []), dtype=np.uint32).view(np.float32)
