"""CPU tier of the bf16 gradient exchange (GradReducer(mode="direct", wire_dtype="bf16")): the numpy
mirror's rounding against torch's CPU conversion, and the exchange itself over gloo on CPU tensors at world 2 and 3 against the
mirror, bit for bit -- which shard goes to whom, the order of the rows in the sum, where the gathered shards land."""
import os

import numpy as np
import pytest
import torch

import abcnet_amd  # noqa: F401
from abcnet_amd import distributed as D

import exchange_oracle as X


def test_mirror_rounding_equals_torch_cpu_conversion_on_the_edge_values():
    x = X.edge_values(nan=False)
    got = X.bf16_rne(x)
    want = torch.from_numpy(x.copy()).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    assert np.array_equal(got, want), [(hex(b), hex(g), hex(w)) for b, g, w in zip(X.EDGE_BITS, got, want) if g != w]
    # spot values spelled out: zeros and infinities kept, subnormals rounded (0x00008000 is a tie to even -> 0, 0x00018000 a tie to
    # odd -> 2), ties to even, the largest finite f32 -> Inf
    spot = {0x00000000: 0x0000, 0x80000000: 0x8000, 0x00008000: 0x0000, 0x00008001: 0x0001, 0x00018000: 0x0002, 0x007FFFFF: 0x0080,
            0x3F808000: 0x3F80, 0x3F818000: 0x3F82, 0x3F807FFF: 0x3F80, 0x3F808001: 0x3F81, 0x7F7F0000: 0x7F7F, 0x7F7F8000: 0x7F80,
            0x7F7FFFFF: 0x7F80, 0xFF7FFFFF: 0xFF80, 0x7F800000: 0x7F80, 0xFF800000: 0xFF80}
    for b, h in spot.items():
        assert int(X.bf16_rne(np.array([b], dtype=np.uint32).view(np.float32))[0]) == h, hex(b)
    # NaN: only NaN-ness (the payload is unspecified), and never Inf
    n = X.bf16_to_f32(X.bf16_rne(np.array(X.NAN_BITS, dtype=np.uint32).view(np.float32)))
    assert np.isnan(n).all()
    assert torch.from_numpy(np.array(X.NAN_BITS, dtype=np.uint32).view(np.float32).copy()).to(torch.bfloat16).float().isnan().all()
    # and on a spread of ordinary values
    r = (np.random.default_rng(3).standard_normal(4096) * 10.0 ** np.random.default_rng(4).uniform(-8, 4, 4096)).astype(np.float32)
    assert np.array_equal(X.bf16_rne(r), torch.from_numpy(r).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16))


def rank_data(world, rank):
    """rank `rank`'s flat f32 gradient for the gloo test: three buckets (256 x W, the minimum 128 x W, 384 x W elements), random
    values over many magnitudes, with edge values and an order-sensitive column planted in every shard of the middle bucket"""
    sizes = [256 * world, 128 * world, 384 * world]
    rng = np.random.default_rng(100 + rank)
    total = sum(sizes)
    g = (rng.standard_normal(total) * 10.0 ** rng.uniform(-8, 4, total)).astype(np.float32)
    lo = sizes[0]
    n = 128
    for r in range(world):
        col = lo + r * n
        # 2^30, 1, -2^30 down the ranks (world 3): the rank-order f32 sum is (2^30 + 1) - 2^30 = 0, any other order gives 1
        g[col] = [2.0 ** 30, 1.0, -2.0 ** 30][rank % 3] if world == 3 else [1.0, 2.0 ** -9][rank % 2]
        g[col + 1] = np.inf if rank == 0 else 1.0
        g[col + 2] = np.inf if rank == 0 else -np.inf      # Inf - Inf: NaN on every rank
        g[col + 3] = np.float32(1.00390625)                # 1 + 2^-8: a tie of the first rounding, and of the second at world 2
        ev = X.edge_values(nan=False)
        g[col + 8:col + 8 + ev.size] = ev if rank == 0 else 0.0
    buckets = [(0, sizes[0], 2), (sizes[0], sizes[0] + sizes[1], 1), (sizes[0] + sizes[1], total, 0)]
    return g, buckets


def _worker(rank, world, port, q):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    g, buckets = rank_data(world, rank)
    t = torch.from_numpy(g.copy())
    red = D.GradReducer(t, buckets, mode="direct", wire_dtype="bf16")
    for lo, hi, _ in buckets:
        red.bucket_ready(lo, hi)
    red.finish()
    q.put((rank, t.numpy().copy(), red.mode, red.wire_dtype, red.fallback_reason, red.wire_bytes_per_step(),
           [red.wire_bytes_per_step(world=w) for w in (2, 4, 8)]))
    dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3])
def test_gloo_bf16_direct_exchange_equals_the_mirror_bit_for_bit(world):
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = D.free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    try:
        res = sorted((q.get(timeout=120) for _ in procs), key=lambda r: r[0])
    finally:
        for p in procs:
            p.join(60)
            if p.is_alive():
                p.terminate()
    assert [r[0] for r in res] == list(range(world))
    data = [rank_data(world, r) for r in range(world)]
    buckets = data[0][1]
    want = np.empty_like(data[0][0])
    for lo, hi, _ in buckets:
        want[lo:hi] = X.exchange([data[r][0][lo:hi] for r in range(world)])
    elems = sum(hi - lo for lo, hi, _ in buckets)
    for rank, got, mode, wire, why, nbytes, table in res:
        assert (mode, wire, why) == ("direct", "bf16", None), (rank, mode, wire, why)
        assert X.same_bits(got, want), "rank %d: %d elements differ from the mirror" % (
            rank, int((got.view(np.uint32) != want.view(np.uint32)).sum()))
        # NaN payloads included: every rank holds the very same bits (each shard is reduced by ONE rank, then copied)
        assert np.array_equal(got.view(np.uint32), res[0][1].view(np.uint32)), rank
        # both legs, 2 bytes per element, (W - 1) / W of the bucket leaves the rank on each
        assert nbytes == 2 * (world - 1) * elems * 2 // world
        assert table == [2 * (w - 1) * elems * 2 // w for w in (2, 4, 8)]
    # the planted columns did what they are there for
    lo = buckets[1][0]
    if world == 3:
        assert want[lo] == 0.0 and want[lo + 128] == 0.0      # (2^30 + 1) + -2^30 in rank order; 1 in any other
    assert np.isinf(want[lo + 1]) and np.isnan(want[lo + 2])


def test_wire_bytes_closed_form_and_bf16_needs_direct():
    g = torch.zeros(1024)
    buckets = [(0, 512, 1), (512, 1024, 0)]
    for mode in ("all_reduce", "rs_ag"):
        with pytest.raises(ValueError, match="direct"):
            D.GradReducer(g, buckets, mode=mode, wire_dtype="bf16")
    with pytest.raises(ValueError):
        D.GradReducer(g, buckets, mode="direct", wire_dtype="fp16")
    # no process group: nothing is exchanged, nothing runs in bf16 -- and the formula for a world of W over the same buckets
    red = D.GradReducer(g, buckets, mode="direct", wire_dtype="bf16")
    assert red.active is False and red.wire_dtype == "f32" and red.wire_bytes_per_step() == 0
    assert [red.wire_bytes_per_step(world=w) for w in (1, 2, 4, 8)] == [0, 4096, 6144, 7168]      # f32: 2 legs x (W-1)/W x 1024 x 4
    assert D.GradReducer.MODES == ("rs_ag", "direct", "all_reduce")


def test_trainer_refuses_bf16_with_another_exchange_mode():
    from abcnet_amd.train import Trainer
    from abcnet_amd.unet import UNet
    m = UNet(1, [1, 14, 3, 2, 1, 360, 60, 60])
    for mode in ("all_reduce", "rs_ag"):
        with pytest.raises(ValueError, match="exchange='direct'"):
            Trainer(m, 2, 64, 64, exchange=mode, exchange_dtype="bf16")
    with pytest.raises(ValueError, match="exchange_dtype"):
        Trainer(m, 2, 64, 64, exchange="direct", exchange_dtype="fp16")
