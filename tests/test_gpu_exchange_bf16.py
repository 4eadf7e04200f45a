"""The three kernels of the bf16 gradient exchange (csrc/exchange.hip) through the C ABI, bit for bit against the numpy mirror
(tests/exchange_oracle.py): every size that takes another path (no whole 8-element unit, exactly one, head / tail elements, more
than one workgroup), sources 0, 1 and 3 elements and destinations 0 and 1 elements past a 16-byte boundary, every destination
between canaries."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import abcnet_amd  # noqa: E402,F401
from abcnet_amd import _lib as L  # noqa: E402
from hiputil import DEV, stream  # noqa: E402

import exchange_oracle as X  # noqa: E402

SIZES = [1, 7, 8, 9, 255, 256, 257, 4099]
SRC_OFFS = [0, 1, 3]
DST_OFFS = [0, 1]
PAD = 16                     # canary elements on either side of a destination (a whole 16-byte store and more)
CANARY_BF16 = 0x4B1D         # as bits; f32 canary 0x4B1D4B1D
WORLDS = [1, 2, 3, 8]


def dev_src(host, off):
    """`host` (f32 or uint16 numpy) on the device, starting `off` elements past a 16-byte boundary (torch's allocations are)"""
    t = torch.from_numpy(host.view(np.int16) if host.dtype == np.uint16 else host)
    buf = torch.zeros(off + t.numel() + 8, dtype=t.dtype, device=DEV)
    assert buf.data_ptr() % 16 == 0
    v = buf[off:off + t.numel()]
    v.copy_(t)
    return buf, v


def dev_dst(n, off, dtype):
    """n destination elements `off` past a 16-byte boundary, PAD canaries on either side; returns (buffer, view)"""
    lead = PAD + off      # PAD is a multiple of 8 elements: a multiple of 16 bytes for both element sizes
    buf = torch.full((lead + n + PAD,), CANARY_BF16, dtype=torch.int16, device=DEV) if dtype == torch.int16 else \
        torch.from_numpy(np.full(lead + n + PAD, 0x4B1D4B1D, dtype=np.uint32).view(np.float32)).to(DEV)
    assert buf.data_ptr() % 16 == 0
    return buf, buf[lead:lead + n]


def canaries_intact(buf, n, off):
    h = buf.cpu().numpy()
    bits = h.view(np.uint16) if h.dtype == np.int16 else h.view(np.uint32)
    want = CANARY_BF16 if h.dtype == np.int16 else 0x4B1D4B1D
    lead = PAD + off
    return bool((bits[:lead] == want).all() and (bits[lead + n:] == want).all())


def plant(x, vals):
    """edge values at the head, the tail and the seams between the one-by-one elements and the 16-byte units"""
    n, k = x.size, vals.size
    for start in (0, 5, 250, n // 2, n - k):
        if 0 <= start and start + k <= n:
            x[start:start + k] = vals
    m = min(n, k)
    x[:m] = vals[:m]
    x[n - m:] = vals[k - m:]
    return x


def pack_input(n, seed):
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal(n) * 10.0 ** rng.uniform(-8, 4, n)).astype(np.float32)
    return plant(x, X.edge_values()) if n >= 255 else plant(x, rng.permutation(X.edge_values())[:max(1, min(n, 9))])


@pytest.mark.parametrize("n", SIZES)
def test_pack_equals_the_mirror(n):
    lib = L.load()
    for so in SRC_OFFS:
        for do in DST_OFFS:
            x = pack_input(n, 17 * n + 3 * so + do)
            _sb, src = dev_src(x, so)
            buf, dst = dev_dst(n, do, torch.int16)
            L.check(lib.abc_grad_pack_bf16(src.data_ptr(), dst.data_ptr(), n, stream()), "grad_pack_bf16")
            got = dst.cpu().numpy().view(np.uint16)
            assert X.same_bits(got, X.bf16_rne(x)), (n, so, do)
            assert canaries_intact(buf, n, do), (n, so, do)


def test_pack_every_edge_value_on_both_paths():
    """all edge values (NaNs included) through the one-by-one elements (n = 7: no whole unit) and through the 16-byte units"""
    lib = L.load()
    ev = X.edge_values()
    for n in (7, 8 * ((ev.size + 7) // 8)):
        for start in range(0, ev.size, n):
            x = np.zeros(n, dtype=np.float32)
            chunk = ev[start:start + n]
            x[:chunk.size] = chunk
            _sb, src = dev_src(x, 0)
            buf, dst = dev_dst(n, 0 if n > 7 else 1, torch.int16)
            L.check(lib.abc_grad_pack_bf16(src.data_ptr(), dst.data_ptr(), n, stream()), "grad_pack_bf16")
            got = dst.cpu().numpy().view(np.uint16)
            assert X.same_bits(got, X.bf16_rne(x)), (n, start)
            nan_in = np.isnan(x)
            assert not np.isinf(X.bf16_to_f32(got)[nan_in]).any()      # a NaN never becomes Inf


def reduce_rows(w, n, seed):
    """[w][n] bf16 bit patterns built by hand: random values, an order-sensitive column, an Inf and a NaN column, subnormals"""
    rng = np.random.default_rng(seed)
    rows = X.bf16_rne((rng.standard_normal((w, n)) * 10.0 ** rng.uniform(-6, 3, (w, n))).astype(np.float32))
    f = lambda v: X.bf16_rne(np.array(v, dtype=np.float32))      # noqa: E731
    for c in sorted(set([0, min(n - 1, 7), min(n - 1, 8), n - 1, n // 2])):      # head, seam, tail, a unit in the middle
        kind = c % 4
        if kind == 0 and w >= 3:
            rows[:, c] = 0
            rows[:3, c] = f([2.0 ** 30, 1.0, -2.0 ** 30])       # rank order: 0; any other order: 1
        elif kind == 0:
            rows[:, c] = f([1.0] + [2.0 ** -9] * (w - 1))       # 1 + 2^-9 in f32, then a tie of the final rounding
        elif kind == 1:
            rows[0, c] = 0x7F80                                  # Inf
        elif kind == 2:
            rows[0, c] = 0x7F80
            rows[w - 1, c] = 0xFF80 if w > 1 else 0x7FC1         # Inf - Inf (w = 1: a NaN as it came)
        else:
            rows[:, c] = 0x0001                                  # bf16 subnormals: the sum must not be flushed
    return rows


@pytest.mark.parametrize("w", WORLDS)
def test_reduce_equals_the_mirror(w):
    lib = L.load()
    for n in SIZES:
        rows = reduce_rows(w, n, 1000 * w + n)
        want = X.reduce_rows(rows)
        for so in SRC_OFFS:
            for do in DST_OFFS:
                _sb, src = dev_src(rows.reshape(-1), so)
                buf, dst = dev_dst(n, do, torch.int16)
                L.check(lib.abc_grad_reduce_bf16(src.data_ptr(), dst.data_ptr(), w, n, stream()), "grad_reduce_bf16")
                got = dst.cpu().numpy().view(np.uint16)
                assert X.same_bits(got, want), (w, n, so, do)
                assert canaries_intact(buf, n, do), (w, n, so, do)
    if w >= 3:
        assert X.bf16_to_f32(X.reduce_rows(reduce_rows(w, 4099, 1000 * w + 4099)))[0] == 0.0      # the order column is in play


@pytest.mark.parametrize("n", SIZES)
def test_unpack_is_exact(n):
    lib = L.load()
    for so in SRC_OFFS:
        for do in DST_OFFS:
            h = X.bf16_rne(pack_input(n, 5 * n + so + do))
            _sb, src = dev_src(h, so)
            buf, dst = dev_dst(n, do, torch.float32)
            L.check(lib.abc_grad_unpack_bf16(src.data_ptr(), dst.data_ptr(), n, stream()), "grad_unpack_bf16")
            got = dst.cpu().numpy()
            # exact: the NaNs' bits too
            assert np.array_equal(got.view(np.uint32), h.astype(np.uint32) << 16), (n, so, do)
            assert canaries_intact(buf, n, do), (n, so, do)


def test_bad_arguments_are_refused_and_nothing_is_launched():
    lib = L.load()
    n = 64
    _sb, src = dev_src(np.ones(n, dtype=np.float32), 0)
    _hb, hsrc = dev_src(X.bf16_rne(np.ones(2 * n, dtype=np.float32)), 0)
    buf, dst = dev_dst(n, 0, torch.int16)
    fbuf, fdst = dev_dst(n, 0, torch.float32)
    st = stream()
    calls = [
        ("n = 0", lambda: lib.abc_grad_pack_bf16(src.data_ptr(), dst.data_ptr(), 0, st)),
        ("n < 0", lambda: lib.abc_grad_pack_bf16(src.data_ptr(), dst.data_ptr(), -5, st)),
        ("null", lambda: lib.abc_grad_pack_bf16(None, dst.data_ptr(), n, st)),
        ("null", lambda: lib.abc_grad_pack_bf16(src.data_ptr(), None, n, st)),
        ("aligned", lambda: lib.abc_grad_pack_bf16(src.data_ptr() + 2, dst.data_ptr(), n - 1, st)),
        ("aligned", lambda: lib.abc_grad_pack_bf16(src.data_ptr(), dst.data_ptr() + 1, n - 1, st)),
        ("n = 0", lambda: lib.abc_grad_reduce_bf16(hsrc.data_ptr(), dst.data_ptr(), 2, 0, st)),
        ("W", lambda: lib.abc_grad_reduce_bf16(hsrc.data_ptr(), dst.data_ptr(), 0, n, st)),
        ("W", lambda: lib.abc_grad_reduce_bf16(hsrc.data_ptr(), dst.data_ptr(), 65, 1, st)),
        ("null", lambda: lib.abc_grad_reduce_bf16(None, dst.data_ptr(), 2, n, st)),
        ("null", lambda: lib.abc_grad_reduce_bf16(hsrc.data_ptr(), None, 2, n, st)),
        ("aligned", lambda: lib.abc_grad_reduce_bf16(hsrc.data_ptr() + 1, dst.data_ptr(), 2, n - 1, st)),
        ("n = 0", lambda: lib.abc_grad_unpack_bf16(hsrc.data_ptr(), fdst.data_ptr(), 0, st)),
        ("null", lambda: lib.abc_grad_unpack_bf16(None, fdst.data_ptr(), n, st)),
        ("null", lambda: lib.abc_grad_unpack_bf16(hsrc.data_ptr(), None, n, st)),
        ("aligned", lambda: lib.abc_grad_unpack_bf16(hsrc.data_ptr(), fdst.data_ptr() + 2, n - 1, st)),
    ]
    for what, call in calls:
        rc = call()
        assert rc != 0, what
        assert lib.abc_last_error().decode() != "", what
        with pytest.raises(L.AbcNetHipError):
            L.check(rc, what)
    torch.cuda.synchronize()
    # nothing ran: both destinations still hold nothing but canaries
    assert (dst.cpu().numpy().view(np.uint16) == CANARY_BF16).all() and canaries_intact(buf, n, 0)
    assert (fdst.cpu().numpy().view(np.uint32) == 0x4B1D4B1D).all() and canaries_intact(fbuf, n, 0)
    # W = 64, the largest world, is served
    w, m = 64, 9
    rows = reduce_rows(w, m, 64)
    _rb, rsrc = dev_src(rows.reshape(-1), 0)
    L.check(lib.abc_grad_reduce_bf16(rsrc.data_ptr(), dst.data_ptr(), w, m, st), "grad_reduce_bf16")
    assert X.same_bits(dst[:m].cpu().numpy().view(np.uint16), X.reduce_rows(rows))
