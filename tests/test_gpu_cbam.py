"""csrc/cbam.hip, every entry point on its own through the C ABI, against tests/cbam_oracle.py (plain f64; held to CPU torch
autograd by tests/test_cbam_host.py): hand-built inputs at small ragged maps, channel slices of wider tensors, both storage
dtypes, every channel count at which the kernels take another form (bf16 16: two vectors per pixel, the narrowest lane group;
f32 512 and bf16 1024: two vectors per lane), several workgroups per image and several passes per thread.

Two kinds of input: random ones for the arithmetic, and cbam_oracle.tie_case for the selections -- exact ties across lanes,
across the two vectors of a lane, across workgroups and inside 2x2 windows, on dyadic grids where every product and sum is
exact, so those comparisons are torch.equal.

Bounds (the project's, not measured here): f32 element-wise 2e-5 of the largest reference element, f32 reductions 1e-4 (as
test_unet2_block_is_exact_in_situ), bf16 outputs and their f32 partial sums U.tol(BF16) relative to max against the f64 oracle on
the stored inputs; integers and everything on the tie inputs exact.

Not covered here: the 4096 / B caps on the grids and the 512-workgroup persistent cap of the 7x7 backward exist only at full
size, where tests/test_gpu_insitu_fullsize.py holds them."""
import ctypes as C
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import abcnet_amd  # noqa: E402,F401
from abcnet_amd import _lib as L  # noqa: E402

import cbam_oracle as O  # noqa: E402
import hiputil as U  # noqa: E402

EINVAL, EUNSUPPORTED = -1, -2
I32MAX = 0x7FFFFFFF
DT_C = [(L.F32, 32), (L.F32, 128), (L.F32, 512), (L.BF16, 16), (L.BF16, 32), (L.BF16, 128), (L.BF16, 512)]
MAPS = [(9, 11), (18, 9), (17, 33), (24, 40)]
BS = [1, 3]
FILL = 7.0


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "these tests need an MI355X"
    return L.load()


def nvec(dt):
    return 8 if dt == L.BF16 else 4


def f32(t):
    return t.float().to(U.DEV).contiguous()


def stored(t, dt):
    return t.to(U.tdt(dt)).to(U.DEV).contiguous()


def wide(t, dt, pad):
    """[..., C] -> (device tensor, ld, channel offset): plain, or a slice of a tensor two vectors wider that is filled with FILL"""
    Cc = t.shape[-1]
    if not pad:
        return stored(t, dt), Cc, 0
    N = nvec(dt)
    full = torch.full(tuple(t.shape[:-1]) + (Cc + 2 * N,), FILL, dtype=U.tdt(dt), device=U.DEV)
    full[..., N:N + Cc] = t.to(U.tdt(dt)).to(U.DEV)
    return full, Cc + 2 * N, N


def fill(d, **kw):
    """set descriptor fields; tensors go in by address and are kept alive on the descriptor"""
    names = {f[0] for f in d._fields_}
    keep = d.__dict__.setdefault("t", {})
    for k, v in kw.items():
        assert k in names, k
        if torch.is_tensor(v):
            keep[k] = v
            v = v.data_ptr()
        setattr(d, k, v)
    return d


def pix(dt, B, H, W, Cc, **kw):
    return fill(L.CbamPixDesc(), dtype=dt, B=B, H=H, W=W, C=Cc, **kw)


def run(fn, *descs, what=""):
    L.check(fn(*[C.byref(d) for d in descs], U.stream()), what)
    torch.cuda.synchronize()


def close(got, ref, dt, reduction=False, what=""):
    bound = U.tol(L.BF16) if dt == L.BF16 else (1e-4 if reduction else 2e-5)
    ref = ref.double().cpu()
    err = (got.double().cpu() - ref).abs().max().item()
    assert err <= bound * ref.abs().max().item() + 1e-30, (what, err, ref.abs().max().item())


def same(got, ref, what=""):
    """bit-for-value equality with the f64 oracle (the tie inputs: every result is exact in the output's format)"""
    assert torch.equal(got.double().cpu(), ref.double().cpu()), (what, (got.double().cpu() - ref.double().cpu()).abs().max().item())


def check(got, ref, dt, kind, **kw):
    if kind == "tie":
        same(got, ref, kw.get("what", ""))
    else:
        close(got, ref, dt, **kw)


@functools.lru_cache(maxsize=2)
def case(kind, dt, B, H, W, Cc):
    """f64 tensors holding what the kernels will read (already rounded to the storage dtype / to f32); never modified"""
    if kind == "tie":
        return O.tie_case(B, H, W, Cc)
    g = torch.Generator().manual_seed(1000 * Cc + 10 * H + B + (7 if dt == L.BF16 else 0))
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    q = lambda x: x.to(U.tdt(dt)).double()
    f = lambda x: x.float().double()
    t = dict(y=q(r(B, H, W, Cc)), scale=f(r(Cc)), shift=f(r(Cc) * 0.3), mean=f(r(Cc) * 0.2), invstd=f(r(Cc).abs() + 0.5),
             ca=f(torch.sigmoid(r(B, Cc))), sa=f(torch.sigmoid(r(B, H, W))), res=q(r(B, H, W, Cc)), out=q(torch.relu(r(B, H, W, Cc))),
             d_same=q(r(B, H, W, Cc)), d_pool=q(r(B, H // 2, W // 2, Cc)), dst=f(r(B, H, W, 2)), d_o1=q(r(B, H, W, Cc)),
             d_avgz=f(r(B, Cc)), d_maxz=f(r(B, Cc)))
    t["g"] = q(t["d_same"] * (t["out"] > 0))
    assert (t["scale"] > 0).any() and (t["scale"] < 0).any()
    return t


def res2(kind, dt, B, H, W, Cc):
    """a residual at twice the resolution"""
    if kind == "tie":
        return O.tie_res(B, 2 * H, 2 * W, Cc)
    g = torch.Generator().manual_seed(Cc + H)
    return torch.randn(B, 2 * H, 2 * W, Cc, generator=g, dtype=torch.float64).to(U.tdt(dt)).double()


cases = pytest.mark.parametrize("kind", ["rand", "tie"])
shapes = lambda f: pytest.mark.parametrize("dt,Cc", DT_C)(pytest.mark.parametrize("B", BS)(pytest.mark.parametrize("H,W", MAPS)(f)))


# ------------------------------------------------------------------ channel attention, forward
T_MAP = {1: (9, 11), 15: (9, 11), 16: (9, 11), 17: (18, 9), 48: (18, 9), 49: (18, 9), 64: (17, 33), 65: (17, 33), 100: (24, 40)}


def _channel_fwd_inputs(T, Cc, mid, B):
    H, W = T_MAP[T]
    g = torch.Generator().manual_seed(T * 1000 + Cc + B)
    r = lambda *s: torch.randn(*s, generator=g).double()
    y = r(B, H, W, Cc)
    y[:, 1::3, ::2] = y[:, :1, :1]       # the pools' extreme values sit in several chunks
    scale, shift = r(Cc), r(Cc) * 0.3
    # (one or two hidden units: biased to be alive in every image -- behind a ReLU zero a wrong dot product does not show)
    few = mid <= 2
    w1, b1, w2, b2 = r(mid, Cc) / Cc ** 0.5, r(mid) * 0.5 + 1.0, r(Cc, mid) / (8.0 if few else 1.0), r(Cc) * 0.2
    if few:
        pools = O.channel_fwd(y, scale, shift, w1, b1, w2, b2)
        pre = torch.cat([pools["avgz"] @ w1.t(), pools["maxz"] @ w1.t()])
        b1 = (1.0 - pre.min(0)[0].clamp(max=0.0)).float().double()
    part = O.conv_partials(y, T)
    assert part.shape == (B * T, 4, Cc)
    ref = O.channel_fwd(y, scale, shift, w1, b1, w2, b2)
    alive_a, alive_m = ref["hid_avg"] > 0, ref["hid_max"] > 0
    assert (alive_a.all() and alive_m.all()) if few else (alive_a.any() and alive_m.any())
    return H, W, y, scale, shift, w1, b1, w2, b2, part, ref


@pytest.mark.parametrize("T", sorted(T_MAP))
@pytest.mark.parametrize("Cc,mid", [(16, 1), (32, 2), (128, 8), (512, 32), (128, 2), (256, 1)])
@pytest.mark.parametrize("B", BS)
def test_channel_fwd(lib, T, Cc, mid, B):
    """abc_cbam_channel_fwd from synthesised conv partials [B*T][4][C]: T on both sides of the 16 tile groups and of the 4 x 16
    unrolled round; mid = C / 16 as the model has it, and (128, 2), (256, 1): a hidden unit shared by more lanes than a wave"""
    H, W, y, scale, shift, w1, b1, w2, b2, part, ref = _channel_fwd_inputs(T, Cc, mid, B)
    outs = {k: torch.full(s, float("nan"), device=U.DEV) for k, s in
            (("ca", (B, Cc)), ("avgz", (B, Cc)), ("maxz", (B, Cc)), ("ext", (B, Cc)), ("hid_avg", (B, mid)), ("hid_max", (B, mid)))}
    first = torch.zeros((B, Cc), dtype=torch.int32, device=U.DEV)
    d = fill(L.CbamChannelDesc(), partial=f32(part), tiles_per_img=T, B=B, C=Cc, mid=mid, HW=float(H * W), scale=f32(scale), shift=f32(shift),
             w1=f32(w1), b1=f32(b1), w2=f32(w2), b2=f32(b2), first=first, **outs)
    run(lib.abc_cbam_channel_fwd, d, what="channel_fwd")
    same(outs["ext"], ref["ext"].float(), "ext")
    assert (first == I32MAX).all()
    close(outs["avgz"], ref["avgz"], L.F32, reduction=True, what="avgz")
    close(outs["maxz"], ref["maxz"], L.F32, what="maxz")
    close(outs["hid_avg"], ref["hid_avg"], L.F32, reduction=True, what="hid_avg")
    close(outs["hid_max"], ref["hid_max"], L.F32, reduction=True, what="hid_max")
    close(outs["ca"], ref["ca"], L.F32, what="ca")


# ------------------------------------------------------------------ per-pixel passes, forward
@cases
@shapes
def test_spatial_stats(lib, kind, dt, Cc, B, H, W):
    """abc_cbam_spatial_stats: [mean, max] over channels, the FIRST channel holding the max (in-lane, across the two vectors of a lane,
    across lanes), and `first` lowered to the first pixel holding the channel's extreme raw value (across workgroups, both signs of
    scale); B = 3 reads y as a channel slice of a wider tensor"""
    t = case(kind, dt, B, H, W, Cc)
    yd, ld_y, cy = wide(t["y"], dt, B == 3)
    ext, first_ref = O.first_extreme(t["y"], t["scale"])
    st = torch.full((B, H, W, 2), float("nan"), device=U.DEV)
    amax = torch.full((B, H, W), -1, dtype=torch.int32, device=U.DEV)
    first = torch.full((B, Cc), I32MAX, dtype=torch.int32, device=U.DEV)
    d = pix(dt, B, H, W, Cc, y=yd, ld_y=ld_y, cy_off=cy, scale=f32(t["scale"]), shift=f32(t["shift"]), ca=f32(t["ca"]), ext=f32(ext),
            first=first, st=st, amax=amax)
    run(lib.abc_cbam_spatial_stats, d, what="spatial_stats")
    st_ref, amax_ref = O.spatial_stats(t["y"], t["scale"], t["shift"], t["ca"])
    assert torch.equal(first.cpu().long(), first_ref)
    check(st[..., 0], st_ref[..., 0], dt, kind, reduction=True, what="mean")
    check(st[..., 1], st_ref[..., 1], dt, kind, what="max")
    if kind == "tie":
        assert torch.equal(amax.cpu().long(), amax_ref)
    else:
        # (f32 rounding may order two channels that differ by less than an ulp the other way: the channel named holds the maximum)
        o1 = O.o1_of(t["y"], t["scale"], t["shift"], t["ca"])
        a = amax.cpu().long()
        assert int(a.min()) >= 0 and int(a.max()) < Cc
        at = o1.gather(-1, a[..., None])[..., 0]
        assert (st_ref[..., 1] - at).abs().max().item() <= 2e-6 * st_ref[..., 1].abs().max().item()
        assert (a == amax_ref).float().mean().item() > 0.999


@cases
@pytest.mark.parametrize("B", BS)
def test_spatial_stats_bf16_two_vectors_per_lane(lib, kind, B):
    """bf16 with 1024 channels: 128 vectors per pixel, the <bf16, 2> form of the kernel (the model stops at 512)"""
    test_spatial_stats(lib, kind, L.BF16, 1024, B, 9, 11)


@cases
@pytest.mark.parametrize("pool", [False, True])
@shapes
def test_apply_fwd(lib, kind, pool, dt, Cc, B, H, W):
    """abc_cbam_apply_fwd: relu(sa * ca * z + r) with an identity residual or the 2x2 max-pool of a 2H x 2W tensor, written into a
    channel slice of a wider, pre-filled tensor whose other channels stay untouched"""
    t = case(kind, dt, B, H, W, Cc)
    res = res2(kind, dt, B, H, W, Cc) if pool else t["res"]
    yd, ld_y, cy = wide(t["y"], dt, B == 3)
    rd, ld_r, cr = wide(res, dt, B == 1)
    N = nvec(dt)
    out = torch.full((B, H, W, Cc + 3 * N), FILL, dtype=U.tdt(dt), device=U.DEV)
    d = pix(dt, B, H, W, Cc, y=yd, ld_y=ld_y, cy_off=cy, scale=f32(t["scale"]), shift=f32(t["shift"]), ca=f32(t["ca"]), sa=f32(t["sa"]),
            res=rd, ld_res=ld_r, cres_off=cr, res_pool=int(pool), out=out, ld_out=Cc + 3 * N, cout_off=2 * N)
    run(lib.abc_cbam_apply_fwd, d, what="apply_fwd")
    ref = O.apply_fwd(t["y"], t["scale"], t["shift"], t["ca"], t["sa"], res, pool)
    check(out[..., 2 * N:2 * N + Cc], ref, dt, kind, what="out")
    assert (out[..., :2 * N] == FILL).all() and (out[..., 2 * N + Cc:] == FILL).all()
    assert float(ref.max()) > 0 and float((ref == 0).double().mean()) > 0.05


# ------------------------------------------------------------------ per-pixel passes, backward
@cases
@pytest.mark.parametrize("src", ["same", "pool", "both"])
@shapes
def test_bwd1(lib, kind, src, dt, Cc, B, H, W):
    """abc_cbam_bwd1: g = (d_same + unpool(d_pool)) * [out > 0] and du, for the three combinations of gradient sources (the other
    pointer null); the pooled gradient goes to the FIRST maximum of its window of `out`, an odd last row / column gets none"""
    t = case(kind, dt, B, H, W, Cc)
    d_same = t["d_same"] if src != "pool" else None
    d_pool = t["d_pool"] if src != "same" else None
    yd, ld_y, cy = wide(t["y"], dt, B == 3)
    od, ld_o, co = wide(t["out"], dt, B == 3)
    g = torch.full((B, H, W, Cc), FILL, dtype=U.tdt(dt), device=U.DEV)
    du = torch.full((B, H, W), float("nan"), device=U.DEV)
    d = pix(dt, B, H, W, Cc, y=yd, ld_y=ld_y, cy_off=cy, scale=f32(t["scale"]), shift=f32(t["shift"]), ca=f32(t["ca"]), sa=f32(t["sa"]),
            out=od, ld_out=ld_o, cout_off=co, g=g, ld_g=Cc, du=du)
    if d_same is not None:
        sd, ld_s, cs = wide(d_same, dt, B == 1)
        fill(d, d_same=sd, ld_same=ld_s, csame_off=cs)
    if d_pool is not None:
        pd, ld_p, cp = wide(d_pool, dt, B == 3)
        fill(d, d_pool=pd, ld_pool=ld_p, cpool_off=cp)
    run(lib.abc_cbam_bwd1, d, what="bwd1")
    g_ref, du_ref = O.bwd1(t["y"], t["scale"], t["shift"], t["ca"], t["sa"], t["out"], d_same, d_pool)
    check(g, g_ref, dt, kind, what="g")
    check(du, du_ref, dt, kind, reduction=True, what="du")
    if src == "pool":
        assert float(g[:, 2 * (H // 2):].float().abs().sum()) == 0 and float(g[:, :, 2 * (W // 2):].float().abs().sum()) == 0
    assert float(g_ref.abs().sum()) > 0


@cases
@pytest.mark.parametrize("src", ["same", "pool", "both"])
@pytest.mark.parametrize("B", BS)
def test_bwd1_bf16_two_vectors_per_lane(lib, kind, src, B):
    """bf16 with 1024 channels: the <bf16, 2> form of the kernel"""
    test_bwd1(lib, kind, src, L.BF16, 1024, B, 9, 11)


@cases
@shapes
def test_bwd2(lib, kind, dt, Cc, B, H, W):
    """abc_cbam_bwd2: d_o1 = g * sa + d_mean / C + [c == amax] * d_max, and the d_ca partials [B][blocks][C] summed over the
    workgroups"""
    t = case(kind, dt, B, H, W, Cc)
    _, amax = O.spatial_stats(t["y"], t["scale"], t["shift"], t["ca"])
    yd, ld_y, cy = wide(t["y"], dt, B == 3)
    dz = torch.full((B, H, W, Cc), FILL, dtype=U.tdt(dt), device=U.DEV)
    d = pix(dt, B, H, W, Cc, y=yd, ld_y=ld_y, cy_off=cy, scale=f32(t["scale"]), shift=f32(t["shift"]), sa=f32(t["sa"]), dst=f32(t["dst"]),
            amax=amax.int().to(U.DEV), g=stored(t["g"], dt), ld_g=Cc, dz=dz, ld_dz=Cc)
    nb = lib.abc_cbam_bwd2_blocks(C.byref(d))
    assert 1 <= nb <= 128
    part = torch.full((B, nb, Cc), float("nan"), device=U.DEV)
    fill(d, partial=part)
    run(lib.abc_cbam_bwd2, d, what="bwd2")
    dz_ref, dca_ref = O.bwd2(t["y"], t["scale"], t["shift"], t["g"], t["sa"], t["dst"], amax)
    check(dz, dz_ref, dt, kind, what="d_o1")
    check(part.double().sum(1), dca_ref, dt, kind, reduction=True, what="d_ca")


@cases
@shapes
def test_bwd3(lib, kind, dt, Cc, B, H, W):
    """abc_cbam_bwd3: d_z = d_o1 * ca + d_avgz / HW + [pixel == first] * d_maxz in place, and the BatchNorm rows (sum d_z,
    sum d_z * xhat) summed over the workgroups; d_maxz lands on exactly one pixel per (image, channel): the first"""
    t = case(kind, dt, B, H, W, Cc)
    _, first = O.first_extreme(t["y"], t["scale"])
    yd, ld_y, cy = wide(t["y"], dt, B == 3)
    dz = stored(t["d_o1"], dt)
    d = pix(dt, B, H, W, Cc, y=yd, ld_y=ld_y, cy_off=cy, mean=f32(t["mean"]), invstd=f32(t["invstd"]), ca=f32(t["ca"]), d_avgz=f32(t["d_avgz"]),
            d_maxz=f32(t["d_maxz"]), first=first.int().to(U.DEV), dz=dz, ld_dz=Cc)
    nb = lib.abc_cbam_bwd3_blocks(C.byref(d))
    assert nb >= B and nb % B == 0
    part = torch.full((nb, 2, Cc), float("nan"), device=U.DEV)
    fill(d, partial=part)
    run(lib.abc_cbam_bwd3, d, what="bwd3")
    dz_ref, rows_ref = O.bwd3(t["y"], t["mean"], t["invstd"], t["d_o1"], t["ca"], t["d_avgz"], t["d_maxz"], first)
    check(dz, dz_ref, dt, kind, what="d_z")
    check(part.double().sum(0), rows_ref, dt, kind, reduction=True, what="BatchNorm rows")
    if kind == "tie":
        # what is left after the other two terms is d_maxz at the first extreme pixel and nothing anywhere else
        rest = dz.double().cpu() - t["d_o1"] * t["ca"][:, None, None, :] - t["d_avgz"][:, None, None, :] / (H * W)
        hit = torch.arange(H * W).view(1, H, W, 1) == first[:, None, None, :]
        assert torch.equal(rest, hit.double() * t["d_maxz"][:, None, None, :])
        assert float((t["d_maxz"] != 0).double().mean()) > 0.5


# ------------------------------------------------------------------ channel attention, backward (+ the 7x7 reduction riding along)
def _conv7(lib, B, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    st, du = torch.randn(B, H, W, 2, generator=g), torch.randn(B, H, W, generator=g)
    w7, b7 = torch.randn(98, generator=g) * 0.1, torch.randn(1, generator=g)
    d = fill(L.CbamConv7Desc(), st=f32(st), w7=f32(w7), b7=f32(b7), du=f32(du), dst=torch.empty(B, H, W, 2, device=U.DEV), B=B, H=H, W=W,
             sa=torch.full((B, H, W), float("nan"), device=U.DEV))
    nb = lib.abc_cbam_conv7_blocks(C.byref(d))
    return fill(d, dw_partial=torch.full((nb, 99), float("nan"), device=U.DEV), dw7=torch.full((98,), float("nan"), device=U.DEV),
                db7=torch.full((1,), float("nan"), device=U.DEV))


def _bwd2_tiles(lib, dt, B, H, W, Cc):
    return lib.abc_cbam_bwd2_blocks(C.byref(pix(dt, B, H, W, Cc)))


CH_BWD = [(Cc, Cc // 16, ("blocks", dt, H, W)) for dt, Cc in DT_C for H, W in ((9, 11), (24, 40))] + \
         [(Cc, Cc // 16, T) for Cc in (32, 512) for T in (1, 7, 8, 9, 64, 65, 15, 16, 17, 225, 256, 257)] + [(128, 2, 9), (256, 1, 17)]


@pytest.mark.parametrize("Cc,mid,T", CH_BWD)
@pytest.mark.parametrize("B", BS)
def test_channel_bwd_both_forms(lib, Cc, mid, T, B):
    """abc_cbam_channel_bwd and abc_cbam_channel_bwd_c7 (the form the engine uses) against the oracle and bit-equal to each other;
    the 7x7 weight / bias gradients that the _c7 form reduces from abc_cbam_conv7_bwd_partial's partials are bit-identical to
    abc_cbam_conv7_bwd's own.  T = abc_cbam_bwd2_blocks of a real map, and synthetic tile counts around the unrolled 8 x KG rounds
    (KG = 32 tile groups at 32 channels: 225 / 256 / 257; KG = 2 at 512: 15 / 16 / 17)"""
    H7, W7 = (24, 40) if B == 1 else (9, 51)      # (one pixel per thread; four from 48 columns up)
    if isinstance(T, tuple):
        _, dt, H, W = T
        T = _bwd2_tiles(lib, dt, B, H, W, Cc)
    g = torch.Generator().manual_seed(Cc * 7 + T + B)
    r = lambda *s: torch.randn(*s, generator=g).double()
    part = r(B * T, Cc)
    ca, ha, hm = torch.sigmoid(r(B, Cc)).float().double(), torch.relu(r(B, mid)), torch.relu(r(B, mid) + 0.3)
    avgz, maxz, w1, w2 = r(B, Cc), r(B, Cc), r(mid, Cc) / Cc ** 0.5, r(Cc, mid)
    ref = O.channel_bwd(part.float().double().view(B, T, Cc).sum(1), ca, ha, hm, avgz, maxz, w1, w2)
    shapes_ = dict(dw1=(mid, Cc), db1=(mid,), dw2=(Cc, mid), db2=(Cc,), d_avgz=(B, Cc), d_maxz=(B, Cc))

    def go(c7):
        outs = {k: torch.full(s, float("nan"), device=U.DEV) for k, s in shapes_.items()}
        d = fill(L.CbamChannelDesc(), partial=f32(part), tiles_per_img=T, B=B, C=Cc, mid=mid, HW=float(99), ca=f32(ca), hid_avg=f32(ha),
                 hid_max=f32(hm), avgz=f32(avgz), maxz=f32(maxz), w1=f32(w1), w2=f32(w2),
                 work=torch.full((B * (Cc + 2 * mid),), float("nan"), device=U.DEV), **outs)
        if c7 is None:
            run(lib.abc_cbam_channel_bwd, d, what="channel_bwd")
        else:
            run(lib.abc_cbam_channel_bwd_c7, d, c7, what="channel_bwd_c7")
        return outs

    c7a, c7b = _conv7(lib, B, H7, W7, 5), _conv7(lib, B, H7, W7, 5)
    run(lib.abc_cbam_conv7_fwd, c7a, what="conv7_fwd")      # (sa itself: test_gpu_kernels.py holds it over more shapes)
    pre = F.conv2d(c7a.t["st"].cpu().double().permute(0, 3, 1, 2), c7a.t["w7"].cpu().double().view(1, 2, 7, 7), c7a.t["b7"].cpu().double(), padding=3)
    close(c7a.t["sa"], torch.sigmoid(pre)[:, 0], L.F32, what="sa")
    run(lib.abc_cbam_conv7_bwd, c7a, what="conv7_bwd")
    run(lib.abc_cbam_conv7_bwd_partial, c7b, what="conv7_bwd_partial")
    assert torch.isnan(c7b.t["dw7"]).all()      # (not reduced yet)
    plain, fused = go(None), go(c7b)
    for k in shapes_:
        close(plain[k], ref[k], L.F32, reduction=True, what=k)
        assert torch.equal(plain[k], fused[k]), k
    for k in ("dw_partial", "dw7", "db7", "dst"):
        assert torch.equal(c7a.t[k], c7b.t[k]) and not torch.isnan(c7a.t[k]).any(), k


# ------------------------------------------------------------------ abc_add_into
@pytest.mark.parametrize("dt", [L.F32, L.BF16])
def test_add_into_slices(lib, dt):
    """dst[.., cdst_off + c] += src[.., csrc_off + c] with slices on both sides; an offset that is no multiple of the vector is refused"""
    N, Cc, npix = nvec(dt), 32, 3 * 17 * 33
    g = torch.Generator().manual_seed(3)
    a = torch.randn(npix, Cc + 3 * N, generator=g).to(U.tdt(dt)).to(U.DEV)
    b = torch.randn(npix, Cc + 2 * N, generator=g).to(U.tdt(dt)).to(U.DEV)
    want = a.clone()
    want[:, 2 * N:2 * N + Cc] = (a[:, 2 * N:2 * N + Cc].float() + b[:, N:N + Cc].float()).to(U.tdt(dt))
    args = lambda co: (a.data_ptr(), Cc + 3 * N, co, b.data_ptr(), Cc + 2 * N, N, Cc, npix, dt, U.stream())
    assert lib.abc_add_into(*args(2 * N + 2)) == EINVAL and b"alignment" in lib.abc_last_error()
    torch.cuda.synchronize()
    L.check(lib.abc_add_into(*args(2 * N)), "add_into")
    torch.cuda.synchronize()
    assert torch.equal(a, want)


# ------------------------------------------------------------------ refusals
def _full_pix(dt, B, H, W, Cc):
    """a descriptor with every buffer present and large enough for the stated shape"""
    z = lambda *s, dtype=torch.float32: torch.zeros(*s, dtype=dtype, device=U.DEV)
    s = U.tdt(dt)
    return pix(dt, B, H, W, Cc, y=z(B, H, W, Cc, dtype=s), ld_y=Cc, scale=z(Cc), shift=z(Cc), mean=z(Cc), invstd=z(Cc), ca=z(B, Cc), maxz=z(B, Cc),
               d_avgz=z(B, Cc), d_maxz=z(B, Cc), sa=z(B, H, W), st=z(B, H, W, 2), amax=z(B, H, W, dtype=torch.int32), du=z(B, H, W),
               dst=z(B, H, W, 2), res=z(B, H, W, Cc, dtype=s), ld_res=Cc, out=z(B, H, W, Cc, dtype=s), ld_out=Cc,
               d_same=z(B, H, W, Cc, dtype=s), ld_same=Cc, g=z(B, H, W, Cc, dtype=s), ld_g=Cc, dz=z(B, H, W, Cc, dtype=s), ld_dz=Cc,
               partial=z(64, 2, Cc), ext=z(B, Cc), first=z(B, Cc, dtype=torch.int32))


PIX_ENTRIES = ["abc_cbam_spatial_stats", "abc_cbam_apply_fwd", "abc_cbam_bwd1", "abc_cbam_bwd2", "abc_cbam_bwd3"]


def test_shapes_the_kernels_cannot_serve_are_refused(lib):
    """by return code, before any launch: C no multiple of the vector, C / vector not dividing 256, more than 128 vectors per pixel for
    the lanes-per-pixel kernels, and the missing ext / first / work pointers"""
    def refused(fn, code, word, *descs):
        assert fn(*[C.byref(d) if d is not None else None for d in descs], U.stream()) == code
        assert word in lib.abc_last_error(), lib.abc_last_error()

    for name in PIX_ENTRIES:
        fn = getattr(lib, name)
        refused(fn, EINVAL, b"multiple of the vector", _full_pix(L.F32, 1, 4, 4, 18))
        refused(fn, EINVAL, b"multiple of the vector", _full_pix(L.BF16, 1, 4, 4, 20))
        refused(fn, EUNSUPPORTED, b"divide 256", _full_pix(L.F32, 1, 4, 4, 48))
        refused(fn, EUNSUPPORTED, b"divide 256", _full_pix(L.BF16, 1, 4, 4, 4096))
    for name in ("abc_cbam_spatial_stats", "abc_cbam_bwd1"):
        refused(getattr(lib, name), EUNSUPPORTED, b"128 channel vectors", _full_pix(L.F32, 1, 2, 2, 1024))
        refused(getattr(lib, name), EUNSUPPORTED, b"128 channel vectors", _full_pix(L.BF16, 1, 2, 2, 2048))
    for field in ("ext", "first"):
        d = _full_pix(L.F32, 1, 4, 4, 32)
        setattr(d, field, None)
        refused(lib.abc_cbam_spatial_stats, EINVAL, b"ext / first", d)
    d = _full_pix(L.F32, 1, 4, 4, 32)
    d.first = None
    refused(lib.abc_cbam_bwd3, EINVAL, b"first", d)
    z = lambda *s, dtype=torch.float32: torch.zeros(*s, dtype=dtype, device=U.DEV)

    def chan(**kw):
        B, Cc, mid = 1, 32, 2
        d = fill(L.CbamChannelDesc(), partial=z(4, 4, Cc), tiles_per_img=1, B=B, C=Cc, mid=mid, HW=16.0, scale=z(Cc), shift=z(Cc), w1=z(mid, Cc),
                 b1=z(mid), w2=z(Cc, mid), b2=z(Cc), ca=z(B, Cc), avgz=z(B, Cc), maxz=z(B, Cc), hid_avg=z(B, 64), hid_max=z(B, 64), dw1=z(64, Cc),
                 db1=z(64), dw2=z(Cc, 64), db2=z(Cc), d_avgz=z(B, Cc), d_maxz=z(B, Cc), work=z(B * (Cc + 128)), ext=z(B, Cc),
                 first=z(B, Cc, dtype=torch.int32))
        for k, v in kw.items():
            setattr(d, k, v)
        return d

    refused(lib.abc_cbam_channel_fwd, EINVAL, b"ext / first", chan(ext=None))
    refused(lib.abc_cbam_channel_fwd, EINVAL, b"ext / first", chan(first=None))
    refused(lib.abc_cbam_channel_bwd, EINVAL, b"work", chan(work=None))
    c7 = _conv7(lib, 1, 9, 11, 1)
    refused(lib.abc_cbam_channel_bwd_c7, EINVAL, b"work", chan(work=None), c7)
    refused(lib.abc_cbam_channel_bwd_c7, EINVAL, b"partials and gradient pointers", chan(), None)
    for field in ("dw_partial", "dw7", "db7"):
        c7 = _conv7(lib, 1, 9, 11, 1)
        setattr(c7, field, None)
        refused(lib.abc_cbam_channel_bwd_c7, EINVAL, b"partials and gradient pointers", chan(), c7)
    for mid in (0, 3, 64):
        for fn in (lib.abc_cbam_channel_fwd, lib.abc_cbam_channel_bwd):
            refused(fn, EUNSUPPORTED, b"power of two", chan(mid=mid))
    torch.cuda.synchronize()
