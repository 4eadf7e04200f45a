"""tests/cbam_oracle.py against CPU torch autograd of the reference formulation of unet2's CBAM + residual block (unet2.py:6-74, as
quoted in test_gpu_model.py::test_unet2_block_is_exact_in_situ: F.adaptive_avg_pool2d / F.adaptive_max_pool2d, torch.mean /
torch.max over dim 1, F.max_pool2d, the BatchNorm affine), on inputs full of exact ties.  This is what ties the oracle's
hand-written "first maximum" rules to what torch does; tests/test_gpu_cbam.py then holds the kernels to the oracle alone.

On the tie inputs (cbam_oracle.tie_case) every product and sum is exact, so every comparison is torch.equal; the chain test
at the end runs the whole block on random MLP weights and compares the sums to 1e-12.  No GPU needed."""
import pytest
import torch
import torch.nn.functional as F

import cbam_oracle as O

# (bf16 storage?, C, B, H, W) -> the ties the input holds (cbam_oracle.tie_counts; asserted below, so the numbers are the input's):
#   lanes  : pixels whose channel arg-max is tied across two lanes of a pixel's lane group      (cbam_spatial_stats_kernel's merge)
#   vectors: ... across the two vectors of one lane (the NVL = 2 form: f32 at 512 channels, bf16 at 1024)
#   groups : (image, channel) pairs whose extreme raw value sits in pixels of two workgroups      (atomicMin into `first`)
#   window : (2x2 window, channel) pairs of `out` holding four equal positive values              (cbam_bwd1_kernel's pool rule)
# The table is generated: after a change to cbam_oracle.tie_case, `python tests/test_cbam_host.py` prints it anew (_print_table below).
TIE_COUNTS = {
    (False, 32, 1, 9, 11): dict(lanes=31, vectors=0, groups=0, window=128),   # 1 workgroup(s) per image, 99 pixels
    (False, 32, 1, 18, 9): dict(lanes=56, vectors=0, groups=16, window=226),   # 2 workgroup(s) per image, 162 pixels
    (False, 32, 1, 17, 33): dict(lanes=228, vectors=0, groups=32, window=832),   # 5 workgroup(s) per image, 561 pixels
    (False, 32, 1, 24, 40): dict(lanes=383, vectors=0, groups=32, window=1545),   # 8 workgroup(s) per image, 960 pixels
    (False, 32, 3, 9, 11): dict(lanes=112, vectors=0, groups=0, window=384),   # 1 workgroup(s) per image, 297 pixels
    (False, 32, 3, 18, 9): dict(lanes=184, vectors=0, groups=48, window=674),   # 2 workgroup(s) per image, 486 pixels
    (False, 32, 3, 17, 33): dict(lanes=668, vectors=0, groups=96, window=2496),   # 5 workgroup(s) per image, 1683 pixels
    (False, 32, 3, 24, 40): dict(lanes=1124, vectors=0, groups=96, window=4636),   # 8 workgroup(s) per image, 2880 pixels
    (False, 128, 1, 9, 11): dict(lanes=67, vectors=0, groups=78, window=512),   # 4 workgroup(s) per image, 99 pixels
    (False, 128, 1, 18, 9): dict(lanes=108, vectors=0, groups=58, window=901),   # 6 workgroup(s) per image, 162 pixels
    (False, 128, 1, 17, 33): dict(lanes=367, vectors=0, groups=104, window=3328),   # 18 workgroup(s) per image, 561 pixels
    (False, 128, 1, 24, 40): dict(lanes=622, vectors=0, groups=128, window=6176),   # 30 workgroup(s) per image, 960 pixels
    (False, 128, 3, 9, 11): dict(lanes=196, vectors=0, groups=234, window=1537),   # 4 workgroup(s) per image, 297 pixels
    (False, 128, 3, 18, 9): dict(lanes=319, vectors=0, groups=174, window=2701),   # 6 workgroup(s) per image, 486 pixels
    (False, 128, 3, 17, 33): dict(lanes=1088, vectors=0, groups=312, window=9984),   # 18 workgroup(s) per image, 1683 pixels
    (False, 128, 3, 24, 40): dict(lanes=1858, vectors=0, groups=384, window=18534),   # 30 workgroup(s) per image, 2880 pixels
    (False, 512, 1, 9, 11): dict(lanes=73, vectors=25, groups=462, window=2050),   # 7 workgroup(s) per image, 99 pixels
    (False, 512, 1, 18, 9): dict(lanes=120, vectors=41, groups=430, window=3608),   # 11 workgroup(s) per image, 162 pixels
    (False, 512, 1, 17, 33): dict(lanes=414, vectors=141, groups=258, window=13312),   # 36 workgroup(s) per image, 561 pixels
    (False, 512, 1, 24, 40): dict(lanes=707, vectors=240, groups=160, window=24707),   # 60 workgroup(s) per image, 960 pixels
    (False, 512, 3, 9, 11): dict(lanes=216, vectors=75, groups=1385, window=6152),   # 7 workgroup(s) per image, 297 pixels
    (False, 512, 3, 18, 9): dict(lanes=353, vectors=123, groups=1287, window=10823),   # 11 workgroup(s) per image, 486 pixels
    (False, 512, 3, 17, 33): dict(lanes=1230, vectors=423, groups=774, window=39936),   # 36 workgroup(s) per image, 1683 pixels
    (False, 512, 3, 24, 40): dict(lanes=2112, vectors=721, groups=480, window=74121),   # 60 workgroup(s) per image, 2880 pixels
    (True, 16, 1, 9, 11): dict(lanes=35, vectors=0, groups=0, window=64),   # 1 workgroup(s) per image, 99 pixels
    (True, 16, 1, 18, 9): dict(lanes=56, vectors=0, groups=0, window=114),   # 1 workgroup(s) per image, 162 pixels
    (True, 16, 1, 17, 33): dict(lanes=194, vectors=0, groups=16, window=416),   # 2 workgroup(s) per image, 561 pixels
    (True, 16, 1, 24, 40): dict(lanes=327, vectors=0, groups=16, window=768),   # 2 workgroup(s) per image, 960 pixels
    (True, 16, 3, 9, 11): dict(lanes=102, vectors=0, groups=0, window=192),   # 1 workgroup(s) per image, 297 pixels
    (True, 16, 3, 18, 9): dict(lanes=170, vectors=0, groups=0, window=338),   # 1 workgroup(s) per image, 486 pixels
    (True, 16, 3, 17, 33): dict(lanes=580, vectors=0, groups=48, window=1248),   # 2 workgroup(s) per image, 1683 pixels
    (True, 16, 3, 24, 40): dict(lanes=985, vectors=0, groups=48, window=2306),   # 2 workgroup(s) per image, 2880 pixels
    (True, 32, 1, 9, 11): dict(lanes=30, vectors=0, groups=0, window=128),   # 1 workgroup(s) per image, 99 pixels
    (True, 32, 1, 18, 9): dict(lanes=52, vectors=0, groups=0, window=226),   # 1 workgroup(s) per image, 162 pixels
    (True, 32, 1, 17, 33): dict(lanes=189, vectors=0, groups=32, window=832),   # 3 workgroup(s) per image, 561 pixels
    (True, 32, 1, 24, 40): dict(lanes=316, vectors=0, groups=32, window=1545),   # 4 workgroup(s) per image, 960 pixels
    (True, 32, 3, 9, 11): dict(lanes=98, vectors=0, groups=0, window=384),   # 1 workgroup(s) per image, 297 pixels
    (True, 32, 3, 18, 9): dict(lanes=163, vectors=0, groups=0, window=674),   # 1 workgroup(s) per image, 486 pixels
    (True, 32, 3, 17, 33): dict(lanes=568, vectors=0, groups=96, window=2496),   # 3 workgroup(s) per image, 1683 pixels
    (True, 32, 3, 24, 40): dict(lanes=956, vectors=0, groups=96, window=4636),   # 4 workgroup(s) per image, 2880 pixels
    (True, 128, 1, 9, 11): dict(lanes=64, vectors=0, groups=78, window=512),   # 2 workgroup(s) per image, 99 pixels
    (True, 128, 1, 18, 9): dict(lanes=104, vectors=0, groups=58, window=901),   # 3 workgroup(s) per image, 162 pixels
    (True, 128, 1, 17, 33): dict(lanes=354, vectors=0, groups=104, window=3328),   # 9 workgroup(s) per image, 561 pixels
    (True, 128, 1, 24, 40): dict(lanes=596, vectors=0, groups=128, window=6176),   # 15 workgroup(s) per image, 960 pixels
    (True, 128, 3, 9, 11): dict(lanes=189, vectors=0, groups=234, window=1537),   # 2 workgroup(s) per image, 297 pixels
    (True, 128, 3, 18, 9): dict(lanes=311, vectors=0, groups=174, window=2701),   # 3 workgroup(s) per image, 486 pixels
    (True, 128, 3, 17, 33): dict(lanes=1059, vectors=0, groups=312, window=9984),   # 9 workgroup(s) per image, 1683 pixels
    (True, 128, 3, 24, 40): dict(lanes=1793, vectors=0, groups=384, window=18534),   # 15 workgroup(s) per image, 2880 pixels
    (True, 512, 1, 9, 11): dict(lanes=98, vectors=0, groups=462, window=2050),   # 7 workgroup(s) per image, 99 pixels
    (True, 512, 1, 18, 9): dict(lanes=161, vectors=0, groups=430, window=3608),   # 11 workgroup(s) per image, 162 pixels
    (True, 512, 1, 17, 33): dict(lanes=555, vectors=0, groups=258, window=13312),   # 36 workgroup(s) per image, 561 pixels
    (True, 512, 1, 24, 40): dict(lanes=947, vectors=0, groups=160, window=24707),   # 60 workgroup(s) per image, 960 pixels
    (True, 512, 3, 9, 11): dict(lanes=291, vectors=0, groups=1385, window=6152),   # 7 workgroup(s) per image, 297 pixels
    (True, 512, 3, 18, 9): dict(lanes=476, vectors=0, groups=1287, window=10823),   # 11 workgroup(s) per image, 486 pixels
    (True, 512, 3, 17, 33): dict(lanes=1653, vectors=0, groups=774, window=39936),   # 36 workgroup(s) per image, 1683 pixels
    (True, 512, 3, 24, 40): dict(lanes=2832, vectors=0, groups=480, window=74121),   # 60 workgroup(s) per image, 2880 pixels
    (True, 1024, 1, 9, 11): dict(lanes=74, vectors=25, groups=974, window=4100),   # 7 workgroup(s) per image, 99 pixels
    (True, 1024, 3, 9, 11): dict(lanes=222, vectors=75, groups=2920, window=12304),   # 7 workgroup(s) per image, 297 pixels
}


def nchw(t):
    return t.permute(0, 3, 1, 2).contiguous()


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def leaf(t):
    return t.detach().clone().requires_grad_(True)


@pytest.mark.parametrize("key", sorted(TIE_COUNTS))
def test_tie_inputs_hold_the_stated_ties_and_are_exact_in_bf16(key):
    bf16, C, B, H, W = key
    t = O.tie_case(B, H, W, C)
    got = O.tie_counts(t, bf16)
    assert got == TIE_COUNTS[key], got
    nwg, _ = O.group_grid(C, bf16, B, H, W)
    assert got["lanes"] >= 1 and got["window"] >= 1 and (got["groups"] >= 1 or nwg == 1)
    assert (got["vectors"] >= 1) == (C // O.vec(bf16) > 64)       # a lane holds two vectors: f32 at 512 channels, bf16 at 1024
    for k in ("y", "scale", "shift", "mean", "invstd", "ca", "sa", "res", "out", "d_same", "d_pool", "g", "d_o1", "d_maxz"):
        assert torch.equal(t[k].bfloat16().double(), t[k]), k
    assert set(torch.sign(t["scale"]).tolist()) == {-1.0, 1.0}


def test_every_kind_of_tie_occurs_in_some_case():
    tot = {k: sum(v[k] for v in TIE_COUNTS.values()) for k in ("lanes", "vectors", "groups", "window")}
    assert all(v >= 1 for v in tot.values()), tot
    assert any(O.group_grid(C, bf16, B, H, W)[0] > 1 and v["groups"] >= 1 for (bf16, C, B, H, W), v in TIE_COUNTS.items())


HOST_CASES = [(False, 32, 1, 9, 11), (True, 16, 3, 18, 9), (False, 128, 3, 17, 33), (True, 128, 1, 24, 40), (False, 512, 1, 9, 11),
              (True, 512, 3, 9, 11)]


def _affine(t):
    """the BatchNorm affine as the reference evaluates it: z = gamma * (y - mean) * invstd + beta, with the gamma / beta that give
    the case's (scale, shift) exactly"""
    gamma = leaf(t["scale"] / t["invstd"])
    beta = leaf(t["shift"] + t["mean"] * t["scale"])
    y = leaf(nchw(t["y"]))
    xhat = (y - t["mean"].view(1, -1, 1, 1)) * t["invstd"].view(1, -1, 1, 1)
    z = xhat * gamma.view(1, -1, 1, 1) + beta.view(1, -1, 1, 1)
    return y, gamma, beta, z


@pytest.mark.parametrize("bf16,C,B,H,W", HOST_CASES)
def test_forward_selections_are_torchs(bf16, C, B, H, W):
    t = O.tie_case(B, H, W, C)
    _, _, _, z = _affine(t)
    assert torch.equal(nhwc(z.detach()), t["y"] * t["scale"] + t["shift"])
    o1 = t["ca"][:, :, None, None] * z
    mx, idx = torch.max(o1, dim=1)
    st, amax = O.spatial_stats(t["y"], t["scale"], t["shift"], t["ca"])
    assert torch.equal(amax, idx)                                    # torch.max over dim returns the first maximum
    assert torch.equal(st[..., 1], mx.detach()) and torch.equal(st[..., 0], torch.mean(o1, dim=1).detach())
    ext, first = O.first_extreme(t["y"], t["scale"])
    pooled, pidx = F.adaptive_max_pool2d(z, 1, return_indices=True)
    assert torch.equal(t["scale"] * ext + t["shift"], pooled.detach().flatten(1))
    assert torch.equal(first, pidx.flatten(1))                       # ... and so does the global max-pool (row-major)
    for pool in (False, True):
        res = O.tie_res(B, 2 * H, 2 * W, C) if pool else t["res"]
        r = F.max_pool2d(nchw(res), 2) if pool else nchw(res)
        want = F.relu(nchw(t["sa"][..., None]) * o1 + r).detach()
        assert torch.equal(nchw(O.apply_fwd(t["y"], t["scale"], t["shift"], t["ca"], t["sa"], res, pool)), want)


@pytest.mark.parametrize("bf16,C,B,H,W", HOST_CASES)
@pytest.mark.parametrize("src", ["same", "pool", "both"])
def test_bwd1_is_autograd_of_relu_and_maxpool(bf16, C, B, H, W, src):
    t = O.tie_case(B, H, W, C)
    d_same = t["d_same"] if src != "pool" else None
    d_pool = t["d_pool"] if src != "same" else None
    out = leaf(nchw(t["out"]))
    loss = 0
    if d_same is not None:
        loss = loss + (out * nchw(d_same)).sum()
    if d_pool is not None:
        loss = loss + (F.max_pool2d(out, 2) * nchw(d_pool)).sum()
    loss.backward()
    g_ref = out.grad * (out.detach() > 0)
    g, du = O.bwd1(t["y"], t["scale"], t["shift"], t["ca"], t["sa"], t["out"], d_same, d_pool)
    assert torch.equal(nchw(g), g_ref)
    if src == "pool":       # an odd last row / column lies in no window
        assert float(g[:, 2 * (H // 2):].abs().sum()) == 0 and float(g[:, :, 2 * (W // 2):].abs().sum()) == 0 and float(g.abs().sum()) > 0
    # d(pre-sigmoid of the 7x7 convolution) = d(sa) * sa (1 - sa), d(sa) by autograd of sa * o1 + r
    _, _, _, z = _affine(t)
    sa, r = leaf(nchw(t["sa"][..., None])), leaf(nchw(t["res"]))
    (sa * (t["ca"][:, :, None, None] * z) + r).backward(g_ref)
    assert torch.equal(r.grad, g_ref)
    s = t["sa"]
    assert torch.equal(du, sa.grad[:, 0] * s * (1 - s))


@pytest.mark.parametrize("bf16,C,B,H,W", HOST_CASES)
def test_bwd2_and_bwd3_are_autograd_of_the_pools(bf16, C, B, H, W):
    t = O.tie_case(B, H, W, C)
    # pass 2: d(o1) and d(ca) of  sum(g * (sa * o1 + r)) + sum(d_st * [mean_c o1, max_c o1])
    y, gamma, beta, z = _affine(t)
    ca = leaf(t["ca"])
    o1 = ca[:, :, None, None] * z
    o1.retain_grad()
    st = torch.cat([torch.mean(o1, dim=1, keepdim=True), torch.max(o1, dim=1, keepdim=True)[0]], 1)
    ((nchw(t["sa"][..., None]) * o1 + nchw(t["res"])) * nchw(t["g"])).sum().add((st * nchw(t["dst"])).sum()).backward()
    _, amax = O.spatial_stats(t["y"], t["scale"], t["shift"], t["ca"])
    d_o1, d_ca = O.bwd2(t["y"], t["scale"], t["shift"], t["g"], t["sa"], t["dst"], amax)
    assert torch.equal(nchw(d_o1), o1.grad)
    assert torch.equal(d_ca, ca.grad)
    # pass 3: d(z) and the BatchNorm rows of  sum(d_o1 * ca * z) + sum(d_avgz * avgpool(z)) + sum(d_maxz * maxpool(z))
    y, gamma, beta, z = _affine(t)
    z.retain_grad()
    loss = (nchw(t["d_o1"]) * (t["ca"][:, :, None, None] * z)).sum()
    loss = loss + (F.adaptive_avg_pool2d(z, 1).flatten(1) * t["d_avgz"]).sum() + (F.adaptive_max_pool2d(z, 1).flatten(1) * t["d_maxz"]).sum()
    loss.backward()
    _, first = O.first_extreme(t["y"], t["scale"])
    dz, rows = O.bwd3(t["y"], t["mean"], t["invstd"], t["d_o1"], t["ca"], t["d_avgz"], t["d_maxz"], first)
    assert torch.equal(nchw(dz), z.grad)
    assert torch.equal(rows[0], beta.grad) and torch.equal(rows[1], gamma.grad)
    # d_maxz lands on exactly one pixel per (image, channel)
    only_max = dz - t["d_o1"] * t["ca"][:, None, None, :] - t["d_avgz"][:, None, None, :] / (H * W)
    assert torch.equal((only_max != 0).sum((1, 2)), (t["d_maxz"] != 0).long())


@pytest.mark.parametrize("C,mid,B,H,W,pool_res", [(32, 2, 2, 9, 11, False), (16, 1, 3, 18, 9, True), (128, 8, 1, 17, 33, False), (128, 2, 2, 10, 7, True)])
def test_whole_block_chain_equals_autograd(C, mid, B, H, W, pool_res):
    """the oracle's passes chained as the engine chains the kernels, against autograd of the block written with torch's own pools: raw
    values on a 1/4 grid (the global max-pool ties in every channel), random MLP / 7x7 weights; sums to 1e-12, selections exact"""
    g_ = torch.Generator().manual_seed(C + H)
    rnd = lambda *s: torch.randn(*s, generator=g_, dtype=torch.float64)
    y = torch.randint(-4, 5, (B, H, W, C), generator=g_).double() / 4
    scale, shift = rnd(C), rnd(C) * 0.3
    mean, invstd = rnd(C) * 0.2, rnd(C).abs() + 0.5
    w1, b1, w2, b2 = rnd(mid, C) / C ** 0.5, rnd(mid) * 0.1, rnd(C, mid), rnd(C) * 0.1
    w7, b7 = rnd(1, 2, 7, 7) * 0.1, rnd(1)
    res = torch.randint(-4, 5, (B, 2 * H, 2 * W, C) if pool_res else (B, H, W, C), generator=g_).double() / 4
    d_same, d_pool = rnd(B, H, W, C), rnd(B, H // 2, W // 2, C)
    # ---- torch
    yl, gl, bl = leaf(nchw(y)), leaf(scale / invstd), leaf(shift + mean * scale)
    w1l, b1l, w2l, b2l, w7l, b7l, rl = (leaf(v) for v in (w1, b1, w2, b2, w7, b7, nchw(res)))
    z = (yl - mean.view(1, -1, 1, 1)) * invstd.view(1, -1, 1, 1) * gl.view(1, -1, 1, 1) + bl.view(1, -1, 1, 1)
    mlp = lambda v: F.linear(F.relu(F.linear(v, w1l, b1l)), w2l, b2l)
    ca = torch.sigmoid(mlp(F.adaptive_avg_pool2d(z, 1).flatten(1)) + mlp(F.adaptive_max_pool2d(z, 1).flatten(1)))
    o1 = ca[:, :, None, None] * z
    st = torch.cat([torch.mean(o1, dim=1, keepdim=True), torch.max(o1, dim=1, keepdim=True)[0]], 1)
    sa = torch.sigmoid(F.conv2d(st, w7l, b7l, padding=3))
    out = F.relu(sa * o1 + (F.max_pool2d(rl, 2) if pool_res else rl))
    ((out * nchw(d_same)).sum() + (F.max_pool2d(out, 2) * nchw(d_pool)).sum()).backward()
    # ---- the oracle's passes
    scale_, shift_ = gl.detach() * invstd, bl.detach() - mean * gl.detach() * invstd
    f = O.channel_fwd(y, scale_, shift_, w1, b1, w2, b2)
    st_o, amax = O.spatial_stats(y, scale_, shift_, f["ca"])
    stl = leaf(nchw(st_o))
    w7o, b7o = leaf(w7), leaf(b7)
    pre = F.conv2d(stl, w7o, b7o, padding=3)
    sa_o = torch.sigmoid(pre.detach())[:, 0]
    out_o = O.apply_fwd(y, scale_, shift_, f["ca"], sa_o, res, pool_res)
    g, du = O.bwd1(y, scale_, shift_, f["ca"], sa_o, out_o, d_same, d_pool)
    pre.backward(du.unsqueeze(1))
    d_o1, d_ca = O.bwd2(y, scale_, shift_, g, sa_o, nhwc(stl.grad), amax)
    cb = O.channel_bwd(d_ca, f["ca"], f["hid_avg"], f["hid_max"], f["avgz"], f["maxz"], w1, w2)
    dz, rows = O.bwd3(y, mean, invstd, d_o1, f["ca"], cb["d_avgz"], cb["d_maxz"], f["first"])

    def close(a, b, what):
        assert (a - b).abs().max().item() <= 1e-12 * max(1.0, b.abs().max().item()), what

    close(f["ca"], ca.detach(), "ca")
    close(nchw(st_o), st.detach(), "st")
    close(nchw(out_o), out.detach(), "out")
    assert torch.equal(nchw(out_o) > 0, out.detach() > 0)
    if pool_res:
        close(nchw(O.unpool(res, g)), rl.grad, "d_res through the pool")
    else:
        close(nchw(g), rl.grad, "g")
    close(nchw(dz) * scale_.view(1, -1, 1, 1), yl.grad, "d_y")
    close(rows[0], bl.grad, "dbeta")
    close(rows[1], gl.grad, "dgamma")
    for k, v in (("dw1", w1l), ("db1", b1l), ("dw2", w2l), ("db2", b2l)):
        close(cb[k], v.grad, k)
    close(w7o.grad, w7l.grad, "dw7")
    close(b7o.grad, b7l.grad, "db7")


def _print_table():
    combos = [(False, 32), (False, 128), (False, 512), (True, 16), (True, 32), (True, 128), (True, 512)]
    keys = [(bf16, C, B, H, W) for bf16, C in combos for B in (1, 3) for H, W in ((9, 11), (18, 9), (17, 33), (24, 40))]
    keys += [(True, 1024, B, 9, 11) for B in (1, 3)]
    print("TIE_COUNTS = {")
    for bf16, C, B, H, W in keys:
        c = O.tie_counts(O.tie_case(B, H, W, C), bf16)
        print("    (%s, %d, %d, %d, %d): dict(lanes=%d, vectors=%d, groups=%d, window=%d),   # %d workgroup(s) per image, %d pixels" % (
            bf16, C, B, H, W, c["lanes"], c["vectors"], c["groups"], c["window"], O.group_grid(C, bf16, B, H, W)[0], B * H * W))
    print("}")


if __name__ == "__main__":
    _print_table()
