"""Host half of tests/insitu_links.py (no GPU): the parts of the in-situ link checks that decide whether they can be trusted.

  * Ledger.finish fails when one parameter name, one record or one unet2 unit is left out, and when a pre-BatchNorm bias gradient is
    not exactly zero; it passes on a complete walk (fake objects).
  * Report.close, at EVERY tolerance the link kinds use, rejects a tensor scaled by 1.02, a 128 x 96 x 96 map with one 32 x 32 tile
    zeroed, and weights with two of nine taps swapped -- no link tolerance is so wide that it would pass a 2 % error -- and accepts
    what the kind must accept: the bf16 rounding of the reference for the links over bf16 tensors, f32 summation noise for the others.
  * the source loaders: a pooled-on-load source equals F.max_pool2d(F.leaky_relu(bn(x))) with floor semantics (9 x 11 -> 4 x 5), the
    stem's source is the raw image with 1 and with 3 channels, a via_pool tensor is held to its producer, and the gradient through a
    pooled route equals autograd's.
"""
import types

import pytest
import torch
import torch.nn.functional as F

from abcnet_amd.engine_types import Src
import insitu_links as IL

# (relative L2, max / max, what the compared tensor is) per link kind: tests/test_gpu_insitu_fullsize.py's bounds, which
# tests/test_gpu_insitu_all_layers.py reuses
BOUNDS = {
    "forward": (4e-3, 1.2e-2, "bf16"),
    "wgrad / dgrad": (5e-3, 3e-2, "bf16"),
    "g = dA * act'": (4e-3, 3e-2, "bf16"),
    "dgrad + residual": (8e-3, 3e-2, "bf16"),
    "stored dY, two-route BatchNorm sums": (1e-2, 3e-2, "bf16"),
    "heads": (1.5e-2, 3e-2, "bf16"),
    "BatchNorm sums, convT bias": (2e-3, 3e-2, "f32"),
    "heads BatchNorm sums": (3e-3, 3e-2, "f32"),
    "logits": (2e-4, 1e-3, "f32"),
}


def _ref_map():
    g = torch.Generator().manual_seed(11)
    return torch.randn((1, 128, 96, 96), generator=g)


def _ref_weights():
    g = torch.Generator().manual_seed(12)
    return torch.randn((32, 16, 3, 3), generator=g)


def _bad(l2, linf, got, ref):
    rep = IL.Report()
    rep.close("x", got, ref, l2, linf)
    return bool(rep.bad)


@pytest.mark.parametrize("kind", list(BOUNDS))
def test_report_rejects_small_defects_and_accepts_rounding(kind):
    l2, linf, storage = BOUNDS[kind]
    ref, w = _ref_map(), _ref_weights()
    assert _bad(l2, linf, ref * 1.02, ref), "a 2 % scale error passes"
    tile = ref.clone()
    tile[:, :, 32:64, 64:96] = 0
    assert _bad(l2, linf, tile, ref), "a zeroed 32 x 32 tile passes"
    swapped = w.clone()
    swapped[..., 0, 1], swapped[..., 1, 0] = w[..., 1, 0], w[..., 0, 1]
    assert _bad(l2, linf, swapped, w), "two swapped taps pass"
    if storage == "bf16":
        assert not _bad(l2, linf, IL._r(ref), ref), "one bf16 rounding of the reference fails"
        assert not _bad(l2, linf, IL._r(w), w)
    else:
        g = torch.Generator().manual_seed(13)
        noise = 1 + (torch.rand(ref.shape, generator=g) - 0.5) * 2.0 ** -20       # (16 f32 roundings' worth)
        assert not _bad(l2, linf, ref * noise, ref)
    with pytest.raises(AssertionError):
        rep = IL.Report()
        rep.close("x", ref * 1.02, ref, l2, linf)
        rep.finish()


def test_report_refuses_broadcast_shapes():
    rep = IL.Report()
    with pytest.raises(AssertionError):
        rep.close("x", torch.ones(4, 1), torch.ones(4), 1e-3)


# ------------------------------------------------------------------ the ledger
class _FakeModel:
    def __init__(self, names, nonzero=()):
        self.names, self.nonzero = names, nonzero

    def named_parameters(self):
        return [(n, None) for n in self.names]

    def grad_of(self, name):
        return torch.full((3,), 1e-9 if name in self.nonzero else 0.0)


NAMES = ["s", "inc1.double_conv.0.weight", "inc1.double_conv.0.bias", "inc1.double_conv.1.weight", "inc1.double_conv.1.bias",
         "up1.up.weight", "up1.up.bias", "out_modules.0.conv1.weight", "out_modules.0.conv1.bias", "out_modules.0.conv2.bias",
         "inc1.double_conv.5.channel_attention.shared_MLP.0.bias"]


def _fake_plan(unet2):
    recs = [types.SimpleNamespace(kind="conv", cname="inc1.double_conv.0"), types.SimpleNamespace(kind="convT", cname="up1.up"),
            types.SimpleNamespace(kind="conv", cname="out_modules.0.conv1", is_head=True)]
    eng = types.SimpleNamespace(recs=recs)
    if unet2:
        eng.units2 = [("blk", types.SimpleNamespace(kind="blk2", prefix="inc1")), ("convT", recs[1])]
    return eng


def _walk(skip_param=None, skip_rec=None, unet2=False, skip_unit=None):
    eng = _fake_plan(unet2)
    led = IL.Ledger()
    for n in NAMES:
        if n != skip_param and not n.endswith(IL.PRE_BN_BIAS):
            led.param(n)
    for r in eng.recs:
        if r.cname != skip_rec:
            led.visit(r)
    for _k, u in getattr(eng, "units2", []):
        if getattr(u, "prefix", None) != skip_unit:
            led.visit(u)
    return led, eng


@pytest.mark.parametrize("unet2", [False, True])
def test_ledger_passes_on_a_complete_walk(unet2):
    led, eng = _walk(unet2=unet2)
    led.finish(_FakeModel(NAMES), eng)


@pytest.mark.parametrize("name", [n for n in NAMES if not n.endswith(IL.PRE_BN_BIAS)])
def test_ledger_fails_on_one_parameter_left_out(name):
    led, eng = _walk(skip_param=name)
    with pytest.raises(AssertionError, match="no link compared"):
        led.finish(_FakeModel(NAMES), eng)


@pytest.mark.parametrize("cname", ["inc1.double_conv.0", "up1.up", "out_modules.0.conv1"])
def test_ledger_fails_on_one_record_left_out(cname):
    led, eng = _walk(skip_rec=cname)
    with pytest.raises(AssertionError, match="no link visited the record"):
        led.finish(_FakeModel(NAMES), eng)


def test_ledger_fails_on_one_unet2_unit_left_out():
    led, eng = _walk(unet2=True, skip_unit="inc1")
    with pytest.raises(AssertionError, match="unet2 unit"):
        led.finish(_FakeModel(NAMES), eng)


def test_ledger_exempts_only_exactly_zero_pre_bn_biases():
    # (an MLP bias whose name merely ends in "0.bias" is no pre-BatchNorm bias: it is in NAMES and must be compared)
    assert not "inc1.double_conv.5.channel_attention.shared_MLP.0.bias".endswith(IL.PRE_BN_BIAS)
    led, eng = _walk()
    with pytest.raises(AssertionError, match="not exactly zero"):
        led.finish(_FakeModel(NAMES, nonzero=("out_modules.0.conv1.bias",)), eng)


# ------------------------------------------------------------------ the source loaders
def _coef(C, slope, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.3, torch.full((C,), slope)


def _bn_act(x_nchw, coef, coff, C):
    sc, sh, sl = (c[coff:coff + C].view(1, -1, 1, 1) for c in coef)
    a = x_nchw * sc + sh
    return torch.where(a > 0, a, a * sl)


@pytest.mark.parametrize("H,W", [(9, 11), (8, 16), (5, 2)])
@pytest.mark.parametrize("slope", [0.0, 0.01])
def test_pooled_on_load_source_is_pool_of_the_activation(H, W, slope):
    g = torch.Generator().manual_seed(H * 100 + W)
    ld, coff, C = 24, 8, 16
    t = torch.randn((2, H, W, ld), generator=g).to(torch.bfloat16)
    coef = _coef(ld, slope, 3)
    want = F.max_pool2d(_bn_act(t.float().permute(0, 3, 1, 2)[:, coff:coff + C], coef, coff, C), 2)
    got = IL._activated(Src(t, None, H, W, ld, coff, C, coef=coef, pool=True))
    assert got.shape == (2, C, H // 2, W // 2) and torch.equal(got, want)
    if slope == 0.01:      # (the same through torch's own leaky_relu: its sign rule is the loader's)
        sc, sh, _sl = (c[coff:coff + C].view(1, -1, 1, 1) for c in coef)
        lr = F.max_pool2d(F.leaky_relu(t.float().permute(0, 3, 1, 2)[:, coff:coff + C] * sc + sh, 0.01), 2)
        assert torch.allclose(got, lr, rtol=1e-6, atol=0)
    plain = IL._activated(Src(t, None, H, W, ld, coff, C, coef=coef))
    assert plain.shape == (2, C, H, W) and torch.equal(F.max_pool2d(plain, 2), got)


@pytest.mark.parametrize("cin", [1, 3])
def test_stem_source_is_the_raw_image(cin):
    g = torch.Generator().manual_seed(cin)
    img = (torch.rand((2, cin, 9, 11), generator=g) < 0.3).float()
    src = Src(img, None, 9, 11, 1, 0, 1) if cin == 1 else Src(img, None, 9, 11, 0, 0, cin, planar=True)
    assert torch.equal(IL._activated(src), img)


def _producer(H, W, seed=5, C=8):
    g = torch.Generator().manual_seed(seed)
    y = torch.randn((2, H, W, C), generator=g).to(torch.bfloat16)
    sc, sh, sl = _coef(C, 0.0, seed)
    return types.SimpleNamespace(kind="conv", y=y, coff=0, cout=C, scale=sc, shift=sh, slopes=sl, grad_same=None, grad_pool=None)


def test_via_pool_tensor_is_held_to_its_producer():
    p = _producer(9, 11)
    act = _bn_act(p.y.float().permute(0, 3, 1, 2), (p.scale, p.shift, p.slopes), 0, p.cout)
    pooled = F.max_pool2d(act, 2).permute(0, 2, 3, 1).to(torch.bfloat16).contiguous()
    src = Src(pooled, None, 4, 5, p.cout, 0, p.cout, producer=p)
    src.via_pool = True
    rep = IL.Report()
    IL._pool_link(src, rep, "x")
    assert len(rep.rows) == 1 and not rep.bad
    # a pooling that took its windows one pixel to the right is seen
    off = F.max_pool2d(act[..., 1:], 2).permute(0, 2, 3, 1).to(torch.bfloat16).contiguous()
    src.t = off
    rep = IL.Report()
    IL._pool_link(src, rep, "x")
    assert rep.bad


@pytest.mark.parametrize("H,W", [(9, 11), (8, 6)])
@pytest.mark.parametrize("both", [False, True])
def test_gradient_through_a_pooled_route_is_autograds(H, W, both):
    p = _producer(H, W, seed=H)
    g = torch.Generator().manual_seed(77)
    d_pool = torch.randn((2, H // 2, W // 2, p.cout), generator=g).to(torch.bfloat16)
    d_same = torch.randn((2, H, W, p.cout), generator=g).to(torch.bfloat16)
    p.grad_pool = (d_pool, p.cout, 0)
    p.grad_same = (d_same, p.cout, 0) if both else None
    y = p.y.float().permute(0, 3, 1, 2).clone().requires_grad_(True)
    act = F.relu(y * p.scale.view(1, -1, 1, 1) + p.shift.view(1, -1, 1, 1))
    out = (F.max_pool2d(act, 2) * IL.nchw(d_pool)).sum()
    if both:
        out = out + (act * IL.nchw(d_same)).sum()
    out.backward()
    _act, f = IL._producer_activation(p)
    got = IL._grad_into(p, p.cout) * f * p.scale.view(1, -1, 1, 1)       # d(y_raw) = dA * act' * scale
    assert torch.allclose(got, y.grad, rtol=1e-6, atol=1e-7)
    if H % 2:      # floor semantics: the odd last row belongs to no window
        assert both or float(got[:, :, H - 1].abs().max()) == 0.0
