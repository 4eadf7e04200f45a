"""The in-situ link checks of the train step as a plain helper module (no test lives here, no pytest hook).

A "link" is ONE launch family of the step -- a forward convolution, a weight gradient, a data gradient, a BatchNorm backward, the
heads' passes, a CBAM block -- compared with torch ops / autograd applied to the ENGINE's OWN tensors: every decision (ReLU sign,
dropout keep, arg-max of a pooling window) is taken from what the engine stored, so no decision can flip and the bounds are those
of one bf16 rounding.  tests/test_gpu_insitu_fullsize.py walks a sample of the plan at 16 x 384 x 384 (the launch shapes that exist
only there); tests/test_gpu_insitu_all_layers.py walks EVERY record of small and ragged plans and closes with Ledger.finish, which
fails when a parameter's gradient or a record of the plan was compared by no link.

The helpers work on whatever device the tensors live on: tests/test_insitu_links_host.py runs the pieces that need no engine on
the CPU (Report's discrimination, the Ledger, the source loaders).
"""
import sys

import torch
import torch.nn.functional as F

from abcnet_amd.dropout import head_keep_masks
from oracle import loss_oracle
from oracle import unet_oracle as uo

HEADS = uo.HEADS
# the convolution biases in front of a BatchNorm: the batch mean absorbs them, their gradient is identically zero
PRE_BN_BIAS = ("double_conv.0.bias", "double_conv.3.bias", "conv1.bias")


def _r(t):
    """what an MFMA operand of the bf16 kernels holds: the f32 value rounded to bf16"""
    return t.to(torch.bfloat16).float()


def nchw(t):
    return t.float().permute(0, 3, 1, 2).contiguous()


class Ledger:
    """which parameters' gradients the links compared and which records of the plan they visited"""

    def __init__(self):
        self.params, self.visited = set(), []

    def param(self, name):
        self.params.add(name)

    def visit(self, rec):
        if not any(r is rec for r in self.visited):
            self.visited.append(rec)

    def seen(self, rec):
        return any(r is rec for r in self.visited)

    def finish(self, model, eng):
        """every name of model.named_parameters() was compared -- but for the pre-BatchNorm convolution biases, whose gradient is
        identically zero: the engine writes none, so its arena must hold exact zeros there -- and every conv / convT record of
        eng.recs, for unet2 every unit of eng.units2, was visited"""
        names = [n for n, _p in model.named_parameters()]
        missing = [n for n in names if n not in self.params and not n.endswith(PRE_BN_BIAS)]
        assert not missing, "no link compared the gradient of %s" % missing
        for n in names:
            if n.endswith(PRE_BN_BIAS) and n not in self.params:
                g = model.grad_of(n)
                assert not bool((g != 0).any()), "the gradient of the pre-BatchNorm bias %s is not exactly zero: max |g| = %g" % (n, g.abs().max().item())
        left = [getattr(r, "cname", "?") for r in eng.recs if getattr(r, "kind", None) in ("conv", "convT") and not self.seen(r)]
        assert not left, "no link visited the record(s) %s" % left
        left = [getattr(u, "prefix", getattr(u, "cname", "?")) for _k, u in getattr(eng, "units2", []) if not self.seen(u)]
        assert not left, "no link visited the unet2 unit(s) %s" % left


class Report:
    """collects (what, relative L2, largest deviation / largest element) and asserts at the end, so that ONE run shows all"""

    def __init__(self):
        self.rows, self.bad, self.notes = [], [], []
        self.ledger = Ledger()

    def close(self, what, got, ref, l2, linf=3e-2):
        got, ref = got.double(), ref.double()
        assert got.shape == ref.shape, (what, tuple(got.shape), tuple(ref.shape))
        e2 = (got - ref).norm().item() / (ref.norm().item() + 1e-30)
        ei = (got - ref).abs().max().item() / (ref.abs().max().item() + 1e-30)
        self.rows.append((what, e2, ei))
        if not (e2 <= l2 and ei <= linf):
            self.bad.append((what, e2, l2, ei, linf))

    def grad(self, what, m, name, ref, l2, linf=3e-2):
        """close() on the engine's gradient of the parameter `name`, entered in the ledger"""
        self.ledger.param(name)
        self.close(what, m.grad_of(name), ref, l2, linf)

    def info(self, what, value):
        """a figure that is printed with the table and asserted nowhere (a reference-only rounding floor)"""
        self.notes.append((what, value))

    def finish(self):
        for what, e2, ei in self.rows:
            print("in-situ %-58s rel-L2 %.2e   max/max %.2e" % (what, e2, ei), file=sys.stderr)
        for what, v in self.notes:
            print("in-situ %-58s rel-L2 %.2e   (reference alone)" % (what, v), file=sys.stderr)
        assert not self.bad, self.bad


def _sum_floor(rep, tag, G, xh):
    """the floor of the reference alone under BatchNorm's two sums: the f32 reference g (NHWC) rounded to bf16 -- what the engine
    stores, and what _bn_backward_ref re-sums -- against the same g unrounded, which is what a kernel sums before it stores"""
    for name, w in (("dbeta", torch.ones_like(xh)), ("dgamma", xh)):
        a, b = (_r(G) * w).sum((0, 1, 2)).double(), (G * w).sum((0, 1, 2)).double()
        rep.info(tag + " floor of " + name, (a - b).norm().item() / (b.norm().item() + 1e-30))


def _raw_nhwc(src):
    """the raw tensor of an engine.Src as f32 NHWC, its channels [coff, coff + C): an NHWC activation, or the input image -- NCHW f32
    as the reference passes it, read channel-planar (three channels) or as NHWC with a pixel stride of 1 (one channel)"""
    t = src.t.float()
    if getattr(src, "planar", False) or (src.C == 1 and src.ld == 1 and tuple(t.shape[1:]) == (1, src.H, src.W)):
        return t.permute(0, 2, 3, 1)[..., src.coff:src.coff + src.C]
    return t[..., src.coff:src.coff + src.C]


def _activated(src):
    """the tensor a consumer's loader makes of `src` (engine.Src: raw tensor + BatchNorm affine + leaky slope on load, then the
    2 x 2 max pool with floor semantics where the source is pooled on load), f32 NCHW -- decisions from the engine's own raw tensor
    and coefficients.  The stem's source is the f32 image itself (coef None); a via_pool source is the tensor abc_pool_act
    materialised, read plain (_pool_link holds that tensor to its producer)"""
    x = _raw_nhwc(src)
    if src.coef is not None:
        sc, sh, sl = (c[src.coff:src.coff + src.C] for c in src.coef)
        a = x * sc + sh
        x = torch.where(a > 0, a, a * sl)
    assert src.drop_p == 0.0      # (the heads' features, the one source behind a dropout, are rebuilt in the heads links)
    x = x.permute(0, 3, 1, 2).contiguous()
    if src.pool:
        x = F.max_pool2d(x, 2)
    return x


def _producer_activation(p):
    """the activated output of the layer record / unet2 block `p`, f32 NCHW, and its derivative factor (None: a block's output is stored
    finished)"""
    if getattr(p, "kind", None) == "blk2":
        return nchw(p.out[..., p.coff_out:p.coff_out + p.cout]), None
    a = p.y.float()[..., p.coff:p.coff + p.cout] * p.scale + p.shift
    act = torch.where(a > 0, a, a * p.slopes)
    f = torch.where(a > 0, torch.ones_like(a), p.slopes.expand_as(a))
    return act.permute(0, 3, 1, 2).contiguous(), f.permute(0, 3, 1, 2).contiguous()


def _pool_link(src, rep, tag):
    """a via_pool source: the tensor the pooling pass materialised against max_pool2d (floor) of its producer's activation rebuilt from
    the producer's raw tensor and coefficients; one bf16 rounding of the output"""
    if not getattr(src, "via_pool", False):
        return
    act, _f = _producer_activation(src.producer)
    rep.close(tag + " pooled input (pool_act)", nchw(src.t[..., src.coff:src.coff + src.C]), F.max_pool2d(act, 2), 4e-3, 1.2e-2)


def _grad_into(p, C_):
    """d(activated output) of the layer / block p from the gradient routes its consumers left: the full-resolution one, plus the pooled
    one through max_pool2d's backward (the FIRST maximal pixel of a window, floor semantics: an odd last row / column gets none)"""
    act, _f = _producer_activation(p)
    dA = torch.zeros_like(act)
    if p.grad_same is not None:
        t, _ld, co = p.grad_same
        dA = dA + nchw(t[..., co:co + C_])
    if p.grad_pool is not None:
        t, _ld, co = p.grad_pool
        leaf = act.detach().clone().requires_grad_(True)
        with torch.enable_grad():
            F.max_pool2d(leaf, 2).backward(nchw(t[..., co:co + C_]))
        dA = dA + leaf.grad
    return dA


def _bn_backward_ref(rec, m, rep, tag, own_sums=False):
    """closed form of BatchNorm backward from the engine's own g (= dA * act'), y_raw and batch statistics; returns dY (f32 NCHW).
    own_sums (the all-layers walk): dY -- the reference of the stored dY, and the input of the convolution's adjoints -- is formed with
    the ENGINE's two sums, which the lines above have just held to their own bound, as every other link starts from the engine's own
    tensors.  With the re-summed ones the sums' rounding (a kernel sums g in f32 BEFORE it rounds g to bf16, this check re-sums the
    stored g: 2e-3 of a sum on a small map) is a per-channel OFFSET of dY, which the weight gradient's sum over the pixels does not
    average out as it does element noise: measured 3.0e-3 .. 5.04e-3 on the weight gradients of the fused-g first convolutions of
    unet2 at 2 x 128 x 128 against 4e-7 .. 2e-4 where the sums agree to 1e-7 -- the sums' error counted twice, not a weight gradient's"""
    G = rec.g.float()
    y = rec.y.float()[..., rec.coff:rec.coff + rec.cout]
    n = G.shape[0] * G.shape[1] * G.shape[2]
    xh = (y - rec.mean) * rec.invstd
    dbeta, dgamma = G.sum((0, 1, 2)), (G * xh).sum((0, 1, 2))
    # a layer with TWO gradient routes (skip connection + max-pool: inc3, down3, down4) rounds g = bf16(dA_same + dA_pool) once
    # more AFTER the kernel took its f32 sums; these sums cancel heavily (both signs), so the rounding noise of 147456 addends
    # shows at ~3e-3 of the sum (measured: 3.0e-3 / 2.6e-3 on inc3.double_conv.3; 1e-7 where g = dA * act' is exact in bf16)
    # (the same holds where g comes out of a data gradient's epilogue, abc_conv_desc.actbwd_*: the kernel sums the f32 values it then
    #  rounds to bf16, this check re-sums the stored bf16 g -- measured 5e-4 .. 2.1e-3 on the twelve such layers of unet.py)
    tol = 1e-2 if ((rec.grad_pool is not None and rec.grad_same is not None) or getattr(rec, "fused_g", None) is not None) else 2e-3
    rep.grad(tag + " dbeta", m, rec.bname + ".bias", dbeta, tol)
    rep.grad(tag + " dgamma", m, rec.bname + ".weight", dgamma, tol)
    gamma = m.state_dict()[rec.bname + ".weight"]
    if own_sums:
        dbeta, dgamma = m.grad_of(rec.bname + ".bias").float(), m.grad_of(rec.bname + ".weight").float()
    dY = gamma * rec.invstd * (G - dbeta / n - xh * dgamma / n)
    if getattr(rec, "dY", None) is not None:
        rep.close(tag + " dY (stored)", rec.dY.float(), dY, 1e-2)
    return dY.permute(0, 3, 1, 2).contiguous()


def _dgrad_tag(rec):
    return " dgrad + act_bwd" if getattr(rec, "dsrc_is_g", False) else " dgrad"


def _dgrad_ref(rec, dX):
    """what rec's data-gradient launch stores: d(input) by autograd -- times the producing layer's activation derivative where
    that layer's act_bwd pass rides in the launch's epilogue (engine: rec.dsrc_is_g; the decisions from the engine's own y_raw and
    BatchNorm coefficients)"""
    if not getattr(rec, "dsrc_is_g", False):
        return dX
    p = rec.src.producer
    a = p.y.float()[..., p.coff:p.coff + p.cout] * p.scale + p.shift
    f = torch.where(a > 0, torch.ones_like(a), p.slopes.expand_as(a))
    return dX * f.permute(0, 3, 1, 2)


def _forward_link(rec, rep, sd, tag, Y):
    """the FORWARD launch of the layer in situ: the raw (pre-BatchNorm) tensor the training-forward kernel stored -- transform of
    the producer's BatchNorm + activation on load, persistent multi-tile workgroups, 768 / 6144 tiles at this size -- against
    conv2d of the engine's OWN activated input and the bf16 weights, + bias; one bf16 rounding of the output (2e-3 relative)"""
    y = nchw(rec.y[..., rec.coff:rec.coff + rec.cout])
    ref = Y.detach() + sd[rec.cname + ".bias"].float().reshape(1, -1, 1, 1)
    rep.close(tag + " forward (y_raw)", y, ref, 4e-3, 1.2e-2)


def _conv_links(rec, m, rep, sd, every_route=False):
    """g -> BatchNorm backward -> dY; then conv2d's adjoints by torch autograd on (activated input, bf16 weights, dY).
    every_route: also the pooled input (_pool_link) and g = dA * act' where the layer has a pooled gradient route, alone or beside
    the full-resolution one (the all-layers walk; the full-size file keeps its own sample of links)"""
    tag = rec.cname
    rep.ledger.visit(rec)
    dY = _bn_backward_ref(rec, m, rep, tag, own_sums=every_route)
    X = _r(_activated(rec.src)).requires_grad_(True)
    W = _r(sd[rec.cname + ".weight"]).requires_grad_(True)
    k = W.shape[-1]
    Y = F.conv2d(X, W, padding=(k - 1) // 2)
    _forward_link(rec, rep, sd, tag, Y)
    Y.backward(_r(dY))
    rep.grad(tag + " wgrad", m, rec.cname + ".weight", W.grad, 5e-3)
    if getattr(rec, "dsrc", None) is not None:
        rep.close(tag + _dgrad_tag(rec), nchw(rec.dsrc), _dgrad_ref(rec, X.grad), 5e-3)
    if every_route:
        _pool_link(rec.src, rep, tag)
    # the g of this layer itself: dA * act'(bn(y)) from the engine's own dA (same + pooled routes)
    # (not where the data gradient in front of it stored g itself -- abc_conv_desc.actbwd_*: checked there, against autograd)
    if rec.grad_pool is None and rec.grad_same is not None and getattr(rec, "fused_g", None) is None:
        t, ld, co = rec.grad_same
        dA = t.float()[..., co:co + rec.cout]
        y = rec.y.float()[..., rec.coff:rec.coff + rec.cout]
        a = y * rec.scale + rec.shift
        rep.close(tag + " g = dA * act'", rec.g.float(), dA * torch.where(a > 0, torch.ones_like(a), rec.slopes.expand_as(a)), 4e-3)
    elif every_route and rec.grad_pool is not None and getattr(rec, "fused_g", None) is None:
        _act, f = _producer_activation(rec)
        routes = "same + pooled" if rec.grad_same is not None else "pooled"
        g_ref = _grad_into(rec, rec.cout) * f
        rep.close(tag + " g = dA(%s) * act'" % routes, nchw(rec.g), g_ref, 4e-3)
        y = rec.y.float()[..., rec.coff:rec.coff + rec.cout]
        _sum_floor(rep, tag, g_ref.permute(0, 2, 3, 1), (y - rec.mean) * rec.invstd)


def _convT_links(rec, m, rep, sd, forward=False):
    """ConvTranspose2d(k3, s2) + the reference's crop of the first row / column (unet.py:51-56), by autograd: an axis whose skip
    tensor has 2n rows loses the first of the 2n + 1 outputs, one with 2n + 1 rows (odd levels) loses none.
    forward: also the stored output, the upper channel half of the concat tensor (the all-layers walk)"""
    tag = rec.cname
    rep.ledger.visit(rec)
    dcat, ld, coff = rec.grad_out
    dOut = nchw(dcat[..., coff:coff + rec.cout])
    X = _r(_activated(rec.src)).requires_grad_(True)
    W = _r(sd[rec.cname + ".weight"]).requires_grad_(True)
    b = sd[rec.cname + ".bias"].clone().requires_grad_(True)
    y = F.conv_transpose2d(X, W, b, stride=2)
    assert y.shape[2] - rec.H in (0, 1) and y.shape[3] - rec.W in (0, 1), (tuple(y.shape), rec.H, rec.W)
    y = y[:, :, y.shape[2] - rec.H:, y.shape[3] - rec.W:]
    if forward:
        rep.close(tag + " forward", nchw(rec.y[..., rec.coff:rec.coff + rec.cout]), y.detach(), 4e-3, 1.2e-2)
    y.backward(dOut)
    rep.grad(tag + " wgrad", m, rec.cname + ".weight", W.grad, 5e-3)
    rep.grad(tag + " dbias", m, rec.cname + ".bias", b.grad, 2e-3)
    rep.close(tag + " dgrad", nchw(rec.dsrc), X.grad, 5e-3)


def _heads_features(eng, B, h, w):
    """the heads' features as conv2 reads them, from the engine's own raw tensor: (y_raw f32, conv2's input rounded to bf16,
    keep / (1 - p), act')"""
    nh = len(HEADS)
    sc, sh, sl = eng.hcoef
    y = eng.hfeat.float()
    # the loaders' fmaf(y, scale, shift): ONE rounding (in f64 the product is exact).  y * sc + sh rounds twice and lands one f32 ulp
    # away now and then; where that ulp decides the rounding of a feature to bf16, the feature moves by 2^-8 of itself and a head
    # with few channels shows it: measured on logits[0] at 2 x 64 x 96 max / max 1.29e-3, rel-L2 1.75e-4 against 1e-7 on the heads
    # without such a feature -- the reference's mistake, not the kernel's
    a = (y.double() * sc.double() + sh.double()).float()
    act = torch.where(a > 0, a, a * sl)
    dact = torch.where(a > 0, torch.ones_like(a), sl.expand_as(a))
    if eng.drop_p > 0:
        masks = head_keep_masks(B, h, w, nh, eng.dropout_seed(1), eng.drop_p)        # 0 / 1, [B,128,h,w] per head
        keep = torch.cat([mk.permute(0, 2, 3, 1) for mk in masks], dim=3).to(y.device) / (1.0 - eng.drop_p)
    else:
        keep = torch.ones_like(act)
    return y, _r(act * keep), keep, dact                                               # conv2's input as the MFMA sees it


def _loss_autograd(eng, m, rep, sd, tg, check_s):
    """train.py:95-137 by autograd on the ENGINE's logits as leaves, so that the comparison of the gradients starts from identical
    values; returns the leaves.  check_s: the engine's gradient of the loss weights `s` against the same autograd (f64 partial sums
    on the device, f32 arithmetic in torch: the bound of the f32 logits)"""
    dev = eng.logits[0].device
    leaves = [lg.detach().clone().requires_grad_(True) for lg in eng.logits]
    s = sd["s"].clone().to(dev).requires_grad_(True)
    total = loss_oracle.abc_loss(leaves, [t.to(dev) for t in tg], s)[0]
    total.backward()
    if check_s:
        rep.grad("loss d(s)", m, "s", s.grad.float(), 2e-4, 1e-3)
    return leaves


def _heads_conv1_links(eng, m, rep, sd, G, y, B, h, w, forward=False):
    """BatchNorm backward of the eight heads from the engine's own g (G: f32, loss factors applied), then the merged conv1 launches.
    forward: also the merged conv1's stored features (the all-layers walk)"""
    nh = len(HEADS)
    for rec in eng.head_recs:
        rep.ledger.visit(rec)
    n = B * h * w
    xh = (y - eng.hmean) * eng.hinvstd
    dbeta, dgamma = G.sum((0, 1, 2)), (G * xh).sum((0, 1, 2))
    gam = torch.cat([sd["out_modules.%d.bn.weight" % i] for i in range(nh)])
    for i in range(nh):
        rep.grad("heads bn[%d] dbeta" % i, m, "out_modules.%d.bn.bias" % i, dbeta[128 * i:128 * (i + 1)], 3e-3)
        rep.grad("heads bn[%d] dgamma" % i, m, "out_modules.%d.bn.weight" % i, dgamma[128 * i:128 * (i + 1)], 3e-3)
    dY = gam * eng.hinvstd * (G - dbeta / n - xh * dgamma / n)
    rep.close("heads conv1 dY (stored, 8 x 128 channels)", eng.dyh.float(), dY, 1e-2)
    X = _r(_activated(eng.trunk)).requires_grad_(True)
    Wall = _r(torch.cat([sd["out_modules.%d.conv1.weight" % i] for i in range(nh)], 0)).requires_grad_(True)
    Y = F.conv2d(X, Wall, padding=1)
    if forward:
        ball = torch.cat([sd["out_modules.%d.conv1.bias" % i] for i in range(nh)]).float()
        rep.close("heads conv1 forward (y_raw, 8 x 128 channels)", nchw(eng.hfeat), Y.detach() + ball.reshape(1, -1, 1, 1), 4e-3, 1.2e-2)
    Y.backward(_r(nchw(dY)))
    for i in range(nh):
        rep.grad("heads conv1[%d] wgrad (1024-row merged launch)" % i, m, "out_modules.%d.conv1.weight" % i,
                 Wall.grad[128 * i:128 * (i + 1)], 5e-3)
    ref = X.grad
    if getattr(eng, "heads_dgrad_is_g", False):
        # the trunk's last layer has no reader but the heads: its act_bwd pass rides in this launch's epilogue (abc_conv_desc.actbwd_*)
        p = eng.trunk.producer
        a = p.y.float()[..., p.coff:p.coff + p.cout] * p.scale + p.shift
        ref = ref * torch.where(a > 0, torch.ones_like(a), p.slopes.expand_as(a)).permute(0, 3, 1, 2)
    rep.close("heads conv1 dgrad (8 x 128 -> 128)" + (" + act_bwd" if getattr(eng, "heads_dgrad_is_g", False) else ""), nchw(eng.dtrunk), ref, 5e-3)


def _heads_links(eng, m, rep, sd, tg, B, h, w, every_link=False):
    """the fused heads pass (conv2 + loss + way back) and the merged conv1 launches behind it, in situ.
    every_link: also d(s) and the merged conv1's forward (the all-layers walk)"""
    nh = len(HEADS)
    y, feat, keep, dact = _heads_features(eng, B, h, w)
    leaves = []
    for i, hc in enumerate(HEADS):
        p = "out_modules.%d.conv2" % i
        W2 = _r(sd[p + ".weight"]).requires_grad_(True)
        b2 = sd[p + ".bias"].clone().requires_grad_(True)
        fi = nchw(feat[..., 128 * i:128 * (i + 1)]).requires_grad_(True)
        lg = F.conv2d(fi, W2, b2)
        rep.close("heads_fused logits[%d]" % i, eng.logits[i], lg.detach(), 2e-4, 1e-3)
        leaves.append((lg, fi, W2, b2))
    # the loss is evaluated on the ENGINE's logits (a leaf), so that the comparison of the gradients starts from identical values
    logits = _loss_autograd(eng, m, rep, sd, tg, every_link)
    for i, (lg, fi, W2, b2) in enumerate(leaves):
        p = "out_modules.%d.conv2" % i
        lg.backward(logits[i].grad.float())
        rep.grad("heads_fused " + p + ".weight", m, p + ".weight", W2.grad, 1.5e-2)
        rep.grad("heads_fused " + p + ".bias", m, p + ".bias", b2.grad, 1.5e-2)
        # g of the head's BatchNorm output: d(feat) * keep * act'; the pass writes the gradient of the loss NUMERATORS, the
        # head's normaliser arrives as chan_scale
        g_ref = fi.grad.permute(0, 2, 3, 1) * (keep * dact)[..., 128 * i:128 * (i + 1)]
        cs = eng.chan_scale[eng.head_off[i]]
        rep.close("heads_fused g[%d]" % i, eng.hf_g.float()[..., 128 * i:128 * (i + 1)] * cs, g_ref, 1.5e-2)
        if every_link:
            _sum_floor(rep, "heads bn[%d]" % i, g_ref, ((y - eng.hmean) * eng.hinvstd)[..., 128 * i:128 * (i + 1)])
    # ---- BatchNorm backward of the eight heads from the engine's own g, then the merged conv1 launches
    G = eng.hf_g.float() * torch.cat([eng.chan_scale[eng.head_off[i]].expand(128) for i in range(nh)])
    _heads_conv1_links(eng, m, rep, sd, G, y, B, h, w, forward=every_link)


def _heads_unfused_links(eng, m, rep, sd, tg, B, h, w):
    """the heads of a plan WITHOUT the fused pass (eng.hf is None: every map whose h * w is no multiple of 128 -- heads.hip's batched
    1 x 1 launches, loss.hip, wgrad_heads.hip, one act_bwd pass over the 8 x 128 channels), then the merged conv1 launches:
      logits            conv2d of the engine's own activated, dropped-out, bf16-rounded features (f32 out: the fused pass's bound);
      d(logits)         the loss pass's d(numerator) times chan_scale (the per-channel factor the finaliser leaves, applied by the
                        consumers on load) against autograd of loss_oracle.abc_loss on the engine's logits; f32 arithmetic;
      conv2 dW, db, g   from that product, as the fused pass's (1.5e-2: the MFMA operand is the bf16 rounding of d(logits))"""
    assert eng.hf is None
    nh = len(HEADS)
    y, feat, keep, dact = _heads_features(eng, B, h, w)
    leaves = []
    for i, hc in enumerate(HEADS):
        p = "out_modules.%d.conv2" % i
        W2 = _r(sd[p + ".weight"]).requires_grad_(True)
        b2 = sd[p + ".bias"].clone().requires_grad_(True)
        fi = nchw(feat[..., 128 * i:128 * (i + 1)]).requires_grad_(True)
        lg = F.conv2d(fi, W2, b2)
        rep.close("heads logits[%d]" % i, eng.logits[i], lg.detach(), 2e-4, 1e-3)
        leaves.append((lg, fi, W2, b2))
    logits = _loss_autograd(eng, m, rep, sd, tg, True)
    g_all = eng.heads_g.float()
    for i, (lg, fi, W2, b2) in enumerate(leaves):
        p = "out_modules.%d.conv2" % i
        hc = HEADS[i]
        cs = eng.chan_scale[eng.head_off[i]:eng.head_off[i] + hc].reshape(1, hc, 1, 1)
        dl = logits[i].grad.float()
        rep.close("heads d(logits[%d]) x chan_scale" % i, eng.dlogits[i] * cs, dl, 2e-4, 1e-3)
        lg.backward(dl)
        rep.grad("heads " + p + ".weight", m, p + ".weight", W2.grad, 1.5e-2)
        rep.grad("heads " + p + ".bias", m, p + ".bias", b2.grad, 1.5e-2)
        rep.close("heads d(feat)[%d]" % i, eng.heads_dfeat.float()[..., 128 * i:128 * (i + 1)], fi.grad.permute(0, 2, 3, 1), 1.5e-2)
        g_ref = fi.grad.permute(0, 2, 3, 1) * (keep * dact)[..., 128 * i:128 * (i + 1)]
        rep.close("heads g[%d]" % i, g_all[..., 128 * i:128 * (i + 1)], g_ref, 1.5e-2)
        _sum_floor(rep, "heads bn[%d]" % i, g_ref, ((y - eng.hmean) * eng.hinvstd)[..., 128 * i:128 * (i + 1)])
    _heads_conv1_links(eng, m, rep, sd, g_all, y, B, h, w, forward=True)


def _conv2_links(eng, rec, m, rep, sd, every_route=False):
    """unet2: a convolution's weight and data gradient from the dY the engine's BatchNorm backward produced (the first conv of a
    block has the plain chain of unet.py; the second one's g comes out of CBAM's backward: its dY is checked from the stored
    dz in _cbam_links).
    every_route (the all-layers walk): also the pooled input, and the residual 1 x 1 convolution of a block whose input has no
    producer (the image: unet2.py:62,135) -- its forward, weight and bias gradient"""
    tag = "unet2 " + rec.cname
    if getattr(rec, "g", None) is not None:
        dY = _bn_backward_ref(rec, m, rep, tag, own_sums=every_route)
    elif getattr(rec, "dY", None) is not None:
        dY = nchw(rec.dY)
    else:
        return
    rep.ledger.visit(rec)
    X = _r(_activated(rec.src)).requires_grad_(True)
    W = _r(sd[rec.cname + ".weight"]).requires_grad_(True)
    k = W.shape[-1]
    Y = F.conv2d(X, W, padding=(k - 1) // 2)
    _forward_link(rec, rep, sd, tag, Y)
    Y.backward(_r(dY))
    rep.grad(tag + " wgrad", m, rec.cname + ".weight", W.grad, 5e-3)
    if every_route:
        _pool_link(rec.src, rep, tag)
    blk = [u for kd, u in eng.units2 if kd == "blk" and u.rec1 is rec]
    rtag = tag[:-len("double_conv.0")]
    if every_route and blk and blk[0].cin != blk[0].cout:
        # the residual branch's own tensors: its output as stored (blk.res), and its bias gradient = the column sums of g
        b_ = blk[0]
        rname = b_.prefix + ".res_conv"
        g = nchw(b_.bw["g"])
        Yr = F.conv2d(X.detach(), _r(sd[rname + ".weight"])) + sd[rname + ".bias"].float().reshape(1, -1, 1, 1)
        rep.close(rtag + "res_conv forward", nchw(b_.res[0][..., b_.res[2]:b_.res[2] + b_.cout]), Yr, 4e-3, 1.2e-2)
        rep.grad(rtag + "res_conv dbias", m, rname + ".bias", g.sum((0, 2, 3)), 2e-3)
        if getattr(rec, "dsrc", None) is None:
            Wr = _r(sd[rname + ".weight"]).requires_grad_(True)
            F.conv2d(X.detach(), Wr).backward(_r(g))
            rep.grad(rtag + "res_conv wgrad", m, rname + ".weight", Wr.grad, 5e-3)
    if getattr(rec, "dsrc", None) is None:
        return
    if blk:
        # the block's FIRST convolution: its data-gradient buffer also receives the residual branch's gradient (unet2.py:62-65,72):
        # d_x = conv^T(dY1) + g for the identity, + res_conv^T(g) for the 1x1 convolution
        blk = blk[0]
        # (where the data gradient was ADDED into the tensor that held g -- abc_conv_desc.accumulate, rec.dsrc_accumulated -- that
        #  tensor now holds d_x: g comes from its own inputs, and this check covers the cbam_bwd1 link "g = dOut * [out > 0]" too)
        g = _block_g_ref(blk) if getattr(rec, "dsrc_accumulated", False) else nchw(blk.bw["g"])
        if blk.cin == blk.cout:
            ref = X.grad + g
        else:
            Wr = _r(sd[blk.prefix + ".res_conv.weight"]).requires_grad_(True)
            F.conv2d(X, Wr).backward(_r(g))
            ref = X.grad
            rep.grad(rtag + "res_conv wgrad", m, blk.prefix + ".res_conv.weight", Wr.grad, 5e-3)
        rep.close(tag + " dgrad + residual", nchw(rec.dsrc), ref, 8e-3)
    else:
        rep.close(tag + _dgrad_tag(rec), nchw(rec.dsrc), _dgrad_ref(rec, X.grad), 5e-3)


def _block_g_ref(blk):
    """g = d(out) * [out > 0] of a unet2 block (unet2.py:73) from the gradient sources its consumers left and its own stored output"""
    C_ = blk.cout
    got_out = nchw(blk.out[..., blk.coff_out:blk.coff_out + C_])
    dOut = torch.zeros_like(got_out)
    if blk.grad_same is not None:
        t, ld, co = blk.grad_same
        dOut = dOut + nchw(t[..., co:co + C_])
    if blk.grad_pool is not None:
        t, ld, co = blk.grad_pool
        oo = got_out.detach().clone().requires_grad_(True)
        F.max_pool2d(oo, 2).backward(nchw(t[..., co:co + C_]))
        dOut = dOut + oo.grad
    return dOut * (got_out > 0).float()


def _cbam_links(eng, blk, m, rep, sd):
    """unet2.py:6-74 forward + backward of one block on the engine's own tensors (as tests/test_gpu_model.py::
    test_unet2_block_is_exact_in_situ, at the bf16 bounds)"""
    prefix = blk.prefix
    tag = "unet2 " + prefix
    rep.ledger.visit(blk)
    rec2 = blk.rec2
    p = prefix + ".double_conv"
    mlp = p + ".5.channel_attention.shared_MLP"
    c7 = p + ".5.spatial_attention.conv2d"
    C_ = blk.cout
    leaf = lambda t: t.detach().clone().requires_grad_(True)
    y2 = leaf(nchw(rec2.y[..., rec2.coff:rec2.coff + C_]))
    w1, b1, w2, b2 = (leaf(sd[mlp + k]) for k in (".0.weight", ".0.bias", ".2.weight", ".2.bias"))
    w7, b7 = leaf(sd[c7 + ".weight"]), leaf(sd[c7 + ".bias"])
    rt, ld_r, c_r, pooled_r = blk.res
    r_full = nchw(rt[..., c_r:c_r + C_])
    if pooled_r:
        r_full = F.max_pool2d(r_full, 2)
    r = leaf(r_full)
    # BatchNorm with the ENGINE's batch statistics (its sums come from the f32 accumulators, before y2 was rounded to bf16)
    gamma, beta = leaf(sd[rec2.bname + ".weight"]), leaf(sd[rec2.bname + ".bias"])
    mean, invstd = rec2.mean.view(1, -1, 1, 1), rec2.invstd.view(1, -1, 1, 1)
    z = (y2 - mean) * invstd * gamma.view(1, -1, 1, 1) + beta.view(1, -1, 1, 1)

    def mlp_f(v):
        return F.linear(F.relu(F.linear(v, w1, b1)), w2, b2)

    # AdaptiveMaxPool2d(1) with torch's arg-max rule spelled out (the FIRST maximal pixel gets the gradient; in bf16 several
    # pixels tie); max over channels at the ENGINE's arg-max channel (a decision: taken from the engine)
    zf = z.flatten(2)
    first = zf.detach().argmax(dim=2, keepdim=True)
    ca = torch.sigmoid(mlp_f(F.adaptive_avg_pool2d(z, 1).flatten(1)) + mlp_f(zf.gather(2, first).squeeze(2)))
    o1 = ca[:, :, None, None] * z
    st = torch.cat([torch.mean(o1, dim=1, keepdim=True), o1.gather(1, blk.amax[:, None].long())], 1)
    rep.close(tag + " arg-max of the global max-pool", blk.first.float(), first.squeeze(2).float(), 0.0, 0.0)
    sa = torch.sigmoid(F.conv2d(st, w7, b7, padding=3))
    out = F.relu(sa * o1 + r)
    rep.close(tag + " ca", blk.ca, ca.detach(), 5e-3)
    rep.close(tag + " [mean, max] over channels", blk.st.permute(0, 3, 1, 2), st.detach(), 5e-3)
    rep.close(tag + " sa", blk.sa.unsqueeze(1), sa.detach(), 5e-3)
    got_out = nchw(blk.out[..., blk.coff_out:blk.coff_out + C_])
    rep.close(tag + " out", got_out, out.detach(), 5e-3)
    dOut = torch.zeros_like(out)
    if blk.grad_same is not None:
        t, ld, co = blk.grad_same
        dOut = dOut + nchw(t[..., co:co + C_])
    if blk.grad_pool is not None:
        t, ld, co = blk.grad_pool
        oo = got_out.detach().clone().requires_grad_(True)
        F.max_pool2d(oo, 2).backward(nchw(t[..., co:co + C_]))
        dOut = dOut + oo.grad
    mask = (got_out > 0).float()
    bw = blk.bw
    g_in = dOut * mask
    # cbam_bwd1 forms g, stores it and takes the spatial branch's du from the f32 g it still holds: the 7 x 7 convolution's gradients
    # come from the UNROUNDED g (measured on down4 at 1 x 72 x 88, 20 pixels: 1.1e-4 so, 2.2e-3 from the stored g)
    dw7_ref, db7_ref = torch.autograd.grad(sa * o1 + r, (w7, b7), g_in, retain_graph=True)
    if not getattr(blk.rec1, "dsrc_accumulated", False):     # (else the tensor holds d_x by now: checked with the first convolution's data gradient)
        rep.close(tag + " g = dOut * [out > 0]", nchw(bw["g"]), g_in, 5e-3)
        # the backward kernels behind cbam_bwd1 (cbam_bwd2, cbam_bwd3) read the g it STORED: the links below start from that tensor, the engine's own, as
        # every link does.  It differs from dOut * mask only on a block with two gradient routes (inc3, down3, down4: bf16(same +
        # pooled), 1.2e-3 in the link above), and there the sums over the pixels of d(ca), which cancel, carry that rounding into the
        # shared MLP's gradients: the floor of the reference alone -- its g rounded against unrounded -- is printed beside them
        g_st = nchw(bw["g"])
        if blk.grad_same is not None and blk.grad_pool is not None:
            pre, mlp_leaves = sa * o1 + r, (w1, b1, w2, b2)
            ga = torch.autograd.grad(pre, mlp_leaves, g_in, retain_graph=True)
            gb = torch.autograd.grad(pre, mlp_leaves, _r(g_in), retain_graph=True)
            for k, a_, b_ in zip((".0.weight", ".0.bias", ".2.weight", ".2.bias"), ga, gb):
                rep.info(tag + " mlp" + k + " floor (g rounded to bf16)", (b_ - a_).double().norm().item() / (a_.double().norm().item() + 1e-30))
        g_in = g_st
    (sa * o1 + r).backward(g_in)
    # d(y2): through CBAM (both attention branches, the global and per-pixel max routes) and BatchNorm's batch statistics
    n = y2.shape[0] * y2.shape[2] * y2.shape[3]
    xh = ((y2 - mean) * invstd).detach()
    # autograd above treated mean / invstd as constants: finish BatchNorm's backward in closed form
    dzz = y2.grad / (invstd * gamma.detach().view(1, -1, 1, 1))          # = d(loss)/d(z)
    dbeta, dgamma = dzz.sum((0, 2, 3)), (dzz * xh).sum((0, 2, 3))
    dy2 = gamma.detach().view(1, -1, 1, 1) * invstd * (dzz - dbeta.view(1, -1, 1, 1) / n - xh * dgamma.view(1, -1, 1, 1) / n)
    rep.grad(tag + " dgamma2", m, rec2.bname + ".weight", dgamma, 1e-2)
    rep.grad(tag + " dbeta2", m, rec2.bname + ".bias", dbeta, 1e-2)
    if getattr(rec2, "dY", None) is not None:
        rep.close(tag + " d(y2) (stored)", nchw(rec2.dY), dy2, 1e-2)       # (measured 2.9e-3: two bf16 roundings, dz and dY)
    rep.grad(tag + " dw7", m, c7 + ".weight", dw7_ref, 2e-3)
    rep.grad(tag + " db7", m, c7 + ".bias", db7_ref, 2e-3)
    for k, t in ((".0.weight", w1), (".0.bias", b1), (".2.weight", w2), (".2.bias", b2)):
        rep.grad(tag + " mlp" + k, m, mlp + k, t.grad, 2e-3)          # (measured <= 1.5e-4)


def walk_unet(eng, m, rep, sd, tg):
    """every link of a unet.py plan: the heads by form, then every conv / convT record of the trunk in plan order"""
    B, h, w = eng.B, eng.h, eng.w
    with torch.enable_grad():
        if eng.hf is not None:
            _heads_links(eng, m, rep, sd, tg, B, h, w, every_link=True)
        else:
            _heads_unfused_links(eng, m, rep, sd, tg, B, h, w)
        for r in eng.recs:
            if getattr(r, "is_head", False):
                continue
            if r.kind == "conv":
                _conv_links(r, m, rep, sd, every_route=True)
            elif r.kind == "convT":
                _convT_links(r, m, rep, sd, forward=True)


def walk_unet2(eng, m, rep, sd, tg):
    """every link of a unet2.py plan: the heads by form, then every unit -- a block's two convolutions, its residual branch and its
    CBAM, or a transposed convolution"""
    B, h, w = eng.B, eng.h, eng.w
    with torch.enable_grad():
        if eng.hf is not None:
            _heads_links(eng, m, rep, sd, tg, B, h, w, every_link=True)
        else:
            _heads_unfused_links(eng, m, rep, sd, tg, B, h, w)
        for kind, u in eng.units2:
            if kind == "convT":
                _convT_links(u, m, rep, sd, forward=True)
                continue
            _conv2_links(eng, u.rec1, m, rep, sd, every_route=True)
            _conv2_links(eng, u.rec2, m, rep, sd, every_route=True)
            _cbam_links(eng, u, m, rep, sd)
