"""GPU parity of the stand-alone loss kernels (csrc/loss.hip: loss_kernel, loss_finalize_kernel, loss_scale_kernel) where the other
loss tests never go: ragged maps (dead lanes, workgroups that straddle two images, map lengths with every n % 4 tail, a block count
that is no multiple of 64) and logits inside the clamp at 1e-5 / 1 - 1e-5 (loss_math.hpp: the derivative through `inside` is zero
there), with the rho head at z == 0 and |z| == t_rho exactly.

Reference: oracle/loss_oracle.abc_loss on the CPU under torch autograd, once in f64 (the truth) and once in f32 (the reference's own
arithmetic, which sets the yardstick).  Gradients are compared element by element, no sampling and no norm: 98 % of the 360-channel
head's gradient is zero, so a wrong branch on a few pixels or a wrong plane on a ragged map disappears in a whole-tensor norm.
"""
import functools

import pytest
import torch

import abcnet_amd  # noqa: F401
from abcnet_amd import _lib as L
from abcnet_amd.engine import head_offsets
from abcnet_amd.loss import abc_loss
from abcnet_amd.ops import HEAD_NAMES, FusedLoss
from abcnet_amd.synthetic import synthetic_targets
from oracle import loss_oracle

HEADS = [1, 14, 3, 2, 1, 360, 60, 60]
SIGMOID, SOFTMAX, RHO = (0, 4, 7), (1, 2, 3, 5), 6
S_INDEX = [0, 2, 3, 9, 1, 4, 6, 7]      # head -> entry of s (train.py:127-135); entries 5 and 8 belong to no term
S_EXPFAC = [1, 1, 1, 1, 1, 1, 0.5, 1]
DEV = "cuda"
LO = 1e-5

# (B, h, w): the edge each one is there for
SHAPES = [
    (1, 3, 3),      # 9 pixels: one workgroup, mostly dead lanes; map lengths below 4 and with tails
    (1, 5, 7),      # 35: map lengths 35 / 490 / 105 / 70 leave n % 4 = 3 / 2 / 1 / 2, every scalar tail of loss_scale_kernel
    (3, 9, 13),     # 351, hw = 117: workgroups straddle images, the last one is ragged
    (2, 8, 16),     # 256: exact
    (1, 64, 65),    # 4160: 65 loss blocks, the finaliser's 64-way strided sum has a remainder
]
# target seed per shape: the first ones at which, after the crop, every denominator is positive and every branch listed in
# test_inputs_reach_every_branch is reached (found on the CPU; the test asserts both)
SEEDS = {(1, 3, 3): 1, (1, 5, 7): 1, (3, 9, 13): 1, (2, 8, 16): 1, (1, 64, 65): 1}

# An activation within 1 % of a clamp bound: the derivative jumps by O(1) across the bound, and an f32 kernel and the f64 oracle may
# legitimately fall on different sides.  Such sigmoid elements, and whole softmax groups with such a class, leave the element check.
BAND = 1e-2
MAX_EXCLUDED = 2e-3     # of all logit elements of a shape; measured share: see test_inputs_reach_every_branch
# Element statistic of a head's gradient: E = max |g - g64| / (|g64| + 1e-6 max|g64|); bound max(3 E(f32 oracle), GRAD_FLOOR).
# The f32 oracle's own E runs from 2e-8 (rho) to 1.9e-5 (atom types), hence the floor.
# Measured kernel E on the MI355X (oracle E beside it), worst head of each shape:
#   1 x 3 x 3   8.8e-06 (8.1e-06, atom_charges)      1 x 5 x 7   3.1e-06 (3.0e-06, bond_t)      3 x 9 x 13  1.9e-05 (2.0e-05, bond_types)
#   2 x 8 x 16  1.3e-05 (1.2e-05, bond_types)        1 x 64 x 65 2.95e-04 (9.6e-05, atom_charges); its other heads at most 2.2e-05
GRAD_FLOOR = 2e-5
# The one figure above the floor is ONE element, atom_charges at 1 x 64 x 65, pixel (20, 31), class 1: logits (0.671, 1.051, 1.539) under
# targets (1, 0.5, 0).  A softmax gradient is q_k (a_k - sum_j a_j q_j), and there a_1 = -1.6436 stands against a sum of -1.6429: the
# gradient, -1.5e-7, is 4340 times smaller than the terms it is the difference of, so ONE f32 rounding of a term moves it by
# 4340 * 2^-24 = 2.6e-4 of itself.  The kernel lands 2.95e-4 away and the f32 oracle 0.96e-4 away, each about one rounding: three times the
# oracle's luck (2.87e-4) is no bound there.  So a softmax head's bound also admits CANCEL_ROUNDINGS f32 roundings at the worst
# cancellation of its own inputs, kappa = max_k q_k (|a_k| + sum_j |a_j q_j|) / (|g_k| + 1e-6 max|g|), computed in f64 on the CPU from
# the inputs alone (reference()): 5.2e-4 for that head, below 2e-5 (so without effect) for every other head and shape, never above 1e-3.
CANCEL_ROUNDINGS = 2


def edge_targets(B, h, w, seed=1):
    """synthetic_targets on the square max(h, w) map cropped to [h, w]: dense enough (one atom and one bond per 12 pixels) that every
    term's denominator survives the crop; rho rounded through f32 so that an f32 logit can equal it exactly"""
    S = max(h, w)
    n = max(S * S // 12, 2)
    tg = [t[..., :h, :w].contiguous() for t in synthetic_targets(B, S, seed=seed, n_atoms=n, n_bonds=n)]
    tg[6] = tg[6].float().double()
    dens = [(tg[0] == 1).sum(), tg[1].sum(), tg[2].sum(), tg[3].sum(), (tg[4] == 1).sum(), tg[5].sum(), tg[7].sum()]
    assert all(d.item() > 0 for d in dens), ("a denominator is empty after the crop", (B, h, w, seed), [d.item() for d in dens])
    return tg


def edge_inputs(B, h, w, seed=None):
    """(preds, targets, s) on the CPU.  Logits: 70 % randn * 2, 25 % saturated +-U(14, 30) (clamped as a sigmoid, and as a softmax
    class against an unsaturated maximum), 5 % exactly 0; on the rho head 30 % of the labelled places sit at +-t_rho exactly and
    10 % at 0."""
    seed = SEEDS.get((B, h, w), 1) if seed is None else seed
    tg = edge_targets(B, h, w, seed)
    g = torch.Generator().manual_seed(7919 * seed + 100 * h + w)
    sign = lambda shape: torch.where(torch.rand(shape, generator=g) < 0.5, -1.0, 1.0)

    def mix(shape):
        u = torch.rand(shape, generator=g)
        z = torch.randn(shape, generator=g) * 2.0
        sat = sign(shape) * (torch.rand(shape, generator=g) * 16.0 + 14.0)
        z = torch.where(u < 0.25, sat, z)
        return torch.where(u >= 0.95, torch.zeros(()), z)

    preds = [mix((B, c, h, w)) for c in HEADS]
    lab = tg[5].sum(1) > 0
    u = torch.rand(lab.shape, generator=g)
    z = torch.where(lab & (u < 0.3), sign(lab.shape) * tg[6].float(), preds[6])
    preds[6] = torch.where(lab & (u >= 0.3) & (u < 0.4), torch.zeros(()), z)
    s = torch.rand(10, generator=g) * 0.4 - 0.2
    return preds, tg, s


def _near(a):
    return (a / LO - 1).abs() < BAND


def clamp_band(logits):
    """per head, a bool map of the logits' shape: True where the element check does not apply (f64 activations on the CPU)"""
    out = []
    for i, z in enumerate(logits):
        z = z.detach().double().cpu()
        if i in SIGMOID:
            out.append(_near(torch.sigmoid(z)) | _near(torch.sigmoid(-z)))
        elif i in SOFTMAX:
            zz = z.view(z.shape[0], 6, 60, *z.shape[2:]) if i == 5 else z
            q = torch.softmax(zz, dim=1)
            out.append((_near(q) | _near(1 - q)).any(1, keepdim=True).expand_as(q).reshape(z.shape))
        else:
            out.append(torch.zeros(z.shape, dtype=torch.bool))
    return out


def _oracle(preds, tg, s, dt):
    p = [x.detach().clone().to(dt).requires_grad_(True) for x in preds]      # (copies: the shared inputs stay plain tensors)
    sv = s.detach().clone().to(dt).requires_grad_(True)
    total, weighted, terms = loss_oracle.abc_loss(p, [t.double() for t in tg] if dt == torch.float64 else tg, sv)
    total.backward()
    out = torch.stack([total.detach().double()] + [weighted[n].detach().double() for n in HEAD_NAMES]
                      + [terms[n].detach().double() for n in HEAD_NAMES])
    return out, sv.grad.double(), [x.grad.double() for x in p]


@functools.lru_cache(maxsize=None)
def reference(B, h, w):
    """everything the tests of one shape share, computed once on the CPU and never modified"""
    preds, tg, s = edge_inputs(B, h, w)
    out64, ds64, g64 = _oracle(preds, tg, s, torch.float64)
    out32, ds32, g32 = _oracle(preds, tg, s, torch.float32)
    excl = clamp_band(preds)
    share = sum(e.sum().item() for e in excl) / sum(e.numel() for e in excl)
    hi = 1 - 1e-5
    cover, zero = {}, [None] * 8
    for i in SIGMOID:
        a = torch.sigmoid(preds[i].double())
        cover["head %d clamped low" % i] = ((a < LO) & ~excl[i]).sum().item()
        cover["head %d clamped high" % i] = ((a > hi) & ~excl[i]).sum().item()
        zero[i] = ((a < LO) | (a > hi)) & ~excl[i]
    for i in SOFTMAX:
        z, t = preds[i].double(), tg[i]
        if i == 5:
            z = z.view(B, 6, 60, h, w)
        q = torch.softmax(z, dim=1)
        clamped, hit = (q < LO) | (q > hi), t != 0
        cover["head %d clamped classes with a target" % i] = (clamped & hit).sum().item()
        # no gradient reaches a group whose every labelled class is clamped (and one that carries no label at all)
        dead = (clamped | ~hit).all(1, keepdim=True)
        cover["head %d labelled groups with every label clamped" % i] = (dead & hit.any(1, keepdim=True)).sum().item()
        zero[i] = dead.expand_as(q).reshape(preds[i].shape) & ~excl[i]
    z, tr, lab = preds[RHO], tg[6], tg[5].sum(1) > 0
    cover["rho z == 0 at a label"] = (lab & (z == 0)).sum().item()
    cover["rho |z| == t_rho at a label"] = (lab & (z.abs().double() == tr)).sum().item()
    cover["rho z < 0 and |z| > t_rho at a label"] = (lab & (z < 0) & (z.abs().double() > tr)).sum().item()
    zero[RHO] = (z == 0) | (z.abs().double() == tr) | ~lab
    kappa = [0.0] * 8
    for i in SOFTMAX:
        z, t = preds[i].double(), tg[i].double()
        if i == 5:
            z = z.view(B, 6, 60, h, w)
        q = torch.softmax(z, dim=1)
        p = q.clamp(LO, hi)
        a = -t * (-2 * (1 - p) * p.log() + (1 - p) ** 2 / p) * ((q >= LO) & (q <= hi))
        if i == 1:
            a = a * torch.tensor(loss_oracle.ATOM_TYPE_WEIGHTS, dtype=torch.float64).view(1, 14, 1, 1)
        g = q * (a - (a * q).sum(1, keepdim=True))
        k = q * (a.abs() + (a * q).abs().sum(1, keepdim=True)) / (g.abs() + 1e-6 * g.abs().max() + 1e-300)
        kappa[i] = torch.where(excl[i].view(k.shape), torch.zeros(()).double(), k).max().item()
        # (g is the oracle's gradient up to the head's factor: the formula above is the one the oracle differentiates)
        f = g64[i].abs().sum() / g.abs().sum().clamp_min(1e-300)
        assert ((g * f).reshape(g64[i].shape) - g64[i]).abs().max() <= 1e-8 * g64[i].abs().max(), i
    # the oracle agrees that these are exact zeros; the kernel is then held to every exact zero of the oracle outside the band
    for i in range(8):
        assert not g64[i][zero[i]].any(), ("the f64 oracle's gradient is not zero where the derivation says so", i)
        zero[i] = (g64[i] == 0) & ~excl[i]
    return dict(preds=preds, tg=tg, s=s, out64=out64, out32=out32, ds64=ds64, ds32=ds32, g64=g64, g32=g32, excl=excl, share=share,
                cover=cover, zero=zero, kappa=kappa)


def elem_err(g, g64, excl):
    g, g64 = g.detach().double().cpu(), g64.double()
    e = (g - g64).abs() / (g64.abs() + 1e-6 * g64.abs().max() + 1e-300)
    e = torch.where(excl, torch.zeros(()).double(), e)
    return e.max().item(), e


def _check_values(got, r, what):
    got = got.detach().double().cpu()
    for k in range(17):
        t64, t32 = r["out64"][k].item(), r["out32"][k].item()
        bound = max(3 * abs(t32 - t64), 1e-6 * abs(t64))
        print("  %s out[%d] kernel %.12g f64 %.12g |d| %.3g bound %.3g" % (what, k, got[k].item(), t64, abs(got[k].item() - t64), bound))
        assert abs(got[k].item() - t64) <= bound, (what, k, got[k].item(), t64, t32, bound)


def _check_ds(ds, r, scale, what):
    ds = ds.detach().double().cpu()
    for k in range(10):
        d64, d32 = r["ds64"][k].item() * scale, r["ds32"][k].item() * scale
        if k in (5, 8):
            assert ds[k].item() == 0.0 and d64 == 0.0, (what, k, ds[k].item())
            continue
        bound = max(3 * abs(d32 - d64), 1e-6 * abs(d64), 1e-7 * scale)
        assert abs(ds[k].item() - d64) <= bound, (what, k, ds[k].item(), d64, d32, bound)


def _check_grads(grads, r, shape, what):
    """grads[i]: the kernel's d(loss)/d(logits of head i), any scale (the statistic is relative) -- r["g64"][i] times that scale"""
    for i in range(8):
        g, excl = grads[i].detach().double().cpu(), r["excl"][i]
        ek, e = elem_err(g, r["g64"][i], excl)
        eo, _ = elem_err(r["g32"][i], r["g64"][i], excl)
        bound = max(3 * eo, GRAD_FLOOR, min(CANCEL_ROUNDINGS * r["kappa"][i] * 2.0 ** -24, 1e-3))
        print("  %s %s head %d (%s): kernel E %.3g, f32 oracle E %.3g, bound %.3g (kappa %.0f), excluded share of the shape %.4f %%"
              % (what, shape, i, HEAD_NAMES[i], ek, eo, bound, r["kappa"][i], 100 * r["share"]))
        if ek > bound:
            bad = (e > bound).nonzero()
            print("    over the bound: %d elements, first %s" % (len(bad), [(tuple(ix.tolist()), g[tuple(ix)].item(),
                  r["g64"][i][tuple(ix)].item(), r["preds"][i][tuple(ix)].item()) for ix in bad[:8]]))
        assert ek <= bound, (what, shape, i, ek, eo, bound)
        z = r["zero"][i]
        assert (g[z] == 0).all(), (what, shape, i, "non-zero where the gradient is exactly zero", (g[z] != 0).sum().item())


@pytest.mark.parametrize("B,h,w", SHAPES)
def test_inputs_reach_every_branch(B, h, w):
    """the inputs themselves, from the f64 oracle on the CPU: few elements near a clamp bound, and every branch the file is about is
    taken in every shape (1 x 3 x 3 is too small to promise them all).  Measured excluded share: 0.00 - 0.08 %."""
    r = reference(B, h, w)
    print("  %s excluded %.4f %% of the logits; %s" % ((B, h, w), 100 * r["share"], r["cover"]))
    assert r["share"] <= MAX_EXCLUDED, r["share"]
    if (B, h, w) != (1, 3, 3):
        for k, v in r["cover"].items():
            assert v > 0, (k, r["cover"])


@pytest.mark.gpu
@pytest.mark.parametrize("B,h,w", SHAPES)
def test_loss_and_every_gradient_element(B, h, w):
    r = reference(B, h, w)
    assert r["share"] <= MAX_EXCLUDED
    pd = [p.to(DEV).requires_grad_(True) for p in r["preds"]]
    sd = r["s"].to(DEV).requires_grad_(True)
    loss, out = abc_loss(pd, [t.to(DEV) for t in r["tg"]], sd, return_terms=True)
    loss.backward()
    assert out[0].item() == loss.item()
    _check_values(out, r, "abc_loss")
    _check_ds(sd.grad, r, 1.0, "abc_loss")
    _check_grads([p.grad for p in pd], r, (B, h, w), "abc_loss")


class _Engine:
    """what ops.FusedLoss reads of an engine"""


@pytest.mark.gpu
@pytest.mark.parametrize("B,h,w", SHAPES)
def test_fused_loss_form_of_the_trainer(B, h, w):
    """ops.FusedLoss: unscaled d(numerator)/d(logits), a per-channel factor weight_i / den_i * grad_scale over all 441 channels, and
    ds times grad_scale"""
    r = reference(B, h, w)
    gs = 0.25
    e = _Engine()
    e.lib, e.B, e.h, e.w, e.heads, e.head_off = L.load(), B, h, w, HEADS, head_offsets(HEADS)
    e.logits = [p.to(DEV).contiguous() for p in r["preds"]]
    e.dlogits = [torch.zeros_like(t) for t in e.logits]
    e.chan_scale = torch.zeros(sum(HEADS), device=DEV)
    sdev, ds = r["s"].to(DEV), torch.zeros(10, device=DEV)
    fl = FusedLoss(e, [t.to(DEV) for t in r["tg"]], sdev.data_ptr(), ds.data_ptr(), grad_scale=gs)
    fl.run(torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    _check_values(fl.out, r, "FusedLoss")
    _check_ds(ds, r, gs, "FusedLoss")
    cs = e.chan_scale.double().cpu()
    s64 = r["s"].double()
    for i, c in enumerate(HEADS):
        wgt = S_EXPFAC[i] * torch.exp(-s64[S_INDEX[i]]) + s64[S_INDEX[i]]
        # weighted term / raw term = weight; raw term = numerator / denominator, so weight / den comes from the oracle's own values
        tg = r["tg"][i]
        den = (tg == 1).sum().double() if i in (0, 4) else r["tg"][5].sum().double() if i == RHO else tg.sum().double()
        if i == 3:
            den = den + 0.1
        assert abs(r["out64"][1 + i].item() / r["out64"][9 + i].item() - wgt.item()) <= 1e-12 * wgt.item()
        want = (wgt / den * gs).item()
        got = cs[e.head_off[i]:e.head_off[i] + c]
        assert ((got - want).abs() <= 1e-6 * abs(want)).all(), ("chan_scale", i, got[0].item(), want)
    grads = [e.dlogits[i].double().cpu() * cs[e.head_off[i]:e.head_off[i] + c].view(1, c, 1, 1) / gs for i, c in enumerate(HEADS)]
    _check_grads(grads, r, (B, h, w), "FusedLoss")


@pytest.mark.gpu
def test_incoming_gradient_reaches_every_tail_element():
    """(2.5 * loss).backward() at 1 x 5 x 7, where every map has a scalar tail in loss_scale_kernel: an element the tail skipped would
    be off by its head's whole factor"""
    r = reference(1, 5, 7)
    tdev = [t.to(DEV) for t in r["tg"]]
    res = []
    for f in (None, 2.5):
        pd = [p.to(DEV).requires_grad_(True) for p in r["preds"]]
        sd = r["s"].to(DEV).requires_grad_(True)
        loss = abc_loss(pd, tdev, sd)
        (loss if f is None else f * loss).backward()
        res.append([p.grad for p in pd] + [sd.grad])
    for a, b in zip(res[1], res[0]):
        assert b.any()
        torch.testing.assert_close(a, 2.5 * b, rtol=1e-6, atol=1e-12)
