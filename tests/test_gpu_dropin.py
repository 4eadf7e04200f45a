"""GPU tier of the drop-in training loop: abcnet_amd.loss.abc_loss (train.py:95-137 as one autograd op) and
abcnet_amd.optim.Adam (train.py:55) against the golden vectors, torch autograd on the oracle, torch.optim.Adam and the
fused Trainer."""
import copy
import os

import numpy as np
import pytest
import torch
import torch.nn as nn

pytestmark = pytest.mark.gpu

import abcnet_amd  # noqa: E402,F401
from abcnet_amd.loss import ABCLoss, abc_loss, terms_dict  # noqa: E402
from abcnet_amd.optim import Adam  # noqa: E402
from abcnet_amd.synthetic import synthetic_images, synthetic_targets  # noqa: E402
from abcnet_amd.unet import UNet  # noqa: E402
from oracle import loss_oracle  # noqa: E402
from oracle import unet_oracle as uo  # noqa: E402

HEADS = uo.HEADS
DEV = "cuda"


def _golden_inputs():
    """the seeded preds / targets / s of tests/golden/loss_128.npz, built as test_fused_loss_matches_golden builds them"""
    g = torch.Generator().manual_seed(11)
    preds = [torch.randn((2, c, 128, 128), generator=g) * 2.0 for c in HEADS]
    tg = synthetic_targets(2, 128, seed=1)
    s = torch.rand(10, generator=g) * 0.4 - 0.2
    return preds, tg, s


def _leaves(preds, s):
    return ([p.to(DEV).requires_grad_(True) for p in preds], s.to(DEV).requires_grad_(True))


def _rel(a, b):
    return ((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-30)).item()


def test_loss_matches_golden(golden_dir):
    gold = np.load(os.path.join(golden_dir, "loss_128.npz"))
    preds, tg, s = _golden_inputs()
    preds, s = _leaves(preds, s)
    loss, out = abc_loss(preds, [t.to(DEV) for t in tg], s, return_terms=True)
    assert loss.dim() == 0 and loss.dtype == torch.float64 and loss.is_cuda
    loss.backward()
    assert abs(loss.item() - gold["loss"].item()) < 1e-5 * abs(gold["loss"].item())
    assert terms_dict(out)["total"] == loss.item()
    np.testing.assert_allclose(s.grad.cpu().double().numpy(), gold["ds"], rtol=1e-4, atol=1e-7)
    for i in range(8):
        f = preds[i].grad.cpu().reshape(-1)         # true gradients: no chan_scale applied here
        step = max(f.numel() // 1031, 1)
        np.testing.assert_allclose(f[::step][:1031].double().numpy(), gold["dlogit%d_sample" % i], rtol=2e-3, atol=1e-7)
        n = gold["dlogit%d_norm" % i].item()
        assert abs(f.double().norm().item() - n) < 1e-4 * n, i


def test_loss_matches_oracle_autograd_and_scales_like_autograd():
    preds, tg, s = _golden_inputs()
    # the oracle in f64, differentiated by torch autograd
    p64 = [p.double().requires_grad_(True) for p in preds]
    s64 = s.double().requires_grad_(True)
    ref, _, _ = loss_oracle.abc_loss(p64, [t.double() for t in tg], s64)
    ref.backward()
    tdev = [t.to(DEV) for t in tg]
    pd, sd = _leaves(preds, s)
    loss = ABCLoss()(pd, tdev, sd)
    loss.backward()
    assert abs(loss.item() - ref.item()) < 1e-5 * abs(ref.item())
    np.testing.assert_allclose(sd.grad.cpu().double().numpy(), s64.grad.numpy(), rtol=1e-4, atol=1e-7)
    for i in range(8):
        assert _rel(pd[i].grad.cpu(), p64[i].grad) < 1e-4, i
    g1 = [p.grad.clone() for p in pd] + [sd.grad.clone()]
    # (2.5 * loss).backward(): the incoming gradient is read on the device
    pd2, sd2 = _leaves(preds, s)
    (2.5 * abc_loss(pd2, tdev, sd2)).backward()
    for a, b in zip([p.grad for p in pd2] + [sd2.grad], g1):
        torch.testing.assert_close(a, 2.5 * b, rtol=1e-6, atol=1e-12)
    # (loss + loss2).backward(): two ops on the same leaves sum as autograd sums
    tg2 = [t.to(DEV) for t in synthetic_targets(2, 128, seed=5)]
    pa, sa = _leaves(preds, s)
    abc_loss(pa, tg2, sa).backward()
    g2 = [p.grad.clone() for p in pa] + [sa.grad.clone()]
    pb, sb = _leaves(preds, s)
    (abc_loss(pb, tdev, sb) + abc_loss(pb, tg2, sb)).backward()
    for a, b, c in zip([p.grad for p in pb] + [sb.grad], g1, g2):
        torch.testing.assert_close(a, b + c, rtol=1e-6, atol=1e-12)
    # one op, one backward: a second backward through the same op is refused, not silently rescaled
    pc, sc = _leaves(preds, s)
    lc = abc_loss(pc, tdev, sc)
    lc.backward(retain_graph=True)
    with pytest.raises(RuntimeError, match="twice"):
        lc.backward()
    # non-contiguous preds are accepted
    pn = [p.to(DEV).transpose(2, 3).contiguous().transpose(2, 3) for p in preds]
    assert not pn[1].is_contiguous()
    assert abs(abc_loss(pn, tdev, s.to(DEV)).item() - loss.item()) < 1e-12 * abs(loss.item())


def _grads(params, seed, none_at=()):
    g = torch.Generator().manual_seed(seed)
    out = []
    for i, p in enumerate(params):
        out.append(None if i in none_at else (torch.randn(p.shape, generator=g) * 10.0 ** (i % 3 - 1)).to(p.device))
    return out


def _set_grads(params, grads):
    for p, g in zip(params, grads):
        p.grad = None if g is None else g.clone()


def _assert_params_close(a, b):
    for x, y in zip(a, b):
        torch.testing.assert_close(x.detach(), y.detach(), rtol=1e-5, atol=1e-7)


def _stack():
    torch.manual_seed(3)
    return nn.Sequential(nn.Conv2d(3, 8, 3), nn.ReLU(), nn.Conv2d(8, 5, 3), nn.Conv2d(5, 7, 1, bias=False)).to(DEV)


def test_adam_matches_torch_on_plain_tensors():
    ma, mb = _stack(), _stack()
    pa, pb = list(ma.parameters()), list(mb.parameters())
    groups = lambda ps: [{"params": ps[:3], "lr": 1e-2, "weight_decay": 1e-2}, {"params": ps[3:], "weight_decay": 0}]
    oa = torch.optim.Adam(groups(pa), lr=3e-3, betas=(0.8, 0.99), foreach=False)
    ob = Adam(groups(pb), lr=3e-3, betas=(0.8, 0.99))
    for k in range(5):
        gr = _grads(pa, k, none_at=(1,) if k == 2 else ())
        _set_grads(pa, gr)
        _set_grads(pb, gr)
        if k == 3:
            oa.param_groups[0]["lr"] = ob.param_groups[0]["lr"] = 5e-4
        oa.step()
        ob.step()
        _assert_params_close(pb, pa)
    for p, q in zip(pa, pb):
        assert oa.state[p]["step"].item() == ob.state[q]["step"].item()
    assert ob.state[pb[1]]["step"].item() == 4.0
    # zero_grad in both modes
    ob.zero_grad(set_to_none=False)
    assert all(p.grad is not None and not p.grad.any() for p in pb[:3] + pb[4:])
    ob.zero_grad()
    assert all(p.grad is None for p in pb)


def _assert_state_close(oa, pa, ob, pb, gmax):
    """exp_avg_sq is a sum of positive terms: the params' tolerance.  exp_avg is a signed average of gradients of magnitude up to gmax
    (_grads draws them at scales 0.1, 1 and 10) and may cancel to nothing, while its error stays that of its terms -- the kernel's
    f32 1 - beta1 is one ulp from torch's f32 0.2, and each update rounds once: the params' atol of 1e-7, which is for unit-size
    terms, times gmax."""
    for p, q, gm in zip(pa, pb, gmax):
        assert oa.state[p]["step"].item() == ob.state[q]["step"].item()
        torch.testing.assert_close(ob.state[q]["exp_avg"], oa.state[p]["exp_avg"], rtol=1e-5, atol=1e-7 * max(1.0, gm))
        torch.testing.assert_close(ob.state[q]["exp_avg_sq"], oa.state[p]["exp_avg_sq"], rtol=1e-5, atol=1e-7)


def _track_gmax(gmax, grads):
    return [max(m, 0.0 if g is None else g.abs().max().item()) for m, g in zip(gmax, grads)]


def test_adam_misaligned_segments_leave_their_neighbours_alone():
    """params that are views into one flat buffer at element offsets 1, 2, 3 mod 4, their grads views of a second buffer at other
    offsets mod 4 (one of them aligned): abc_adam_multi's scalar path for a segment whose p | g | m | v is not 16-byte aligned, on
    counts below, at and above one chunk.  Gaps between the views hold a sentinel that no step may touch."""
    counts = [1, 3, 5, 1023, 1024, 1025, 2051]
    sent = -7.25
    po, go, spans = 0, 0, []
    for k, n in enumerate(counts):
        pm = (1, 2, 3)[k % 3]
        gm = (pm + 1 + k // 3) % 4 if (pm + 1 + k // 3) % 4 != pm else (pm + 2) % 4
        po += 8 + (pm - po) % 4       # at least 8 sentinels before each view, so that no two are adjacent
        go += 8 + (gm - go) % 4
        assert po % 4 == pm and go % 4 == gm and pm != gm and pm != 0
        spans.append((po, go, n))
        po, go = po + n, go + n
    g = torch.Generator().manual_seed(21)
    pbuf = torch.full((po + 8,), sent, device=DEV)
    gbuf = torch.full((go + 8,), sent, device=DEV)
    pgap, ggap = torch.ones(po + 8, dtype=torch.bool, device=DEV), torch.ones(go + 8, dtype=torch.bool, device=DEV)
    pa, pb = [], []
    for o, og, n in spans:
        init = torch.randn(n, generator=g).to(DEV)
        v = pbuf[o:o + n]
        v.copy_(init)
        pgap[o:o + n] = False
        ggap[og:og + n] = False
        pb.append(v.requires_grad_(True))
        pa.append(init.clone().requires_grad_(True))
    assert all(p.data_ptr() % 16 != 0 for p in pb)
    oa = torch.optim.Adam(pa, lr=1e-2, betas=(0.8, 0.99), weight_decay=1e-3, foreach=False)
    ob = Adam(pb, lr=1e-2, betas=(0.8, 0.99), weight_decay=1e-3)
    gmax = [0.0] * len(pa)
    for k in range(4):
        gr = _grads(pa, 30 + k)
        gmax = _track_gmax(gmax, gr)
        _set_grads(pa, gr)
        for p, (o, og, n), x in zip(pb, spans, gr):
            p.grad = gbuf[og:og + n]
            p.grad.copy_(x)
            assert p.grad.data_ptr() == gbuf.data_ptr() + 4 * og
        assert sum(p.grad.data_ptr() % 16 == 0 for p in pb) >= 1 and sum(p.grad.data_ptr() % 16 != 0 for p in pb) >= 4
        oa.step()
        ob.step()
        assert ob.last_segments == len(counts)
        _assert_params_close(pb, pa)
    _assert_state_close(oa, pa, ob, pb, gmax)
    assert (pbuf[pgap] == sent).all() and (gbuf[ggap] == sent).all()
    for p, x in zip(pb, gr):
        assert torch.equal(p.grad, x)         # the gradients are read, never written


def test_adam_aligned_segments_with_tails_across_chunks():
    """separate allocations of 1025, 2050 and 4099 elements: the vector path's last 1, 2 and 3 elements, each in a chunk after full
    ones, with weight decay"""
    g = torch.Generator().manual_seed(22)
    init = [torch.randn(n, generator=g) for n in (1025, 2050, 4099)]
    pa = [x.to(DEV).requires_grad_(True) for x in init]
    pb = [x.to(DEV).requires_grad_(True) for x in init]
    assert all(p.data_ptr() % 16 == 0 for p in pb)
    oa = torch.optim.Adam(pa, lr=1e-2, betas=(0.8, 0.99), weight_decay=1e-2, foreach=False)
    ob = Adam(pb, lr=1e-2, betas=(0.8, 0.99), weight_decay=1e-2)
    gmax = [0.0] * len(pa)
    for k in range(4):
        gr = _grads(pa, 40 + k)
        gmax = _track_gmax(gmax, gr)
        _set_grads(pa, gr)
        _set_grads(pb, gr)
        assert all(p.grad.data_ptr() % 16 == 0 for p in pb)
        oa.step()
        ob.step()
        assert ob.last_segments == 3
        _assert_params_close(pb, pa)
    _assert_state_close(oa, pa, ob, pb, gmax)


def test_adam_more_classes_than_one_launch_takes():
    """40 param groups with their own lr: 40 (group, step) classes, two launches of abc_adam_multi (32 + 8), the second with its
    classes renumbered from 0 and its segments further down the uploaded table.  Two groups decay, and one param skips step 2 so
    that its step count (its bias corrections) differs from its neighbours'."""
    from abcnet_amd import _lib as L
    ngroups = 40
    assert ngroups > L.ADAM_MAX_CLASSES
    g = torch.Generator().manual_seed(23)
    init = [torch.randn(5 + k, generator=g) for k in range(ngroups)]
    pa = [x.to(DEV).requires_grad_(True) for x in init]
    pb = [x.to(DEV).requires_grad_(True) for x in init]
    groups = lambda ps: [{"params": [p], "lr": 1e-3 * (1 + k), "weight_decay": 1e-2 if k in (3, 36) else 0}
                         for k, p in enumerate(ps)]
    oa = torch.optim.Adam(groups(pa), betas=(0.8, 0.99), foreach=False)
    ob = Adam(groups(pb), betas=(0.8, 0.99))
    before = [p.detach().clone() for p in pb]
    gmax = [0.0] * len(pa)
    for k in range(4):
        gr = _grads(pa, 50 + k, none_at=(34,) if k == 2 else ())
        gmax = _track_gmax(gmax, gr)
        _set_grads(pa, gr)
        _set_grads(pb, gr)
        oa.step()
        ob.step()
        assert ob.last_segments == ngroups - (1 if k == 2 else 0)
        _assert_params_close(pb, pa)
    _assert_state_close(oa, pa, ob, pb, gmax)
    assert ob.state[pb[34]]["step"].item() == 3.0 and ob.state[pb[35]]["step"].item() == 4.0
    # groups 33-40 (the second launch) did move, each as torch moved it under its own lr
    for k in range(L.ADAM_MAX_CLASSES, ngroups):
        assert (pb[k].detach() != before[k]).all(), k


def test_adam_state_dict_interchanges_with_torch():
    ma, mb = _stack(), _stack()
    pa, pb = list(ma.parameters()), list(mb.parameters())
    oa = torch.optim.Adam(pa, lr=1e-3, weight_decay=1e-4, foreach=False)
    ob = Adam(pb, lr=1e-3, weight_decay=1e-4)
    for k in range(3):
        gr = _grads(pa, k)
        _set_grads(pa, gr)
        _set_grads(pb, gr)
        oa.step()
        ob.step()
    # torch's state into ours, ours into torch's, each on a copy of the params
    pc = [p.detach().clone() for p in pa]
    pd = [p.detach().clone() for p in pb]
    oc = Adam(pc, lr=1e-3)
    oc.load_state_dict(copy.deepcopy(oa.state_dict()))
    od = torch.optim.Adam(pd, lr=1e-3, foreach=False)
    od.load_state_dict(copy.deepcopy(ob.state_dict()))
    assert od.param_groups[0]["weight_decay"] == 1e-4 and oc.param_groups[0]["weight_decay"] == 1e-4
    for k in range(3, 5):
        gr = _grads(pa, k)
        for ps in (pa, pb, pc, pd):
            _set_grads(ps, gr)
        for o in (oa, ob, oc, od):
            o.step()
        for ps in (pb, pc, pd):
            _assert_params_close(ps, pa)


def test_adam_matches_torch_on_the_unet_arena():
    """on UNet(...).parameters() with the gradients of a real backward (views of one buffer): the arena coalesces -- two
    segments, because s.grad alone is a fresh tensor (autograd sums the network's and the loss's contributions to s)"""
    m = UNet(1, HEADS, dtype="fp32", dropout_p=0.0)
    m.load_state_dict(uo.filled_state("unet", 1, HEADS, seed=0))
    mb = m.to(DEV)
    ma = copy.deepcopy(mb)
    x = synthetic_images(2, 64, seed=7).to(DEV)
    tg = [t.to(DEV) for t in synthetic_targets(2, 16, seed=1)]
    oa = torch.optim.Adam(ma.parameters(), lr=2.5e-4, weight_decay=1e-8, foreach=False)
    ob = Adam(mb.parameters(), lr=2.5e-4, weight_decay=1e-8)
    for k in range(5):
        ob.zero_grad()
        abc_loss(mb(x), tg, mb.s).backward()
        for p, q in zip(ma.parameters(), mb.parameters()):
            p.grad = q.grad.clone()
        oa.step()
        ob.step()
        assert ob.last_segments <= 2
        _assert_params_close(list(mb.parameters()), list(ma.parameters()))
        off, cnt = mb._lay_p["out_modules.5.conv2.weight"]
        assert mb._flat[off:off + cnt].data_ptr() == dict(mb.named_parameters())["out_modules.5.conv2.weight"].data_ptr()


def _flat_rel(ma, mb):
    a = torch.cat([p.detach().reshape(-1) for p in ma.parameters()])
    b = torch.cat([p.detach().reshape(-1) for p in mb.parameters()])
    return _rel(b, a)


def test_reference_loop_fp32_two_steps():
    """Loop A (the reference: torch loss + torch Adam) against loop B (abc_loss + abcnet_amd.optim.Adam).  Adam's first steps
    are ~lr * sign(g): entries whose gradient is near zero move by a whole lr on last-bit differences, and step 2 forwards
    through the moved weights.  So the bound on the parameters is the reference's own spread under a change of loss
    rounding only -- loop C, the same torch loop with the loss evaluated in f64 -- or 1e-5, whichever is larger."""
    B, S = 2, 128
    x = synthetic_images(B, S, seed=7).to(DEV)
    tg = [t.to(DEV) for t in synthetic_targets(B, S // 4, seed=1)]
    tg64 = [t.double() for t in tg]
    torch.manual_seed(0)
    m0 = UNet(1, HEADS, dtype="fp32").to(DEV)
    ma, mb, mc = copy.deepcopy(m0), copy.deepcopy(m0), copy.deepcopy(m0)
    for m in (ma, mb, mc):
        m.train()
    oa = torch.optim.Adam(ma.parameters(), lr=2.5e-4, weight_decay=1e-8)
    ob = Adam(mb.parameters(), lr=2.5e-4, weight_decay=1e-8)
    oc = torch.optim.Adam(mc.parameters(), lr=2.5e-4, weight_decay=1e-8)
    for k in range(2):
        la = loss_oracle.abc_loss(ma(x), tg, ma.s)[0]
        oa.zero_grad()
        la.backward()
        oa.step()
        lb = abc_loss(mb(x), tg, mb.s)
        ob.zero_grad()
        lb.backward()
        ob.step()
        lc = loss_oracle.abc_loss([p.double() for p in mc(x)], tg64, mc.s.double())[0]
        oc.zero_grad()
        lc.backward()
        oc.step()
        assert abs(lb.item() - la.item()) < 1e-5 * abs(la.item())
        rel, floor = _flat_rel(ma, mb), _flat_rel(ma, mc)
        print("fp32 loop step %d: loss %.9g / %.9g, params rel L2 %.3g (reference with an f64 loss: %.3g)"
              % (k + 1, la.item(), lb.item(), rel, floor))
        assert rel < max(1e-5, 3.0 * floor)


# whole-model gradient, relative L2, of the drop-in loop against the Trainer's step in bf16.  The two paths differ only in where
# the f32 head scale is applied: the Trainer multiplies chan_scale into the unscaled dlogits on load in the heads' backward, the
# drop-in op hands over dlogits already scaled in f32 by the same factor -- the same f32 product either way.  Measured: 0 (bit for
# bit); the bound leaves room for nothing more than a reassociation.
BF16_GRAD_BOUND = 1e-6


def test_reference_loop_bf16_against_trainer():
    from abcnet_amd.train import Trainer
    B, S = 2, 128
    x = synthetic_images(B, S, seed=7).to(DEV)
    tg = [t.to(DEV) for t in synthetic_targets(B, S // 4, seed=1)]
    torch.manual_seed(0)
    m0 = UNet(1, HEADS, dtype="bf16").to(DEV)
    ma, mb, mc = copy.deepcopy(m0), copy.deepcopy(m0), copy.deepcopy(m0)
    tr = Trainer(ma, B, S, S, use_graph=False, fused_heads=False)
    tr.load_batch(x, tg)
    tr.step()
    torch.cuda.synchronize()
    lt = tr.loss_value()["total"]
    gt = ma._flat_grad.detach().clone()
    mb.train()
    lb = abc_loss(mb(x), tg, mb.s)
    lb.backward()
    gb = torch.cat([p.grad.reshape(-1) for p in mb.parameters()])
    assert abs(lb.item() - lt) < 1e-6 * abs(lt)
    rel = _rel(gb, gt[:gb.numel()])
    print("bf16 loop vs Trainer: loss %.9g / %.9g, gradient rel L2 %.3g" % (lb.item(), lt, rel))
    assert rel < BF16_GRAD_BOUND
    mc.train()
    dp = nn.DataParallel(mc, device_ids=[0])
    lc = abc_loss(dp(x), tg, dp.module.s)
    assert abs(lc.item() - lb.item()) <= 1e-12 * abs(lb.item())
