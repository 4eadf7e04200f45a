"""GPU parity of the fused heads pass (csrc/heads_fused.hip + the blocked weight gradient in csrc/wgrad.hip), kernel level,
through the C ABI:

  * logits against torch's 1x1 convolution of the same bf16-rounded operands (unet.py:70);
  * d(logits) against the stand-alone loss kernel to one bf16 ulp (same formulas; hardware exp / log here) (abc_loss_fwd_bwd, itself held to the reference-exec golden)
    run on the fused kernel's own logits, through the packed row order -- and the reduced loss against it and the oracle;
  * g (gradient w.r.t. the BatchNorm outputs), the BatchNorm-backward sums, conv2.weight.grad and conv2.bias.grad against
    torch autograd of the ORACLE's loss (oracle/loss_oracle.py, train.py:95-137) over the same graph in f32.
Tolerances are relative L2 of whole tensors: the kernel rounds d(logits), the data gradient and g to bf16 (8 significant bits).
"""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import abcnet_amd  # noqa: E402,F401
from abcnet_amd import _lib as L  # noqa: E402
from abcnet_amd.dropout import keep_mask  # noqa: E402
from abcnet_amd.engine import head_offsets  # noqa: E402
from abcnet_amd.ops import FusedLoss  # noqa: E402
from abcnet_amd.synthetic import synthetic_targets  # noqa: E402
from oracle import loss_oracle  # noqa: E402
from test_gpu_loss_edges import clamp_band, edge_targets  # noqa: E402

HEADS = [1, 14, 3, 2, 1, 360, 60, 60]
DEV = "cuda"


def rel(a, b):
    return ((a.double() - b.double()).norm() / (b.double().norm() + 1e-30)).item()


def _run(B, h, drop_p, seed=3, keepmask=False, w=None, bias_shift=False, fma=False):
    """w: the map is h x w with the cropped targets of test_gpu_loss_edges (default: square, the targets this file always used).
    bias_shift: +30 on about 15 % of each head's conv2 biases and -30 on another 15 % -- the conv part of the logits has a standard
    deviation of about 1.7, so those channels sit beyond |z| > 22, deep inside the clamp at |z| > 11.5 and far from its bound.
    fma: the reference forms scale * x + shift with one rounding, as the kernel's fmaf does, instead of two (see
    test_fused_heads_pass_nonsquare_and_saturated)."""
    lib = L.load()
    g = torch.Generator().manual_seed(seed)
    tg = synthetic_targets(B, h, seed=1, n_atoms=12, n_bonds=14) if w is None else edge_targets(B, h, w)
    w = h if w is None else w
    npix, ld = B * h * w, 1024
    feat = (torch.randn((npix, ld), generator=g) * 1.5).to(torch.bfloat16)
    sc = torch.rand(ld, generator=g) * 0.8 + 0.4
    sh = torch.randn(ld, generator=g) * 0.3
    sl = torch.full((ld,), 0.01)
    mean = torch.randn(ld, generator=g) * 0.2
    invstd = torch.rand(ld, generator=g) + 0.5
    w2 = [torch.randn((c, 128), generator=g) * 0.15 for c in HEADS]
    b2 = [torch.randn((c,), generator=g) * 0.5 for c in HEADS]
    s = torch.rand(10, generator=g) * 0.4 - 0.2
    if bias_shift:
        for i, c in enumerate(HEADS):
            u = torch.rand(c, generator=g)
            b2[i] = b2[i] + torch.where(u < 0.15, 30.0, torch.where(u < 0.30, -30.0, 0.0))
    dseed = 0x1234567

    dev = lambda t: t.to(DEV).contiguous()
    d = L.HeadsFusedDesc()
    keep = {k: dev(v) for k, v in dict(feat=feat, sc=sc, sh=sh, sl=sl, mean=mean, invstd=invstd).items()}
    d.feat, d.ld = keep["feat"].data_ptr(), ld
    d.scale, d.shift, d.slope, d.mean, d.invstd = (keep[k].data_ptr() for k in ("sc", "sh", "sl", "mean", "invstd"))
    d.drop_p, d.drop_seed, d.drop_salt = drop_p, dseed, None
    w2d, b2d = [dev(t) for t in w2], [dev(t) for t in b2]
    pack = torch.zeros(lib.abc_heads_fused_pack_bytes(), dtype=torch.uint8, device=DEV)
    logits = [torch.zeros((B, c, h, w), device=DEV) for c in HEADS]
    tgd = [dev(t) for t in tg]
    for i in range(8):
        d.w2[i], d.b2[i], d.logits[i] = w2d[i].data_ptr(), b2d[i].data_ptr(), logits[i].data_ptr()
    d.w2_pack = pack.data_ptr()
    (d.t_atom, d.t_types, d.t_charges, d.t_hs, d.t_bond, d.t_btypes, d.t_rho, d.t_omega) = (t.data_ptr() for t in tgd)
    d.B, d.h, d.w = B, h, w
    nchunk = lib.abc_heads_fused_chunks(C.byref(d))
    assert nchunk == npix // 128
    dl = torch.zeros(lib.abc_heads_fused_dl_elems(C.byref(d)), dtype=torch.bfloat16, device=DEV)
    gbuf = torch.zeros((npix, ld), dtype=torch.bfloat16, device=DEV)
    bnp = torch.zeros((nchunk, 2, ld), device=DEV)
    nlb = lib.abc_heads_fused_loss_blocks(C.byref(d))
    lp = torch.zeros((nlb, 16), dtype=torch.float64, device=DEV)
    d.dl, d.g, d.bn_partial, d.loss_partial = dl.data_ptr(), gbuf.data_ptr(), bnp.data_ptr(), lp.data_ptr()
    work = torch.zeros(lib.abc_heads_fused_wgrad_floats(C.byref(d)), device=DEV)
    d.wgrad_work = work.data_ptr()
    kmask = torch.zeros((3, npix, 2, 8), dtype=torch.uint8, device=DEV) if keepmask else None
    if keepmask:
        d.keep_mask = kmask.data_ptr()
    st = torch.cuda.current_stream().cuda_stream
    L.check(lib.abc_heads_fused_pack(C.byref(d), st), "pack")
    L.check(lib.abc_heads_fused_fwd_bwd(C.byref(d), st), "fwd_bwd")
    # loss finalisation on the fused partial sums -> per-channel factors
    off = head_offsets(HEADS)
    chan_scale = torch.zeros(sum(HEADS), device=DEV)
    out = torch.zeros(17, dtype=torch.float64, device=DEV)
    sdev, ds = dev(s), torch.zeros(10, device=DEV)
    f = L.LossFinDesc()
    f.partial, f.nblk, f.s, f.ds, f.out = lp.data_ptr(), nlb, sdev.data_ptr(), ds.data_ptr(), out.data_ptr()
    f.chan_scale, f.nchan, f.grad_scale = chan_scale.data_ptr(), chan_scale.numel(), 1.0
    for i in range(8):
        f.chan_off[i], f.head_c[i] = off[i], HEADS[i]
    L.check(lib.abc_loss_finalize(C.byref(f), st), "loss_finalize")
    # weight / bias gradients
    d.chan_scale = chan_scale.data_ptr()
    dw2 = [torch.zeros((c, 128), device=DEV) for c in HEADS]
    db2 = [torch.zeros((c,), device=DEV) for c in HEADS]
    for i in range(8):
        d.chan_off[i], d.dw2[i], d.db2[i] = off[i], dw2[i].data_ptr(), db2[i].data_ptr()
    L.check(lib.abc_heads_fused_wgrad(C.byref(d), st), "wgrad")
    torch.cuda.synchronize()

    # ---- stand-alone loss kernel on the fused kernel's logits
    class E:
        pass

    e = E()
    e.lib, e.B, e.h, e.w, e.heads, e.head_off = lib, B, h, w, HEADS, off
    e.logits = logits
    e.dlogits = [torch.zeros_like(t) for t in logits]
    e.chan_scale = torch.zeros(sum(HEADS), device=DEV)
    ds2 = torch.zeros(10, device=DEV)
    fl = FusedLoss(e, tgd, sdev.data_ptr(), ds2.data_ptr())
    fl.run(st)
    torch.cuda.synchronize()

    # ---- torch autograd of the oracle's loss over the same graph (f32, same bf16-rounded operands, same dropout mask)
    x = feat.float()
    y = (x.double() * sc.double() + sh.double()).float() if fma else x * sc + sh
    a = torch.maximum(y, sl * y)
    idx = torch.arange(npix * ld, dtype=torch.int64).view(npix, ld)
    km = keep_mask(idx, dseed, drop_p).float() / (1.0 - drop_p) if drop_p > 0 else torch.ones_like(a)
    a = (a * km).to(torch.bfloat16).float()
    leaves, preds, ws, bs = [], [], [], []
    for i, c in enumerate(HEADS):
        ai = a[:, 128 * i:128 * (i + 1)].reshape(B, h, w, 128).permute(0, 3, 1, 2).contiguous().requires_grad_(True)
        wi = w2[i].to(torch.bfloat16).float().requires_grad_(True)
        bi = b2[i].clone().requires_grad_(True)
        p = F.conv2d(ai, wi.view(c, 128, 1, 1), bi)
        p.retain_grad()
        leaves.append(ai); preds.append(p); ws.append(wi); bs.append(bi)
    total, _, _ = loss_oracle.abc_loss(preds, tg, s)
    total.backward()
    return dict(lib=lib, d=d, B=B, h=h, w=w, ld=ld, npix=npix, nchunk=nchunk, logits=logits, dl=dl, g=gbuf, bnp=bnp, out=out, ds=ds,
                chan_scale=chan_scale, off=off, dw2=dw2, db2=db2, alone=e, alone_out=fl.out, alone_ds=ds2,
                ref=dict(total=total.item(), preds=preds, leaves=leaves, ws=ws, bs=bs, y=y, km=km, x=x, mean=mean, invstd=invstd, sl=sl),
                kmask=kmask, keep=(keep, w2d, b2d, pack, tgd, lp, work, sdev))


@pytest.mark.parametrize("B,hw,drop_p,keepmask", [(2, 32, 0.2, False), (1, 48, 0.0, False), (2, 32, 0.2, True)])
def test_fused_heads_pass(B, hw, drop_p, keepmask):
    """keepmask: abc_heads_fused_desc.keep_mask set -- the fused pass leaves the wide heads' dropout keep bits for its conv2
    weight gradient (checked against the host mirror of the hash below, and through dW2 of heads 5-7 like the hashed form)"""
    _check(_run(B, hw, drop_p, keepmask=keepmask), keepmask)


# d(logits) of the edge cases: elements left out because a class of their softmax group lies within 1 % of a clamp bound, where the
# hardware exp of the fused kernel and the library exp of the stand-alone one may fall on different sides.  Estimated 0 on the CPU.
MAX_BAND_SHARE = 1e-3


def _bf16_floor(r):
    """what rounding d(logits) to bf16 alone costs groups 4 and 5: their statistics for the oracle graph itself, with autograd's
    d(loss)/d(logits) rounded to bf16 (and g rounded to bf16 after it, as the kernel stores it), against the same graph unrounded"""
    ref, npix = r["ref"], r["npix"]
    lk = torch.where(ref["y"] > 0, torch.ones_like(ref["y"]), ref["sl"].expand_as(ref["y"])) * ref["km"]
    xhat = (ref["x"] - ref["mean"]) * ref["invstd"]
    out = []
    for i, c in enumerate(HEADS):
        sl_ = slice(128 * i, 128 * (i + 1))
        dq = ref["preds"][i].grad.to(torch.bfloat16).float().permute(0, 2, 3, 1).reshape(npix, c)
        ai = ref["leaves"][i].detach().permute(0, 2, 3, 1).reshape(npix, 128)
        want = ref["leaves"][i].grad.permute(0, 2, 3, 1).reshape(npix, 128) * lk[:, sl_]
        gq = ((dq @ ref["ws"][i].detach()) * lk[:, sl_]).to(torch.bfloat16).float()
        scale = want.double().abs().sum(0).mean().item() + 1e-300
        out.append(dict(g=rel(gq, want), dw=rel(dq.t() @ ai, ref["ws"][i].grad), db=rel(dq.sum(0), ref["bs"][i].grad),
                        s1=(gq.double().sum(0) - want.double().sum(0)).abs().max().item() / scale,
                        s2=((gq.double() - want.double()) * xhat[:, sl_].double()).sum(0).abs().max().item() / scale))
    return out


def _check(r, keepmask, edges=False):
    """the six check groups.  edges (the non-square and saturated cases): group 3 leaves out the clamp band of test_gpu_loss_edges,
    computed in f64 from the logits the fused kernel wrote, and holds the fused kernel to every exact zero of the stand-alone one.
    Groups 4 and 5 keep their tolerances, in the saturated cases too.  Measured there, worst head: g 2.6e-3 (1e-2 allowed), BatchNorm
    sums at most 0.7 of their bounds, dW2 1.3e-3 and db2 8.6e-4 (6e-3); a head all of whose labels are clamped (atom_t at
    2 x 32 x 32, atom_types / atom_charges / bond_t at 3 x 8 x 16) has g, sums, dW2 and db2 of exactly zero, as autograd has."""
    lib, ref, B = r["lib"], r["ref"], r["B"]
    floor = _bf16_floor(r) if edges else None
    if edges:
        for i in range(8):
            print("  head %d: bf16 floor of the oracle graph: %s" % (i, ", ".join("%s %.3g" % kv for kv in floor[i].items())))
            # drop_p of these cases was chosen so that this floor, a property of the oracle graph alone, leaves the tolerances room
            assert 3 * floor[i]["g"] <= 1e-2 and 3 * floor[i]["dw"] <= 6e-3 and 3 * floor[i]["db"] <= 6e-3, (i, floor[i])
    # 1. logits
    for i, c in enumerate(HEADS):
        got, want = r["logits"][i].cpu(), ref["preds"][i].detach()
        assert (got - want).abs().max().item() <= 2e-4 * max(1.0, want.abs().max().item()), ("logits", i)
    # 2. the loss: against the stand-alone kernel on the same logits, and the oracle
    o, oa = r["out"].cpu(), r["alone_out"].cpu()
    # (the fused kernel evaluates exp / log / 1/x with the hardware approximations, ~1e-6 relative: loss_math.hpp)
    assert torch.allclose(o, oa, rtol=5e-6, atol=1e-12), (o, oa)
    assert torch.allclose(r["ds"].cpu(), r["alone_ds"].cpu(), rtol=2e-5, atol=1e-8)
    assert torch.allclose(r["chan_scale"].cpu(), r["alone"].chan_scale.cpu(), rtol=1e-6, atol=0)
    assert abs(o[0].item() - ref["total"]) <= 2e-5 * abs(ref["total"])
    # 3. d(logits): the blocked bf16 buffer holds bf16(the stand-alone kernel's values), row by row
    nchunk, row0 = r["nchunk"], 0
    dl = r["dl"].cpu()
    band = clamp_band(r["logits"]) if edges else None
    nband = 0
    for i, c in enumerate(HEADS):
        rows = lib.abc_heads_fused_rows(i)
        blk = dl[row0 * nchunk * 128:(row0 + rows) * nchunk * 128].view(nchunk, rows, 128)
        want = r["alone"].dlogits[i].cpu().to(torch.bfloat16)            # [B][c][HW]
        want = want.view(B, c, -1).permute(1, 0, 2).reshape(c, nchunk, 128)  # channel, chunk, pixel
        if edges:
            packed = lambda t: t.reshape(B, c, -1).permute(1, 0, 2).reshape(c, nchunk, 128)
            ok, exact = ~packed(band[i]), packed(r["alone"].dlogits[i].cpu())
            nband += (~ok).sum().item()
        for m in range(rows):
            ch = lib.abc_heads_fused_chan_of_row(i, m)
            if ch < 0:
                assert not blk[:, m, :].any(), ("padding row not zero", i, m)
            else:
                # equal up to the hardware exp / log (a few f32 ulps before the bf16 rounding: at most one bf16 ulp apart,
                # and only where the f32 value sat on a rounding boundary)
                a_, b_ = blk[:, m, :].float(), want[ch].float()
                if edges:
                    assert not a_[ok[ch] & (exact[ch] == 0)].any(), ("d(logits) not zero where the stand-alone kernel's is", i, m, ch)
                    a_, b_ = a_[ok[ch]], b_[ok[ch]]
                assert ((a_ - b_).abs() <= 2.0 ** -7 * b_.abs() + 1e-30).all(), ("d(logits)", i, m, ch)
                assert (a_ != b_).float().mean().item() <= 0.02, ("d(logits) mismatches", i, m, ch, (a_ != b_).float().mean().item())
        row0 += rows
    if edges:
        print("  d(logits): %d of %d elements in the clamp band" % (nband, sum(HEADS) * r["npix"]))
        assert nband <= MAX_BAND_SHARE * sum(HEADS) * r["npix"], nband
    # 4. g and the BatchNorm-backward sums: autograd's d(loss)/d(features) through LeakyReLU' and the dropout mask
    npix, ld = r["npix"], r["ld"]
    cs = r["chan_scale"].cpu()
    g = r["g"].float().cpu()
    lk = torch.where(ref["y"] > 0, torch.ones_like(ref["y"]), ref["sl"].expand_as(ref["y"])) * ref["km"]
    xhat = (ref["x"] - ref["mean"]) * ref["invstd"]
    part = r["bnp"].cpu().double().sum(0)
    for i, c in enumerate(HEADS):
        da = ref["leaves"][i].grad.permute(0, 2, 3, 1).reshape(npix, 128)
        want = da * lk[:, 128 * i:128 * (i + 1)]
        got = g[:, 128 * i:128 * (i + 1)] * cs[r["off"][i]]
        print("  head %d: g %.3g" % (i, rel(got, want)))
        assert rel(got, want) <= 1e-2, ("g", i, rel(got, want))
        s1, s2 = want.double().sum(0), (want.double() * xhat[:, 128 * i:128 * (i + 1)].double()).sum(0)
        k1, k2 = part[0, 128 * i:128 * (i + 1)] * cs[r["off"][i]].double(), part[1, 128 * i:128 * (i + 1)] * cs[r["off"][i]].double()
        scale = want.double().abs().sum(0).mean()   # (sums of signed terms: error relative to the sum of magnitudes)
        print("  head %d: bn sums %.3g %.3g of %.3g" % (i, (k1 - s1).abs().max().item(), (k2 - s2).abs().max().item(), scale.item()))
        assert (k1 - s1).abs().max().item() <= 5e-3 * scale.item(), ("bn sum g", i)
        assert (k2 - s2).abs().max().item() <= 1e-2 * scale.item(), ("bn sum g xhat", i)
    # 5. conv2 weight / bias gradients
    for i, c in enumerate(HEADS):
        print("  head %d: dW2 %.3g db2 %.3g" % (i, rel(r["dw2"][i].cpu(), ref["ws"][i].grad), rel(r["db2"][i].cpu(), ref["bs"][i].grad)))
        assert rel(r["dw2"][i].cpu(), ref["ws"][i].grad) <= 6e-3, ("dW2", i, rel(r["dw2"][i].cpu(), ref["ws"][i].grad))
        assert rel(r["db2"][i].cpu(), ref["bs"][i].grad) <= 6e-3, ("db2", i, rel(r["db2"][i].cpu(), ref["bs"][i].grad))
    # 6. the keep bits: byte kk of half h of a pixel = channels 16 kk + 8 h .. + 7 of the head's 128 features
    if keepmask:
        km = (ref["km"] > 0).view(npix, 8, 128)                       # [pixel][head][channel]
        bits = r["kmask"].cpu()                                        # [3][pixel][h][kk]
        for i in (5, 6, 7):
            want = km[:, i, :].view(npix, 8, 2, 8).permute(0, 2, 1, 3)   # [pixel][h][kk][j]
            wbyte = (want.to(torch.int32) << torch.arange(8, dtype=torch.int32)).sum(-1).to(torch.uint8)
            assert torch.equal(bits[i - 5], wbyte), ("keep bits", i)


@pytest.mark.parametrize("B,h,w,drop_p,bias_shift", [(3, 8, 16, 0.0, False), (1, 16, 24, 0.2, False), (2, 32, 32, 0.2, True),
                                                     (3, 8, 16, 0.2, True)])
def test_fused_heads_pass_nonsquare_and_saturated(B, h, w, drop_p, bias_shift):
    """h != w (3 x 8 x 16: one chunk per image; 1 x 16 x 24: three chunks that do not end on rows), and logits deep inside the clamp:
    group 3 then compares the hardware exp / log / rcp of the fused kernel with the exact math where `inside` is false.

    The reference of these cases rounds scale * x + shift once (fma=True), as the kernel does.  With two roundings about one
    activation in 70 000 falls on the other side of a bf16 rounding boundary, a whole bf16 ulp of one of the 128 features of a
    logit: at 3 x 8 x 16 with drop_p 0.2 that is feature 86 of bond_t at pixel 3 (2.46875 against 2.453125), which alone moves the
    logit by 9.57e-4 where group 1 allows 8.5e-4.  The three cases above carry such flips too (up to 7.3e-4) and stay inside.
    drop_p: 1 x 16 x 24 without dropout leaves db2 of atom_hs, two sums of opposite sign over 384 pixels, at 3e-4 of its terms;
    the oracle graph with bf16 d(logits) is then 4e-2 from itself there (_bf16_floor), which the 6e-3 of group 5 cannot hold, so
    the case runs with dropout, where that floor is 1.1e-3.  _check asserts that every case here has that room.
    Measured: no element of d(logits) in the clamp band but 6 of 1 026 048 at 2 x 32 x 32."""
    _check(_run(B, h, drop_p, w=w, bias_shift=bias_shift, fma=True), False, edges=True)


@pytest.mark.parametrize("keep_logits", [True, False])
def test_sparse_targets_give_the_same_step_bit_for_bit(keep_logits):
    """Trainer.use_sparse_targets (abc_heads_fused_desc.target_flags): the fused heads pass reads a head's target planes only in the
    32-pixel groups the rasteriser flagged; everywhere else the same loads hit 512 zero bytes.  Same records through the sparse
    rasteriser + flags and through the plain rasteriser + every plane: the loss terms, d(logits) in the stored logits' gradient
    chain -- i.e. EVERY parameter gradient -- and the parameters after three steps (three different batches: the sparse form erases
    its previous drawing) are bit-identical; and the flags did switch reads off (most groups carry no target).  Since round 5 a wave
    without a target of a softmax head also SKIPS that head's loss / data gradient / epilogue (run_head_skip: logits + zeros) -- the
    stored logits must be the same bits too, and with keep_logits=False (nothing of the head's forward is observable) the skipped
    waves write zeros only."""
    from abcnet_amd.raster import TargetRasterizer, parse_record
    from abcnet_amd.synthetic import random_annotations, synthetic_images
    from abcnet_amd.train import Trainer
    from abcnet_amd.unet import UNet
    B, S = 2, 192
    h = S // 4
    res = []
    for sparse in (False, True):
        m = UNet(1, HEADS, dtype="bf16", dropout_p=0.2)
        m.reset_parameters(seed=77)
        m = m.to(DEV)
        tr = Trainer(m, B, S, S, use_graph=False, keep_logits=keep_logits)
        rz = TargetRasterizer(B, h, max_atoms=64, max_bonds=64, targets=tr.targets, sparse=sparse)
        if sparse:
            tr.use_sparse_targets(rz)
            with pytest.raises(Exception, match="sparse"):
                tr.load_batch(synthetic_images(B, S, seed=1).to(DEV), [t.clone() for t in tr.targets])
        grads, losses, logits = [], [], []
        for step in range(3):
            tr.load_batch(synthetic_images(B, S, seed=11 + step).to(DEV))
            rz.load([parse_record(*random_annotations(12 + 9 * step, 10 + 11 * step, 4000 + 10 * step + i, size=S), h=h) for i in range(B)])
            rz.run()
            tr.step()
            torch.cuda.synchronize()
            grads.append(m._flat_grad.clone())
            losses.append(tr.loss.out.clone())
            if keep_logits:
                logits.append([t.clone() for t in tr.eng.logits])
        frac = None
        if sparse:
            f = rz.group_flags.cpu().numpy().astype("uint32")
            frac = float(((f & 0xFF) != 0).mean())
        res.append((grads, losses, m._flat.detach().clone(), frac, logits))
        del tr, rz, m
    (g0, l0, p0, _, z0), (g1, l1, p1, frac, z1) = res
    for step in range(3):
        if keep_logits:
            for i in range(8):
                assert torch.equal(z0[step][i], z1[step][i]), ("stored logits", step, i)
        assert torch.equal(l0[step], l1[step]), ("loss terms", step, l0[step], l1[step])
        assert torch.equal(g0[step], g1[step]), ("gradients", step, (g0[step] - g1[step]).abs().max().item())
    assert torch.equal(p0, p1)
    assert 0.0 < frac < 1.0, frac      # (48 x 48 maps with up to 62 items: most groups carry something; still not all)
