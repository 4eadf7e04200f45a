"""The zero skip of the fused heads pass (csrc/heads_fused.hip, csrc/wgrad_heads.hip; abc_heads_fused_desc.dl_tiles / no_zero_skip):
a softmax head's row tile without a target in any of the wave's 32 pixels runs no loss arithmetic and no data-gradient MFMAs, a
bond-type tile of that kind is not stored into the blocked d(logits) buffer, and the blocked weight gradient reads the buffer only
where the tile mask says it was written.  None of that may move a bit:

  * kernel level, through the C ABI: every case runs with no_zero_skip = 1 (every tile computed and stored: the form before the
    skip) and with no_zero_skip = 0, both with dl_tiles; the = 0 run starts from a d(logits) buffer filled with bf16 NaN, so a read
    of an unwritten tile could not stay unseen.  Logits, loss partial sums and the finalised 17 values, g, the BatchNorm sums, every
    conv2 weight and bias gradient, the keep bits and the written part of d(logits) are compared with torch.equal; the stored tile
    mask against one computed on the host from the targets;
  * the synthetic-targets case is held to the oracle by the checks of test_gpu_heads_fused at their tolerances, in both forms;
  * step level: Trainer(zero_skip=False) against the default over three different batches, eager and under the captured graph,
    with dense targets and with the rasteriser's group flags on top.
"""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import abcnet_amd  # noqa: E402,F401
from abcnet_amd import _lib as L  # noqa: E402
from abcnet_amd.contract import alloc_targets  # noqa: E402
from abcnet_amd.dropout import keep_mask  # noqa: E402
from abcnet_amd.engine import head_offsets  # noqa: E402
from abcnet_amd.ops import FusedLoss  # noqa: E402
from abcnet_amd.synthetic import synthetic_targets  # noqa: E402
from oracle import loss_oracle  # noqa: E402
from test_gpu_heads_fused import DEV, HEADS, _check  # noqa: E402

NAN_BF16 = 0x7FC0
ALL_TILES = (1 << 60) - 1        # 15 row tiles x 4 waves


def _pixel(tg, p):
    """flat pixel index (over batch and map) -> (image, y, x) of the target maps"""
    B, _, h, w = tg[0].shape
    b, q = divmod(p, h * w)
    return b, q // w, q % w


def _bond(tg, p, kind, omega_bin):
    b, y, x = _pixel(tg, p)
    tg[5][b, kind, omega_bin, y, x] = 1.0
    tg[4][b, 0, y, x] = 1.0
    tg[6][b, omega_bin, y, x] = 5.0
    tg[7][b, omega_bin, y, x] = 1.0


def _atom(tg, p, kind, charge, hs):
    b, y, x = _pixel(tg, p)
    tg[0][b, 0, y, x] = 1.0
    tg[1][b, kind, y, x] = 1.0
    tg[2][b, charge, y, x] = 1.0
    if hs is not None:
        tg[3][b, hs, y, x] = 1.0


def _targets(case, B, h, w):
    """pixels are named by (chunk, wave, pixel of the wave): flat index 128 chunk + 32 wave + i"""
    if case == "synthetic":
        return synthetic_targets(B, h, seed=1, n_atoms=12, n_bonds=14)
    tg = alloc_targets(B, h, w, "cpu")
    at = lambda chunk, wave, i: 128 * chunk + 32 * wave + i
    if case == "zero":
        pass
    elif case == "one_tile":
        _bond(tg, at(0, 0, 5), 2, 0)
    elif case == "boundaries":
        # bins 7 | 8: row tiles 3 | 4, the last of m-group 0 and the first of m-group 1; bin 29: tile 14, the last (m-group 3 has three
        # tiles); bins 30 and 59: the h = 1 lane half, tiles 0 and 14.  Chunk 4 has one bond: m-group 3 flagged in quarter 1 alone
        _bond(tg, at(0, 0, 3), 0, 7)
        _bond(tg, at(0, 1, 31), 5, 8)
        _bond(tg, at(0, 2, 0), 3, 29)
        _bond(tg, at(0, 3, 17), 1, 30)
        _bond(tg, at(4, 1, 9), 4, 59)
        _atom(tg, at(0, 1, 2), 13, 2, 1)        # atom targets in some waves only: chunks 1, 3, 5 see none
        _atom(tg, at(2, 3, 30), 0, 0, None)     # (no hydrogen target: the wave fires for types and charges, not for hydrogens)
        _atom(tg, at(4, 0, 0), 7, 1, 0)
    elif case == "dense":
        g = torch.Generator().manual_seed(5)
        n = B * h * w
        kinds, odd, half = (torch.randint(0, k, (n,), generator=g).tolist() for k in (6, 2, 2))
        for p in range(n):
            # pixel i of a wave: row tile i % 15 (bins 2 mt + {0, 1} of either lane half), so every tile of every wave fires
            _bond(tg, p, kinds[p], 30 * half[p] + 2 * ((p % 32) % 15) + odd[p])
            _atom(tg, p, p % 14, p % 3, p % 2)
    else:
        raise ValueError(case)
    return tg


def _host_tile_mask(lib, tg):
    """bit 4 mt + w of chunk c: some bond-type target of packed rows 32 mt .. 32 mt + 31 is non-zero in pixels 32 w .. of the chunk"""
    t = tg[5]
    B, npix = t.shape[0], t.shape[0] * t.shape[3] * t.shape[4]
    nz = (t.reshape(B, 360, -1) != 0).permute(1, 0, 2).reshape(360, npix)       # [channel][pixel]
    words = [0] * (npix // 128)
    for mt in range(15):
        chans = [lib.abc_heads_fused_chan_of_row(5, m) for m in range(32 * mt, 32 * mt + 32)]
        hit = nz[[c for c in chans if c >= 0]].any(0).view(-1, 4, 32).any(-1)    # [chunk][wave]
        for c, w in hit.nonzero().tolist():
            words[c] |= 1 << (4 * mt + w)
    return words


def _run(tg, drop_p, keepmask, no_zero_skip, seed=3, unit_scale=False):
    """the harness of test_gpu_heads_fused._run with the targets given, the tile mask set and the switch; the = 0 form starts from a
    d(logits) buffer of bf16 NaN.  Returns what _check of that file takes, too."""
    lib = L.load()
    g = torch.Generator().manual_seed(seed)
    B, _, h, w = tg[0].shape
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
    ndl = lib.abc_heads_fused_dl_elems(C.byref(d))
    dl = torch.full((ndl,), NAN_BF16, dtype=torch.int16, device=DEV).view(torch.bfloat16) if not no_zero_skip else \
        torch.zeros(ndl, dtype=torch.bfloat16, device=DEV)
    tiles = torch.full((nchunk,), -1 if not no_zero_skip else 0, dtype=torch.int64, device=DEV)    # (a stale word either way)
    d.dl_tiles, d.no_zero_skip = tiles.data_ptr(), int(no_zero_skip)
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
    d.chan_scale = chan_scale.data_ptr()
    dw2 = [torch.zeros((c, 128), device=DEV) for c in HEADS]
    db2 = [torch.zeros((c,), device=DEV) for c in HEADS]
    for i in range(8):
        d.chan_off[i], d.dw2[i], d.db2[i] = off[i], dw2[i].data_ptr(), db2[i].data_ptr()
    L.check(lib.abc_heads_fused_wgrad(C.byref(d), st), "wgrad")
    torch.cuda.synchronize()
    unit = None
    if unit_scale:
        # the weight gradient once more with factors of one (a head without any target has the factor 1 / 0 from abc_loss_finalize,
        # as the reference's loss has, and its scaled gradient is 0 x inf whatever the kernel summed)
        scaled = ([t.clone() for t in dw2], [t.clone() for t in db2])
        ones = torch.ones_like(chan_scale)
        d.chan_scale = ones.data_ptr()
        L.check(lib.abc_heads_fused_wgrad(C.byref(d), st), "wgrad")
        torch.cuda.synchronize()
        unit = (dw2, db2)
        dw2, db2 = scaled
    return dict(unit=unit, lib=lib, d=d, B=B, h=h, w=w, ld=ld, npix=npix, nchunk=nchunk, logits=logits, dl=dl, g=gbuf, bnp=bnp, out=out, ds=ds, lp=lp,
                chan_scale=chan_scale, off=off, dw2=dw2, db2=db2, kmask=kmask, tiles=tiles, tgd=tgd, sdev=sdev, st=st,
                host=dict(feat=feat, sc=sc, sh=sh, sl=sl, mean=mean, invstd=invstd, w2=w2, b2=b2, s=s, dseed=dseed, drop_p=drop_p, tg=tg),
                keep=(keep, w2d, b2d, pack, work))


def _with_references(r):
    """what test_gpu_heads_fused._check compares with: the stand-alone loss kernel on the fused kernel's logits, and torch autograd
    of the oracle's loss over the same graph (as test_gpu_heads_fused._run builds them)"""
    hs, B, h, w, npix, ld = r["host"], r["B"], r["h"], r["w"], r["npix"], r["ld"]

    class E:
        pass

    e = E()
    e.lib, e.B, e.h, e.w, e.heads, e.head_off = r["lib"], B, h, w, HEADS, r["off"]
    e.logits = r["logits"]
    e.dlogits = [torch.zeros_like(t) for t in r["logits"]]
    e.chan_scale = torch.zeros(sum(HEADS), device=DEV)
    ds2 = torch.zeros(10, device=DEV)
    fl = FusedLoss(e, r["tgd"], r["sdev"].data_ptr(), ds2.data_ptr())
    fl.run(r["st"])
    torch.cuda.synchronize()
    x = hs["feat"].float()
    y = x * hs["sc"] + hs["sh"]
    a = torch.maximum(y, hs["sl"] * y)
    idx = torch.arange(npix * ld, dtype=torch.int64).view(npix, ld)
    drop_p = hs["drop_p"]
    km = keep_mask(idx, hs["dseed"], drop_p).float() / (1.0 - drop_p) if drop_p > 0 else torch.ones_like(a)
    a = (a * km).to(torch.bfloat16).float()
    leaves, preds, ws, bs = [], [], [], []
    for i, c in enumerate(HEADS):
        ai = a[:, 128 * i:128 * (i + 1)].reshape(B, h, w, 128).permute(0, 3, 1, 2).contiguous().requires_grad_(True)
        wi = hs["w2"][i].to(torch.bfloat16).float().requires_grad_(True)
        bi = hs["b2"][i].clone().requires_grad_(True)
        p = F.conv2d(ai, wi.view(c, 128, 1, 1), bi)
        p.retain_grad()
        leaves.append(ai); preds.append(p); ws.append(wi); bs.append(bi)
    total, _, _ = loss_oracle.abc_loss(preds, hs["tg"], hs["s"])
    total.backward()
    return dict(alone=e, alone_out=fl.out, alone_ds=ds2,
                ref=dict(total=total.item(), preds=preds, leaves=leaves, ws=ws, bs=bs, y=y, km=km, x=x, mean=hs["mean"],
                         invstd=hs["invstd"], sl=hs["sl"]))


def _bond_rows(r):
    """the bond types' block of the d(logits) buffer as raw bits, [chunk][tile][32 rows][wave][32 pixels], and its first element"""
    lib, nchunk = r["lib"], r["nchunk"]
    row0 = sum(lib.abc_heads_fused_rows(i) for i in range(5))
    blk = r["dl"].view(torch.int16)[row0 * nchunk * 128:(row0 + 480) * nchunk * 128]
    return blk.view(nchunk, 15, 32, 4, 32).cpu(), row0 * nchunk * 128


def _written(words, nchunk):
    """[chunk][tile][wave] bool of the mask words"""
    m = torch.zeros((nchunk, 15, 4), dtype=torch.bool)
    for c in range(nchunk):
        for mt in range(15):
            for w in range(4):
                m[c, mt, w] = bool((words[c] >> (4 * mt + w)) & 1)
    return m


CASES = {
    "zero": (1, 16, 16, 0.0, False),
    "one_tile": (1, 16, 16, 0.2, True),
    "boundaries": (2, 16, 24, 0.2, True),
    "dense": (1, 16, 16, 0.0, False),
    "synthetic": (2, 32, 32, 0.2, True),
}


@pytest.mark.parametrize("case", list(CASES))
def test_zero_skip_changes_no_bit(case):
    B, h, w, drop_p, keepmask = CASES[case]
    tg = _targets(case, B, h, w)
    lib = L.load()
    want = _host_tile_mask(lib, tg)
    nchunk = B * h * w // 128
    nset = sum(bin(x).count("1") for x in want)
    print("  %s: %d of %d tile bits set" % (case, nset, 60 * nchunk))
    if case == "zero":
        assert nset == 0
    elif case == "one_tile":
        assert want == [1, 0]                     # tile 0, wave 0 of chunk 0
    elif case == "boundaries":
        bit = lambda mt, wv: 1 << (4 * mt + wv)
        assert want == [bit(3, 0) | bit(4, 1) | bit(14, 2) | bit(0, 3), 0, 0, 0, bit(14, 1), 0]
    elif case == "dense":
        assert want == [ALL_TILES] * nchunk       # nothing is skipped
    else:
        assert 0 < nset < 60 * nchunk             # (a condition on the inputs: the synthetic targets are neither empty nor dense)
    r1 = _run(tg, drop_p, keepmask, 1, unit_scale=case == "zero")
    r0 = _run(tg, drop_p, keepmask, 0, unit_scale=case == "zero")
    # ---- the tile mask
    unsigned = lambda t: [int(x) & ((1 << 64) - 1) for x in t.cpu().tolist()]
    assert unsigned(r1["tiles"]) == [ALL_TILES] * nchunk
    assert unsigned(r0["tiles"]) == want
    # ---- everything the pass and its weight gradient hand on, bit for bit
    # (as raw bits: a head without any target has 0 / 0 among its 17 values and 0 x inf in its scaled gradients, in both forms)
    bits = lambda t: t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])
    same = lambda a, b: torch.equal(bits(a), bits(b))
    for i in range(8):
        assert same(r0["logits"][i], r1["logits"][i]), ("logits", i)
        assert same(r0["dw2"][i], r1["dw2"][i]), ("dw2", i)
        assert same(r0["db2"][i], r1["db2"][i]), ("db2", i)
    if case != "zero":
        assert torch.isfinite(r0["dw2"][5]).all() and torch.isfinite(r0["db2"][5]).all(), "the NaN fill was read"
    assert same(r0["lp"], r1["lp"]), "loss_partial"
    assert same(r0["out"], r1["out"]), ("loss_finalize", r0["out"], r1["out"])
    assert same(r0["ds"], r1["ds"]) and same(r0["chan_scale"], r1["chan_scale"])
    assert same(r0["g"], r1["g"]), "g"
    assert same(r0["bnp"], r1["bnp"]), "bn_partial"
    if keepmask:
        assert same(r0["kmask"], r1["kmask"]), "keep bits"
    if case == "zero":
        # every chunk skipped: conv2's gradients of the bond types are exactly zero (with factors of one, see _run), as are those of
        # the small softmax heads
        for i in (1, 2, 3, 5):
            for r in (r0, r1):
                assert not r["unit"][0][i].any() and not r["unit"][1][i].any(), ("gradient of a head without targets", i)
        for i in range(8):
            assert same(r0["unit"][0][i], r1["unit"][0][i]) and same(r0["unit"][1][i], r1["unit"][1][i]), ("unit-factor gradients", i)
    # ---- d(logits): all rows of the other heads; the bond types where a tile is flagged, the NaN fill left alone elsewhere
    b0, first = _bond_rows(r0)
    b1, _ = _bond_rows(r1)
    d0, d1 = r0["dl"].view(torch.int16), r1["dl"].view(torch.int16)
    assert torch.equal(d0[:first], d1[:first]) and torch.equal(d0[first + b0.numel():], d1[first + b0.numel():]), "d(logits) of the other heads"
    wr = _written(want, nchunk)[:, :, None, :, None].expand_as(b0)
    assert torch.equal(b0[wr], b1[wr]), "d(logits) of the flagged bond-type tiles"
    assert (b0[~wr] == NAN_BF16).all(), "an unflagged bond-type tile was written"
    assert not b1[~wr].any(), "d(logits) of a tile without a target is not zero in the full form"
    if case == "synthetic":
        # ---- both forms against the oracle (the = 0 form with its unwritten tiles as the weight gradient takes them: zero)
        refs = _with_references(r1)       # (computed once: the logits of the two forms are the same bits)
        _check({**r1, **refs}, keepmask)
        seen = r0["dl"].clone()
        sb = seen.view(torch.int16)[first:first + b0.numel()].view(nchunk, 15, 32, 4, 32)
        sb[(~wr).to(DEV)] = 0
        _check({**r0, **refs, "dl": seen}, keepmask)


def _trainer_steps(zero_skip, use_graph, sparse):
    from abcnet_amd.raster import TargetRasterizer, parse_record
    from abcnet_amd.synthetic import random_annotations, synthetic_images
    from abcnet_amd.train import Trainer
    from abcnet_amd.unet import UNet
    B, S = 2, 192
    h = S // 4
    m = UNet(1, HEADS, dtype="bf16", dropout_p=0.2)
    m.reset_parameters(seed=77)
    m = m.to(DEV)
    tr = Trainer(m, B, S, S, use_graph=use_graph, zero_skip=zero_skip)
    assert tr.eng.hf is not None and tr.eng.hf.no_zero_skip == (0 if zero_skip else 1)
    rz = None
    if sparse:
        rz = TargetRasterizer(B, h, max_atoms=64, max_bonds=64, targets=tr.targets, sparse=True)
        tr.use_sparse_targets(rz)
    grads, losses, logits, masks = [], [], [], []
    for step in range(3):
        imgs = synthetic_images(B, S, seed=11 + step).to(DEV)
        if sparse:
            tr.load_batch(imgs)
            rz.load([parse_record(*random_annotations(12 + 9 * step, 10 + 11 * step, 4000 + 10 * step + i, size=S), h=h) for i in range(B)])
            rz.run()
        else:
            tr.load_batch(imgs, [t.to(DEV) for t in synthetic_targets(B, h, seed=21 + step, n_atoms=8 + 6 * step, n_bonds=6 + 7 * step)])
        tr.step()
        torch.cuda.synchronize()
        grads.append(m._flat_grad.clone())
        losses.append(tr.loss.out.clone())
        logits.append([t.clone() for t in tr.eng.logits])
        masks.append(tr.eng.hf_tiles.clone())
    return grads, losses, logits, masks, m._flat.detach().clone()


@pytest.mark.parametrize("use_graph", [False, True])
@pytest.mark.parametrize("sparse", [False, True])
def test_zero_skip_gives_the_same_step_bit_for_bit(sparse, use_graph):
    """Trainer(zero_skip=False) against the default at B = 2, 192 x 192: three steps on three different batches (the tile mask changes
    under the same buffers; under the graph steps 2 and 3 are replays), dense targets through load_batch or the sparse rasteriser's
    flags on top of the skip.  The loss terms, every parameter gradient, the stored logits and the parameters after step 3."""
    g0, l0, z0, k0, p0 = _trainer_steps(False, use_graph, sparse)
    g1, l1, z1, k1, p1 = _trainer_steps(True, use_graph, sparse)
    for step in range(3):
        for i in range(8):
            assert torch.equal(z0[step][i], z1[step][i]), ("stored logits", step, i)
        assert torch.equal(l0[step], l1[step]), ("loss terms", step, l0[step], l1[step])
        assert torch.equal(g0[step], g1[step]), ("gradients", step, (g0[step] - g1[step]).abs().max().item())
        share = sum(bin(int(x) & ((1 << 64) - 1)).count("1") for x in k1[step].cpu().tolist()) / (60.0 * k1[step].numel())
        assert 0.0 < share < 1.0, (step, share)       # (the skip did act, and not everywhere)
        assert (k0[step] == ALL_TILES).all(), step    # (zero_skip=False stores every tile and says so)
    assert not torch.equal(k1[0], k1[1]) and not torch.equal(k1[1], k1[2])
    assert torch.equal(p0, p1)
