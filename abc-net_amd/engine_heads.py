"""Launch plans of the output heads (unet.py:62-69,116-118; unet2.py shares them): the part of the engine that builds, per head,
conv3x3(128 -> 128) + BatchNorm + LeakyReLU(0.01) + Dropout + conv1x1(128 -> head width) on the trunk's last activation, and its backward.

HeadsPlan is a mixin of engine.Engine: it uses the engine's memory helpers and emitters through `self` and leaves the heads'
buffers and records on the engine.  Which of the forms a plan takes is decided once (HeadsForm, _heads_form); the builder reads it.
"""
from __future__ import annotations

import ctypes as C
from typing import NamedTuple

import torch

from . import _lib as L
from . import arch
from .engine_types import Rec, Src, taps_mirror, taps_square


class HeadsForm(NamedTuple):
    """how one plan serves its heads (decided by HeadsPlan._heads_form; the builder asks nothing else)"""
    conv1: str           # "merged": the conv1's of all heads as ONE 128 -> nh x 128 convolution / "per_head"
    batch_fin: bool      # the heads' BatchNorm finalisers (training) as one launch
    f8_feat: bool        # fp8 graph: the heads' features are e4m3 (each head its own calibrated scale: hfeat_q)
    conv2: str           # who serves the 1x1 convolutions -- "fused": the Trainer's fused heads pass (they leave the forward plan) /
    #                      "epilogue": the merged conv1, from the table hepi / "kernel": the batched heads launch / "one_by_one"
    nms: bool            # eval: |rho| and the omega-bin NMS mask are asked of the 1x1 kernel as second outputs (nms_rho, nms_omega)
    decode: bool         # on top of them: the bond-type arg-max map instead of the bond-type and rho maps (btype_idx)


class HeadsPlan:
    # ------------------------------------------------------------------ the form
    def _heads_form(self, trunk: Src):
        h, w = trunk.H, trunk.W
        nh = len(self.heads)
        batch_fin = nh <= 8 and self.batched_heads
        # the eight conv1's (unet.py:66,116-118: the same 128-channel trunk into 8 x 128 channels) as ONE 128 -> 8 x 128
        # convolution: the input halo tile is shared by the 8 n-blocks of a pixel tile (same XCD, its L2), and 8 x 768 tiles
        # fill the 512 workgroup slots 12.0 times instead of 8 x 1.5
        merged = batch_fin and self.dt == L.BF16 and trunk.C == 128
        # (fp8 graph: the heads' features are e4m3 too when the merged conv1 and the heads' own 1x1 kernel serve them)
        f8_feat = self.fp8 and trunk.dt == L.FP8 and trunk.C == 128 and nh <= 8 and self.batched_heads and (h * w) % 64 == 0
        if self.want_fused_heads and merged and (h * w) % 128 == 0 and self.B * h * w * 128 * nh < (1 << 30):
            conv2 = "fused"
        # folded graph: the heads' 1x1 convolutions in the epilogue of the merged conv1 (abc_conv_desc.heads_epi): no feature tensor
        elif self.fold and self.heads_epilogue and self.batched_heads and self.dt == L.BF16 and trunk.C == 128 and nh <= 8 and \
                (trunk.dt == L.BF16 or f8_feat):
            conv2 = "epilogue"
        else:
            conv2 = "kernel" if batch_fin else "one_by_one"      # (emit_heads_batch: one launch each where the library refuses the batch)
        # (the second outputs belong to the 1x1 kernel's launches over the head list of train.py:47; nms_heads is eval only)
        nms = self.nms_heads and self.heads == arch.TRAIN_HEADS and conv2 in ("kernel", "one_by_one")
        return HeadsForm("merged" if merged else "per_head", batch_fin, f8_feat, conv2, nms, nms and self.decode)

    # ------------------------------------------------------------------ forward plan
    def _build_heads(self, trunk: Src):
        self.h, self.w = trunk.H, trunk.W
        self.heads_form = form = self._heads_form(trunk)
        self._heads_alloc(form)
        shared = self._heads_conv1_merged(trunk, form) if form.conv1 == "merged" else None
        fins, conv2s = [], []
        # (one loop for conv1 and conv2: the weight-packing table holds each head's conv1 in front of its conv2)
        for i in range(len(self.heads)):
            f = self._head_conv1(i, trunk, form, shared, fins)
            self._head_conv2(i, f, form, conv2s)
        if fins:
            arr = (L.BnFwdDesc * len(fins))(*fins)
            self._emit(self.fwd_ops, self.lib.abc_bn_finalize_fwd_batch, (arr, len(fins), 128 * len(self.heads) if form.conv1 == "merged" else 0),
                       "bn out_modules.*.bn", meta={"kernel": "bn", "flops": 0, "bytes": 0})
        if form.conv2 == "fused":
            self._heads_fused_setup()
        elif form.conv2 == "epilogue":
            self._heads_epilogue_table(conv2s)
        else:
            # (the conv1 launches above wrote the slices of hfeat; the 1x1 convolutions go as one launch)
            self._heads_second_outputs(conv2s, form)
            self.emit_heads_batch(self.fwd_ops, conv2s, 0, "fwd out_modules.*.conv2")

    def _heads_alloc(self, form):
        """features, statistics and output maps of all heads"""
        h, w, nh = self.h, self.w, len(self.heads)
        self.hepi = None
        if form.conv2 == "epilogue":
            self.hepi = torch.zeros(nh * C.sizeof(L.HeadsEpi), dtype=torch.uint8, device=self.dev)
            self.keep.append(self.hepi)
            # (a placeholder: with heads_epi the convolution does not write its y)
            self.hfeat = self.new((1, 1, 1, 128 * nh), self._tdt(L.FP8) if form.f8_feat else None)
            self.hcoef = None
        else:
            self.hfeat, self.hcoef = self.act_buf(h, w, 128 * nh, L.FP8 if form.f8_feat else None)
        if form.f8_feat:
            self.hfeat_q = (self.new((nh,), torch.float32, 0.0), self.new((nh,), torch.float32, 1.0), self.new((nh,), torch.float32, 1.0))
        # the list forward() returns: one contiguous NCHW f32 map per head (unet.py:119), written directly
        self.logits = [self.new((self.B, hc, h, w), torch.float32) for hc in self.heads]
        self.head_recs, self.head2 = [], []
        # batch statistics of the eight heads' BatchNorms side by side (one act_bwd pass over all 8 x 128 channels)
        self.hmean, self.hinvstd = self.new((128 * nh,), torch.float32), self.new((128 * nh,), torch.float32, 1.0)

    def _heads_conv1_merged(self, trunk: Src, form):
        """pack the eight conv1 weights one below the other ([tap][chunk][8 x 128][CK]), gather their biases, emit the one
        convolution into hfeat; returns (stats partials [nblk][2][8 x 128] or None, nblk)"""
        h, w, nh = self.h, self.w, len(self.heads)
        Ct = 128 * nh
        taps = taps_square(3)
        f8 = self.fold and trunk.dt == L.FP8      # fp8 graph: e4m3 trunk and weights (the features: form.f8_feat)
        wf = self.packed(len(taps), 128, Ct, cdt=L.FP8 if f8 else None)
        bias_all = self.new((Ct,), torch.float32)
        if self.fold:
            scale_all = self.new((Ct,), torch.float32, 1.0)
            row_scale, deq_all = scale_all, None
            if f8:
                row_scale, deq_all = self.new((Ct,), torch.float32, 1.0), self.new((Ct,), torch.float32, 1.0)
            for i in range(nh):
                p = "out_modules.%d" % i
                sl = slice(128 * i, 128 * (i + 1))
                self._fold_coeffs(p + ".conv1", p + ".bn", 128, scale_all[sl], bias_all[sl])
                if f8:
                    self._fp8_weight_scales(p + ".conv1.weight", 128, 128 * 9, scale_all[sl], trunk.q[1], row_scale[sl], deq_all[sl])
                self.emit_pack(p + ".conv1.weight", wf, 0, 128, 128, 3, 128, 128, rows_total=Ct, rows_off=128 * i,
                               row_scale=row_scale[sl].data_ptr(), cdt=L.FP8 if f8 else None)
            self.emit_conv(self.fwd_ops, trunk, wf, bias_all.data_ptr(), self.hfeat, L.FP8 if form.f8_feat else self.dt, h, w, Ct, 0, Ct, taps,
                           what="fwd out_modules.*.conv1", out_slope=0.01, cdt=L.FP8 if f8 else None, out_scale=deq_all,
                           out_quant=self.hfeat_q[2] if form.f8_feat else None, out_quant_stride=1 if form.f8_feat else 0,
                           heads_epi=self.hepi)
            return None, 0
        for i in range(nh):
            self.emit_pack("out_modules.%d.conv1.weight" % i, wf, 0, 128, 128, 3, 128, 128, rows_total=Ct, rows_off=128 * i)
        srcs = (C.c_void_p * nh)(*[self.P("out_modules.%d.conv1.bias" % i) for i in range(nh)])
        counts = (C.c_int32 * nh)(*([128] * nh))
        bp = bias_all.data_ptr()
        self._emit(self.pack_ops, self.lib.abc_concat_f32, (srcs, counts, nh, bp), "gather out_modules.*.conv1.bias",
                   meta={"kernel": "concat", "flops": 0, "bytes": 0})
        return self.emit_conv(self.fwd_ops, trunk, wf, bp, self.hfeat, self.dt, h, w, Ct, 0, Ct, taps, stats=self.train,
                              what="fwd out_modules.*.conv1")

    def _head_conv1(self, i, trunk: Src, form, shared, fins):
        """head i's conv1 + BatchNorm record -- its own convolution, or its 128 columns of the merged one (shared); the finaliser goes
        to fins where the form batches them.  Returns the Src of its features as conv2 reads them"""
        nh = len(self.heads)
        p = "out_modules.%d" % i
        rec, f = self.conv_bn(p + ".conv1", p + ".bn", trunk, 128, 3, (self.hfeat, self.hcoef, self.h, self.w, 128 * nh, 128 * i), 0.01,
                              stat_out=(self.hmean[128 * i:128 * (i + 1)], self.hinvstd[128 * i:128 * (i + 1)]),
                              collect_fin=fins if form.batch_fin else None, shared=shared)
        rec.is_head = True
        self.head_recs.append(rec)
        f.drop_p, f.drop_seed, f.drop_salt = self.drop_p, self.drop_seed, self.drop_salt
        return f

    def _head_conv2(self, i, f: Src, form, conv2s):
        """head i's 1x1 convolution over its features f: the packed weights, then by form the collected launch (for
        emit_heads_batch) or the item of the epilogue table; the fused pass packs and computes all of it itself"""
        hc = self.heads[i]
        p = "out_modules.%d.conv2" % i
        self.head2.append(Rec(kind="head2", cname=p, src=f, cout=hc, idx=i))
        if form.conv2 == "fused":
            return
        rows_pad = -(-hc // 32) * 32
        cdt = row_scale = deq = None
        if form.f8_feat:
            f.dt, f.q = L.FP8, tuple(t[i:i + 1] for t in self.hfeat_q)
            qmul, deq = self._fp8_weight_scales(p + ".weight", hc, 128, None, f.q[1], self.new((hc,), torch.float32, 1.0),
                                                self.new((hc,), torch.float32, 1.0))
            cdt, row_scale = L.FP8, qmul.data_ptr()
        w2 = self.packed(1, 128, rows_pad, cdt=cdt)
        self.emit_pack(p + ".weight", w2, 0, hc, 128, 1, rows_pad, 128, row_scale=row_scale, cdt=cdt)
        if form.conv2 == "epilogue":
            conv2s.append((w2, self.P(p + ".bias"), deq, self.logits[i], hc, rows_pad))
        else:
            self.emit_conv(self.fwd_ops, f, w2, self.P(p + ".bias"), self.logits[i], L.F32, self.h, self.w, hc, 0, hc, [(0, 0)],
                           what="fwd %s" % p, planar_out=True, collect=conv2s, cdt=cdt, out_scale=deq)

    def _heads_epilogue_table(self, items):
        """the table the merged conv1 reads in its epilogue: static pointers, written once"""
        host = (L.HeadsEpi * len(items))()
        for i, (w2, bias_ptr, deq, lg, hc, rows_pad) in enumerate(items):
            host[i].w2, host[i].bias, host[i].oscale = w2.data_ptr(), bias_ptr, (None if deq is None else deq.data_ptr())
            host[i].y, host[i].Cout, host[i].Cout_pad = lg.data_ptr(), hc, rows_pad
        self.hepi.copy_(torch.frombuffer(bytearray(bytes(host)), dtype=torch.uint8))
        self.keep.append(items)

    def _heads_try(self, changes, asked):
        """set descriptor fields -- changes = [(descriptor, field, value)] -- if the heads' 1x1 kernel (abc_conv_variant 3) then still
        serves every descriptor of `asked`; else put them back as they were.  Returns whether they stay"""
        old = [(d, name, getattr(d, name)) for d, name, _v in changes]
        for d, name, v in changes:
            setattr(d, name, v)
        if all(self.lib.abc_conv_variant(C.byref(d)) == 3 for d in asked):
            return True
        for d, name, v in old:
            setattr(d, name, v)
        return False

    def _heads_second_outputs(self, convs, form):
        """NMS / decode outputs of the collected 1x1 convolutions (emit_conv(collect=...) items of train.py:47's eight heads), where
        the form asks for them and the library grants them.  Returns what was granted: (), (nms_rho, nms_omega) or those and btype_idx"""
        if not form.nms:
            return ()
        B, h, w = self.B, self.h, self.w
        (d5, _w5, m5), (d6, _w6, m6), (d7, _w7, m7) = convs[5:8]
        rho, om = self.new((B, 60, h, w), torch.float32), self.new((B, 60, h, w), torch.float32)
        if not self._heads_try([(d6, "head_aux", rho.data_ptr()), (d6, "head_aux_mode", 1), (d7, "head_aux", om.data_ptr()), (d7, "head_aux_mode", 2)],
                               (d6, d7)):
            return ()
        self.nms_rho, self.nms_omega = rho, om
        m7["bytes"] += float(B * 60 * h * w * 4)
        m6["bytes"] += float(B * 60 * h * w * 4)
        if not form.decode:
            return rho, om
        idx = self.new((B, 60, h, w), torch.uint8)
        if not self._heads_try([(d5, "head_aux", idx.data_ptr()), (d5, "head_aux_mode", 3), (d5, "y", None), (d6, "y", None)], (d5, d6)):
            self.decode = False
            return rho, om
        self.btype_idx = idx
        m5["bytes"] -= float(B * 360 * h * w * 4 - B * 60 * h * w)
        m6["bytes"] -= float(B * 60 * h * w * 4)
        # (the bond-type and rho maps are neither written nor read in decode mode: release them -- 1.7 GB at b64 @ 512 x 512)
        for dead in (self.logits[5], self.logits[6]):
            self.keep[:] = [t for t in self.keep if t is not dead]
        self.logits[5] = self.logits[6] = None
        return rho, om, idx

    def _heads_fused_setup(self):
        """descriptor + buffers of the fused heads pass (abc_heads_fused_*): the conv2 forward leaves the forward plan -- the
        Trainer runs abc_heads_fused_fwd_bwd + abc_loss_finalize between forward and backward (ops.FusedHeadsLoss, which also
        binds the targets) -- and the backward plan starts from its outputs (_heads_backward)"""
        lib, nh, B, h, w = self.lib, len(self.heads), self.B, self.h, self.w
        Ct = 128 * nh
        d = L.HeadsFusedDesc()
        sc, sh, sl = self.hcoef
        d.feat, d.ld = self.hfeat.data_ptr(), Ct
        d.scale, d.shift, d.slope = sc.data_ptr(), sh.data_ptr(), sl.data_ptr()
        d.mean, d.invstd = self.hmean.data_ptr(), self.hinvstd.data_ptr()
        d.drop_p, d.drop_seed = self.drop_p, self.drop_seed
        d.drop_salt = self.drop_salt.data_ptr() if self.drop_p > 0 else None
        d.B, d.h, d.w = B, h, w
        nchunk = lib.abc_heads_fused_chunks(C.byref(d))
        self.hf_pack = self.new((lib.abc_heads_fused_pack_bytes() // 4 + 4,), torch.float32)
        self.hf_dl = self.new((lib.abc_heads_fused_dl_elems(C.byref(d)),), torch.bfloat16)
        self.hf_g = self.new((B, h, w, Ct))
        self.hf_bnpart = self.new((nchunk, 2, Ct), torch.float32)
        self.hf_lossblocks = lib.abc_heads_fused_loss_blocks(C.byref(d))
        self.hf_losspart = torch.zeros((self.hf_lossblocks, 16), dtype=torch.float64, device=self.dev)
        self.chan_scale = self.new((sum(self.heads),), torch.float32, 0.0)
        self.hf_work = self.new((lib.abc_heads_fused_wgrad_floats(C.byref(d)),), torch.float32)
        d.w2_pack, d.dl, d.g = self.hf_pack.data_ptr(), self.hf_dl.data_ptr(), self.hf_g.data_ptr()
        d.bn_partial, d.loss_partial = self.hf_bnpart.data_ptr(), self.hf_losspart.data_ptr()
        d.chan_scale, d.wgrad_work = self.chan_scale.data_ptr(), self.hf_work.data_ptr()
        if self.drop_p > 0:
            # the dropout keep bits of the three wide heads' features, from the fused pass to its conv2 weight gradient
            self.hf_keep = self.new((3 * B * h * w * 16,), torch.uint8, 0)
            d.keep_mask = self.hf_keep.data_ptr()
        # which bond-type row tiles carried a target (abc_heads_fused_desc.dl_tiles): the fused pass writes d(logits) only there and
        # its conv2 weight gradient reads only those; one word per 128-pixel chunk, rewritten by every step
        self.hf_tiles = self.new((nchunk,), torch.int64, 0)
        d.dl_tiles = self.hf_tiles.data_ptr()
        d.no_zero_skip = 0 if self.zero_skip else 1
        for i in range(nh):
            p = "out_modules.%d.conv2" % i
            d.w2[i], d.b2[i], d.logits[i] = self.P(p + ".weight"), self.P(p + ".bias"), self.logits[i].data_ptr()
            d.dw2[i], d.db2[i], d.chan_off[i] = self.G(p + ".weight"), self.G(p + ".bias"), self.head_off[i]
        self.hf, self.hf_chunks = d, nchunk
        self._emit(self.pack_ops, lib.abc_heads_fused_pack, (d,), "pack out_modules.*.conv2", meta={"kernel": "heads_fused_pack", "flops": 0, "bytes": 0})

    def emit_heads_batch(self, ops, items, which, what):
        """the heads' 1x1 convolutions collected by emit_conv(collect=...) as ONE launch (abc_heads_batch) when every one of
        them is served by the dedicated heads kernel (which = 0 forward / 1 data gradient), else one launch each"""
        want = 3 if which == 0 else 4
        ok = 1 <= len(items) <= 8 and all(self.lib.abc_conv_variant(C.byref(d)) == want for d, _w, _m in items) and self.batched_heads
        if not ok:
            for d, w, m in items:
                self._emit(ops, self.lib.abc_conv_fwd, (d,), w, meta=m)
            return
        arr, meta = self._batch([d for d, _w, _m in items], [m for _d, _w, m in items], "heads_%s_batch" % ("fwd" if which == 0 else "dgrad"))
        self._emit(ops, self.lib.abc_heads_batch, (arr, len(items), which), what, meta=meta)

    def _calibrate_fp8_heads(self, ref, stream, margin):
        """calibrate_fp8 for the heads' e4m3 features, where the plan has them: 128 columns each of one tensor, each head its own scale"""
        if not self.heads_form.f8_feat:
            return
        lib = self.lib
        amax, s, inv_s = self.hfeat_q
        nh = amax.numel()
        npx = ref.hfeat.numel() // (128 * nh)
        L.check(lib.abc_fill_f32(amax.data_ptr(), 0.0, nh, stream), "fill")
        for i in range(nh):
            L.check(lib.abc_absmax_cols(ref.hfeat.data_ptr(), L.BF16, npx, 128 * nh, 128 * i, 128, amax.data_ptr() + 4 * i, stream), "absmax_cols")
            L.check(lib.abc_fp8_act_scale(amax.data_ptr() + 4 * i, margin, s.data_ptr() + 4 * i, inv_s.data_ptr() + 4 * i, stream), "fp8_act_scale")

    # ------------------------------------------------------------------ backward plan
    def _heads_backward(self, ops):
        """conv2 backward by form, down to d(BatchNorm output) g of all heads; then, for both forms, the batched BatchNorm finalisers where
        g is one tensor, conv1's weight gradients (merged, else per head) and conv1's merged data gradient"""
        nh = len(self.heads)
        taps = taps_square(3)
        dyh = self.new((self.B, self.h, self.w, 128 * nh))
        fused = self.heads_form.conv2 == "fused"
        if fused:
            wide, dfeat = self._heads_conv2_backward_fused(ops), None
        else:
            wide, dfeat = self._heads_conv2_backward(ops)
        merged = None if wide is None else self._heads_bn_bwd_batch(ops, *wide)
        if merged is None or not self._heads_conv1_wgrad_merged(ops, merged, dyh, taps):
            if fused:
                raise RuntimeError("fused heads: the merged conv1 weight gradient was refused")
            self._heads_conv1_wgrad_per_head(ops, merged, dfeat, dyh, taps)
        self._heads_conv1_dgrad(ops, dyh, taps)

    def _heads_conv2_backward_fused(self, ops):
        """behind the fused heads pass: conv2's weight / bias gradients from the blocked d(logits).  Returns the pass's g and its
        BatchNorm partial sums, to be scaled by the head's loss factor (the arguments of _heads_bn_bwd_batch)"""
        nh = len(self.heads)
        npx = self.B * self.h * self.w
        writes = tuple(n for i in range(nh) for n in ("out_modules.%d.conv2.weight" % i, "out_modules.%d.conv2.bias" % i))
        self._emit(ops, self.lib.abc_heads_fused_wgrad, (self.hf,), "wgrad out_modules.*.conv2", writes,
                   {"kernel": "heads_fused_wgrad", "flops": 2.0 * npx * sum(self.heads) * 128,
                    "bytes": float(npx * 128 * nh * 2 + self.hf_dl.numel() * 2 + self.hf_work.numel() * 4)})
        return self.hf_g, self.hf_bnpart, self.hf_chunks, self.chan_scale

    def _heads_drop(self):
        return (self.drop_p, self.drop_seed) if self.drop_p > 0 else None

    def _heads_conv2_backward(self, ops):
        """from dlogits (written by the loss): conv2's weight, bias and data gradients, then -- where one pass serves all heads -- act_bwd.
        Returns (the arguments of _heads_bn_bwd_batch or None, dfeat = d(conv2 input) of all heads side by side)"""
        B, h, w = self.B, self.h, self.w
        nh = len(self.heads)
        self.dlogits = [self.new((B, hc, h, w), torch.float32) for hc in self.heads]
        self.chan_scale = self.new((sum(self.heads),), torch.float32, 0.0)
        one = self.new((max(self.heads),), torch.float32, 1.0)
        zero = self.new((max(self.heads),), torch.float32, 0.0)
        dfeat = self.new((B, h, w, 128 * nh))
        # ---- heads' 1x1 convs (weight gradients one by one, the eight data gradients as one launch)
        head_dgrads, head_wgrads = [], []
        # K-splits of the heads' batched 1x1 weight gradient: ONE round of ~256 workgroups over all heads, instead of 256 splits
        # per head = 8 rounds of workgroups that each lived for 4 chunks and wrote a 64 KB slab.  Shared out by the measured
        # cost of a 128-pixel chunk: ~4 us for the feature tile alone, ~9 us with 128 rows of dL beside it (the rows of the
        # channel-planar dL are 36 KB apart: 128 concurrent 512-byte streams per workgroup, poor DRAM page locality)
        units = [-(-(-(-hc // 32)) // 4) for hc in self.heads]
        cost = [4.0 + 5.2 * (hc / u) / 128.0 for hc, u in zip(self.heads, units)]
        tot = sum(u * c for u, c in zip(units, cost))
        head_splits = [max(1, int(256 * c / tot)) for c in cost] if self.batched_heads else [None] * nh
        for r2 in self.head2:
            i, hc = r2.idx, r2.cout
            cs = self.chan_scale[self.head_off[i]:self.head_off[i] + hc]
            dl = Src(self.dlogits[i], L.F32, h, w, 0, 0, hc, coef=(cs, zero, one), planar=True)
            got = self.emit_wgrad(ops, dl, r2.src, hc, 128, [(0, 0)], 1, r2.cname + ".weight", "wgrad " + r2.cname,
                                  rowsum_to=r2.cname + ".bias", collect=head_wgrads, nsplit=head_splits[i])
            if got != "rowsum":
                psw = self.new((self.lib.abc_plane_sum_work(hc),), torch.float32)
                a = (self.dlogits[i].data_ptr(), B, hc, h * w, cs.data_ptr(), psw.data_ptr(), self.G(r2.cname + ".bias"))
                self._emit(ops, self.lib.abc_plane_sum, a, "dbias " + r2.cname, (r2.cname + ".bias",),
                           {"kernel": "plane_sum", "flops": 0, "bytes": float(B * hc * h * w * 4)})
            wd = self._pack_weights(r2.cname + ".weight", 1, hc, 128, 1)
            self.emit_conv(ops, dl, wd, None, dfeat, self.dt, h, w, 128 * nh, 128 * i, 128, [(0, 0)], what="dgrad " + r2.cname,
                           collect=head_dgrads)
        self.emit_wgrad_heads_batch(ops, head_wgrads, "wgrad out_modules.*.conv2")
        self.emit_heads_batch(ops, head_dgrads, 1, "dgrad out_modules.*.conv2")
        # (the one act_bwd pass over 128 x nh channels takes 16 nh bf16 vectors per pixel, which must divide its 256 threads: 1, 2, 4
        #  or 8 heads; unet.py's default six heads and other counts take the per-head passes of _heads_conv1_wgrad_per_head)
        if not (self.dt == L.BF16 and self.batched_heads and nh in (1, 2, 4, 8)):
            return None, dfeat
        # BN -> LeakyReLU -> Dropout backward of ALL heads as one pass over the 8 x 128 channels of hfeat / dfeat (their
        # coefficient and statistics arrays sit side by side), one batched finalisation
        g = self.new((B, h, w, 128 * nh))
        sc, sh, sl = self.hcoef
        wide = Rec(bname="out_modules.*.bn", y=self.hfeat, ld=128 * nh, coff=0, cout=128 * nh, H=h, W=w, scale=sc, shift=sh, slopes=sl,
                   mean=self.hmean, invstd=self.hinvstd)
        part, nblk = self._act_bwd(ops, wide, (dfeat, 128 * nh, 0), None, g.data_ptr(), 128 * nh, self._heads_drop())
        self.heads_dfeat, self.heads_g = dfeat, g      # (handles for the in-situ parity tests)
        return (g, part, nblk), dfeat

    def _heads_conv1_wgrad_per_head(self, ops, merged, dfeat, dyh, taps):
        """conv1's weight gradient one launch per head, each leaving its dY in its channel slice of dyh.  merged: the per-head Srcs of
        _heads_bn_bwd_batch, or None -- then every head's BatchNorm backward (act_bwd over its slice of dfeat, finaliser) comes first"""
        nh = len(self.heads)
        drop = self._heads_drop()
        for i, rec in enumerate(self.head_recs):
            if self.dt == L.BF16:
                # bf16: the weight-gradient kernel applies the BN-backward correction on load and writes dY into this
                # head's channel slice of dyh (no separate apply pass)
                gsrc = merged[i] if merged is not None else self._bn_backward(ops, rec, (dfeat, 128 * nh, 128 * i), drop=drop, defer=True)[0]
                ok = self.emit_wgrad(ops, gsrc, rec.src, 128, 128, taps, 1, rec.cname + ".weight", "wgrad " + rec.cname,
                                     dual=(rec.y, rec.ld, rec.coff, dyh.data_ptr() + 128 * i * dyh.element_size(), 128 * nh))
                if not ok:
                    raise RuntimeError("fused BN-backward apply was refused for " + rec.cname)
            else:
                dY = self._bn_backward(ops, rec, (dfeat, 128 * nh, 128 * i), drop=drop, g=(dyh, 128 * nh, 128 * i), in_place=True)
                self.emit_wgrad(ops, dY, rec.src, 128, 128, taps, 1, rec.cname + ".weight", "wgrad " + rec.cname)

    def _heads_bn_bwd_batch(self, ops, g, part, nblk, in_scale=None):
        """the finalisers of all heads' BatchNorm backward as one launch, from partial sums [nblk][2][nh x 128] (in_scale: the flat
        per-channel loss-scale array, each head's factors from its offset); returns per head the Src of its 128 channels of g with the
        deferred-apply coefficients (as _bn_backward(defer=True))"""
        nh = len(self.heads)
        Ct = 128 * nh
        # the deferred-apply coefficients are indexed by the ABSOLUTE channel of g (abc_act_src): one array of 8 x 128 per
        # quantity, every head's finalisation writing its own slice
        ca_all, cb_all, cc_all = (self.new((Ct,), torch.float32) for _ in range(3))
        descs, writes, out = [], (), []
        for i, rec in enumerate(self.head_recs):
            sl = slice(128 * i, 128 * (i + 1))
            f, _k, wr = self._bn_bwd_desc(rec, part.data_ptr() + 4 * 128 * i, nblk, (ca_all[sl], cb_all[sl], cc_all[sl]),
                                          None if in_scale is None else in_scale.data_ptr() + 4 * self.head_off[i])
            descs.append(f)
            writes += wr
            out.append(Src(g, self.dt, rec.H, rec.W, Ct, 128 * i, 128, coef=(ca_all, cc_all, cb_all)))
        self._emit(ops, self.lib.abc_bn_finalize_bwd_batch, ((L.BnBwdDesc * nh)(*descs), nh, Ct), "bn_bwd out_modules.*.bn", writes,
                   {"kernel": "bn_bwd", "flops": 0, "bytes": 0})
        return out

    def _heads_conv1_wgrad_merged(self, ops, merged, dyh, taps):
        """The eight heads' conv1 weight gradients (unet.py:66, 8 x [128,128,3,3]) as ONE weight gradient with 8 x 128
        a-channels: the eight share their Q operand (the trunk activation), their P operands sit side by side in g / hfeat,
        so one launch of 8 x 2 tiles x 16 splits reads Q once per XCD, writes an eighth of the split-K slabs (16 instead
        of 128 slabs per head) and runs 72 instead of 9 patches per workgroup.  The slab reduction scatters the eight
        row blocks to the eight parameters' gradients (one batched launch).  False when the library does not serve the
        fused BatchNorm-backward load for this descriptor (the caller then emits one launch per head)."""
        nh = len(self.heads)
        Ct = 128 * nh
        q = self.head_recs[0].src
        g0 = merged[0]
        p = Src(g0.t, self.dt, g0.H, g0.W, Ct, 0, Ct, coef=g0.coef)
        got = self._wgrad_desc(p, q, Ct, 128, taps, 1, dual=(self.hfeat, Ct, 0, dyh.data_ptr(), Ct))
        if got is None:
            return False
        d, (ca_pad, cb_pad), _tile, nsplit, meta = got      # (the default K-split: emit_wgrad's per-tile overrides are not for this launch)
        d.nsplit = nsplit
        need = nsplit * len(taps) * ca_pad * cb_pad
        slabs = self.new((need,), torch.float32)
        d.partial = slabs.data_ptr()
        npx = self.B * g0.H * g0.W
        # g + y_raw read, dY written, Q read once, the slabs written
        meta["bytes"] = float(3 * npx * Ct * self._esz(self.dt) + npx * 128 * self._esz(q.dt) + need * 4)
        self._emit(ops, self.lib.abc_wgrad, (d,), "wgrad out_modules.*.conv1", meta=meta)
        # (this head's 128 rows of every slab)
        reduces = [self._reduce_desc(slabs.data_ptr() + 4 * 128 * i * cb_pad, nsplit, len(taps), 128, 128, ca_pad, cb_pad, self.G(rec.cname + ".weight"))
                   for i, rec in enumerate(self.head_recs)]
        self._emit(ops, self.lib.abc_wgrad_reduce_batch, ((L.WgradReduceDesc * nh)(*reduces), nh), "wgrad out_modules.*.conv1 reduce",
                   tuple(rec.cname + ".weight" for rec in self.head_recs),
                   {"kernel": "wgrad_reduce_batch", "flops": 0, "bytes": float(need * 4 + Ct * 128 * len(taps) * 4)})
        return True

    def _heads_conv1_dgrad(self, ops, dyh, taps):
        """the tail of both heads-backward plans: the eight heads' conv1 data gradients as ONE 8 x 128 -> 128 convolution over dyh, their dY
        side by side (unet.py:66,116-118 backward); the trunk's last layer has no reader but the heads, so its act_bwd pass rides in
        this launch's epilogue where the library serves it"""
        h, w = self.h, self.w
        Ct = 128 * len(self.heads)
        wd_all = self.packed(9, Ct, 128)
        for i, rec in enumerate(self.head_recs):
            self.emit_pack(rec.cname + ".weight", wd_all, 1, 128, 128, 3, 128, 128, red_total=Ct, red_off=128 * i)
        dtrunk = self.new((self.B, h, w, 128))
        self.dyh, self.dtrunk = dyh, dtrunk      # (handles for the in-situ parity tests)
        dy_all = Src(dyh, self.dt, h, w, Ct, 0, Ct)
        p = self.trunk.producer
        what = "dgrad heads.conv1"
        p.grad_same = (dtrunk, 128, 0)
        if (self.actbwd_epilogue and self.train and self.dt == L.BF16 and isinstance(p, Rec) and p.kind == "conv" and self.trunk.t is p.y and
                not self.trunk.pool and self.trunk.drop_p == 0 and p.coff == 0 and p.ld == p.cout == 128 and (p.H, p.W) == (h, w) and
                all(getattr(r, "is_head", False) for r in self.recs + list(self.head_recs)
                    if getattr(r, "src", None) is not None and (r.src.producer is p or r.src.t is p.y))):
            got = self.emit_conv(ops, dy_all, wd_all, None, dtrunk, self.dt, h, w, 128, 0, 128, taps_mirror(taps),
                                 what=what + " + act_bwd " + p.bname, actbwd=p)
            if got is not None:
                p.fused_g = (dtrunk, got[0], got[1])
                p.g = dtrunk
                self.heads_dgrad_is_g = True
                return
        self.emit_conv(ops, dy_all, wd_all, None, dtrunk, self.dt, h, w, 128, 0, 128, taps_mirror(taps), what=what)

    def emit_wgrad_heads_batch(self, ops, items, what):
        """the heads' 1x1 weight gradients collected by emit_wgrad(collect=...) as ONE launch (abc_wgrad_heads_batch) when the
        heads kernel serves every one of them ((0, 0) tile), else one launch each; their slab reductions follow"""
        def tile(d):
            at_, bt_ = L.i32(), L.i32()
            L.check(self.lib.abc_wgrad_tile(C.byref(d), C.byref(at_), C.byref(bt_)), "wgrad_tile")
            return at_.value, bt_.value
        ok = 1 <= len(items) <= 8 and all(tile(d) == (0, 0) for d, _w, _m, _p in items) and self.batched_heads
        if ok:
            arr, meta = self._batch([d for d, _w, _m, _p in items], [m for _d, _w, m, _p in items], "heads_wgrad_batch")
            self._emit(ops, self.lib.abc_wgrad_heads_batch, (arr, len(items)), what, meta=meta)
        else:
            for d, w, m, _p in items:
                self._emit(ops, self.lib.abc_wgrad, (d,), w, meta=m)
        posts = [p for _d, _w, _m, post in items for p in post]
        if ok and len(posts) <= 16:
            # the 8 weight-gradient and 8 bias row-sum reductions as one launch too
            rarr, meta = self._batch([rd for rd, _w, _wr, _m in posts], [m for _rd, _w, _wr, m in posts], "wgrad_reduce_batch")
            self._emit(ops, self.lib.abc_wgrad_reduce_batch, (rarr, len(posts)), what + " reduce",
                       tuple(w for _rd, _w, wr, _m in posts for w in wr), meta)
        else:
            for rd, w, wr, m in posts:
                self._emit(ops, self.lib.abc_wgrad_reduce, (rd,), w, writes=wr, meta=m)
