"""The loss of the reference training loop (train.py:95-137) as ONE autograd op on the HIP kernels:

    loss = abc_loss(model(imgs), targets, model.s)      # replaces train.py:95-137
    loss.backward()                                     # d/dpreds and d/ds

``preds`` are the 8 NCHW f32 device maps of heads [1,14,3,2,1,360,60,60] (train.py:47) from any producer (UNet,
nn.DataParallel(UNet), a plain torch module); ``targets`` the 8 tensors of collate_fn in the contract of
contract.check_targets (rho / omega f64); ``s`` the 10 uncertainty weights (model.s / model.module.s).
The result is a 0-d f64 device tensor, as in the reference, and nothing here synchronises with the host.

Forward: abc_loss_fwd_bwd (activations, the 8 terms' partial sums and the unscaled d(numerator)/d(logits) in one pass)
+ abc_loss_finalize, into buffers this call owns.  Backward: abc_loss_scale_grads turns those into true gradients in place,
times the incoming gradient read on the device, so (0.5 * loss).backward() and (loss_a + loss_b).backward() stay exact.
The meters of train.py:145-215 take the same logits: ops.FusedMetrics.
"""
from __future__ import annotations

import ctypes as C

import torch
import torch.nn as nn
from torch.autograd.function import once_differentiable

from . import _lib as L
from .contract import HEADS, TARGET_CHANNELS, TARGET_DTYPES, check_targets, current_stream, set_target_ptrs  # noqa: F401
from .ops import _fin_desc, terms_dict  # noqa: F401


def _check(preds, targets, s):
    """shapes and dtypes first (ValueError, nothing touches a device), then placement (AbcNetHipError: no CPU fallback)"""
    preds, targets = list(preds), list(targets)
    if len(preds) != 8 or len(targets) != 8:
        raise ValueError("abc_loss: 8 head maps and 8 targets (train.py:94), got %d and %d" % (len(preds), len(targets)))
    if not all(isinstance(t, torch.Tensor) for t in preds + targets + [s]):
        raise ValueError("abc_loss: preds, targets and s must be tensors")
    if any(p.dim() != 4 for p in preds):
        raise ValueError("abc_loss: preds must be NCHW maps")
    B, _, h, w = preds[0].shape
    got = tuple(int(p.shape[1]) for p in preds)
    if got != HEADS or any(tuple(p.shape) != (B, c, h, w) for p, c in zip(preds, HEADS)):
        raise ValueError("abc_loss is defined for heads %s on one [B, C, h, w] grid (train.py:47); got %s"
                         % (list(HEADS), [tuple(p.shape) for p in preds]))
    if any(p.dtype != torch.float32 for p in preds):
        raise ValueError("abc_loss: preds must be float32, got %s" % sorted({str(p.dtype) for p in preds}))
    # (forward() makes the targets contiguous itself, as it does the predictions)
    check_targets(targets, B, h, w, "abc_loss", ValueError, require_cuda=False, require_contiguous=False)
    if tuple(s.shape) != (10,) or s.dtype != torch.float32:
        raise ValueError("abc_loss: s must be the 10 float32 uncertainty weights (model.s), got %s %s" % (tuple(s.shape), s.dtype))
    dev = preds[0].device
    if any(not t.is_cuda or t.device != dev for t in preds + targets + [s]):
        raise L.AbcNetHipError("abc_loss: preds, targets and s must be on one GPU (no CPU fallback); got %s"
                               % sorted({str(t.device) for t in preds + targets + [s]}))
    return B, h, w


class _AbcLossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, box, targets, s, *preds):
        lib = L.load()
        B, h, w = preds[0].shape[0], preds[0].shape[2], preds[0].shape[3]
        dev = preds[0].device
        logits = [p.contiguous() for p in preds]
        tg = [t.contiguous() for t in targets]
        s = s.detach().contiguous()
        d = L.LossDesc()
        dl = [torch.empty_like(z) for z in logits]
        for i in range(8):
            d.logits[i], d.dlogits[i] = logits[i].data_ptr(), dl[i].data_ptr()
        set_target_ptrs(d, tg)
        d.B, d.h, d.w = B, h, w
        nblk = lib.abc_loss_blocks(C.byref(d))
        partial = torch.empty((nblk, 16), dtype=torch.float64, device=dev)
        out = torch.empty(17, dtype=torch.float64, device=dev)
        head_scale = torch.empty(8, dtype=torch.float32, device=dev)
        ds = torch.empty(10, dtype=torch.float32, device=dev)
        d.partial = partial.data_ptr()
        # one factor per head: channel i of head_scale is head i's
        f = _fin_desc(partial, s.data_ptr(), ds.data_ptr(), out, head_scale, range(8), [1] * 8, 1.0)
        with torch.cuda.device(dev):
            st = current_stream(dev)
            L.check(lib.abc_loss_fwd_bwd(C.byref(d), st), "loss_fwd_bwd")
            L.check(lib.abc_loss_finalize(C.byref(f), st), "loss_finalize")
        ctx.dl, ctx.ds, ctx.head_scale = dl, ds, head_scale
        box.append(out)
        return out[0]

    @staticmethod
    @once_differentiable
    def backward(ctx, g_total):
        if ctx.dl is None:
            raise RuntimeError("abc_loss: backward through the same loss twice is not supported (the gradients are scaled "
                               "in place in the buffers the forward wrote; compute the loss again)")
        dl, ds = ctx.dl, ctx.ds
        dev = dl[0].device
        g = g_total.to(device=dev, dtype=torch.float64).contiguous()
        d = L.LossScaleDesc()
        for i in range(8):
            d.dlogits[i], d.n[i] = dl[i].data_ptr(), dl[i].numel()
        d.head_scale, d.ds, d.grad_out = ctx.head_scale.data_ptr(), ds.data_ptr(), g.data_ptr()
        with torch.cuda.device(dev):
            L.check(L.load().abc_loss_scale_grads(C.byref(d), current_stream(dev)), "loss_scale_grads")
        ctx.dl = ctx.ds = ctx.head_scale = None
        return (None, None, ds) + tuple(dl)


def abc_loss(preds, targets, s, return_terms=False):
    """train.py:95-137 as one op: the total loss, a 0-d f64 device tensor (no host sync).
    return_terms=True: also the 17-entry f64 vector [total, 8 weighted terms, 8 raw terms] (head order of ops.HEAD_NAMES;
    not differentiable)."""
    _check(preds, targets, s)
    box = []
    total = _AbcLossFn.apply(box, list(targets), s, *preds)
    return (total, box[0]) if return_terms else total


class ABCLoss(nn.Module):
    """nn.Module form of abc_loss: ABCLoss()(preds, targets, s)"""

    def __init__(self, return_terms=False):
        super().__init__()
        self.return_terms = return_terms

    def forward(self, preds, targets, s):
        return abc_loss(preds, targets, s, return_terms=self.return_terms)
