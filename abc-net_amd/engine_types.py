"""What a launch plan is made of: the op record, an activation as a consumer sees it, a layer's record, tap lists.  Shared by
engine.py (the core and the trunk) and engine_heads.py (the heads)."""
from __future__ import annotations

from typing import NamedTuple

from . import _lib as L


def taps_square(k):
    p = (k - 1) // 2
    return [(ky - p, kx - p) for ky in range(k) for kx in range(k)]


def taps_mirror(taps):
    return [(-dy, -dx) for dy, dx in taps]


class Op(NamedTuple):
    """one launch of a plan: fn(*args, stream).  args keeps what it points to alive (byref objects hold their structure); it is a list
    because a workspace pointer may be patched in once the plan knows its size (_finish_build)"""
    fn: object
    args: list
    what: str
    writes: tuple   # names of parameters whose GRADIENT is final once this op has run (bucketed all-reduce)
    meta: dict      # {kernel, flops, bytes}: algorithmic work of this launch (for the roofline report)


class Src:
    """an activation as a consumer sees it: raw tensor + on-load transform"""

    def __init__(self, t, dt, H, W, ld, coff, C, coef=None, pool=False, drop_p=0.0, drop_seed=0, producer=None, planar=False):
        self.t, self.dt, self.H, self.W, self.ld, self.coff, self.C = t, dt, H, W, ld, coff, C
        self.coef, self.pool, self.drop_p, self.drop_seed, self.producer = coef, pool, drop_p, drop_seed, producer
        self.drop_salt = None  # device uint32 scalar added to drop_seed (the engine's per-step counter)
        self.planar = planar  # NCHW f32 [B][C][H][W] (head maps / their gradients)
        self.q = None         # fp8 tensors: (amax, s, 1 / s) device scalars of the per-tensor scale

    def lh(self):  # logical dims
        return (self.H // 2, self.W // 2) if self.pool else (self.H, self.W)

    def fill(self, a: L.ActSrc):
        a.x = self.t.data_ptr()
        a.planar, a.ctot = (1, self.C) if self.planar else (0, 0)
        if self.coef is not None:
            a.scale, a.shift, a.slope = (c.data_ptr() for c in self.coef)
        else:
            a.scale = a.shift = a.slope = None
        a.Hx, a.Wx, a.ldx, a.pool = self.H, self.W, self.ld, 1 if self.pool else 0
        a.drop_p, a.drop_seed = self.drop_p, self.drop_seed
        a.drop_salt = self.drop_salt.data_ptr() if (self.drop_salt is not None and self.drop_p > 0) else None


class Rec:
    """one conv (+BN) layer: what forward produced and what backward needs"""

    def __init__(self, **kw):
        self.grad_same = None  # (tensor, ld, coff): grad wrt the activated output, full resolution
        self.grad_pool = None  # (tensor, ld, coff): grad wrt the pooled activated output
        self.__dict__.update(kw)
