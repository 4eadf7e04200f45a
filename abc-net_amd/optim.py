"""``torch.optim.Adam`` as one HIP launch per step (train.py:55: ``optim.Adam(model.parameters(), lr=2.5e-4,
weight_decay=1e-8)``):

    from abcnet_amd.optim import Adam
    optimizer = Adam(model.parameters(), lr=2.5e-4, weight_decay=1e-8)

Same semantics as torch.optim.Adam: L2 weight decay added to the gradient (not AdamW), param groups with ``lr`` read at
every step (schedulers work), params without ``.grad`` skipped (their step count does not advance), per-param state
``step`` / ``exp_avg`` / ``exp_avg_sq`` so that state_dict() / load_state_dict() are interchangeable with torch's.

abc_adam_multi updates every tensor of every group in one launch from a device table of segments {p, g, m, v, n}.  The
moments are allocated as one buffer per device laid out like the params, so runs of adjacent params with adjacent grads
(the UNet arena, whose .grad tensors are views of one gradient buffer) coalesce into a few segments.  The table is
uploaded with one async copy from pinned memory, and only when a pointer changed; the hyper-parameters (bias corrections
computed on the host from each param's step, as torch does) travel by value in the launch.
"""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib as L

_SEG_BYTES = C.sizeof(L.AdamSeg)


def _check_param(p):
    if not isinstance(p, torch.Tensor):
        raise TypeError("abcnet_amd.optim.Adam: params must be tensors")
    if p.dtype != torch.float32 or not p.is_cuda:
        raise L.AbcNetHipError("abcnet_amd.optim.Adam updates float32 GPU tensors only (no CPU fallback); got %s on %s"
                               % (p.dtype, p.device))
    if not p.is_contiguous():
        raise ValueError("abcnet_amd.optim.Adam: params must be contiguous")


class _Table:
    """the segment table of one device: pinned staging (two buffers, so that a new upload never overwrites one whose copy
    may still be queued) + the device copy the kernel reads"""

    def __init__(self, device):
        self.device = device
        self.blob = None          # bytes of the last upload
        self.dev = None
        self.pinned = [None, None]
        self.events = [None, None]
        self.turn = 0

    def upload(self, blob, stream):
        if blob == self.blob:
            return
        n = len(blob)
        k = self.turn
        self.turn ^= 1
        if self.events[k] is not None:
            self.events[k].synchronize()
        if self.pinned[k] is None or self.pinned[k].numel() < n:
            self.pinned[k] = torch.empty(max(n, 4096), dtype=torch.uint8, pin_memory=True)
        if self.dev is None or self.dev.numel() < n:
            self.dev = torch.empty(max(n, 4096), dtype=torch.uint8, device=self.device)
        C.memmove(self.pinned[k].data_ptr(), blob, n)
        with torch.cuda.stream(stream):
            self.dev[:n].copy_(self.pinned[k][:n], non_blocking=True)
            ev = torch.cuda.Event()
            ev.record(stream)
        self.events[k] = ev
        self.blob = blob


class Adam(torch.optim.Optimizer):
    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, amsgrad=False, *, foreach=None,
                 maximize=False, capturable=False, differentiable=False, fused=None, decoupled_weight_decay=False):
        if isinstance(lr, torch.Tensor):
            lr = float(lr)
        if not 0.0 <= lr:
            raise ValueError("Invalid learning rate: %s" % lr)
        if not 0.0 <= eps:
            raise ValueError("Invalid epsilon value: %s" % eps)
        if not 0.0 <= betas[0] < 1.0 or not 0.0 <= betas[1] < 1.0:
            raise ValueError("Invalid beta parameters: %s" % (betas,))
        if not 0.0 <= weight_decay:
            raise ValueError("Invalid weight_decay value: %s" % weight_decay)
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=amsgrad, maximize=maximize,
                        foreach=foreach, capturable=capturable, differentiable=differentiable, fused=fused,
                        decoupled_weight_decay=decoupled_weight_decay)
        self._refuse(defaults)
        self._tables = {}
        self._packed = False
        self.last_segments = 0      # segments of the last launch (the UNet arena after loss.backward(): 2, s.grad apart)
        super().__init__(params, defaults)

    @staticmethod
    def _refuse(group):
        for k in ("amsgrad", "maximize", "capturable", "differentiable", "fused", "decoupled_weight_decay"):
            if group.get(k):
                raise ValueError("abcnet_amd.optim.Adam: %s=%r is not supported (torch.optim.Adam semantics with L2 decay "
                                 "only; use torch.optim.Adam for it)" % (k, group[k]))

    def add_param_group(self, param_group):
        self._refuse(param_group)
        params = param_group["params"]
        param_group["params"] = [params] if isinstance(params, torch.Tensor) else list(params)
        for p in param_group["params"]:
            _check_param(p)
        super().add_param_group(param_group)
        self._packed = False

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        for g in self.param_groups:
            self._refuse(g)
        self._packed = False

    # ------------------------------------------------------------------ moments
    def _pack(self, need):
        """(re)allocate exp_avg / exp_avg_sq of every param that has state or is about to get it as one buffer per device,
        in param order, adjacent where the params are adjacent (a new run starts 16-byte aligned); existing values move in"""
        order, seen = [], set()
        for g in self.param_groups:
            for p in g["params"]:
                if id(p) not in seen and (p in need or len(self.state.get(p, {})) > 0):
                    seen.add(id(p))
                    order.append(p)
        per_dev = {}
        for p in order:
            per_dev.setdefault(p.device, []).append(p)
        for dev, ps in per_dev.items():
            offs, off, end = [], 0, None
            for p in ps:
                if p.data_ptr() != end:
                    off = (off + 3) // 4 * 4
                offs.append(off)
                off += p.numel()
                end = p.data_ptr() + 4 * p.numel()
            m = torch.zeros(max(off, 1), dtype=torch.float32, device=dev)
            v = torch.zeros(max(off, 1), dtype=torch.float32, device=dev)
            for p, o in zip(ps, offs):
                st = self.state[p]
                mv = m[o:o + p.numel()].view_as(p)
                vv = v[o:o + p.numel()].view_as(p)
                if len(st) == 0:
                    st["step"] = torch.tensor(0.0, dtype=torch.float32)
                else:
                    mv.copy_(st["exp_avg"])
                    vv.copy_(st["exp_avg_sq"])
                st["exp_avg"], st["exp_avg_sq"] = mv, vv
        self._packed = True

    # ------------------------------------------------------------------ step
    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        live = []   # (group index, param)
        for gi, group in enumerate(self.param_groups):
            self._refuse(group)
            for p in group["params"]:
                if p.grad is None:
                    continue
                if p.grad.is_sparse:
                    raise ValueError("abcnet_amd.optim.Adam does not support sparse gradients")
                _check_param(p)
                if p.grad.dtype != torch.float32 or p.grad.device != p.device or p.grad.shape != p.shape:
                    raise ValueError("abcnet_amd.optim.Adam: .grad must be a float32 tensor of the param's shape on its device")
                live.append((gi, p))
        if not live:
            return loss
        need = {p for _, p in live if len(self.state.get(p, {})) == 0}
        if need or not self._packed:
            self._pack(need)
        steps = [self.state[p]["step"] for _, p in live]
        torch._foreach_add_(steps, 1)
        stepv = [s.item() for s in steps]
        keep = []   # grads made contiguous for the launch
        per_dev = {}
        for (gi, p), t in zip(live, stepv):
            g = p.grad if p.grad.is_contiguous() else p.grad.contiguous()
            if g is not p.grad:
                keep.append(g)
            st = self.state[p]
            per_dev.setdefault(p.device, []).append(((gi, t), p, g, st["exp_avg"], st["exp_avg_sq"]))
        for dev, items in per_dev.items():
            self._launch(dev, items)
        return loss

    def _launch(self, dev, items):
        lib = L.load()
        chunk = lib.abc_adam_multi_chunk()
        # classes = distinct (group, step); segments = runs of adjacent (p, g, m, v) within a class
        cls_of, segs = {}, []
        for key, p, g, m, v in items:
            c = cls_of.setdefault(key, len(cls_of))
            n = p.numel()
            if n == 0:
                continue
            pp, gp, mp, vp = p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr()
            if segs:
                s = segs[-1]
                if s[0] == c and s[1] + 4 * s[5] == pp and s[2] + 4 * s[5] == gp and s[3] + 4 * s[5] == mp and s[4] + 4 * s[5] == vp:
                    s[5] += n
                    continue
            segs.append([c, pp, gp, mp, vp, n])
        self.last_segments = len(segs)
        if not segs:
            return
        keys = sorted(cls_of, key=cls_of.get)
        # launches of at most ADAM_MAX_CLASSES classes each (one launch unless the groups' steps diverge that far)
        segs.sort(key=lambda s: s[0])
        table = (L.AdamSeg * len(segs))()
        launches, start = [], 0
        while start < len(segs):
            base = segs[start][0]
            stop = start
            while stop < len(segs) and segs[stop][0] < base + L.ADAM_MAX_CLASSES:
                stop += 1
            first = 0
            for j in range(start, stop):
                c, pp, gp, mp, vp, n = segs[j]
                table[j].p, table[j].g, table[j].m, table[j].v = pp, gp, mp, vp
                table[j].n, table[j].first_chunk, table[j].cls = n, first, c - base
                first += (n + chunk - 1) // chunk
            launches.append((start, stop, base, first))
            start = stop
        stream = torch.cuda.current_stream(dev)
        tab = self._tables.get(dev)
        if tab is None:
            tab = self._tables[dev] = _Table(dev)
        with torch.cuda.device(dev):
            tab.upload(bytes(table), stream)
            for start, stop, base, nchunk in launches:
                d = L.AdamMultiDesc()
                d.segs = tab.dev.data_ptr() + start * _SEG_BYTES
                d.nseg, d.chunk_total = stop - start, nchunk
                ncls = min(len(keys) - base, L.ADAM_MAX_CLASSES)
                d.nclass = ncls
                for k in range(ncls):
                    gi, t = keys[base + k]
                    group = self.param_groups[gi]
                    lr = float(group["lr"])
                    b1, b2 = group["betas"]
                    b1, b2 = float(b1), float(b2)
                    e = d.cls[k]
                    e.step_size = lr / (1.0 - b1 ** t)
                    e.bc2_sqrt = (1.0 - b2 ** t) ** 0.5
                    e.beta1, e.beta2, e.eps, e.weight_decay = b1, b2, float(group["eps"]), float(group["weight_decay"])
                L.check(lib.abc_adam_multi(C.byref(d), stream.cuda_stream), "adam_multi")
