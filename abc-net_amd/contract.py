"""What the host wrappers around single kernels (ops, loss, raster, augment) and the two harnesses (train, infer) agree on,
stated once: the 8 heads of train.py:47 and the 8 target tensors of the reference's collate_fn (utils.py:300) with their one
checker and their one descriptor assignment, the head-map and device-tensor checks, the stream default, the pinned staging of
the three `load` methods, and the device / sparse-target rules Trainer and InferenceRunner share."""
from __future__ import annotations

import torch

from . import _lib as L
from .arch import TRAIN_HEADS

HEADS = tuple(TRAIN_HEADS)      # head widths (train.py:47): what the loss, the meters, extract.hip and eval_tables.hip read
HEAD_NAMES = ["atom_t", "atom_types", "atom_charges", "atom_hs", "bond_t", "bond_types", "bond_rhos", "bond_omega"]
# the targets in collate_fn order: [B, *channels, h, w]; rho / omega are f64 (numpy's default in the reference, utils.py:91)
TARGET_CHANNELS = ((1,), (14,), (3,), (2,), (1,), (6, 60), (60,), (60,))
TARGET_DTYPES = (torch.float32,) * 6 + (torch.float64,) * 2


def target_shapes(B, h, w):
    return [(B,) + c + (h, w) for c in TARGET_CHANNELS]


def alloc_targets(B, h, w, device):
    """the 8 target tensors, zeroed"""
    return [torch.zeros(s, dtype=dt, device=device) for s, dt in zip(target_shapes(B, h, w), TARGET_DTYPES)]


def check_targets(targets, B, h, w, what, exc, require_cuda=True, require_contiguous=True):
    """raise exc("<what>: target i ...") unless `targets` are the 8 tensors of the contract (contiguous, on a device)"""
    for i, (t, exp, dt) in enumerate(zip(targets, target_shapes(B, h, w), TARGET_DTYPES)):
        if tuple(t.shape) != exp or t.dtype != dt or (require_contiguous and not t.is_contiguous()) or (require_cuda and not t.is_cuda):
            raise exc("%s: target %d (%s) is %s %s%s, the contract is %s %s%s (collate_fn order; rho / omega f64)"
                      % (what, i, HEAD_NAMES[i], tuple(t.shape), t.dtype, "" if t.is_contiguous() else " non-contiguous", exp, dt,
                         " on the device (no CPU fallback)" if require_cuda else ""))


def set_target_ptrs(desc, targets):
    """the t_* fields of LossDesc, HeadsFusedDesc, MetricsDesc, EvalDesc and RasterDesc"""
    d = desc
    (d.t_atom, d.t_types, d.t_charges, d.t_hs, d.t_bond, d.t_btypes, d.t_rho, d.t_omega) = (t.data_ptr() for t in targets)


def check_head_maps(logits, B, h, w, optional, what):
    """the 8 head maps [B, HEADS[i], h, w]; None only at the indices in `optional` (decode mode stores neither the raw rho nor
    the 360 bond-type planes).  Shapes only: nothing touches a device."""
    for i, (t, c) in enumerate(zip(logits, HEADS)):
        if t is None and i in optional:
            continue
        if t is None or tuple(t.shape) != (B, c, h, w):
            raise ValueError("%s: head %d must be [%d, %d, %d, %d] (heads %s), got %s"
                             % (what, i, B, c, h, w, list(HEADS), None if t is None else tuple(t.shape)))


def require_device_tensor(t, dtype, what, exc=L.AbcNetHipError):
    """`t` is a contiguous device tensor of `dtype` (one dtype, or a tuple of admissible ones)"""
    dtypes = dtype if isinstance(dtype, tuple) else (dtype,)
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.is_contiguous() and t.dtype in dtypes):
        raise exc("%s must be a contiguous %s device tensor (no CPU fallback)" % (what, " / ".join(str(d)[6:] for d in dtypes)))


def current_stream(device=None):
    """the raw handle of torch's current stream on `device` (None: the current device)"""
    return torch.cuda.current_stream(device).cuda_stream


def stream_or_current(stream, device=None):
    """the default of every run(stream=None)"""
    if stream is None:
        stream = current_stream(device)
    return stream


class PinnedStaging:
    """Pinned host buffers, their device twins and the event of the last host-to-device copy: what a `load` that ships a few KB
    per step needs.  buffers: {name: (shape, dtype[, fill])}; .host / .dev hold the tensors under those names, in that order.

        ... validate (anything that can raise) ...
        staging.wait()
        ... fill staging.host[...] ...
        staging.commit()

    The host buffers are reused, and a loop that never syncs runs many steps ahead of the device: without wait() a later batch
    would overwrite them while an earlier copy is still reading -- the maps would be rasterised from a LATER batch's records."""

    def __init__(self, device, buffers):
        self.host, self.dev = {}, {}
        for name, (shape, dtype, *fill) in buffers.items():
            self.host[name] = torch.full(shape, fill[0] if fill else 0, dtype=dtype, pin_memory=True)
            self.dev[name] = self.host[name].to(device)
        self.device = torch.device(device)
        self._copied = None

    def wait(self):
        """block until the previous commit()'s copies have left the host buffers"""
        if self._copied is not None:
            self._copied.synchronize()

    def commit(self):
        """asynchronous copies of every buffer on the twins' current stream, then the event wait() waits for"""
        for name, src in self.host.items():
            self.dev[name].copy_(src, non_blocking=True)
        self._copied = torch.cuda.Event()
        self._copied.record(torch.cuda.current_stream(self.device))


# ---------------------------------------------------------------------------------------------- Trainer and InferenceRunner
def resolve_device(model, device, who):
    """the GPU `who` runs on: `device`, else the model's, with its index filled in"""
    if not torch.cuda.is_available():
        raise L.AbcNetHipError("%s needs an MI355X; abcnet_amd has no CPU fallback" % who)
    dev = torch.device(device or next(model.parameters()).device)
    if dev.type != "cuda":
        raise L.AbcNetHipError("%s: the model must live on a GPU (got %s); abcnet_amd has no CPU fallback" % (who, dev))
    if dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    return dev


def check_sparse_rasterizer(rasterizer, targets, who):
    """use_sparse_targets(rasterizer): its group flags describe `targets` only if it is sparse and draws into these very tensors"""
    if not getattr(rasterizer, "sparse", False) or any(a.data_ptr() != b.data_ptr() for a, b in zip(rasterizer.targets, targets)):
        raise L.AbcNetHipError("use_sparse_targets: a TargetRasterizer(sparse=True) over this %s's own target tensors" % who)


def refuse_dense_targets(rasterizer):
    """load_batch(dense targets) while a sparse rasteriser owns the target tensors"""
    if rasterizer is not None:
        raise L.AbcNetHipError("load_batch(dense targets) under use_sparse_targets(): the rasteriser's group flags would no longer "
                               "describe the maps; load records into the rasteriser, or call use_sparse_targets(None) first")
