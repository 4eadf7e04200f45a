"""Thin host wrappers over single C-ABI kernels used outside the engine's static plan:
fused loss (train.py:95-137), inference NMS (img2smiles2.py:61-79), candidate extraction and graph assembly
(img2smiles2.py:113-311), the mol block text of the assembled molecules (generate_smiles.py:18-105) and a SMILES string of each, their
score against their annotations, fused Adam (train.py:55,141)."""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib as L
from .contract import (HEAD_NAMES, HEADS, REC_BOND_W, CandidateLists, DerivedGraphRecords, GraphRecords, MoleculeRows, PinnedStaging, check_head_maps,
                       check_targets, current_stream, require_device_tensor, set_target_ptrs, stream_or_current)

EXTRACT_HEADS = HEADS      # the head widths extract.hip reads (train.py:47)


def _fin_desc(partial, s_ptr, ds_ptr, out, chan_scale, chan_off, head_c, grad_scale):
    """abc_loss_finalize's descriptor: the partial sums of a loss pass -> `out` (17 terms), d(s), and one gradient factor per
    channel of `chan_scale`, head i's at chan_off[i] .. chan_off[i] + head_c[i]"""
    f = L.LossFinDesc()
    f.partial, f.nblk, f.s, f.ds, f.out = partial.data_ptr(), partial.shape[0], s_ptr, ds_ptr, out.data_ptr()
    f.chan_scale, f.nchan = chan_scale.data_ptr(), chan_scale.numel()
    for i in range(8):
        f.chan_off[i], f.head_c[i] = chan_off[i], head_c[i]
    f.grad_scale = grad_scale
    return f


def terms_dict(out):
    """the 17-entry vector of a loss (FusedLoss.out, abc_loss(..., return_terms=True)) as {total, <head>, raw_<head>} floats
    (host sync)"""
    o = out.detach().cpu()
    r = {"total": o[0].item()}
    for i, n in enumerate(HEAD_NAMES):
        r[n] = o[1 + i].item()
        r["raw_" + n] = o[9 + i].item()
    return r


class FusedLoss:
    """activation + 8-term loss + dlogits for fixed shapes; targets are read from the given (static) tensors"""

    def __init__(self, eng, targets, s_ptr, ds_ptr, grad_scale=1.0):
        self.eng, self.lib = eng, eng.lib
        self.targets = targets  # keep alive
        check_targets(targets, eng.B, eng.h, eng.w, "fused loss", ValueError, require_cuda=False)
        if tuple(eng.heads) != HEADS:
            raise ValueError("the fused loss is defined for heads %s (train.py:47), got heads %s" % (list(HEADS), eng.heads))
        self.d, self.partial = self._loss_desc(eng, targets)
        self.nblk = self.partial.shape[0]
        self.out = torch.zeros(17, dtype=torch.float64, device=eng.logits[0].device)
        self.f = _fin_desc(self.partial, s_ptr, ds_ptr, self.out, eng.chan_scale, eng.head_off, eng.heads, grad_scale)

    def _loss_desc(self, eng, targets):
        """(the descriptor of the loss pass, its [nblk, 16] partial sums)"""
        d = L.LossDesc()
        for i in range(8):
            d.logits[i], d.dlogits[i] = eng.logits[i].data_ptr(), eng.dlogits[i].data_ptr()
        set_target_ptrs(d, targets)
        d.B, d.h, d.w = eng.B, eng.h, eng.w
        partial = torch.zeros((self.lib.abc_loss_blocks(C.byref(d)), 16), dtype=torch.float64, device=eng.logits[0].device)
        d.partial = partial.data_ptr()
        return d, partial

    def run(self, stream):
        L.check(self.lib.abc_loss_fwd_bwd(C.byref(self.d), stream), "loss_fwd_bwd")
        L.check(self.lib.abc_loss_finalize(C.byref(self.f), stream), "loss_finalize")

    def total_device(self):
        """the total loss of the last step as a 0-d f64 DEVICE tensor (a view of the finaliser's output: no host sync)"""
        return self.out[0]

    def result(self):
        """dict: total + weighted terms + raw terms (device sync)"""
        return terms_dict(self.out)


class FusedHeadsLoss(FusedLoss):
    """The fused train step's heads (engine built with fused_heads=True): out_modules[i].conv2 + activation + loss +
    d(logits) + the gradient back to the heads' BatchNorm outputs in one pass (abc_heads_fused_fwd_bwd), then the same
    finalisation as FusedLoss.  Same interface."""

    def __init__(self, eng, targets, s_ptr, ds_ptr, grad_scale=1.0, keep_logits=True):
        """keep_logits=False: the logits never leave the kernel (eng.logits keep their old contents) -- for a training
        loop without the meters of train.py:145-215, the only other reader of the outputs"""
        self.keep_logits = keep_logits
        super().__init__(eng, targets, s_ptr, ds_ptr, grad_scale)

    def _loss_desc(self, eng, targets):
        d = eng.hf      # (the engine's own descriptor and partial sums: the pass is part of its plan)
        for i in range(8):
            d.logits[i] = eng.logits[i].data_ptr() if self.keep_logits else None
        set_target_ptrs(d, targets)
        return d, eng.hf_losspart

    def use_target_flags(self, flags):
        """flags: TargetRasterizer(sparse=True).group_flags of the rasteriser that draws THESE target tensors (or None: read every
        target plane).  A wave whose 32 pixels carry no target of a head then reads zeros from a 512-byte buffer instead of the maps
        (abc_heads_fused_desc.target_flags): the same loss and gradients bit for bit, 0.37 GB less read per step at b16 @ 384 x 384."""
        if flags is None:
            self.d.target_flags, self.d.zero_bytes = None, None
            self._tflags = None
            return
        n = self.eng.B * self.eng.h * self.eng.w // 32
        _check_target_flags(flags, n, "target flags")
        self._tzero = torch.zeros(512, dtype=torch.uint8, device=flags.device)
        self._tflags = flags
        self.d.target_flags, self.d.zero_bytes = flags.data_ptr(), self._tzero.data_ptr()

    def run(self, stream):
        L.check(self.lib.abc_heads_fused_fwd_bwd(C.byref(self.d), stream), "heads_fused_fwd_bwd")
        L.check(self.lib.abc_loss_finalize(C.byref(self.f), stream), "loss_finalize")


def _check_target_flags(flags, n, what):
    """TargetRasterizer(sparse=True).group_flags: one 32-bit word per 32 pixels of the batch"""
    require_device_tensor(flags, (torch.int32, torch.uint32), what)
    if flags.numel() != n:
        raise L.AbcNetHipError("%s: one 32-bit word per 32 pixels of the batch (%d words), got %d" % (what, n, flags.numel()))


METER_NAMES = [
    "atom_targets_precision", "atom_targets_precision3", "atom_targets_recall", "atom_targets_recall3",
    "atom_types_acc", "atom_charges_acc", "atom_hs_acc",
    "bond_targets_precision", "bond_targets_precision3", "bond_targets_recall", "bond_targets_recall3",
    "bond_types_acc", "bond_rhos_mae",
    "bond_omega_precision", "bond_omega_recall3", "bond_omega_recall", "bond_omega_precision3",
]


def meters_dict(totals, last=None, extra=None):
    """a [17, 2] table of (sum, count) rows -> {name: {"sum", "count", "avg"}} in METER_NAMES order (nan for an empty count);
    last: the table of the last batch alone adds "val", the AverageMeter field; extra: {key: 17 values} adds a column each"""
    totals = totals.cpu()
    out = {}
    for i, n in enumerate(METER_NAMES):
        s, c = totals[i, 0].item(), totals[i, 1].item()
        out[n] = {"sum": s, "count": c, "avg": s / c if c else float("nan")}
    if last is not None:
        for n, (ln, ld) in zip(METER_NAMES, last.cpu().tolist()):
            out[n]["val"] = ln / ld if ld else float("nan")
    for key, column in (extra or {}).items():
        for n, v in zip(METER_NAMES, column.cpu().tolist()):
            out[n][key] = v
    return out


class FusedMetrics:
    """The 17 AverageMeters of train.py:145-215 as one device-resident table: `run` adds the current batch
    (logits + targets already in HBM), `result` reads it (the only host sync), `reset` is the new-epoch
    re-creation of the meters (train.py:58-81)."""

    def __init__(self, logits, targets):
        lib = L.load()
        self.lib = lib
        B, _, h, w = logits[0].shape
        check_targets(targets, B, h, w, "metrics", L.AbcNetHipError)
        for t, c in zip(logits, HEADS):
            if tuple(t.shape) != (B, c, h, w) or t.dtype != torch.float32 or not t.is_contiguous() or not t.is_cuda:
                raise L.AbcNetHipError("metrics: logits must be the 8 contiguous NCHW f32 device maps of heads %s" % (list(HEADS),))
        self.keep = (list(logits), list(targets))
        dev = logits[0].device
        d = L.MetricsDesc()
        for i in range(8):
            d.logits[i] = logits[i].data_ptr()
        set_target_ptrs(d, targets)
        d.B, d.h, d.w = B, h, w
        self.peaks = torch.zeros((2, B, h, w), dtype=torch.uint8, device=dev)
        self.partial = torch.zeros((lib.abc_metrics_blocks(C.byref(d)), 24), dtype=torch.float64, device=dev)
        self.totals = torch.zeros((17, 2), dtype=torch.float64, device=dev)
        self.last = torch.zeros((17, 2), dtype=torch.float64, device=dev)
        d.peaks, d.partial, d.totals, d.last = self.peaks.data_ptr(), self.partial.data_ptr(), self.totals.data_ptr(), self.last.data_ptr()
        self.d = d

    def run(self, stream=None):
        L.check(self.lib.abc_metrics_update(C.byref(self.d), stream_or_current(stream)), "metrics_update")

    def reset(self):
        self.totals.zero_()

    def result(self):
        """{name: {"sum", "count", "avg", "val"}} -- the AverageMeter fields (device sync)"""
        return meters_dict(self.totals, self.last)


EVAL_TABLES = ["atom_detection", "atom_type", "atom_charge", "bond_detection", "bond_type"]   # test_accuracy.py:33-38


def eval_tables_from_counts(counts):
    """the 301 counts of abc_eval_desc (any integer array) -> the five float64 [n, 4] tables of test_accuracy.py:33-38
    (columns tp, tn, fp, fn; the detection tables never write tn) and the three confusion matrices C[target][predicted]"""
    import numpy as np
    c = np.asarray(counts).astype(np.float64)
    out, conf = {}, {}
    for name, off, n in (("atom_detection", 0, 14), ("bond_detection", 42, 6)):
        d = c[off:off + 3 * n].reshape(n, 3)
        out[name] = np.stack([d[:, 0], np.zeros(n), d[:, 1], d[:, 2]], axis=1)
    for name, off, n in (("atom_type", 60, 14), ("atom_charge", 256, 3), ("bond_type", 265, 6)):
        m = c[off:off + n * n].reshape(n, n)
        tp, row, col = np.diag(m), m.sum(1), m.sum(0)
        out[name] = np.stack([tp, m.sum() - row - col + tp, col - tp, row - tp], axis=1)
        conf[name] = m
    return out, conf


class EvalTables:
    """The per-class tables and the 17 inference-flavour meters of test_accuracy.py:105-298 as one device-resident table
    (csrc/eval_tables.hip).  Inputs are what an inference step leaves on the device -- the masks and |rho| of nms_peaks /
    InferenceRunner, the 8 head maps (decode mode: logits[5] / logits[6] may be None, the bond type then comes from
    `btype_idx`) -- and the 8 target maps of the loss.  `run` adds the current batch, `result` reads (the only host sync),
    `reset` starts over.  n_valid: a 1-element int32 DEVICE tensor; only images 0 .. n_valid - 1 count (read by the kernel, so a
    captured graph can evaluate a short last batch).  target_flags: TargetRasterizer(sparse=True).group_flags of the rasteriser
    that draws THESE target tensors (int32 or uint32, B * h * w / 32 words) -- `run` then reads the target planes only in the
    32-pixel groups an atom / a bond was drawn into (abc_eval_tables_update_sparse); the results are the dense call's bit for bit.

    The running totals are plain sums of counts and of (num, den) pairs: ranks that evaluate disjoint images can add (all-reduce)
    `counts_totals` and `meters_totals` and derive everything else from the sums."""

    def __init__(self, atom_mask, bond_mask, omega_mask, rho_abs, logits, targets, btype_idx=None, n_valid=None, target_flags=None):
        if len(logits) != 8 or len(targets) != 8 or logits[1] is None:
            raise ValueError("EvalTables wants the 8 head maps and the 8 target maps of heads %s" % (list(HEADS),))
        B, _, h, w = logits[1].shape
        # (|rho| comes as rho_abs; decode mode stores neither the raw rho nor the 360 bond-type planes)
        check_head_maps(logits, B, h, w, {6} if btype_idx is None else {5, 6}, "EvalTables")
        for name, t, c in (("atom_mask", atom_mask, 1), ("bond_mask", bond_mask, 1), ("omega_mask", omega_mask, 60), ("rho_abs", rho_abs, 60)):
            if tuple(t.shape) != (B, c, h, w):
                raise ValueError("EvalTables: %s must be [%d, %d, %d, %d], got %s" % (name, B, c, h, w, tuple(t.shape)))
        if btype_idx is not None and tuple(btype_idx.shape) != (B, 60, h, w):
            raise ValueError("EvalTables: btype_idx must be [%d, 60, %d, %d], got %s" % (B, h, w, tuple(btype_idx.shape)))
        check_targets(targets, B, h, w, "EvalTables", L.AbcNetHipError)
        read = [atom_mask, bond_mask, omega_mask, rho_abs, logits[1], logits[2], logits[3]] + ([logits[5]] if btype_idx is None else [])
        for t in read:
            require_device_tensor(t, torch.float32, "EvalTables: every mask and head map read")
        if btype_idx is not None:
            require_device_tensor(btype_idx, torch.uint8, "EvalTables: btype_idx")
        if n_valid is not None:
            require_device_tensor(n_valid, torch.int32, "EvalTables: n_valid (one element)")
            if n_valid.numel() != 1:
                raise L.AbcNetHipError("EvalTables: n_valid must be a one-element int32 device tensor")
        if target_flags is not None:
            if (h * w) % 32:
                raise L.AbcNetHipError("EvalTables: target_flags needs h * w a multiple of 32")
            _check_target_flags(target_flags, B * h * w // 32, "EvalTables: target_flags")
        lib = L.load()
        self.lib = lib
        dev = atom_mask.device
        d = L.EvalDesc()
        d.atom_mask, d.bond_mask, d.omega_mask, d.rho_abs = (t.data_ptr() for t in (atom_mask, bond_mask, omega_mask, rho_abs))
        d.types, d.charges, d.hs = logits[1].data_ptr(), logits[2].data_ptr(), logits[3].data_ptr()
        d.btypes = None if btype_idx is not None else logits[5].data_ptr()
        d.btype_idx = None if btype_idx is None else btype_idx.data_ptr()
        set_target_ptrs(d, targets)
        d.n_valid = None if n_valid is None else n_valid.data_ptr()
        d.B, d.h, d.w = B, h, w
        nblk = lib.abc_eval_tables_blocks(C.byref(d))
        if nblk < 1:
            L.check(nblk, "eval_tables_blocks")
        self.partial = torch.zeros((nblk, 24), dtype=torch.float64, device=dev)
        # (uint64 on the device; int64 here: the counts stay far below 2^63)
        self.counts_last = torch.zeros(L.EVAL_NCOUNT, dtype=torch.int64, device=dev)
        self.counts_totals = torch.zeros(L.EVAL_NCOUNT, dtype=torch.int64, device=dev)
        self.meters_last = torch.zeros((17, 2), dtype=torch.float64, device=dev)
        self.meters_totals = torch.zeros((17, 2), dtype=torch.float64, device=dev)
        d.partial = self.partial.data_ptr()
        d.counts_last, d.counts_totals = self.counts_last.data_ptr(), self.counts_totals.data_ptr()
        d.meters_last, d.meters_totals = self.meters_last.data_ptr(), self.meters_totals.data_ptr()
        self.d = d
        self.target_flags = target_flags
        self.keep = (atom_mask, bond_mask, omega_mask, rho_abs, list(logits), list(targets), btype_idx, n_valid)

    def run(self, stream=None):
        stream = stream_or_current(stream)
        if self.target_flags is not None:
            L.check(self.lib.abc_eval_tables_update_sparse(C.byref(self.d), self.target_flags.data_ptr(), stream), "eval_tables_update_sparse")
        else:
            L.check(self.lib.abc_eval_tables_update(C.byref(self.d), stream), "eval_tables_update")

    def reset(self):
        self.counts_totals.zero_()
        self.meters_totals.zero_()

    def result(self):
        """dict (device sync): the five tables of test_accuracy.py:33-38 as float64 [n, 4] (tp, tn, fp, fn) under their names,
        "confusion" {atom_type, atom_charge, bond_type: C[target][predicted]}, "precision" / "recall" {table: tp / (tp + fp + 1e-4),
        tp / (tp + fn + 1e-4)} (lines 285-298), "meters" {name: {"sum", "count", "avg", "val"}} (the AverageMeter fields), and
        "last": the tables of the last call alone"""
        counts, last = self.counts_totals.cpu().numpy(), self.counts_last.cpu().numpy()
        out, conf = eval_tables_from_counts(counts)
        out["confusion"] = conf
        out["precision"] = {k: out[k][:, 0] / (out[k][:, 0] + out[k][:, 2] + 1e-4) for k in EVAL_TABLES}
        out["recall"] = {k: out[k][:, 0] / (out[k][:, 0] + out[k][:, 3] + 1e-4) for k in EVAL_TABLES}
        out["last"] = eval_tables_from_counts(last)[0]
        out["meters"] = meters_dict(self.meters_totals, self.meters_last)
        return out


def check_nms_heads(heads, what):
    """img2smiles2.py:61-79 reads heads 0 and 4 as one-plane centre maps and heads 6 and 7 as rho / omega maps of the same
    number of bins: refuse a head list that does not have that form (the NMS kernel would read and write past its maps)"""
    heads = list(heads)
    if not (len(heads) == 8 and heads[0] == heads[4] == 1 and heads[6] == heads[7] >= 1):
        raise ValueError("%s needs 8 heads with heads[0] == heads[4] == 1 and heads[6] == heads[7] (the maps of img2smiles2.py:61-79), "
                         "got heads %s" % (what, heads))


def nms_peaks(atom, bond, rho, omega):
    """img2smiles2.py:61-79 on the NCHW f32 head maps: (atom_mask[B,1,h,w], bond_mask[B,1,h,w],
    |rho|[B,n,h,w], omega_mask[B,n,h,w]).  The kernel reads atom / bond as one plane per image and rho / omega as n planes
    each with n = omega.shape[1]: any other shape is refused before the device is touched."""
    shapes = [tuple(t.shape) for t in (atom, bond, rho, omega)]
    if any(len(s) != 4 for s in shapes):
        raise ValueError("nms_peaks wants four NCHW maps, got shapes %s" % (shapes,))
    B, n, h, w = shapes[3]
    if shapes[0] != (B, 1, h, w) or shapes[1] != (B, 1, h, w) or shapes[2] != (B, n, h, w) or n < 1:
        raise ValueError("nms_peaks: atom and bond must be [B,1,h,w] and rho and omega [B,n,h,w] with the same B, h, w and n; got "
                         "atom %s, bond %s, rho %s, omega %s" % tuple(shapes))
    for t in (atom, bond, rho, omega):
        require_device_tensor(t, torch.float32, "nms_peaks: every map")
    lib = L.load()
    am, bm, r, om = torch.empty_like(atom), torch.empty_like(bond), torch.empty_like(rho), torch.empty_like(omega)
    d = L.NmsDesc()
    d.atom, d.bond, d.rho, d.omega = atom.data_ptr(), bond.data_ptr(), rho.data_ptr(), omega.data_ptr()
    d.B, d.h, d.w, d.n_omega = B, h, w, n
    d.atom_mask, d.bond_mask, d.rho_abs, d.omega_mask = am.data_ptr(), bm.data_ptr(), r.data_ptr(), om.data_ptr()
    L.check(lib.abc_nms_peaks(C.byref(d), current_stream()), "nms_peaks")
    return am, bm, r, om


OMEGA_RULES = {"raw": L.OMEGA_RAW, "peaks": L.OMEGA_PEAKS}      # PeakExtractor(omega_rule=...) -> enum abc_omega_rule


class PeakExtractor:
    """img2smiles2.py:113-191 on the device: NMS masks + raw head maps -> compact ordered candidate lists (the wire
    format into the graph-assembly stage: GraphAssembler below, or the reference's own code on the host).  Static buffers, one launch, graph-capture safe; `lists()` is the
    only host sync (one small D2H per batch instead of hundreds of .item() calls per image).

    omega_rule: which omega bins of a bond peak are tried as candidates before the opposite-direction test.  "raw" (the default):
    every bin whose raw logit is non-zero, img2smiles2.py:139 -- the driver this package is measured against.  "peaks": every bin
    that is a circular 3-tap peak of the omega logits above -1 (the mask of img2smiles3.py:75-81), as img2smiles.py:139 and
    img2smiles3.py:140 walk it; the kernel recomputes the mask from logits[7], omega_mask is not an input.  `.omega_rule` names it."""

    def __init__(self, logits, atom_mask, bond_mask, cap_atoms=512, cap_bonds=16384, btype_idx=None, rho_abs=None, omega_rule="raw"):
        """btype_idx / rho_abs (decode mode, InferenceRunner(decode=True)): the uint8 arg-max map of the bond-type head and the |rho| map
        the heads kernel wrote instead of the raw maps logits[5] / logits[6] (which may then be None)"""
        # (extract.hip reads the head widths of train.py:47 -- 14 atom types, 3 charges, 2 hs, 360 bond-type planes, 60 rho and 60
        #  omega planes -- and one-plane masks: every shape is checked here, before the device is touched)
        if omega_rule not in OMEGA_RULES:
            raise ValueError("PeakExtractor: omega_rule must be one of %s, got %r" % (sorted(OMEGA_RULES), omega_rule))
        self.omega_rule = omega_rule
        if len(logits) != 8 or logits[0] is None:
            raise ValueError("PeakExtractor wants the 8 head maps of heads %s, got %d" % (list(HEADS), len(logits)))
        B, _, h, w = logits[0].shape
        optional = ({5} if btype_idx is not None else set()) | ({6} if rho_abs is not None else set())
        check_head_maps(logits, B, h, w, optional, "PeakExtractor")
        for name, t, c in (("atom_mask", atom_mask, 1), ("bond_mask", bond_mask, 1), ("rho_abs", rho_abs, 60)):
            if t is not None and tuple(t.shape) != (B, c, h, w):
                raise ValueError("PeakExtractor: %s must be [%d, %d, %d, %d], got %s" % (name, B, c, h, w, tuple(t.shape)))
        if btype_idx is not None and tuple(btype_idx.shape) != (B, 60, h, w):
            raise ValueError("PeakExtractor: btype_idx must be [%d, 60, %d, %d], got %s" % (B, h, w, tuple(btype_idx.shape)))
        lib = L.load()
        self.lib = lib
        need = [t for i, t in enumerate(logits) if i not in optional]
        for t in need + [atom_mask, bond_mask] + ([rho_abs] if rho_abs is not None else []):
            require_device_tensor(t, torch.float32, "PeakExtractor: every mask and head map read")
        if btype_idx is not None:
            require_device_tensor(btype_idx, torch.uint8, "PeakExtractor: btype_idx")
        dev = logits[0].device
        d = L.ExtractDesc()
        d.atom_mask, d.bond_mask = atom_mask.data_ptr(), bond_mask.data_ptr()
        d.types, d.charges, d.hs = logits[1].data_ptr(), logits[2].data_ptr(), logits[3].data_ptr()
        d.btypes = None if btype_idx is not None else logits[5].data_ptr()
        d.btype_idx = None if btype_idx is None else btype_idx.data_ptr()
        d.rho = rho_abs.data_ptr() if rho_abs is not None else logits[6].data_ptr()
        d.omega = logits[7].data_ptr()
        d.B, d.h, d.w, d.cap_atoms, d.cap_bonds = B, h, w, cap_atoms, cap_bonds
        d.omega_rule = OMEGA_RULES[omega_rule]
        self.counts = torch.zeros((B, 4), dtype=torch.int32, device=dev)
        self.atoms = torch.zeros((B, cap_atoms, 5), dtype=torch.int32, device=dev)
        self.bonds = torch.zeros((B, cap_bonds, 4), dtype=torch.int32, device=dev)
        self.bond_rho = torch.zeros((B, cap_bonds), dtype=torch.float32, device=dev)
        self.work = torch.zeros((lib.abc_extract_work_ints(C.byref(d)),), dtype=torch.int32, device=dev)
        self.work_masks = torch.zeros((lib.abc_extract_work_masks(C.byref(d)),), dtype=torch.int64, device=dev)
        d.counts, d.atoms, d.bonds, d.bond_rho = self.counts.data_ptr(), self.atoms.data_ptr(), self.bonds.data_ptr(), self.bond_rho.data_ptr()
        d.work, d.work_masks = self.work.data_ptr(), self.work_masks.data_ptr()
        self.d, self.keep = d, (list(logits), atom_mask, bond_mask, btype_idx, rho_abs)
        self.B, self.cap_atoms, self.cap_bonds = B, cap_atoms, cap_bonds
        self.candidates = CandidateLists(self.counts, self.atoms, self.bonds, self.bond_rho)

    def run(self, stream=None):
        L.check(self.lib.abc_extract_peaks(C.byref(self.d), stream_or_current(stream)), "extract_peaks")

    def lists(self):
        """per image: dict(atoms int32 [n,5], bonds int32 [m,4], rho f32 [m], counts (4,), truncated bool) on the host"""
        cnt = self.counts.cpu()
        na = int(min(int(cnt[:, 1].max()), self.cap_atoms))
        nb = int(min(int(cnt[:, 3].max()), self.cap_bonds))
        atoms, bonds, rho = self.atoms[:, :na].cpu(), self.bonds[:, :nb].cpu(), self.bond_rho[:, :nb].cpu()
        out = []
        for b in range(self.B):
            a, m = int(cnt[b, 1]), int(cnt[b, 3])
            trunc = a > self.cap_atoms or m > self.cap_bonds or int(cnt[b, 0]) > self.cap_atoms or int(cnt[b, 2]) > L.MAX_BOND_PEAKS
            a, m = min(a, self.cap_atoms), min(m, self.cap_bonds)
            out.append({"atoms": atoms[b, :a], "bonds": bonds[b, :m], "rho": rho[b, :m], "counts": cnt[b].tolist(), "truncated": trunc})
        return out


class GraphAssembler:
    """img2smiles2.py:193-311 on the device: the extractor's candidate lists -> the molecule of every image (csrc/assemble.hip:
    bond ends by float64 arg-mins in the reference's operation order, first bond of every atom pair, valence repair, atom
    compaction, implicit-hydrogen list).  Reads the list buffers in place; static outputs, one launch, graph-capture safe;
    `molecules()` is the only host sync (one small D2H per batch).

    An image without an atom peak or without a bond peak gives None (the reference's results.append(None), :126-129).  One input
    the reference does not define -- bond peaks exist but no candidate survives the bin rule; its np.flip raises on the empty
    array -- gives a molecule with zero atoms and zero bonds here, the same as "no bond survives the edge filter"."""

    def __init__(self, counts, atoms=None, bonds=None, bond_rho=None, cap_mol_bonds=None):
        """a contract.CandidateLists (PeakExtractor.candidates), or its four device tensors (hand-made lists).  cap_mol_bonds: bonds
        kept per image (default 4 * cap_atoms, at most cap_bonds); more are reported as `truncated`."""
        from .decode import omega_table
        lists = CandidateLists.checked("GraphAssembler", counts, atoms, bonds, bond_rho)
        counts, atoms, bonds, bond_rho = lists.tensors
        B, cap_atoms, cap_bonds = lists.B, lists.cap_atoms, lists.cap_bonds
        if cap_mol_bonds is None:
            cap_mol_bonds = min(4 * cap_atoms, cap_bonds)
        lib = L.load()
        self.lib = lib
        dev = atoms.device
        self.trig = torch.from_numpy(omega_table()).to(dev)
        d = L.AssembleDesc()
        d.counts, d.atoms, d.bonds, d.bond_rho, d.trig = counts.data_ptr(), atoms.data_ptr(), bonds.data_ptr(), bond_rho.data_ptr(), self.trig.data_ptr()
        d.B, d.cap_atoms, d.cap_bonds, d.cap_mol_bonds = B, cap_atoms, cap_bonds, cap_mol_bonds
        self.mol_counts = torch.zeros((B, 4), dtype=torch.int32, device=dev)
        self.mol_atoms = torch.zeros((B, cap_atoms, 5), dtype=torch.int32, device=dev)
        self.mol_bonds = torch.zeros((B, max(cap_mol_bonds, 1), 4), dtype=torch.int32, device=dev)
        self.mol_implh = torch.zeros((B, cap_atoms), dtype=torch.int32, device=dev)
        self.work = torch.zeros((max(lib.abc_assemble_work_ints(C.byref(d)), 1),), dtype=torch.int32, device=dev)
        d.mol_counts, d.mol_atoms, d.mol_bonds, d.mol_implh = (self.mol_counts.data_ptr(), self.mol_atoms.data_ptr(), self.mol_bonds.data_ptr(),
                                                               self.mol_implh.data_ptr())
        d.work = self.work.data_ptr()
        self.d, self.keep = d, (counts, atoms, bonds, bond_rho)
        self.B, self.cap_atoms, self.cap_bonds, self.cap_mol_bonds = B, cap_atoms, cap_bonds, cap_mol_bonds
        self.rows = MoleculeRows(self.mol_counts, self.mol_atoms, self.mol_bonds, self.mol_implh)

    @classmethod
    def from_extractor(cls, ex, cap_mol_bonds=None):
        return cls(ex.candidates, cap_mol_bonds=cap_mol_bonds)

    def run(self, stream=None):
        L.check(self.lib.abc_assemble_graphs(C.byref(self.d), stream_or_current(stream)), "assemble_graphs")

    def molecules(self):
        """per image: a decode.Molecule, or None for an image without an atom peak or without a bond peak (host sync)"""
        from .decode import Molecule
        cnt = self.mol_counts.cpu().numpy()
        na, nb, nh = (int(cnt[:, i].max()) for i in range(3))
        atoms, bonds, implh = self.mol_atoms[:, :na].cpu().numpy(), self.mol_bonds[:, :nb].cpu().numpy(), self.mol_implh[:, :nh].cpu().numpy()
        out = []
        for b in range(self.B):
            a, m, k, status = (int(v) for v in cnt[b])
            if status & L.MOL_EMPTY:
                out.append(None)
                continue
            out.append(Molecule.from_device_rows(atoms[b, :a], bonds[b, :m], implh[b, :k], truncated=bool(status & L.MOL_TRUNCATED)))
        return out


def _column_sums(stat, columns):
    """an int32 [B, len(columns)] device table as {column: its sum over the batch} and "rows", the table as lists (host sync)"""
    rows = stat.cpu().tolist()
    out = {name: sum(r[i] for r in rows) for i, name in enumerate(columns)}
    out["rows"] = rows
    return out


def _structured_rows(stat, columns):
    """an int32 [B, len(columns)] device table as a structured numpy array [B] with the int32 fields `columns` (host sync)"""
    rows = np.ascontiguousarray(stat.cpu().numpy())
    return rows.view(np.dtype([(c, np.int32) for c in columns])).reshape(len(rows))


class PackedText:
    """what the device text writers (MolBlockWriter, SmilesWriter) share: .text, the batch's texts back to back, and .index,
    offsets [B + 1] then status words [B], read back through the pinned .h_index"""

    def _index(self):
        """(offsets [B + 1], status [B]) of the last run as host lists: one D2H into the pinned buffer (host sync)"""
        self.h_index.copy_(self.index, non_blocking=True)
        torch.cuda.current_stream(self.index.device).synchronize()
        v = self.h_index.tolist()
        return v[:self.B + 1], v[self.B + 1:]

    def status(self):
        """the B status words of the last run: abc_mol_status | abc_text_status bits (host sync)"""
        return self._index()[1]

    def _texts(self):
        off, status = self._index()
        for b, s in enumerate(status):
            for bit, name in self.STATUS_NAMES:
                if s & bit:
                    raise L.AbcNetHipError("%s: image %d has status %s" % (type(self).__name__, b, name))
        raw = self.text[:off[self.B]].cpu().numpy().tobytes()
        return [None if s & L.MOL_EMPTY else raw[off[b]:off[b + 1]].decode("ascii") for b, s in enumerate(status)]

    def _bind_text(self, d, rows, cap_text, text_bytes, work_ints=None):
        """the half of a writer's constructor behind `rows.fill(d)`: cap_text (default B * text_bytes(d), the bound of one image)
        checked, the four buffers, the descriptor's text / index / work / cap_text.  work_ints(d): the int32 words of .work, default B"""
        B, dev = rows.B, rows.device
        self.image_bytes = int(text_bytes(C.byref(d)))
        cap_text = B * self.image_bytes if cap_text is None else int(cap_text)
        if not (1 <= cap_text <= 2 ** 31 - 1):
            raise ValueError("%s: cap_text must be 1..2^31-1 bytes, got %d (B = %d images of at most %d bytes)"
                             % (type(self).__name__, cap_text, B, self.image_bytes))
        self.B, self.cap_atoms, self.cap_mol_bonds, self.cap_text = B, rows.cap_atoms, rows.cap_mol_bonds, cap_text
        self.text = torch.zeros(cap_text, dtype=torch.uint8, device=dev)
        self.index = torch.zeros(2 * B + 1, dtype=torch.int32, device=dev)
        self.work = torch.zeros(B if work_ints is None else int(work_ints(C.byref(d))), dtype=torch.int32, device=dev)
        self.h_index = torch.zeros(2 * B + 1, dtype=torch.int32, pin_memory=True)
        d.text, d.index, d.work, d.cap_text = self.text.data_ptr(), self.index.data_ptr(), self.work.data_ptr(), cap_text
        self.d, self.keep = d, rows.tensors


class MolBlockWriter(PackedText):
    """the mol block text of the assembled molecules, written on the device (csrc/molblock.hip, abc_write_molblocks): the bytes of
    `Molecule.from_device_rows(...).molblock()` for every image of a GraphAssembler's rows, read in place, packed back to back
    into one static buffer.  Two launches, static buffers, graph-capture safe; `molblocks()` is the only host sync (two small D2H
    copies per batch, no per-atom host work).  `Molecule.molblock()` stays the host form and the oracle."""

    STATUS_NAMES = ((L.TEXT_BAD_ROW, "ABC_TEXT_BAD_ROW (a vocabulary index outside 0..13 or a position outside 0..199999)"),
                    (L.TEXT_OVERFLOW, "ABC_TEXT_OVERFLOW (the batch's text does not fit cap_text)"))

    def __init__(self, mol_counts, mol_atoms=None, mol_bonds=None, mol_implh=None, cap_text=None):
        """a contract.MoleculeRows (GraphAssembler.rows), or its four device tensors (hand-made rows).  cap_text: bytes of the text
        buffer; default B * abc_molblock_text_bytes, the bound of one image with every number at its widest -- 224 867 bytes per
        image at the runner's default capacities (512 atoms, 2048 bonds), 14.4 MB for a batch of 64; at most 2^31 - 1"""
        rows = MoleculeRows.checked("MolBlockWriter", mol_counts, mol_atoms, mol_bonds, mol_implh, need_implh=True)
        self.lib = L.load()
        d = L.MolBlockDesc()
        rows.fill(d)
        self._bind_text(d, rows, cap_text, self.lib.abc_molblock_text_bytes)

    @classmethod
    def from_assembler(cls, asm, cap_text=None):
        return cls(asm.rows, cap_text=cap_text)

    def run(self, stream=None):
        L.check(self.lib.abc_write_molblocks(C.byref(self.d), stream_or_current(stream)), "write_molblocks")

    def molblocks(self):
        """per image: the mol block as a str (the argument of Chem.MolFromMolBlock), or None for an image without an atom peak
        or without a bond peak.  Raises AbcNetHipError when an image was refused (BAD_ROW) or did not fit (OVERFLOW).  Host sync:
        the index, then the text that was written."""
        return self._texts()


class SmilesWriter(PackedText):
    """a SMILES string for every assembled molecule, written on the device (csrc/smiles.hip, abc_write_smiles): the bytes of
    `Molecule.from_device_rows(...).smiles()` for every image of a GraphAssembler's rows, read in place, packed back to back into
    one static buffer.  Two launches, static buffers, graph-capture safe; `smiles()` is the only host sync (two small D2H copies
    per batch).  The text is deterministic and its graph is the rows' graph; it is NOT RDKit's canonical SMILES (DESIGN.md
    section 7: the rule, and what it leaves out).  stereo=True (abc_write_smiles_stereo): the bytes of `.smiles(stereo=True)`, the
    tetrahedral centres of the wedge rows written as `@` / `@@`; stereo_stats() and parities() say what became of every candidate.
    double_bonds=True (abc_write_smiles_ez, with or without stereo): the bytes of `.smiles(double_bonds=True)`, the single bonds at
    every double bond the positions decide written as `/` or `\\`; double_bond_stats() and double_bond_codes() say what became of
    every class-2 row."""

    STATUS_NAMES = ((L.TEXT_BAD_ROW, "ABC_TEXT_BAD_ROW (a vocabulary index outside 0..13, a charge outside -15..15, a bond order "
                                     "outside 1..6, a bond end outside 1..n or on one atom twice, or an atom pair listed twice)"),
                    (L.TEXT_RING_LIMIT, "ABC_TEXT_RING_LIMIT (more than 99 ring bonds are open at once)"),
                    (L.TEXT_OVERFLOW, "ABC_TEXT_OVERFLOW (the batch's text does not fit cap_text)"))
    # (double_bonds, stereo) -> the descriptor and the stem of abc_write_<stem>, abc_<stem>_text_bytes, abc_<stem>_work_ints (the ez entry
    # writes the tetrahedral marks too, under its descriptor's `tetrahedral`)
    VARIANTS = {(False, False): (L.SmilesDesc, "smiles"), (False, True): (L.SmilesStereoDesc, "smiles_stereo"),
                (True, False): (L.SmilesEzDesc, "smiles_ez"), (True, True): (L.SmilesEzDesc, "smiles_ez")}

    def __init__(self, mol_counts, mol_atoms=None, mol_bonds=None, mol_implh=None, cap_text=None, stereo=False, double_bonds=False):
        """a contract.MoleculeRows (GraphAssembler.rows), or its four device tensors (hand-made rows); cap_atoms at most
        L.MAX_SMILES_ATOMS, cap_mol_bonds at most L.MAX_SMILES_BONDS.  cap_text: bytes of the text buffer; default
        B * abc_smiles_text_bytes, the bound of one image with every token at its widest -- 20 480 bytes per image at the
        runner's default capacities (512 atoms, 2048 bonds), 21 504 with stereo (abc_smiles_stereo_text_bytes); at most 2^31 - 1"""
        rows = MoleculeRows.checked("SmilesWriter", mol_counts, mol_atoms, mol_bonds, mol_implh, max_cap_atoms=L.MAX_SMILES_ATOMS,
                                    max_cap_mol_bonds=L.MAX_SMILES_BONDS, need_implh=True)
        B, cap_atoms, cap_mol_bonds, dev = rows.B, rows.cap_atoms, rows.cap_mol_bonds, rows.device
        self.lib = L.load()
        self.stereo, self.double_bonds = bool(stereo), bool(double_bonds)
        desc, entry = self.VARIANTS[self.double_bonds, self.stereo]
        d = desc()
        self._write, self._what = getattr(self.lib, "abc_write_" + entry), "write_" + entry
        rows.fill(d)
        if self.double_bonds:
            d.tetrahedral = int(self.stereo)
        self._bind_text(d, rows, cap_text, getattr(self.lib, "abc_%s_text_bytes" % entry), getattr(self.lib, "abc_%s_work_ints" % entry))
        self.stats = self.codes = None
        if self.stereo:
            self.stats = torch.zeros((B, len(L.SMILES_STEREO_COLUMNS)), dtype=torch.int32, device=dev)
            self.codes = torch.zeros((B, cap_atoms), dtype=torch.int32, device=dev)
            d.stereo_stats, d.stereo_out = self.stats.data_ptr(), self.codes.data_ptr()
        self.ez_stats = self.ez_codes = None
        if self.double_bonds:
            self.ez_stats = torch.zeros((B, len(L.SMILES_EZ_COLUMNS)), dtype=torch.int32, device=dev)
            self.ez_codes = torch.zeros((B, cap_mol_bonds), dtype=torch.int32, device=dev)
            d.ez_stats, d.ez_out = self.ez_stats.data_ptr(), self.ez_codes.data_ptr()

    @classmethod
    def from_assembler(cls, asm, cap_text=None, stereo=False, double_bonds=False):
        return cls(asm.rows, cap_text=cap_text, stereo=stereo, double_bonds=double_bonds)

    def run(self, stream=None):
        L.check(self._write(C.byref(self.d), stream_or_current(stream)), self._what)

    def _need_stereo(self, what):
        if not self.stereo:
            raise L.AbcNetHipError("SmilesWriter.%s: the writer was built without stereo=True" % what)

    def stereo_stats(self):
        """stereo=True: what became of the wedge rows of the last run -- {"marked", "flat", "unqualified", "wedge_rows"} summed
        over the batch, and "rows", the four counts of every image (zeros for an image without text).  Host sync."""
        self._need_stereo("stereo_stats")
        return _column_sums(self.stats, L.SMILES_STEREO_COLUMNS)

    def parities(self):
        """stereo=True: int32 [B, cap_atoms] on the host, the code of every atom row of the last run: 0 no candidate, +1 / -1 the
        local parity s(a) of a marked centre, L.STEREO_FLAT, L.STEREO_UNQUALIFIED; 0 past an image's atoms.  Host sync."""
        self._need_stereo("parities")
        return self.codes.cpu()

    def _need_double_bonds(self, what):
        if not self.double_bonds:
            raise L.AbcNetHipError("SmilesWriter.%s: the writer was built without double_bonds=True" % what)

    def double_bond_stats(self):
        """double_bonds=True: what became of the candidate double bonds of the last run -- {"marked", "flat", "ring", "twin"}
        summed over the batch, and "rows", the four counts of every image (zeros for an image without text).  Host sync."""
        self._need_double_bonds("double_bond_stats")
        return _column_sums(self.ez_stats, L.SMILES_EZ_COLUMNS)

    def double_bond_codes(self):
        """double_bonds=True: int32 [B, cap_mol_bonds] on the host, the code of every bond row of the last run: 0 not a candidate,
        +1 / -1 a marked double bond (together / opposite), L.EZ_FLAT, L.EZ_RING, L.EZ_TWIN; 0 past an image's bonds.  Host sync."""
        self._need_double_bonds("double_bond_codes")
        return self.ez_codes.cpu()

    def smiles(self):
        """per image: the SMILES as a str, or None for an image without an atom peak or without a bond peak.  Raises
        AbcNetHipError when an image was refused (BAD_ROW, RING_LIMIT) or did not fit (OVERFLOW).  Host sync: the index, then the
        text that was written."""
        return self._texts()


class SmilesReader:
    """graph records read from a batch of SMILES strings on the device (csrc/smiles_read.hip, abc_read_smiles): what
    `decode.parse_smiles` gives for every string, written into the device twins of an existing contract.GraphRecords, so that every
    reader of those records -- the three scores, AromaticityPerceiver.from_records, GraphCanonicalizer.from_records -- needs nothing
    new.  The reading rule is this project's ("Reading a SMILES"): a stated subset of OpenSMILES; a string it
    refuses leaves an empty record, which the scores count as a miss.  One launch per load; `status()` and `stats()` are the host
    syncs."""

    def __init__(self, records, cap_text=None):
        """records: the contract.GraphRecords to fill (not a derived one); cap_text: bytes of the batch's text, default
        B * L.MAX_SMILES_READ_BYTES (every string at the limit)"""
        if not isinstance(records, GraphRecords) or isinstance(records, DerivedGraphRecords):
            raise ValueError("SmilesReader: records must be a contract.GraphRecords that is loaded from the host, got %s" % type(records).__name__)
        B = records.B
        cap_text = B * L.MAX_SMILES_READ_BYTES if cap_text is None else int(cap_text)
        if not (1 <= cap_text <= 2 ** 31 - 1):
            raise ValueError("SmilesReader: cap_text must be 1..2^31-1 bytes, got %d" % cap_text)
        self.lib = L.load()
        self.records, self.B, self.cap_text = records, B, cap_text
        dev = records.staging.device
        with torch.cuda.device(dev):
            self.staging = PinnedStaging(dev, {"text": ((cap_text,), torch.uint8), "offsets": ((B + 1,), torch.int32)})
            self.status_words = torch.zeros(B, dtype=torch.int32, device=dev)
            self.stat = torch.zeros((B, len(L.READ_STATS_COLUMNS)), dtype=torch.int32, device=dev)
        d = L.SmilesReadDesc()
        d.text, d.offsets = (t.data_ptr() for t in self.staging.dev.values())
        d.rec_atoms, d.rec_bonds, d.rec_counts = (t.data_ptr() for t in records.staging.dev.values())
        d.B, d.max_atoms, d.max_bonds, d.cap_text = B, records.max_atoms, records.max_bonds, cap_text
        d.status, d.stats = self.status_words.data_ptr(), self.stat.data_ptr()
        self.d = d

    def load(self, strings):
        """n <= B str, one SMILES each (stripping a CSV field is the caller's job: every byte counts); the rows past n are empty
        strings.  Asynchronous H2D of the bytes and offsets, then the launch, on the current stream; the records count as loaded."""
        strings = list(strings)
        if len(strings) > self.B:
            raise ValueError("SmilesReader.load: expected at most %d strings, got %d" % (self.B, len(strings)))
        for k, s in enumerate(strings):
            if not isinstance(s, str):
                raise ValueError("SmilesReader.load: string %d is a %s, not a str" % (k, type(s).__name__))
        raw = [s.encode("ascii", "replace") for s in strings]      # (decode.smiles_bytes: `?`, a syntax error, for a character outside ASCII)
        ends = np.cumsum([len(r) for r in raw], dtype=np.int64) if raw else np.zeros(0, dtype=np.int64)
        total = int(ends[-1]) if len(ends) else 0
        if total > self.cap_text:
            raise ValueError("SmilesReader.load: %d bytes of text, cap_text is %d" % (total, self.cap_text))
        h_text, h_off = self.staging.host.values()
        self.staging.wait()
        if total:
            h_text[:total] = torch.from_numpy(np.frombuffer(b"".join(raw), dtype=np.uint8).copy())
        h_off[0] = 0
        h_off[1:len(raw) + 1] = torch.from_numpy(ends.astype(np.int32))
        h_off[len(raw) + 1:] = total
        with torch.cuda.device(self.staging.device):
            self.staging.commit()
            L.check(self.lib.abc_read_smiles(C.byref(self.d), current_stream()), "read_smiles")
        self.records.loaded = True

    def status(self):
        """the B status words of the last load: one L.READ_* value per string (host sync)"""
        return self.status_words.cpu().tolist()

    def stats(self):
        """{"bytes", "atoms", "bonds", "ring_bonds"} of the last load summed over the batch, and "rows", the four per string (host sync)"""
        return _column_sums(self.stat, L.READ_STATS_COLUMNS)


def stroke_max_iter(thin, what="StrokeNormalizer"):
    """abc_stroke_desc.max_iter of a `thin` argument: None or 0 -> 0 (no thinning), an int >= 1 -> that bound, "stable" -> until
    stable"""
    if thin is None:
        return 0
    if isinstance(thin, str):
        if thin != "stable":
            raise ValueError("%s: thin must be None, 0, an int >= 1 or 'stable', got %r" % (what, thin))
        return L.STROKE_UNTIL_STABLE
    if isinstance(thin, bool) or not isinstance(thin, int) or thin < 0:
        raise ValueError("%s: thin must be None, 0, an int >= 1 or 'stable', got %r" % (what, thin))
    return thin


class StrokeNormalizer:
    """stroke width of a {0, 1} batch normalised on the device (csrc/stroke.hip; the contract: include/abcnet_hip.h,
    abc_stroke_desc): per image, delete the ink pixels without a neighbour (`drop_isolated`), peel the drawing toward its skeleton
    by the Guo-Hall two-subiteration rule (`thin`: None or 0 for none, an int >= 1 for at most that many iterations, "stable" for
    until nothing changes), then grow it back by a disk of `radius` 0 .. 3.  `images` is any f32 [B, 1, S, S] device tensor, S a
    multiple of 8 up to L.STROKE_MAX_SIZE; the result goes to `out`, or over `images` when `out` is None.  `skip`: an int32 device
    vector of B words (any stride: a column of a table does); an image whose word is non-zero is carried over bit for bit and
    reported as skipped.  One launch, static buffers, graph-capture safe; stats() is the only host sync.  No CPU fallback."""

    def __init__(self, images, out=None, thin=None, radius=0, drop_isolated=False, skip=None):
        max_iter = stroke_max_iter(thin)
        if isinstance(radius, bool) or not isinstance(radius, int) or not 0 <= radius <= 3:
            raise ValueError("StrokeNormalizer: radius must be an int in 0 .. 3, got %r" % (radius,))
        if not torch.cuda.is_available():
            raise L.AbcNetHipError("StrokeNormalizer needs an MI355X; abcnet_amd has no CPU fallback")
        require_device_tensor(images, torch.float32, "StrokeNormalizer: images")
        if images.dim() != 4 or images.shape[1] != 1 or images.shape[2] != images.shape[3] or images.shape[0] < 1:
            raise L.AbcNetHipError("StrokeNormalizer: images %s is not [B, 1, S, S]" % (tuple(images.shape),))
        B, S = int(images.shape[0]), int(images.shape[2])
        if S < 8 or S % 8 or S > L.STROKE_MAX_SIZE:
            raise ValueError("StrokeNormalizer: the size must be a multiple of 8 (8 .. %d), got %d" % (L.STROKE_MAX_SIZE, S))
        if out is None:
            out = images
        else:
            require_device_tensor(out, torch.float32, "StrokeNormalizer: out")
            if tuple(out.shape) != tuple(images.shape) or out.device != images.device:
                raise L.AbcNetHipError("StrokeNormalizer: out %s does not match images %s" % (tuple(out.shape), tuple(images.shape)))
        if skip is not None:
            if not (isinstance(skip, torch.Tensor) and skip.is_cuda and skip.dtype == torch.int32 and skip.device == images.device):
                raise L.AbcNetHipError("StrokeNormalizer: skip must be an int32 device tensor (no CPU fallback)")
            if skip.dim() != 1 or skip.shape[0] != B or (B > 1 and skip.stride(0) < 1):
                raise L.AbcNetHipError("StrokeNormalizer: skip %s is not a vector of %d words" % (tuple(skip.shape), B))
        self.lib = L.load()
        self.images, self.out, self.skip, self.B, self.S = images, out, skip, B, S
        self.thin, self.radius, self.drop_isolated = thin, radius, bool(drop_isolated)
        self.stat = torch.zeros((B, len(L.STROKE_STAT_COLUMNS)), dtype=torch.int32, device=images.device)
        d = L.StrokeDesc()
        d.src, d.dst, d.stats = images.data_ptr(), out.data_ptr(), self.stat.data_ptr()
        d.B, d.S, d.drop_isolated, d.max_iter, d.radius = B, S, int(self.drop_isolated), max_iter, radius
        if skip is not None:
            d.skip, d.skip_stride = skip.data_ptr(), max(1, int(skip.stride(0)))
        self.d = d

    def run(self, stream=None):
        """one launch (graph-capturable): the normalised batch into self.out, the stats rows beside it"""
        L.check(self.lib.abc_normalize_strokes(C.byref(self.d), stream_or_current(stream, self.out.device)), "normalize_strokes")
        return self.out

    def stats(self):
        """the stats rows of the last run() as a structured numpy array [B] with the int32 fields L.STROKE_STAT_COLUMNS
        (iterations, converged, ink_in, ink_out, skipped).  The only call here that synchronises."""
        return _structured_rows(self.stat, L.STROKE_STAT_COLUMNS)


class _RecordScorer:
    """What GraphScore and GraphSimilarity share: molecule rows against graph records, one launch per call; the COLUMNS of every image
    of the last call in .rows (int32), their running sums in .totals.  MAX_RECORD: the largest max_atoms and max_bonds (None: any)."""

    def _bind(self, d, mol, n_valid, records, max_atoms, max_bonds):
        """check what both take and fill the descriptor fields both have (records: made here when None, else theirs the capacities)"""
        who = type(self).__name__
        if records is not None:
            if not isinstance(records, GraphRecords):
                raise ValueError("%s: records must be a GraphRecords, got %s" % (who, type(records).__name__))
            max_atoms, max_bonds = records.max_atoms, records.max_bonds
        for name, n, top in zip(("max_atoms", "max_bonds"), (int(max_atoms), int(max_bonds)), self.MAX_RECORD):
            if n < 1 or (top is not None and n > top):
                raise ValueError("%s: %s must be %s, got %d" % (who, name, ">= 1" if top is None else "1..%d" % top, n))
        rows = MoleculeRows.checked(who, *mol, max_cap_atoms=self.MAX_CAP_ATOMS, n_valid=n_valid)
        if records is not None and records.B != rows.B:
            raise ValueError("%s: records stages %d images, the molecules are %d" % (who, records.B, rows.B))
        self.lib = L.load()
        self._own_records = records is None
        self.records = GraphRecords(rows.B, max_atoms, max_bonds, rows.device) if records is None else records
        self.B, self.cap_atoms, self.cap_mol_bonds = rows.B, rows.cap_atoms, rows.cap_mol_bonds
        self.max_atoms, self.max_bonds = self.records.max_atoms, self.records.max_bonds
        self.rows = torch.zeros((rows.B, len(self.COLUMNS)), dtype=torch.int32, device=rows.device)
        # (uint64 on the device; int64 here: the sums stay far below 2^63)
        self.totals = torch.zeros(len(self.COLUMNS), dtype=torch.int64, device=rows.device)
        rows.fill(d)
        self.records.fill(d)
        d.n_valid = L.ptr(n_valid)
        d.rows, d.totals = self.rows.data_ptr(), self.totals.data_ptr()
        self.d, self.keep = d, rows.tensors[:3] + (n_valid,)

    @classmethod
    def from_assembler(cls, asm, **kw):
        return cls(asm.rows, **kw)

    def run(self, stream=None):
        L.check(getattr(self.lib, "abc_" + self.UPDATE)(C.byref(self.d), stream_or_current(stream)), self.UPDATE)

    @property
    def loaded(self):
        return self.records.loaded

    def load(self, graphs):
        """GraphRecords.load, for the op that made its records; records handed in are loaded once, by their owner"""
        if not self._own_records:
            raise ValueError("%s(records=...) reads records it did not make, a scorer's or a runner's: load them there "
                             "(GraphRecords.load, InferenceRunner.load_graphs)" % type(self).__name__)
        self.records.load(graphs)

    def reset(self):
        self.totals.zero_()

    def _totals(self):
        """the running totals under their column names (int) and "rows", the table of the last call (device sync)"""
        out = {k: int(v) for k, v in zip(self.COLUMNS, self.totals.cpu().tolist())}
        out["rows"] = self.rows.cpu().numpy()
        return out


class GraphScore(_RecordScorer):
    """how many assembled molecules ARE the annotated molecule (csrc/graph_score.hip, abc_graph_score_update): the molecules of a
    GraphAssembler, read in place, against the graph records of raster.parse_graph -- bonded atoms located by mutual nearest cell
    within `radius`, matched by symbol and charge; bonds paired by their located ends, matched by order.  One launch, static
    buffers, graph-capture safe; the 14 columns (L.GRAPH_SCORE_COLUMNS) of every image of the last call in .rows, their running
    sums in .totals; `result()` is the only host sync."""

    UPDATE, COLUMNS = "graph_score_update", L.GRAPH_SCORE_COLUMNS
    MAX_CAP_ATOMS, MAX_RECORD = L.MAX_CAP_ATOMS, (L.MAX_SCORE_RECORD, L.MAX_SCORE_RECORD)

    def __init__(self, mol_counts, mol_atoms=None, mol_bonds=None, max_atoms=256, max_bonds=256, radius=0, n_valid=None, records=None):
        """a contract.MoleculeRows (GraphAssembler.rows), or its mol_counts, mol_atoms and mol_bonds device tensors (hand-made rows);
        max_atoms / max_bonds: the capacity of a record; radius >= 0 in cells; n_valid: a one-element int32 device tensor, only the
        first n_valid images count; records: a contract.GraphRecords over the same batch, read in place -- default: made here"""
        self.radius = int(radius)
        if not (0 <= self.radius <= 32768):
            raise ValueError("GraphScore: radius must be 0..32768 cells, got %d" % self.radius)
        d = L.GraphScoreDesc()
        d.radius = self.radius
        self._bind(d, (mol_counts, mol_atoms, mol_bonds), n_valid, records, max_atoms, max_bonds)

    def result(self):
        """dict (device sync): the 14 running totals under their names (int), "share_exact" = exact / counted, "share_atoms" =
        atoms_matched / atoms_true, "share_bonds" = bonds_matched / bonds_true (nan for an empty denominator), and "rows": the
        int32 [B, 14] table of the last call"""
        out = self._totals()
        for share, num, den in (("share_exact", "exact", "counted"), ("share_atoms", "atoms_matched", "atoms_true"),
                                ("share_bonds", "bonds_matched", "bonds_true")):
            out[share] = out[num] / out[den] if out[den] else float("nan")
        return out


class GraphSimilarity(_RecordScorer):
    """how NEAR the assembled molecules are to the annotated ones, free of positions (csrc/graph_sim.hip,
    abc_graph_similarity_update): the multiset of the radius-0..3 atom environments of a GraphAssembler's molecule, read in place,
    against that of the raster.parse_graph record -- the stand-in for the Dice similarity of Morgan fingerprints of cal_acc.py:38-43
    (the exact definition: include/abcnet_hip.h; what of RDKit's it leaves out: DESIGN.md section 7).  One launch, static buffers,
    graph-capture safe; the 12 columns (L.GRAPH_SIM_COLUMNS) of every image of the last call in .rows, their running sums in
    .totals; `result()` is the only host sync.  `refine_equal` is an UPPER bound of "the same molecule" (colour refinement),
    GraphScore's `exact` the positional lower one."""

    UPDATE, COLUMNS = "graph_similarity_update", L.GRAPH_SIM_COLUMNS
    MAX_CAP_ATOMS, MAX_RECORD = L.MAX_SIM_ATOMS, (L.MAX_SIM_ATOMS, None)

    def __init__(self, mol_counts, mol_atoms=None, mol_bonds=None, max_atoms=256, max_bonds=256, n_valid=None, records=None, debug_ids=False):
        """the rows, n_valid, max_atoms / max_bonds: as GraphScore.  records: a contract.GraphRecords over the same batch, or a
        GraphScore, whose records are taken -- read in place (no second staging: `load` is refused here, max_atoms / max_bonds
        are theirs).  debug_ids: keep the fingerprint ids of every image in .ids (int64 [B, 2, 2048] holding the uint64 bit
        patterns: molecule, then record; layer-major, atom-minor)"""
        d = L.GraphSimilarityDesc()
        records = records.records if isinstance(records, GraphScore) else records
        self._bind(d, (mol_counts, mol_atoms, mol_bonds), n_valid, records, max_atoms, max_bonds)
        self.ids = torch.zeros((self.B, 2, L.GRAPH_SIM_IDS), dtype=torch.int64, device=self.rows.device) if debug_ids else None
        d.ids_out = L.ptr(self.ids)

    def result(self):
        """dict (device sync): the 12 running totals under their names (int), "similarity" = dice_q20 / 2^20 / counted, the mean
        Dice similarity over every counted image, an image without a molecule counting 0 as a failed row does in cal_acc.py:45-47
        (nan when nothing was counted), and "rows": the int32 [B, 12] table of the last call"""
        out = self._totals()
        out["similarity"] = out["dice_q20"] / float(1 << 20) / out["counted"] if out["counted"] else float("nan")
        return out


class GraphIdentity(_RecordScorer):
    """whether the assembled molecules ARE the annotated ones, free of positions and with certainty (csrc/graph_ident.hip,
    abc_graph_identity_update): an individualise-and-refine isomorphism test of a GraphAssembler's molecule, read in place, against
    the raster.parse_graph record, on the graphs GraphSimilarity defines (the algorithm: include/abcnet_hip.h; what of RDKit's
    canonical SMILES it leaves out: DESIGN.md section 7).  `same` is a bijection VERIFIED atom by atom and bond by bond, `different`
    an exhausted search or unequal sizes, `undecided` a budget that ran out -- reported, never hidden.  GraphScore's `exact` <=
    `same` <= GraphSimilarity's `refine_equal`.  One launch, static buffers, graph-capture safe; the 11 columns
    (L.GRAPH_IDENT_COLUMNS) of every image of the last call in .rows, their running sums in .totals; `result()` is the only host
    sync."""

    UPDATE, COLUMNS = "graph_identity_update", L.GRAPH_IDENT_COLUMNS
    MAX_CAP_ATOMS, MAX_RECORD = L.MAX_SIM_ATOMS, (L.MAX_SIM_ATOMS, None)

    def __init__(self, mol_counts, mol_atoms=None, mol_bonds=None, max_atoms=256, max_bonds=256, n_valid=None, records=None,
                 max_tries=None, max_rounds=None, witness=False):
        """the rows, n_valid, max_atoms / max_bonds and records: as GraphSimilarity (records may also be a GraphScore or a
        GraphSimilarity, whose records are taken).  max_tries: record-side individualisations per image, max_rounds: refinement rounds
        per image, both sides -- None: L.IDENT_DEFAULT_TRIES / L.IDENT_DEFAULT_ROUNDS.  witness: keep the bijection of every `same`
        image in .map (int32 [B, cap_atoms]: the ORIGINAL record atom index of every molecule atom, -1 everywhere else)"""
        d = L.GraphIdentityDesc()
        d.max_tries, d.max_rounds = self.max_tries, self.max_rounds = _budgets(
            "GraphIdentity", max_tries, max_rounds, (L.IDENT_DEFAULT_TRIES, L.IDENT_DEFAULT_ROUNDS))
        records = records.records if isinstance(records, _RecordScorer) else records
        self._bind(d, (mol_counts, mol_atoms, mol_bonds), n_valid, records, max_atoms, max_bonds)
        self.map = torch.full((self.B, self.cap_atoms), -1, dtype=torch.int32, device=self.rows.device) if witness else None
        d.map_out = L.ptr(self.map)

    def result(self):
        """dict (device sync): the 11 running totals under their names (int), "share_same" = same / counted, "share_undecided" =
        undecided / counted (nan when nothing was counted), and "rows": the int32 [B, 11] table of the last call"""
        out = self._totals()
        for share, num in (("share_same", "same"), ("share_undecided", "undecided")):
            out[share] = out[num] / out["counted"] if out["counted"] else float("nan")
        return out


def _budgets(who, max_tries, max_rounds, defaults):
    """[max_tries, max_rounds] of a search op, None replaced by its default, each 1..2^31-1 (ValueError)"""
    budgets = []
    for name, v, default in zip(("max_tries", "max_rounds"), (max_tries, max_rounds), defaults):
        v = default if v is None else int(v)
        if not (1 <= v < 1 << 31):
            raise ValueError("%s: %s must be 1..2^31-1, got %d" % (who, name, v))
        budgets.append(v)
    return budgets


class _OneSideOp:
    """What GraphCanonicalizer and AromaticityPerceiver share: ONE side, the molecule rows or the graph records, bound to a descriptor with
    the mol_* / rec_* fields of abc_canon_desc; .B, .cap, .cap_bonds of that side; .out, the op's own MoleculeRows when it writes rows."""

    def _bind(self, d, mol, records, want_rows, max_cap_mol_bonds=None):
        """check the side that was given and fill its descriptor fields (out_counts .. out_implh too, with want_rows on the molecule
        side).  mol: (mol_counts, mol_atoms, mol_bonds, mol_implh); records: a GraphRecords, or a scorer, whose records are taken.
        Returns (the records or None, the device)."""
        who = type(self).__name__
        if (mol[0] is None) == (records is None):
            raise ValueError("%s: give the molecule rows or records=GraphRecords, one side" % who)
        self.out = None
        if records is not None:
            records = records.records if isinstance(records, _RecordScorer) else records
            if not isinstance(records, GraphRecords):
                raise ValueError("%s: records must be a GraphRecords, got %s" % (who, type(records).__name__))
            if not 1 <= records.max_atoms <= L.MAX_SIM_ATOMS or records.max_bonds < 1:
                raise ValueError("%s: max_atoms must be 1..%d and max_bonds >= 1, got %d, %d"
                                 % (who, L.MAX_SIM_ATOMS, records.max_atoms, records.max_bonds))
            records.fill(d)
            d.B = records.B
            self.keep = ()
            self.B, self.cap, self.cap_bonds, dev = records.B, records.max_atoms, records.max_bonds, records.staging.device
        else:
            given = mol[0].tensors[3] if isinstance(mol[0], MoleculeRows) else mol[3]
            mr = MoleculeRows.checked(who, *mol, max_cap_atoms=L.MAX_SIM_ATOMS, need_implh=given is not None, max_cap_mol_bonds=max_cap_mol_bonds)
            mr.fill(d)
            self.keep = mr.tensors
            self.B, self.cap, self.cap_bonds, dev = mr.B, mr.cap_atoms, mr.cap_mol_bonds, mr.device
            if want_rows:
                out = tuple(torch.zeros(s, dtype=torch.int32, device=dev) for s in MoleculeRows.SHAPES(mr.B, mr.cap_atoms, mr.cap_mol_bonds))
                self.out = MoleculeRows(*out)
                d.out_counts, d.out_atoms, d.out_bonds, d.out_implh = (t.data_ptr() for t in out)
        self.lib = L.load()
        return records, dev

    @classmethod
    def from_assembler(cls, asm, **kw):
        return cls(asm.rows, **kw)

    @classmethod
    def from_records(cls, records, **kw):
        return cls(records=records, **kw)


class StereoPerceiver:
    """the stereo elements of every assembled molecule, perceived on the device (csrc/stereo.hip, abc_perceive_stereo; the contract:
    include/abcnet_hip.h): what SmilesWriter(stereo=True, double_bonds=True) decides about every centre and
    every double bond of the same rows, as the element table GraphCanonicalizer(stereo=True) reads.  The molecule side only.  One
    launch, static buffers, graph-capture safe; elements() and stats() are the host syncs.  No CPU fallback (the host form is
    decode.stereo_elements)."""

    def __init__(self, mol_counts, mol_atoms=None, mol_bonds=None, mol_implh=None):
        """a contract.MoleculeRows (GraphAssembler.rows), or its four device tensors (hand-made rows); cap_atoms at most
        L.MAX_SMILES_ATOMS, cap_mol_bonds at most L.MAX_SMILES_BONDS"""
        rows = MoleculeRows.checked("StereoPerceiver", mol_counts, mol_atoms, mol_bonds, mol_implh, max_cap_atoms=L.MAX_SMILES_ATOMS,
                                    max_cap_mol_bonds=L.MAX_SMILES_BONDS, need_implh=True)
        self.lib = L.load()
        self.keep = rows.tensors
        self.B, self.cap = rows.B, rows.cap_atoms
        self.table = torch.zeros((rows.B, rows.cap_atoms, L.STEREO_W), dtype=torch.int32, device=rows.device)
        self.stat = torch.zeros((rows.B, len(L.STEREO_STATS_COLUMNS)), dtype=torch.int32, device=rows.device)
        d = L.StereoDesc()
        rows.fill(d)
        d.elements, d.stats = self.table.data_ptr(), self.stat.data_ptr()
        self.d = d

    @classmethod
    def from_assembler(cls, asm):
        return cls(asm.rows)

    def run(self, stream=None):
        """one launch (graph-capturable): every word of the table and of the stats"""
        L.check(self.lib.abc_perceive_stereo(C.byref(self.d), stream_or_current(stream)), "perceive_stereo")

    def elements(self):
        """int32 [B, cap_atoms, L.STEREO_W] on the host: the element table of the last run (contract.STEREO_ELEMENT names the
        words; decode.STEREO_NONE_ROW past an image's atoms and for an image that is EMPTY or refused).  Host sync."""
        return self.table.cpu()

    def stats(self):
        """the stats rows of the last run as a structured numpy array [B] with the int32 fields L.STEREO_STATS_COLUMNS (marked
        centres, marked double bonds, flat of both kinds, status: L.MOL_EMPTY | L.MOL_TRUNCATED | L.TEXT_BAD_ROW).  Host sync."""
        return _structured_rows(self.stat, L.STEREO_STATS_COLUMNS)


class GraphCanonicalizer(_OneSideOp):
    """a canonical atom order for every image (csrc/graph_canon.hip, abc_canonical_order; the algorithm: include/abcnet_hip.h,
    DESIGN.md section 7): the least leaf of an individualise-and-refine search over every branch of the graph GraphIdentity defines,
    plus a tag on the atoms mol_implh lists.  The molecule side -- a GraphAssembler's rows, read in place -- also gets the CANONICAL
    ROWS, the same molecule renumbered, which SmilesWriter and MolBlockWriter take like the assembler's: their text is then equal
    if and only if the graphs are equal (this project's text rule on a canonical order, NOT RDKit's canonical SMILES).  The records
    side orders the atoms of contract.GraphRecords.  Certain whenever the status says so: UNDECIDED (a budget ran out) and COLLISION
    are reported per image, never hidden.  One launch, static buffers, graph-capture safe; orders(), stats(), keys() and
    certificates() are the host syncs.  No CPU fallback (the host form is decode.Molecule.canonical()).
    stereo=True (abc_canonical_order_stereo, the molecule side only): the canonical ISOMERIC order -- the op owns a StereoPerceiver
    of the same rows and its run() is two launches, perceive then order; the search reads the stereo elements as a third key, so
    SmilesWriter(rows(), stereo=True, double_bonds=True) writes equal strings if and only if the STEREO graphs are equal (the host
    form is decode.Molecule.smiles(isomeric=True)).  stereo_search() and stereo_elements() are its read-backs."""

    def __init__(self, mol_counts=None, mol_atoms=None, mol_bonds=None, mol_implh=None, records=None, max_tries=None, max_rounds=None,
                 cert=False, rows=True, stereo=False):
        """a contract.MoleculeRows (GraphAssembler.rows) or its device tensors (mol_implh optional: no tags without it), OR
        records=contract.GraphRecords.  max_tries: individualisations per image, max_rounds: refinement rounds per image, replays
        included -- None: L.CANON_DEFAULT_TRIES / L.CANON_DEFAULT_ROUNDS.  cert: keep the relabelled graph of every image in .cert
        (int32 [B, 2 + cap + 3 cap_bonds]).  rows (molecule side): write the canonical rows (cap_mol_bonds <= 4096)."""
        self.stereo = bool(stereo)
        if self.stereo and records is not None:
            raise ValueError("GraphCanonicalizer: stereo=True is the molecule side's (graph records carry no implicit-H list, so the "
                             "stereo rules are not defined on them)")
        d = L.CanonStereoDesc() if self.stereo else L.CanonDesc()
        d.max_tries, d.max_rounds = self.max_tries, self.max_rounds = _budgets(
            "GraphCanonicalizer", max_tries, max_rounds, (L.CANON_DEFAULT_TRIES, L.CANON_DEFAULT_ROUNDS))
        self.records, dev = self._bind(d, (mol_counts, mol_atoms, mol_bonds, mol_implh), records, bool(rows),
                                       L.MAX_SMILES_BONDS if rows else None)
        self.order = torch.full((self.B, self.cap), -1, dtype=torch.int32, device=dev)
        self.stat = torch.zeros((self.B, len(L.CANON_COLUMNS)), dtype=torch.int32, device=dev)
        self.key = torch.zeros((self.B, 2), dtype=torch.int64, device=dev)
        self.cert = torch.full((self.B, 2 + self.cap + 3 * self.cap_bonds), -1, dtype=torch.int32, device=dev) if cert else None
        d.order, d.stats, d.key, d.cert_out = self.order.data_ptr(), self.stat.data_ptr(), self.key.data_ptr(), L.ptr(self.cert)
        self.perceiver = self.search = None
        if self.stereo:
            self.perceiver = StereoPerceiver(mol_counts, mol_atoms, mol_bonds, mol_implh)
            self.search = torch.zeros((self.B, len(L.STEREO_SEARCH_COLUMNS)), dtype=torch.int32, device=dev)
            d.elements, d.stereo_search = self.perceiver.table.data_ptr(), self.search.data_ptr()
        self.d = d

    def run(self, stream=None):
        """one launch (graph-capturable): order, stats, key, and cert / the canonical rows when they were asked for; stereo=True:
        two launches on the one stream, the perception first"""
        if self.stereo:
            self.perceiver.run(stream)
            L.check(self.lib.abc_canonical_order_stereo(C.byref(self.d), stream_or_current(stream)), "canonical_order_stereo")
            return
        L.check(self.lib.abc_canonical_order(C.byref(self.d), stream_or_current(stream)), "canonical_order")

    def _need_stereo(self, what):
        if not self.stereo:
            raise L.AbcNetHipError("GraphCanonicalizer.%s: the op was built without stereo=True" % what)

    def stereo_search(self):
        """stereo=True: the stereo_search rows of the last run as a structured numpy array [B] with the int32 fields
        L.STEREO_SEARCH_COLUMNS (leaves of equal h and unequal word, stereo improvements, stereo automorphisms, 0).  Host sync."""
        self._need_stereo("stereo_search")
        return _structured_rows(self.search, L.STEREO_SEARCH_COLUMNS)

    def stereo_elements(self):
        """stereo=True: StereoPerceiver.elements() of the op's own perceiver.  Host sync."""
        self._need_stereo("stereo_elements")
        return self.perceiver.elements()

    def rows(self):
        """the canonical rows of the last run as a contract.MoleculeRows on the device: what SmilesWriter(...) and
        MolBlockWriter(...) take in place of GraphAssembler.rows"""
        if self.out is None:
            raise L.AbcNetHipError("GraphCanonicalizer.rows: built on graph records or with rows=False, there are no canonical rows")
        return self.out

    def orders(self):
        """int32 [B, cap] on the host: orders()[b][k] is the 0-based row (for a record: the original record index) of the atom at
        canonical position k, -1 beyond the image's atoms.  Host sync."""
        return self.order.cpu()

    def stats(self):
        """the stats rows of the last run as a structured numpy array [B] with the int32 fields L.CANON_COLUMNS; `status` holds the
        L.CANON_* bits.  Host sync."""
        return _structured_rows(self.stat, L.CANON_COLUMNS)

    def keys(self):
        """int64 [B, 2] on the host: two HASH words of the relabelled graph (equal for equal graphs; equal keys prove nothing --
        certificates() does).  Host sync."""
        return self.key.cpu()

    def certificates(self):
        """cert=True: int32 [B, 2 + cap + 3 cap_bonds] on the host, the relabelled graph of every image -- equal rows ARE equal
        graphs.  Host sync."""
        if self.cert is None:
            raise L.AbcNetHipError("GraphCanonicalizer.certificates: the op was built without cert=True")
        return self.cert.cpu()


class AromaticityPerceiver(_OneSideOp):
    """the aromatic rings of every image, perceived on the device (csrc/aromatic.hip, abc_perceive_aromatic; the rule:
    include/abcnet_hip.h): the rows of a GraphAssembler -- or the bond rows of contract.GraphRecords -- copied with
    the bonds of every aromatic cycle set to order 4, so that a Kekule drawing and an order-4 drawing of one ring are one graph.
    rows() / records() are what GraphCanonicalizer, SmilesWriter, MolBlockWriter, GraphScore, GraphSimilarity and GraphIdentity take in
    place of the input.  The rule is this project's own (a function of the graph, integers only), NOT RDKit's.  One launch, static
    buffers, graph-capture safe; stats() and codes() are the host syncs.  No CPU fallback (the host form is
    decode.Molecule.aromatized())."""

    def __init__(self, mol_counts=None, mol_atoms=None, mol_bonds=None, mol_implh=None, records=None, codes=False):
        """a contract.MoleculeRows (GraphAssembler.rows) or its device tensors (mol_implh optional: no atom counts as listed without
        it), OR records=contract.GraphRecords (or a scorer, whose records are taken).  codes: keep the code of every atom in .code
        (int32 [B, cap]: L.AROM_NOT_CANDIDATE, L.AROM_NONE or its electrons)."""
        d = L.AromaticDesc()
        self._records = None
        self.source, dev = self._bind(d, (mol_counts, mol_atoms, mol_bonds, mol_implh), records, True)
        if self.source is not None:
            self.out_bonds = torch.zeros((self.B, self.cap_bonds, REC_BOND_W), dtype=torch.int32, device=dev)
            d.out_rec_bonds = self.out_bonds.data_ptr()
            atoms, _, cnt = self.source.staging.dev.values()
            self._records = DerivedGraphRecords(self.source, atoms, self.out_bonds, cnt, "AromaticityPerceiver")
        self.stat = torch.zeros((self.B, len(L.AROMATIC_COLUMNS)), dtype=torch.int32, device=dev)
        self.code = torch.full((self.B, self.cap), L.AROM_NOT_CANDIDATE, dtype=torch.int32, device=dev) if codes else None
        d.stats, d.code_out = self.stat.data_ptr(), L.ptr(self.code)
        self.d = d

    def run(self, stream=None):
        """one launch (graph-capturable): the perceived rows (or record bonds), stats, and the codes when they were asked for"""
        L.check(self.lib.abc_perceive_aromatic(C.byref(self.d), stream_or_current(stream)), "perceive_aromatic")

    def rows(self):
        """the perceived rows of the last run as a contract.MoleculeRows on the device: what the canonicaliser, the writers and the
        scorers take in place of GraphAssembler.rows"""
        if self.out is None:
            raise L.AbcNetHipError("AromaticityPerceiver.rows: built on graph records, which have no molecule rows (records())")
        return self.out

    def records(self):
        """the perceived records of the last run as a contract.GraphRecords on the device: the source's atoms and counts, this op's
        bond rows; what the scorers and GraphCanonicalizer take as records=; its `load` is refused (load the source)"""
        if self._records is None:
            raise L.AbcNetHipError("AromaticityPerceiver.records: built on molecule rows, there are no records (rows())")
        return self._records

    def stats(self):
        """the stats rows of the last run as a structured numpy array [B] with the int32 fields L.AROMATIC_COLUMNS.  Host sync."""
        return _structured_rows(self.stat, L.AROMATIC_COLUMNS)

    def codes(self):
        """codes=True: int32 [B, cap] on the host, per atom L.AROM_NOT_CANDIDATE, L.AROM_NONE or its electrons.  Host sync."""
        if self.code is None:
            raise L.AbcNetHipError("AromaticityPerceiver.codes: the op was built without codes=True")
        return self.code.cpu()


def timed(stream, marks, label, flops, nbytes, fn, operand_bytes=None):
    """profile(): fn() between a HIP event pair recorded on `stream` (a torch stream, the one fn launches on); the pair and the
    launch's accounting go to `marks`.  Returns what fn returned."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    rc = fn()
    e1.record(stream)
    marks.append((label, e0, e1, {"flops": flops, "bytes": nbytes, "operand_bytes": nbytes if operand_bytes is None else operand_bytes}))
    return rc


def fold_marks(acc, marks, fields):
    """profile(), after a device sync: add every mark of one iteration to acc[label] = {"calls", "ms", *fields}"""
    for label, e0, e1, cost in marks:
        r = acc.setdefault(label, dict({"calls": 0, "ms": 0.0}, **{f: 0.0 for f in fields}))
        r["calls"] += 1
        r["ms"] += e0.elapsed_time(e1)
        for f in fields:
            r[f] += cost[f]


def per_iteration(acc, iters):
    for r in acc.values():
        for f in r:
            r[f] /= iters
    return acc


class FusedAdam:
    """torch.optim.Adam(lr, weight_decay) over the flat arena as one kernel (train.py:55).  Re-create it to
    reset the moments, as the reference does at the learning-rate drop (train.py:84-85)."""

    def __init__(self, params, grads, lr=2.5e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-8, grad_scale=1.0):
        self.lib = L.load()
        self.p, self.g = params, grads
        self.m = torch.zeros_like(params)
        self.v = torch.zeros_like(params)
        self.step_t = torch.zeros(1, dtype=torch.int64, device=params.device)
        d = L.AdamDesc()
        d.p, d.g, d.m, d.v, d.n = params.data_ptr(), grads.data_ptr(), self.m.data_ptr(), self.v.data_ptr(), params.numel()
        d.step = self.step_t.data_ptr()
        d.lr, d.beta1, d.beta2, d.eps, d.weight_decay, d.grad_scale = lr, betas[0], betas[1], eps, weight_decay, grad_scale
        self.d = d

    def step(self, stream=None):
        L.check(self.lib.abc_adam_step(C.byref(self.d), stream_or_current(stream)), "adam_step")
