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


# ---------- the decoder: rows and records its stages hand to each other; words per row as csrc/mol_rows.hpp, DESIGN.md section 7
ATOM_W, CAND_W, MOL_BOND_W, REC_ATOM_W, REC_BOND_W = 5, 4, 4, 4, 3
# the element table of StereoPerceiver, int32 [B, cap_atoms, STEREO_W] (csrc/mol_rows.hpp; decode.stereo_elements is its host form): the
# name of every word; "none" (decode.STEREO_NONE_ROW) is 0 in `centre` and `bond_code`, -1 elsewhere
from .decode import STEREO_W  # noqa: E402
STEREO_ELEMENT = ("centre", "nb0", "nb1", "nb2", "nb3", "bond_code", "bond_row", "partner", "sub0", "sub1", "partner_sub0", "partner_sub1")
assert len(STEREO_ELEMENT) == STEREO_W


def _require_layout(who, names, tensors, shapes):
    """every one a tensor, then of its shape in shapes(B, cap_a, cap_b), B and cap_a read from tensors[1], cap_b from tensors[2]"""
    for name, t in zip(names, tensors):
        if not isinstance(t, torch.Tensor):
            raise ValueError("%s: %s must be a tensor, got %s" % (who, name, type(t).__name__))
    dims = tuple(tensors[1].shape[:2]) + tuple(tensors[2].shape[1:2])
    if len(dims) != 3 or [tuple(t.shape) for t in tensors] != shapes(*dims)[:len(tensors)]:
        raise ValueError("%s: %s must be %s, got %s" % (who, ", ".join(names[:len(tensors)]), shapes("B", "cap_a", "cap_b")[:len(tensors)],
                                                        [tuple(t.shape) for t in tensors]))
    return dims


class CandidateLists:
    """PeakExtractor's output, GraphAssembler's input: int32 counts, atoms and bonds, f32 bond_rho, of SHAPES"""
    NAMES = ("counts", "atoms", "bonds", "bond_rho")
    SHAPES = staticmethod(lambda B, cap_atoms, cap_bonds: [(B, 4), (B, cap_atoms, ATOM_W), (B, cap_bonds, CAND_W), (B, cap_bonds)])

    def __init__(self, counts, atoms, bonds, bond_rho):
        self.tensors = (counts, atoms, bonds, bond_rho)
        self.B, self.cap_atoms, self.cap_bonds = atoms.shape[0], atoms.shape[1], bonds.shape[1]

    @classmethod
    def checked(cls, who, counts, atoms=None, bonds=None, bond_rho=None):
        """a CandidateLists or the four tensors (hand-made lists): type, shape (ValueError), then device and dtype (AbcNetHipError)"""
        if isinstance(counts, cls):
            counts, atoms, bonds, bond_rho = counts.tensors
        _require_layout(who, cls.NAMES, (counts, atoms, bonds, bond_rho), cls.SHAPES)
        for name, t in zip(cls.NAMES, (counts, atoms, bonds, bond_rho)):
            require_device_tensor(t, torch.float32 if t is bond_rho else torch.int32, "%s: %s (the extractor's layout)" % (who, name))
        return cls(counts, atoms, bonds, bond_rho)


class MoleculeRows:
    """GraphAssembler's output, read in place by MolBlockWriter, SmilesWriter, GraphScore and GraphSimilarity: int32 tensors of SHAPES; a row of
    mol_counts is (atoms, bonds, implicit-H entries, L.MOL_* status bits); mol_implh is read by the text alone"""
    NAMES = ("mol_counts", "mol_atoms", "mol_bonds", "mol_implh")
    SHAPES = staticmethod(lambda B, cap_atoms, cap_mol_bonds: [(B, 4), (B, cap_atoms, ATOM_W), (B, cap_mol_bonds, MOL_BOND_W), (B, cap_atoms)])

    def __init__(self, mol_counts, mol_atoms, mol_bonds, mol_implh=None):
        self.tensors = (mol_counts, mol_atoms, mol_bonds, mol_implh)
        self.B, self.cap_atoms, self.cap_mol_bonds, self.device = mol_atoms.shape[0], mol_atoms.shape[1], mol_bonds.shape[1], mol_atoms.device

    @classmethod
    def checked(cls, who, mol_counts, mol_atoms=None, mol_bonds=None, mol_implh=None, max_cap_atoms=None, need_implh=False, n_valid=None,
                max_cap_mol_bonds=None):
        """a MoleculeRows or the separate tensors (hand-made rows): type, shape, range, n_valid's form (ValueError), then device (AbcNetHipError)"""
        if isinstance(mol_counts, cls):
            mol_counts, mol_atoms, mol_bonds, mol_implh = mol_counts.tensors
        read = (mol_counts, mol_atoms, mol_bonds) + ((mol_implh,) if need_implh else ())
        B, cap_atoms, cap_mol_bonds = _require_layout(who, cls.NAMES, read, cls.SHAPES)
        if (B < 1 or cap_atoms < 1 or cap_mol_bonds < 1 or (max_cap_atoms is not None and cap_atoms > max_cap_atoms)
                or (max_cap_mol_bonds is not None and cap_mol_bonds > max_cap_mol_bonds)):
            raise ValueError("%s: B >= 1, cap_atoms %s and cap_mol_bonds %s, got %d, %d, %d"
                             % (who, ">= 1" if max_cap_atoms is None else "1..%d" % max_cap_atoms,
                                ">= 1" if max_cap_mol_bonds is None else "1..%d" % max_cap_mol_bonds, B, cap_atoms, cap_mol_bonds))
        if n_valid is not None and not (isinstance(n_valid, torch.Tensor) and n_valid.numel() == 1):
            raise ValueError("%s: n_valid must be a one-element int32 device tensor" % who)
        for t in read + (() if n_valid is None else (n_valid,)):
            require_device_tensor(t, torch.int32, "%s: %s (the assembler's layout)%s"
                                  % (who, ", ".join(cls.NAMES[:len(read)]), "" if n_valid is None else " and n_valid"))
        return cls(mol_counts, mol_atoms, mol_bonds, mol_implh if need_implh else None)

    def fill(self, d):
        """the mol_*, B and cap_* fields every descriptor that reads the rows has; mol_implh (null when these rows have none) where the
        descriptor has the field"""
        d.mol_counts, d.mol_atoms, d.mol_bonds = (t.data_ptr() for t in self.tensors[:3])
        if hasattr(d, "mol_implh"):
            d.mol_implh = L.ptr(self.tensors[3])
        d.B, d.cap_atoms, d.cap_mol_bonds = self.B, self.cap_atoms, self.cap_mol_bonds


class GraphRecords:
    """One raster.parse_graph record per image in pinned staging and its device twins: atoms int32 [B, max_atoms, 4], bonds int32
    [B, max_bonds, 3], counts int32 [2, B].  One object may serve several readers of a batch: it is loaded once, by its owner."""

    def __init__(self, B, max_atoms, max_bonds, device):
        self.B, self.max_atoms, self.max_bonds = int(B), int(max_atoms), int(max_bonds)
        self.staging = PinnedStaging(device, {"atoms": ((self.B, self.max_atoms, REC_ATOM_W), torch.int32),
                                              "bonds": ((self.B, self.max_bonds, REC_BOND_W), torch.int32), "cnt": ((2, self.B), torch.int32)})
        self.loaded = False

    @staticmethod
    def validate(graphs, B, max_atoms, max_bonds):
        """the half of load that needs no device: `graphs` as contiguous int32 (atoms [n, 4], bonds [m, 3]) pairs, or ValueError"""
        import numpy as np
        if len(graphs) > B:
            raise ValueError("expected at most %d graph records, got %d" % (B, len(graphs)))
        recs = []
        for b, (a, q) in enumerate(graphs):
            a, q = np.asarray(a), np.asarray(q)
            if a.ndim != 2 or a.shape[1] != REC_ATOM_W or q.ndim != 2 or q.shape[1] != REC_BOND_W:
                raise ValueError("record %d: atoms must be [n, 4] and bonds [m, 3], got %s and %s" % (b, a.shape, q.shape))
            if len(a) > max_atoms or len(q) > max_bonds:
                raise ValueError("record %d has %d atoms / %d bonds (capacity %d / %d)" % (b, len(a), len(q), max_atoms, max_bonds))
            if len(q) and not ((0 <= q[:, 0]) & (q[:, 0] < q[:, 1]) & (q[:, 1] < len(a))).all():
                raise ValueError("record %d: every bond must name atoms 0 <= i < j < %d" % (b, len(a)))
            recs.append((np.ascontiguousarray(a, dtype=np.int32), np.ascontiguousarray(q, dtype=np.int32)))
        return recs

    def load(self, graphs):
        """n <= B (atoms, bonds) pairs of raster.parse_graph; the rows past n get an empty record.  Asynchronous H2D of a few KB."""
        recs = self.validate(graphs, self.B, self.max_atoms, self.max_bonds)
        h_atoms, h_bonds, h_cnt = self.staging.host.values()
        self.staging.wait()
        h_cnt.zero_()
        for b, (a, q) in enumerate(recs):
            h_cnt[0, b], h_cnt[1, b] = len(a), len(q)
            if len(a):
                h_atoms[b, :len(a)] = torch.from_numpy(a)
            if len(q):
                h_bonds[b, :len(q)] = torch.from_numpy(q)
        self.staging.commit()
        self.loaded = True

    def fill(self, d):
        """the rec_* and max_* fields of GraphScoreDesc and GraphSimilarityDesc"""
        d.rec_atoms, d.rec_bonds, d.rec_counts = (t.data_ptr() for t in self.staging.dev.values())
        d.max_atoms, d.max_bonds = self.max_atoms, self.max_bonds


class _DeviceTwins:
    """the `.dev` / `.device` half of a PinnedStaging, for tensors a device stage writes"""

    def __init__(self, device, dev):
        self.device, self.dev = torch.device(device), dict(dev)


class DerivedGraphRecords(GraphRecords):
    """The records of `source` as a device stage rewrote them (ops.AromaticityPerceiver.records()): a GraphRecords for every reader,
    whose device twins are that stage's outputs (and the source's own tensors where the stage copies nothing).  It is loaded when its
    source is, and only there: `load` is refused."""

    def __init__(self, source, atoms, bonds, cnt, owner):
        self.B, self.max_atoms, self.max_bonds = source.B, source.max_atoms, source.max_bonds
        self.source, self.owner = source, owner
        self.staging = _DeviceTwins(source.staging.device, {"atoms": atoms, "bonds": bonds, "cnt": cnt})

    @property
    def loaded(self):
        return self.source.loaded

    def load(self, graphs):
        raise ValueError("these records are written on the device by %s: load its source (GraphRecords.load, InferenceRunner.load_graphs) "
                         "and run it" % self.owner)
