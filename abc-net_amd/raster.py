"""Targets from annotations on the device: the rasteriser of /root/reference/src/utils.py:83-228
(MolecularImageDataset.__getitem__) split into a tiny host half and a device half.

    host   parse_record(): the string handling, vocabulary look-ups and the float64 atan / floor of utils.py:94-163 --
           exactly the reference's Python arithmetic -- into (atoms int32 [n,5], bonds int32 [m,5], rho float64 [m]);
    device TargetRasterizer: zero + rasterise the 8 target maps in HBM (csrc/raster.hip, abc_rasterize_targets), in
           record order, into static buffers (optionally the Trainer's own target buffers).

A batch-16 step then ships a few KB of records over PCIe instead of 376 MB of mostly-zero maps.  No CPU fallback.
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np
import torch

from . import _lib as L
from .contract import PinnedStaging, alloc_targets, check_targets, set_target_ptrs, stream_or_current

ATOM_VOCAB = {'<unkonw>': 0, 'C': 1, 'N': 2, 'O': 3, 'P': 4, 'F': 5, 'Cl': 6, 'S': 7, 'Br': 8, 'B': 9,
              'Se': 10, 'I': 11, 'H': 12, 'Si': 13}        # utils.py:12-13
CHARGE_VOCAB = {0: 0, 1: 1, -1: 2}                          # utils.py:14
BOND_VOCAB = {1: 0, 2: 1, 3: 2, 4: 3}                       # utils.py:15


def parse_record(atoms_string, bonds_string, scale_x=1, scale_y=1, ddx=0, ddy=0, h=128):
    """utils.py:94-112 (atoms) and 135-163 (bonds): annotation strings -> compact records.
    atoms[i] = (x, y, type, charge, hs) with hs = -1 unless 0 or 1; bonds[i] = (x, y, type, omega bin, single)."""
    atoms = []
    for atom_string in atoms_string.split(';')[:-1]:
        atom, position = atom_string.split(':')
        if len(atom) == 1:
            atom = atom.upper()
        f = position.split(',')
        x, y, charge = int(int(f[0]) * scale_x + ddx) // 4, int(int(f[1]) * scale_y + ddy) // 4, int(f[2])
        hs = int(f[3]) if len(f) == 4 else -1
        if not (0 <= x < h and 0 <= y < h):
            raise ValueError("atom at (%d, %d) falls outside the %d x %d map" % (x, y, h, h))
        atoms.append((x, y, ATOM_VOCAB.get(atom, 0), CHARGE_VOCAB.get(charge, 0), hs if hs in (0, 1) else -1))
    bonds, rhos = [], []
    delta_omega = np.pi / 30
    for bond_string in bonds_string.split(';')[:-1]:
        bond, position = bond_string.split(':')
        type_idx = BOND_VOCAB.get(int(bond), 0)
        f = position.split(',')
        x, y = int(int(f[0]) * scale_x + ddx) // 4, int(int(f[1]) * scale_y + ddy) // 4
        delta_x, delta_y = (int(f[2]) * scale_x) / 4, (int(f[3]) * scale_y) / 4
        stereo, direction = int(f[4]), int(f[5])
        if stereo == 5 or stereo == 1:
            type_idx = 4
        elif stereo == 6:
            type_idx = 5
        if delta_x < 0:
            delta_x, delta_y = -delta_x, -delta_y
        elif delta_x == 0:
            if delta_y > 0:
                direction = 1
            delta_y = -abs(delta_y)
        rho = np.sqrt(delta_x * delta_x + delta_y * delta_y)
        omega = math.atan(delta_y / (delta_x + 1e-6))
        k = int(np.floor((omega + np.pi / 2) / delta_omega))
        single = 1 if type_idx in (4, 5) else 0
        if single and direction == 1:
            k += 30
        if not (0 <= x < h and 0 <= y < h) or not (0 <= k < (60 if single else 30)):
            raise ValueError("bond at (%d, %d), omega bin %d falls outside the maps" % (x, y, k))
        bonds.append((x, y, type_idx, k, single))
        rhos.append(float(rho))
    return (np.array(atoms, dtype=np.int32).reshape(-1, 5), np.array(bonds, dtype=np.int32).reshape(-1, 5),
            np.array(rhos, dtype=np.float64))


def parse_graph(atoms_string, bonds_string, scale_x=1, scale_y=1, ddx=0, ddy=0, h=128):
    """the annotated molecule as a graph on the head-map grid, for ops.GraphScore: (atoms int32 [n,4], bonds int32 [m,3]).
    atoms[i] = (x, y, element, charge): the cell of parse_record, the ATOM_VOCAB index (-1 for an element outside the vocabulary)
    and the annotated charge as written.  bonds[k] = (i, j, code): i < j 0-based atom indices and parse_record's bond type index
    + 1 (1-4 the orders, 5 a wedge of stereo 1 / 5, 6 of stereo 6).  An end of a bond is the atom nearest to centre -/+ half vector,
    measured between the transformed, un-floored positions in float64 (the first atom of the string wins a tie); a bond whose
    ends are one atom, or whose pair an earlier bond has, is dropped; the others keep the order of the string."""
    atoms, px, py = [], [], []
    for atom_string in atoms_string.split(';')[:-1]:
        atom, position = atom_string.split(':')
        if len(atom) == 1:
            atom = atom.upper()
        f = position.split(',')
        fx, fy = int(f[0]) * scale_x + ddx, int(f[1]) * scale_y + ddy
        x, y = int(fx) // 4, int(fy) // 4
        if not (0 <= x < h and 0 <= y < h):
            raise ValueError("atom at (%d, %d) falls outside the %d x %d map" % (x, y, h, h))
        atoms.append((x, y, ATOM_VOCAB.get(atom, -1), int(f[2])))
        px.append(float(fx))
        py.append(float(fy))

    def nearest(ex, ey):
        best, at = None, -1
        for i in range(len(atoms)):
            dx, dy = px[i] - ex, py[i] - ey
            d2 = dx * dx + dy * dy
            if best is None or d2 < best:
                best, at = d2, i
        return at

    bonds, seen = [], set()
    for bond_string in bonds_string.split(';')[:-1]:
        bond, position = bond_string.split(':')
        type_idx = BOND_VOCAB.get(int(bond), 0)
        f = position.split(',')
        X, Y, DX, DY, stereo = int(f[0]), int(f[1]), int(f[2]), int(f[3]), int(f[4])
        if stereo == 5 or stereo == 1:
            type_idx = 4
        elif stereo == 6:
            type_idx = 5
        i = nearest(float((X - DX) * scale_x + ddx), float((Y - DY) * scale_y + ddy))
        j = nearest(float((X + DX) * scale_x + ddx), float((Y + DY) * scale_y + ddy))
        pair = (min(i, j), max(i, j))
        if i == j or pair in seen:
            continue
        seen.add(pair)
        bonds.append(pair + (type_idx + 1,))
    return np.array(atoms, dtype=np.int32).reshape(-1, 4), np.array(bonds, dtype=np.int32).reshape(-1, 3)


class TargetRasterizer:
    """device-side utils.py:83-228 for a batch; `targets` may be the Trainer's static target tensors (then `run` writes
    the loss inputs in place), otherwise fresh ones are allocated with the reference collate shapes / dtypes"""

    def __init__(self, batch, h, w=None, max_atoms=256, max_bonds=256, targets=None, device="cuda", sparse=False):
        """sparse=True: the maps are zeroed ONCE; every later run() erases the pixels the previous records drew instead of zeroing
        23 MB per image (the target tensors must not be written by anybody else in between: invalidate() after that), and
        .group_flags says which 32-pixel groups of the batch hold targets of which head -- Trainer.use_sparse_targets(rasterizer)
        lets the fused heads pass skip the all-zero planes (abc_raster_desc.group_flags)."""
        w = h if w is None else w
        if not torch.cuda.is_available():
            raise L.AbcNetHipError("TargetRasterizer needs an MI355X; abcnet_amd has no CPU fallback")
        self.lib = L.load()
        B = batch
        if targets is None:
            targets = alloc_targets(B, h, w, device)
        check_targets(targets, B, h, w, "raster", L.AbcNetHipError)
        self.targets = list(targets)
        dev = targets[0].device
        self.B, self.h, self.w, self.max_atoms, self.max_bonds = B, h, w, max_atoms, max_bonds
        # host staging (pinned) + device record buffers
        self.staging = PinnedStaging(dev, {"atoms": ((B, max_atoms, 5), torch.int32), "bonds": ((B, max_bonds, 5), torch.int32),
                                           "rho": ((B, max_bonds), torch.float64), "cnt": ((2, B), torch.int32)})
        self.h_atoms, self.h_bonds, self.h_rho, self.h_cnt = self.staging.host.values()
        self.d_atoms, self.d_bonds, self.d_rho, self.d_cnt = self.staging.dev.values()
        d = L.RasterDesc()
        set_target_ptrs(d, self.targets)
        d.B, d.h, d.w, d.max_atoms, d.max_bonds = B, h, w, max_atoms, max_bonds
        d.atoms, d.bonds, d.rho = self.d_atoms.data_ptr(), self.d_bonds.data_ptr(), self.d_rho.data_ptr()
        d.n_atoms, d.n_bonds = self.d_cnt[0].data_ptr(), self.d_cnt[1].data_ptr()
        self.sparse = bool(sparse)
        self.group_flags = None
        self._drawn = False          # sparse: do the maps hold exactly what the prev_* records say?
        if self.sparse:
            if (h * w) % 32:
                raise L.AbcNetHipError("sparse rasteriser: h * w must be a multiple of 32")
            self.group_flags = torch.zeros(B * h * w // 32, dtype=torch.int32, device=dev)
            self.p_atoms, self.p_bonds = torch.zeros_like(self.d_atoms), torch.zeros_like(self.d_bonds)
            self.p_rho, self.p_cnt = torch.zeros_like(self.d_rho), torch.zeros_like(self.d_cnt)
            d.group_flags = self.group_flags.data_ptr()
            d.prev_atoms, d.prev_bonds, d.prev_rho, d.prev_counts = (t.data_ptr() for t in (self.p_atoms, self.p_bonds, self.p_rho, self.p_cnt))
        self.d = d

    def invalidate(self):
        """sparse: somebody else wrote the target tensors -- the next run() zeroes them completely again"""
        self._drawn = False

    def load(self, records):
        """records = list of B (atoms, bonds, rho) triples from parse_record; async H2D of a few KB"""
        if len(records) != self.B:
            raise ValueError("expected %d records" % self.B)
        for b, (a, q, _r) in enumerate(records):
            if len(a) > self.max_atoms or len(q) > self.max_bonds:
                raise ValueError("record %d has %d atoms / %d bonds (capacity %d / %d)" % (b, len(a), len(q), self.max_atoms, self.max_bonds))
        self.staging.wait()
        for b, (a, q, r) in enumerate(records):
            self.h_cnt[0, b], self.h_cnt[1, b] = len(a), len(q)
            if len(a):
                self.h_atoms[b, :len(a)] = torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32))
            if len(q):
                self.h_bonds[b, :len(q)] = torch.from_numpy(np.ascontiguousarray(q, dtype=np.int32))
                self.h_rho[b, :len(q)] = torch.from_numpy(np.ascontiguousarray(r, dtype=np.float64))
        self.staging.commit()

    def run(self, stream=None):
        if self.sparse:
            self.d.incremental = 1 if self._drawn else 0
        L.check(self.lib.abc_rasterize_targets(C.byref(self.d), stream_or_current(stream)), "rasterize_targets")
        self._drawn = True
        return self.targets
