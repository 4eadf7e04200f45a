"""Oracle (test infrastructure, not product): the graph assembly of the reference inference driver, img2smiles2.py:193-311,
restated as a function of one image's candidate lists -- scalar float64 Python, one rounding per operation, in the order the
kernel (abc-net_amd/csrc/assemble.hip) uses.  Deliberately not vectorised: every line is one IEEE operation, so this file IS
the specification of the operation order.  Pinned by tests/golden/assemble_128.npz (exec of the reference text by
tests/golden/make_golden_assemble.py), arg-min arrays included.

Input lists (the extractor's wire format): atoms int [n, 5] = (x, y, type index, charge index, hs), bonds int [m, 4] =
(x, y, omega bin, bond type index), rho float32 [m].
"""
import math

import numpy as np

ATOM_SYMBOLS = ("C", "C", "N", "O", "P", "F", "Cl", "S", "Br", "B", "Se", "I", "H", "Si")      # utils.py:12-13, index 0 as 'C'
CHARGE_VALUE = (0, 1, -1)                                                                        # utils.py:14 inverted
MAX_VALENCE = {"O": 2, "C": 4, "N": 3, "F": 1, "H": 1, "S": 6, "Cl": 1, "P": 5, "Br": 1, "B": 3, "I": 1, "Si": 4, "Se": 6}
REPAIR = {2: "O", 3: "N", 4: "C", 5: "P", 6: "S", 7: "Cl"}
SYMBOL_INDEX = {"C": 1, "N": 2, "O": 3, "P": 4, "S": 7, "Cl": 6}
EMPTY, TRUNCATED = 1, 2


def omega_table():
    """cos / sin of the 60 bin angles, by scalar numpy calls on Python floats as img2smiles2.py:160-164 makes them"""
    omega = [k * (np.pi / 30) + np.pi / 60 - np.pi / 2 for k in range(60)]
    return [float(np.cos(o)) for o in omega], [float(np.sin(o)) for o in omega]


def lrelu(x):
    h = 0.5 * x
    return x if x > h else h


def bond_ends_numpy(atoms, bonds, rho, chunk=512):
    """bond_ends() as array expressions, for lists too long for the scalar loop (thousands of candidates x hundreds of atoms).
    Every array operation is the scalar one element by element, so the bits are the same; tests/test_assemble_host.py holds
    it to bond_ends() on the goldens."""
    COS, SIN = (np.array(t) for t in omega_table())
    A = np.asarray(atoms)[:, :2].astype(np.float64)
    bonds = np.asarray(bonds)
    r = np.asarray(rho, dtype=np.float32).astype(np.float64)
    idx1, idx2 = np.zeros(len(bonds), dtype=np.int64), np.zeros(len(bonds), dtype=np.int64)
    if len(A) == 0:
        return idx1.tolist(), idx2.tolist()
    for lo in range(0, len(bonds), chunk):
        sl = slice(lo, lo + chunk)
        ok = (r[sl] > 0) & np.isfinite(r[sl])
        rr = np.where(ok, r[sl], 1.0)
        dx, dy = rr * COS[bonds[sl, 2]], rr * SIN[bonds[sl, 2]]
        n = np.sqrt(dx * dx + dy * dy)
        e1x, e1y = (dx / n)[:, None], (dy / n)[:, None]
        px, py = bonds[sl, 0].astype(np.float64), bonds[sl, 1].astype(np.float64)
        u, v = (px + dx)[:, None] - A[None, :, 0], (py + dy)[:, None] - A[None, :, 1]
        s = u * e1x + v * e1y
        dist1 = np.abs(np.maximum(s, 0.5 * s)) + np.abs((2.0 * u) * -e1y + (2.0 * v) * e1x)
        u, v = (px - dx)[:, None] - A[None, :, 0], (py - dy)[:, None] - A[None, :, 1]
        s = -(u * e1x + v * e1y)
        dist2 = np.abs(np.maximum(s, 0.5 * s)) + np.abs((2.0 * u) * -e1y + (2.0 * v) * e1x)
        idx1[sl] = np.where(ok, dist2.argmin(1), 0)
        idx2[sl] = np.where(ok, dist1.argmin(1), 0)
    return idx1.tolist(), idx2.tolist()


def bond_ends(atoms, bonds, rho):
    """(atom_index1, atom_index2) per candidate; a candidate with rho == 0 (the reference's NaN rows: both arg-mins 0) or a rho that
    is not finite gets (0, 0) and is dropped by the edge filter"""
    COS, SIN = omega_table()
    A = [(float(int(a[0])), float(int(a[1]))) for a in atoms]
    idx1, idx2 = [], []
    for c, r in zip(bonds, rho):
        r = float(np.float32(r))
        k = int(c[2])
        if not (len(A) > 0 and 0.0 < r < math.inf):
            idx1.append(0)
            idx2.append(0)
            continue
        dx = r * float(COS[k])
        dy = r * float(SIN[k])
        n = math.sqrt(dx * dx + dy * dy)
        e1x = dx / n
        e1y = dy / n
        e2x = -e1y
        e2y = e1x
        p1x = float(int(c[0])) + dx
        p1y = float(int(c[1])) + dy
        p2x = float(int(c[0])) - dx
        p2y = float(int(c[1])) - dy
        best1 = best2 = None
        i1 = i2 = 0
        for j, (ax, ay) in enumerate(A):
            u = p1x - ax
            v = p1y - ay
            s = u * e1x + v * e1y
            dist1 = abs(lrelu(s)) + abs((2.0 * u) * e2x + (2.0 * v) * e2y)
            u = p2x - ax
            v = p2y - ay
            s = -(u * e1x + v * e1y)
            dist2 = abs(lrelu(s)) + abs((2.0 * u) * e2x + (2.0 * v) * e2y)
            if best1 is None or dist1 < best1:
                best1, i2 = dist1, j
            if best2 is None or dist2 < best2:
                best2, i1 = dist2, j
        idx1.append(i1)
        idx2.append(i2)
    return idx1, idx2


def assemble(atoms, bonds, rho, cap_mol_bonds=None, vectorised=False):
    """one image's lists -> dict(atom_index1, atom_index2, symbols, types (vocabulary index after repair), charges, hs, positions,
    bonds (1-based), orders, sources (candidate index of every kept bond), implicit_hs, truncated)"""
    atoms = np.asarray(atoms).reshape(-1, 5)
    bonds = np.asarray(bonds).reshape(-1, 4)
    idx1, idx2 = (bond_ends_numpy if vectorised else bond_ends)(atoms, bonds, rho)
    seen = set()
    kept = []                                   # (end 1, end 2, order, candidate)
    truncated = False
    for i, (a, b) in enumerate(zip(idx1, idx2)):
        if a == b:
            continue
        key = (min(a, b), max(a, b))
        if key in seen:
            continue
        seen.add(key)
        if cap_mol_bonds is not None and len(kept) >= cap_mol_bonds:
            truncated = True
            continue
        kept.append((a, b, int(bonds[i, 3]) + 1, i))
    n = len(atoms)
    types = [int(t) for t in atoms[:, 2]]
    symbols = [ATOM_SYMBOLS[t] for t in types]
    charges = [CHARGE_VALUE[int(c)] for c in atoms[:, 3]]
    count = [-c for c in charges]
    shown = [False] * n
    for a, b, order, _ in kept:
        v = 1 if order >= 4 else order
        count[a] += v
        count[b] += v
        shown[a] = shown[b] = True
    for a in range(n):
        if MAX_VALENCE[symbols[a]] < count[a] and count[a] in REPAIR:
            symbols[a] = REPAIR[count[a]]
            types[a] = SYMBOL_INDEX[symbols[a]]
    new = {}
    for a in range(n):
        if shown[a]:
            new[a] = len(new) + 1
    keep = [a for a in range(n) if shown[a]]
    out_bonds = [[new[a], new[b]] for a, b, _, _ in kept]
    fs, fh = [symbols[a] for a in keep], [int(atoms[a, 4]) for a in keep]
    implicit = []
    for (x, y), (_, _, order, _) in zip(out_bonds, kept):
        if order != 4:
            continue
        for e in (x, y):
            if fs[e - 1] != "C" and fh[e - 1] != 0 and e not in implicit:
                implicit.append(e)
    return {"atom_index1": idx1, "atom_index2": idx2, "symbols": fs, "types": [types[a] for a in keep],
            "charges": [charges[a] for a in keep], "hs": fh, "positions": [[int(atoms[a, 0]), int(atoms[a, 1])] for a in keep],
            "bonds": out_bonds, "orders": [k[2] for k in kept], "sources": [k[3] for k in kept], "implicit_hs": implicit,
            "truncated": truncated}


def assemble_counts(counts, atoms, bonds, rho, cap_atoms, cap_bonds, cap_mol_bonds, vectorised=False):
    """the device's view of one image: counts (4,) as the extractor reports them, lists possibly truncated to the capacities.
    Returns None for an image the reference skips (:126-129), else assemble()'s dict with `truncated` as the device reports it."""
    if counts[0] == 0 or counts[2] == 0:
        return None
    na, nc = min(int(counts[1]), cap_atoms), min(int(counts[3]), cap_bonds)
    res = assemble(np.asarray(atoms)[:na], np.asarray(bonds)[:nc], np.asarray(rho)[:nc], cap_mol_bonds, vectorised)
    res["truncated"] = bool(res["truncated"] or counts[0] > cap_atoms or counts[1] > cap_atoms or counts[2] > 4096 or counts[3] > cap_bonds)
    return res
