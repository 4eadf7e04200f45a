"""Oracle (test infrastructure, not product): the graph records of abcnet_amd.raster.parse_graph and the score of
abc-net_amd/csrc/graph_score.hip, restated with sets and brute force -- no LDS tables, no running minima, no pair keys.

    parse_graph(atoms_string, bonds_string, ...)  -> (atoms [(x, y, element, charge)], bonds [(i, j, code)])
    score(mol, atoms, bonds, radius)              -> the 14 columns of one image, as a dict
    rows(mols, records, radius, n_valid)          -> int [B, 14]

`mol` is None (ABC_MOL_EMPTY) or anything with symbols / charges / positions / bonds (1-based) / orders / truncated: a
decode.Molecule, or the dict of assemble_oracle.assemble.

closed_loop(): the CPU chain annotation -> raster_oracle -> ideal logits -> nms_oracle -> decode_oracle -> assemble_oracle ->
score on drawn_molecules(6, 512, seed=5), computed once and shared by the host and the device tests.
"""
import functools
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if p not in sys.path:
        sys.path.insert(0, p)

COLUMNS = ("counted", "none", "truncated", "exact", "atoms_equal", "bonds_equal", "atoms_true", "atoms_pred", "atoms_located",
           "atoms_matched", "bonds_true", "bonds_pred", "bonds_paired", "bonds_matched")
ATOM_VOCAB = {'<unkonw>': 0, 'C': 1, 'N': 2, 'O': 3, 'P': 4, 'F': 5, 'Cl': 6, 'S': 7, 'Br': 8, 'B': 9, 'Se': 10, 'I': 11, 'H': 12, 'Si': 13}
ATOM_SYMBOLS = ("C", "C", "N", "O", "P", "F", "Cl", "S", "Br", "B", "Se", "I", "H", "Si")


def _fields(string):
    return [s.split(":") for s in string.split(";")[:-1]]


def parse_graph(atoms_string, bonds_string, scale_x=1, scale_y=1, ddx=0, ddy=0):
    atoms, pos = [], []
    for name, rest in _fields(atoms_string):
        f = [int(v) for v in rest.split(",")]
        name = name.upper() if len(name) == 1 else name
        fx, fy = f[0] * scale_x + ddx, f[1] * scale_y + ddy
        atoms.append((int(fx) // 4, int(fy) // 4, ATOM_VOCAB[name] if name in ATOM_VOCAB else -1, f[2]))
        pos.append((fx, fy))
    pos = np.array(pos, dtype=np.float64).reshape(-1, 2)
    listed = {}      # unordered pair -> code of its first listing (dicts keep insertion order)
    for order, rest in _fields(bonds_string):
        X, Y, DX, DY, stereo, _direction = (int(v) for v in rest.split(","))
        code = {1: 1, 2: 2, 3: 3, 4: 4}.get(int(order), 1)
        code = {1: 5, 5: 5, 6: 6}.get(stereo, code)
        if len(pos) == 0:
            continue
        ends = []
        for sign in (-1, 1):
            e = np.array([(X + sign * DX) * scale_x + ddx, (Y + sign * DY) * scale_y + ddy], dtype=np.float64)
            d = pos - e
            ends.append(int(np.argmin(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1])))      # (argmin: the first minimum)
        pair = (min(ends), max(ends))
        if ends[0] != ends[1] and pair not in listed:
            listed[pair] = code
    return atoms, [(i, j, c) for (i, j), c in listed.items()]


def _get(mol, key):
    return mol[key] if isinstance(mol, dict) else getattr(mol, key)


def score(mol, atoms, bonds, radius=0):
    atoms = [tuple(int(v) for v in a) for a in np.asarray(atoms).reshape(-1, 4)]
    bonds = [tuple(int(v) for v in q) for q in np.asarray(bonds).reshape(-1, 3)]
    T = sorted({i for i, _, _ in bonds} | {j for _, j, _ in bonds})
    out = dict.fromkeys(COLUMNS, 0)
    out["counted"], out["atoms_true"], out["bonds_true"] = 1, len(T), len(bonds)
    if mol is None:
        out["none"] = 1
        return out
    P = [tuple(int(v) for v in p) for p in _get(mol, "positions")]
    syms, charges = list(_get(mol, "symbols")), [int(c) for c in _get(mol, "charges")]
    mbonds = [(int(b[0]) - 1, int(b[1]) - 1, int(o)) for b, o in zip(_get(mol, "bonds"), _get(mol, "orders"))]

    def d2(a, p):
        return (atoms[a][0] - P[p][0]) ** 2 + (atoms[a][1] - P[p][1]) ** 2

    def nearest(cands, dist):
        within = [t for t in ((dist(c), c) for c in cands) if t[0] <= radius * radius]
        return min(within)[1] if within else None

    near_p = {a: nearest(range(len(P)), lambda p: d2(a, p)) for a in T}
    near_t = {p: nearest(T, lambda a: d2(a, p)) for p in range(len(P))}
    located = {(a, p) for a, p in near_p.items() if p is not None and near_t[p] == a}
    t_of = {p: a for a, p in located}
    matched = {(a, p) for a, p in located
               if atoms[a][2] != -1 and ATOM_SYMBOLS[atoms[a][2]] == syms[p] and atoms[a][3] == charges[p]}
    first = {}
    for i, j, c in bonds:
        first.setdefault(frozenset((i, j)), c)
    paired = [(frozenset((t_of[e1], t_of[e2])), o) for e1, e2, o in mbonds if e1 in t_of and e2 in t_of
              and frozenset((t_of[e1], t_of[e2])) in first]
    out["truncated"] = int(bool(_get(mol, "truncated")))
    out["atoms_pred"], out["bonds_pred"] = len(P), len(mbonds)
    out["atoms_located"], out["atoms_matched"] = len(located), len(matched)
    out["bonds_paired"] = len(paired)
    out["bonds_matched"] = sum(first[k] == o for k, o in paired)
    out["atoms_equal"] = int(out["atoms_matched"] == len(T) == len(P))
    out["bonds_equal"] = int(out["bonds_matched"] == len(bonds) == len(mbonds))
    out["exact"] = int(out["atoms_equal"] and out["bonds_equal"])
    return out


def rows(mols, records, radius=0, n_valid=None):
    """int64 [B, 14]: B = len(mols); records may be shorter (the rest are empty records); rows at or past n_valid are zero"""
    B = len(mols)
    n_valid = B if n_valid is None else n_valid
    out = np.zeros((B, len(COLUMNS)), dtype=np.int64)
    empty = (np.zeros((0, 4), dtype=np.int32), np.zeros((0, 3), dtype=np.int32))
    for b in range(min(B, n_valid)):
        a, q = records[b] if b < len(records) else empty
        s = score(mols[b], a, q, radius)
        out[b] = [s[c] for c in COLUMNS]
    return out


def ideal_logits(targets):
    """head logits that say exactly what the target maps say (torch ops, on the maps' device): a centre is the only local
    maximum above the NMS threshold of -1 in its 3x3 ring, every class head has its arg max at the target class, rho is the target"""
    t_at, t_ty, t_ch, t_hs, t_bt, t_bty, t_rho, t_om = targets
    B, _, h, w = t_at.shape
    return [5.0 * t_at - 2.5, 4.0 * t_ty, 4.0 * t_ch, 4.0 * t_hs, 5.0 * t_bt - 2.5, 4.0 * t_bty.reshape(B, 360, h, w),
            t_rho.float(), (5.0 * t_om - 2.5).float()]


CLOSED_LOOP = dict(batch=6, size=512, seed=5)


@functools.lru_cache(maxsize=None)
def closed_loop():
    """(notes, records, mols, rows at radius 0) of the CPU chain on drawn_molecules(6, 512, seed=5)"""
    from abcnet_amd.synthetic import drawn_molecules
    from oracle import decode_oracle, nms_oracle, raster_oracle
    import assemble_oracle as ao
    B, S = CLOSED_LOOP["batch"], CLOSED_LOOP["size"]
    _x, notes = drawn_molecules(B, S, seed=CLOSED_LOOP["seed"])
    h = S // 4
    maps = [raster_oracle.rasterize(a, q, h=h) for a, q in notes]
    targets = [torch.from_numpy(np.stack([m[i] for m in maps])) for i in range(8)]
    lg = ideal_logits(targets)
    am, bm, rho, _om = nms_oracle.nms(lg[0], lg[4], lg[6], lg[7])
    mols = []
    for b in range(B):
        atoms, bonds, r = decode_oracle.extract(am[b, 0], bm[b, 0], lg[1][b], lg[2][b], lg[3][b], lg[5][b], rho[b], lg[7][b])
        counts = (int(am[b].sum()), len(atoms), int(bm[b].sum()), len(bonds))
        mols.append(ao.assemble_counts(counts, atoms.numpy(), bonds.numpy(), r.numpy(), 512, 16384, 2048))
    records = [parse_graph(a, q) for a, q in notes]
    return notes, records, mols, rows(mols, records, 0)
