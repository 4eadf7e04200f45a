"""Oracle (test infrastructure, not product): the environment similarity of abc-net_amd/csrc/graph_sim.hip, twice.

    ids(graph, rounds)            -> the uint64 recurrence of include/abcnet_hip.h in Python ints: [id_0, .., id_rounds], a list per atom
    structural(g1, g2, rounds)    -> the same environments WITHOUT a hash: nested sorted tuples, every distinct tuple numbered through
                                     one table shared by the two graphs (equal numbers <=> equal tuples)
    score(mol, atoms, bonds)      -> the 12 columns of one image, as a dict, built on ids()
    rows(mols, records, n_valid)  -> int [B, 12]
    fingerprint(graph)            -> the flat list ids_out holds for one side: id_r of atom a at r * n + a, r = 0 .. 3

A graph is (classes [n], charges [n], bonds [(a, j, order class)]) after the normalisation both sides share: `of_molecule`
(every atom takes part) and `of_record` (only the atoms a valid bond row names, renumbered in index order).

`mol` is None (ABC_MOL_EMPTY), a dict of hand-made rows {"atoms": [(x, y, vocabulary index, charge)], "bonds": [(end 1, end 2
(1-based), order)], "truncated"}, or anything with symbols / charges / bonds (1-based) / orders / truncated (a decode.Molecule).
"""
import numpy as np

COLUMNS = ("counted", "none", "truncated", "size_equal", "refine_equal", "dice_one", "atoms_pred", "atoms_true", "envs_pred",
           "envs_true", "envs_common", "dice_q20")
ATOM_SYMBOLS = ("C", "C", "N", "O", "P", "F", "Cl", "S", "Br", "B", "Se", "I", "H", "Si")
RADIUS, MAX_ROUNDS, IDS = 3, 64, 2048
M64 = (1 << 64) - 1


def mix(x):
    """the splitmix64 finaliser"""
    x &= M64
    x ^= x >> 30
    x = (x * 0xBF58476D1CE4E5B9) & M64
    x ^= x >> 27
    x = (x * 0x94D049BB133111EB) & M64
    x ^= x >> 31
    return x


def atom_class(t):
    t = int(t)
    return 0 if t < 0 or t > 13 else (1 if t == 0 else t)


def bond_class(c):
    c = int(c)
    return 1 if c in (5, 6) else (c if 1 <= c <= 4 else 0)


def _get(mol, key):
    return mol[key] if isinstance(mol, dict) else getattr(mol, key)


def of_molecule(mol):
    """every atom takes part; a bond row with an end out of range, or both ends on one atom, is skipped"""
    if isinstance(mol, dict) and "atoms" in mol:
        classes = [atom_class(a[2]) for a in mol["atoms"]]
        charges = [int(a[3]) for a in mol["atoms"]]
        rows = [(int(q[0]), int(q[1]), int(q[2])) for q in mol["bonds"]]
    else:
        classes = [atom_class(ATOM_SYMBOLS.index(s)) for s in _get(mol, "symbols")]
        charges = [int(c) for c in _get(mol, "charges")]
        rows = [(int(q[0]), int(q[1]), int(o)) for q, o in zip(_get(mol, "bonds"), _get(mol, "orders"))]
    n = len(classes)
    bonds = [(i - 1, j - 1, bond_class(o)) for i, j, o in rows if 1 <= i <= n and 1 <= j <= n and i != j]
    return classes, charges, bonds


def of_record(atoms, bonds):
    """only the atoms some valid bond row names take part, in index order"""
    atoms = [tuple(int(v) for v in a) for a in np.asarray(atoms).reshape(-1, 4)]
    rows = [tuple(int(v) for v in q) for q in np.asarray(bonds).reshape(-1, 3)]
    n = len(atoms)
    rows = [(i, j, c) for i, j, c in rows if 0 <= i < n and 0 <= j < n and i != j]
    T = sorted({i for i, _, _ in rows} | {j for _, j, _ in rows})
    num = {a: k for k, a in enumerate(T)}
    return [atom_class(atoms[a][2]) for a in T], [atoms[a][3] for a in T], [(num[i], num[j], bond_class(c)) for i, j, c in rows]


def _ends(n, bonds):
    """per atom: (neighbour, order class) of every bond end (a pair listed twice appears twice)"""
    nb = [[] for _ in range(n)]
    for i, j, o in bonds:
        nb[i].append((j, o))
        nb[j].append((i, o))
    return nb


def ids(graph, rounds=RADIUS):
    classes, charges, bonds = graph
    n = len(classes)
    nb = _ends(n, bonds)
    layer = [mix(mix(mix(classes[a] + 1) + (charges[a] & M64)) + len(nb[a])) for a in range(n)]
    out = [layer]
    for r in range(1, rounds + 1):
        acc = [sum(mix(mix(layer[j]) + o) for j, o in nb[a]) & M64 for a in range(n)]
        layer = [mix(mix(layer[a] + r) + acc[a]) for a in range(n)]
        out.append(layer)
    return out


def structural(g1, g2, rounds=RADIUS):
    """([layer_0, ..], [layer_0, ..]) for the two graphs: the number of atom a's radius-r environment, equal exactly where the
    nested tuples (r, own environment, sorted (order class, neighbour's environment) pairs) are equal"""
    table = {}
    number = lambda key: table.setdefault(key, len(table))
    sides = []
    for classes, charges, bonds in (g1, g2):
        nb = _ends(len(classes), bonds)
        sides.append((nb, [[number((0, classes[a], charges[a], len(nb[a]))) for a in range(len(classes))]]))
    for r in range(1, rounds + 1):
        for nb, layers in sides:
            prev = layers[-1]
            layers.append([number((r, prev[a], tuple(sorted((o, prev[j]) for j, o in nb[a])))) for a in range(len(prev))])
    return sides[0][1], sides[1][1]


def common(A, B):
    """the size of the multiset intersection"""
    count = {}
    for e in B:
        count[e] = count.get(e, 0) + 1
    c = 0
    for e in A:
        if count.get(e, 0) > 0:
            count[e] -= 1
            c += 1
    return c


def flat(layers, upto=RADIUS):
    return [e for layer in layers[:upto + 1] for e in layer]


def fingerprint(graph):
    return flat(ids(graph))


def counts(layers_p, layers_t):
    """(envs_common, envs_pred, envs_true) of two lists of layers"""
    A, B = flat(layers_p), flat(layers_t)
    return common(A, B), len(A), len(B)


def refine_equal(gp, gt, layers=ids):
    """equal atom counts, equal valid bond counts, and equal multisets of id_T after T = min(n, 64) rounds"""
    n = len(gp[0])
    if n != len(gt[0]) or len(gp[2]) != len(gt[2]):
        return 0
    T = min(n, MAX_ROUNDS)
    if layers is ids:
        A, B = ids(gp, T)[T], ids(gt, T)[T]
    else:
        A, B = (side[T] for side in structural(gp, gt, T))
    return int(sorted(A) == sorted(B))


def score(mol, atoms, bonds):
    out = dict.fromkeys(COLUMNS, 0)
    gt = of_record(atoms, bonds)
    out["counted"], out["envs_true"] = 1, (RADIUS + 1) * len(gt[0])
    if mol is None:
        out["none"] = 1
        return out
    gp = of_molecule(mol)
    c, p, t = counts(ids(gp), ids(gt))
    out["truncated"] = int(bool(_get(mol, "truncated")))
    out["size_equal"] = int(len(gp[0]) == len(gt[0]) and len(gp[2]) == len(gt[2]))
    out["refine_equal"] = refine_equal(gp, gt)
    out["dice_one"] = int(c == p == t > 0)
    out["atoms_pred"], out["atoms_true"] = len(gp[0]), len(gt[0])
    out["envs_pred"], out["envs_common"] = p, c
    out["dice_q20"] = (2 * c << 20) // (p + t) if p + t else 0
    return out


def rows(mols, records, n_valid=None):
    """int64 [B, 12]: B = len(mols); records may be shorter (the rest are empty records); rows at or past n_valid are zero"""
    B = len(mols)
    n_valid = B if n_valid is None else n_valid
    out = np.zeros((B, len(COLUMNS)), dtype=np.int64)
    empty = (np.zeros((0, 4), dtype=np.int32), np.zeros((0, 3), dtype=np.int32))
    for b in range(min(B, n_valid)):
        a, q = records[b] if b < len(records) else empty
        s = score(mols[b], a, q)
        out[b] = [s[c] for c in COLUMNS]
    return out


def ids_out(mols, records, n_valid=None):
    """uint64 [B, 2, 2048] as abc_graph_similarity_desc.ids_out holds it for the images below n_valid (zero elsewhere here)"""
    B = len(mols)
    out = np.zeros((B, 2, IDS), dtype=np.uint64)
    for b in range(B if n_valid is None else min(B, n_valid)):
        a, q = records[b] if b < len(records) else ([], [])
        for side, g in ((0, None if mols[b] is None else of_molecule(mols[b])), (1, of_record(a, q))):
            if g is not None:
                f = fingerprint(g)
                out[b, side, :len(f)] = np.array(f, dtype=np.uint64)
    return out


# ------------------------------------------------------------------------------------------------------------------- molecules
def mol(classes, bonds, charges=None, truncated=False):
    """hand-made rows from vocabulary indices and 1-based (end, end, order) rows; the cells are never read"""
    charges = [0] * len(classes) if charges is None else charges
    return dict(atoms=[(0, 0, t, c) for t, c in zip(classes, charges)], bonds=[tuple(q) for q in bonds], truncated=truncated)


def record(classes, bonds, charges=None):
    """a record from vocabulary indices (-1: outside the vocabulary) and 0-based (i, j, code) rows"""
    charges = [0] * len(classes) if charges is None else charges
    return ([(0, 0, t, c) for t, c in zip(classes, charges)], [tuple(q) for q in bonds])


def as_mol(rec):
    """the molecule rows that say what a record says (an unknown element becomes vocabulary index 99: class 0 too)"""
    atoms, bonds = rec
    return dict(atoms=[(a[0], a[1], 99 if a[2] < 0 else a[2], a[3]) for a in atoms], bonds=[(i + 1, j + 1, c) for i, j, c in bonds],
                truncated=False)


DECALIN = record([1] * 10, [(i, i + 1, 1) for i in range(9)] + [(0, 9, 1), (4, 9, 1)])          # two fused six-rings
BICYCLOPENTYL = record([1] * 10, [(0, 1, 1), (1, 2, 1), (2, 3, 1), (3, 4, 1), (0, 4, 1), (5, 6, 1), (6, 7, 1), (7, 8, 1), (8, 9, 1),
                                  (5, 9, 1), (0, 5, 1)])                                         # two five-rings joined by a bond


def random_graph(rng, n, extra=2):
    """a random tree on n atoms plus `extra` more edges (a repeated pair now and then), mixed classes, charges and orders"""
    classes = [int(rng.choice([1, 1, 1, 2, 3, 6, 7, -1])) for _ in range(n)]
    charges = [int(rng.choice([0, 0, 0, 0, 1, -1])) for _ in range(n)]
    bonds = [(int(rng.randint(0, k)), k, int(rng.randint(1, 7))) for k in range(1, n)]
    for _ in range(extra if n > 2 else 0):
        i, j = sorted(int(v) for v in rng.choice(n, size=2, replace=False))
        bonds.append((i, j, int(rng.randint(1, 7))))
    return record(classes, bonds, charges)


def one_atom_changed(rng, rec):
    atoms, bonds = rec
    atoms = list(atoms)
    k = int(rng.randint(len(atoms)))
    x, y, t, c = atoms[k]
    atoms[k] = (x, y, 2 if t != 2 else 3, c) if rng.rand() < 0.5 else (x, y, t, c + 1)
    return atoms, list(bonds)


def permuted(rng, rec):
    """the same graph with its atoms renumbered, its bond rows in another order and their ends swapped at random"""
    atoms, bonds = rec
    n = len(atoms)
    perm = rng.permutation(n)                       # old index -> new index
    new_atoms = [None] * n
    for old, new in enumerate(perm):
        new_atoms[new] = atoms[old]
    new_bonds = []
    for k in rng.permutation(len(bonds)):
        i, j, c = bonds[k]
        e = (int(perm[i]), int(perm[j]))
        new_bonds.append((e if rng.rand() < 0.5 else e[::-1]) + (c,))
    return new_atoms, new_bonds
