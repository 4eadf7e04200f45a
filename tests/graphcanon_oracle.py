"""Oracle (test infrastructure, not product): the canonical atom order of abc-net_amd/csrc/graph_canon.hip.

The pruned search -- the statement of record, with the kernel's budgets and counters -- is decode.canonical_labelling (the host form
Molecule.canonical() runs; product code may import nothing from tests, so it lives there and is re-exported here).  What this module
adds is everything the search is held against:

    brute(graph)                      -> (key, certificate) of the least leaf over the WHOLE tree: no pruning, no budget, its own
                                         refinement in Python ints (nothing shared with the search but the definitions of mix, id_0,
                                         the round, indiv and the leaf hash)
    canon(graph, ...)                 -> dict(rank, stats, key, cert) of the pruned search
    of_molecule / of_record           -> the graph (classes, charges, bonds, tags) of rows / of a record, graphsim_oracle's plus tags
    outputs(graphs, ...)              -> order, stats, key, cert_out as abc_canonical_order writes them
    canonical_rows(mol, ...)          -> the canonical rows of one image as arrays

The tree (include/abcnet_hip.h, abc_canon_desc): a node is a sequence of individualised atoms; per level, rounds until one no longer
raises the class count, the trace (rounds, classes, sum of mix(id)), then the next atom is individualised; the target cell is the
non-singleton class of the least id value, its atoms in index order are the children; a leaf is a discrete colouring, its key
(trace_0, trace_1, .., h); the canonical leaf is the least.
"""
import numpy as np

import abcnet_amd  # noqa: F401
from abcnet_amd import decode as D

import graphsim_oracle as so

COLUMNS = D.CANON_COLUMNS
EMPTY, TRUNCATED, UNDECIDED, COLLISION = D.CANON_EMPTY, D.CANON_TRUNCATED, D.CANON_UNDECIDED, D.CANON_COLLISION
DEFAULT_TRIES, DEFAULT_ROUNDS, ORBIT_LEVELS = D.CANON_DEFAULT_TRIES, D.CANON_DEFAULT_ROUNDS, D.CANON_ORBIT_LEVELS
M64 = (1 << 64) - 1
mix = so.mix


# ------------------------------------------------------------------------------------------------------------------- graphs
def of_molecule(mol):
    """graphsim_oracle.of_molecule plus the tags: 1 for an atom that mol["implh"] (1-based, optional) lists"""
    classes, charges, bonds = so.of_molecule(mol)
    tags = [0] * len(classes)
    for a in (mol.get("implh", ()) if isinstance(mol, dict) else so._get(mol, "implicit_hs")):
        if 1 <= a <= len(classes):
            tags[a - 1] = 1
    return classes, charges, bonds, tags


def of_record(atoms, bonds):
    """(graph, T): graphsim_oracle.of_record with all tags 0, and the original index of every atom of the graph"""
    classes, charges, rows = so.of_record(atoms, bonds)
    n = len(np.asarray(atoms).reshape(-1, 4))
    valid = [tuple(int(v) for v in q) for q in np.asarray(bonds).reshape(-1, 3)]
    T = sorted({e for i, j, _ in valid if 0 <= i < n and 0 <= j < n and i != j for e in (i, j)})
    return (classes, charges, rows, [0] * len(classes)), T


def canon(graph, max_tries=DEFAULT_TRIES, max_rounds=DEFAULT_ROUNDS):
    rank, st, traces = D.canonical_labelling(graph, max_tries, max_rounds)
    return dict(rank=rank, stats=st, key=D.canon_key(graph, rank, traces), cert=D.canon_certificate(graph, rank), traces=traces)


# -------------------------------------------------------------------------------------------------------------- brute force
def _id0(graph):
    classes, charges, bonds, tags = graph
    deg = [0] * len(classes)
    for i, j, _ in bonds:
        deg[i] += 1
        deg[j] += 1
    out = []
    for a in range(len(classes)):
        e = mix(mix(mix(classes[a] + 1) + (charges[a] & M64)) + deg[a])
        out.append(mix(e + 0xD6E8FEB86659FD93 * tags[a]) if tags[a] else e)
    return out


def _round(graph, ids, r):
    acc = [0] * len(ids)
    for i, j, o in graph[2]:
        acc[i] += mix(mix(ids[j]) + o)
        acc[j] += mix(mix(ids[i]) + o)
    return [mix(mix(ids[a] + r) + (acc[a] & M64)) for a in range(len(ids))]


def brute(graph):
    """(key, certificate) of the least leaf of the whole tree; key = (trace_0, .., (h,))"""
    n = len(graph[0])
    if n == 0:
        return (), D.canon_certificate(graph, [])
    best = [None, None]

    def node(ids, r, level, prev, traces):
        k = 0
        while True:
            r, k = r + 1, k + 1
            ids = _round(graph, ids, r)
            c = len(set(ids))
            if c <= prev or k >= n:
                break
            prev = c
        traces = traces + ((k, c, sum(mix(e) for e in ids) & M64),)
        if c == n:
            rank = [sorted(ids).index(e) for e in ids]
            key = traces + ((D.canon_leaf_hash(graph, rank),),)
            if best[0] is None or key < best[0]:
                best[0], best[1] = key, rank
            return
        cell = min(e for e in ids if ids.count(e) > 1)
        for v in range(n):
            if ids[v] == cell:
                child = list(ids)
                child[v] = mix(mix(child[v]) + 0x9E3779B97F4A7C15 * (level + 1))
                node(child, r, level + 1, c + 1, traces)

    ids = _id0(graph)
    node(ids, 0, 0, len(set(ids)), ())
    return best[0], D.canon_certificate(graph, best[1])


def leaf_key(res):
    """the key of canon()'s leaf in brute()'s form"""
    return tuple(res["traces"]) + ((res["key"][0],),) if res["traces"] else ()


# ------------------------------------------------------------------------------------------------------ the device's outputs
def _signed(x):
    return x - (1 << 64) if x >> 63 else x


def outputs(images, cap_atoms, cap_bonds, **budgets):
    """images: per image None (EMPTY), or (graph, original index of every atom, truncated) -> order int32 [B, cap_atoms], stats int32
    [B, 9], key int64 [B, 2], cert int32 [B, 2 + cap_atoms + 3 cap_bonds]"""
    B = len(images)
    order = np.full((B, cap_atoms), -1, dtype=np.int32)
    stats = np.zeros((B, len(COLUMNS)), dtype=np.int32)
    key = np.zeros((B, 2), dtype=np.int64)
    cert = np.full((B, 2 + cap_atoms + 3 * cap_bonds), -1, dtype=np.int32)
    for b, im in enumerate(images):
        if im is None:
            stats[b, 0] = EMPTY | TRUNCATED                          # (molrows.upload_molecules gives an empty image both bits)
            cert[b, :2] = 0
            continue
        graph, orig, truncated = im
        res = canon(graph, **budgets)
        for a, k in enumerate(res["rank"]):
            order[b, k] = orig[a]
        stats[b] = [res["stats"][c] for c in COLUMNS]
        stats[b, 0] |= TRUNCATED if truncated else 0
        key[b] = [_signed(res["key"][0]), _signed(res["key"][1])]
        cert[b, :len(res["cert"])] = res["cert"]
    return order, stats, key, cert


def molecule_image(mol):
    if mol is None:
        return None
    g = of_molecule(mol)
    return g, list(range(len(g[0]))), bool(so._get(mol, "truncated"))


def record_image(rec):
    g, T = of_record(*rec)
    return g, T, False


def canonical_rows(mol, cap_atoms, cap_mol_bonds, **budgets):
    """(mol_counts [4], mol_atoms [cap_atoms, 5], mol_bonds [cap_mol_bonds, 4], mol_implh [cap_atoms]) of one uploaded image
    (molrows.upload_molecules: hs = -1, source = row index, no implicit H unless mol["implh"]): zero past the counts"""
    atoms = np.zeros((cap_atoms, 5), dtype=np.int32)
    bonds = np.zeros((cap_mol_bonds, 4), dtype=np.int32)
    implh = np.zeros(cap_atoms, dtype=np.int32)
    if mol is None:
        return np.array([3, 2, 0, EMPTY | TRUNCATED], dtype=np.int32), atoms, bonds, implh
    listed = list(mol.get("implh", ()))
    cnt = np.array([len(mol["atoms"]), len(mol["bonds"]), len(listed), TRUNCATED if mol["truncated"] else 0], dtype=np.int32)
    rank = canon(of_molecule(mol), **budgets)["rank"]
    n = len(rank)
    for a, t in enumerate(mol["atoms"]):
        atoms[rank[a]] = (t[0], t[1], t[2], t[3], -1)
    valid, rest = [], []
    for q, (e1, e2, o) in enumerate(mol["bonds"]):
        if 1 <= e1 <= n and 1 <= e2 <= n and e1 != e2:
            f1, f2 = rank[e1 - 1] + 1, rank[e2 - 1] + 1
            valid.append((min(f1, f2), max(f1, f2), q, (f1, f2, o, q)))
        else:
            rest.append((e1, e2, o, q))
    for k, row in enumerate([v[3] for v in sorted(valid)] + rest):
        bonds[k] = row
    out = sorted(rank[a - 1] + 1 for a in listed if 1 <= a <= n) + [a for a in listed if not 1 <= a <= n]
    implh[:len(out)] = out
    return cnt, atoms, bonds, implh


# ---------------------------------------------------------------------------------------------------------------- fixtures
def ring(n, order=1, cls=1):
    return so.record([cls] * n, [(k, (k + 1) % n, order) for k in range(n)])


BENZENE = ring(6, order=4)
CUBANE = so.record([1] * 8, [(0, 1, 1), (1, 2, 1), (2, 3, 1), (0, 3, 1), (4, 5, 1), (5, 6, 1), (6, 7, 1), (4, 7, 1),
                             (0, 4, 1), (1, 5, 1), (2, 6, 1), (3, 7, 1)])
PRISMANE = so.record([1] * 6, [(0, 1, 1), (1, 2, 1), (0, 2, 1), (3, 4, 1), (4, 5, 1), (3, 5, 1), (0, 3, 1), (1, 4, 1), (2, 5, 1)])
PETERSEN = so.record([1] * 10, [(k, (k + 1) % 5, 1) for k in range(5)] + [(k, k + 5, 1) for k in range(5)]
                     + [(5 + k, 5 + (k + 2) % 5, 1) for k in range(5)])
K4 = so.record([1] * 4, [(i, j, 1) for i in range(4) for j in range(i + 1, 4)])
TERT_BUTYL_X2 = so.record([1] * 8, [(0, 1, 1), (0, 2, 1), (0, 3, 1), (0, 4, 1), (1, 5, 1), (1, 6, 1), (1, 7, 1)])      # two tert-butyl groups, joined
HUB = so.record([2] + [1] * 40, [(0, k, 1 + k % 4) for k in range(1, 41)])


def union(a, b):
    na = len(a[0])
    return list(a[0]) + list(b[0]), list(a[1]) + [(i + na, j + na, c) for i, j, c in b[1]]


def benzenes(count):
    out = BENZENE
    for _ in range(count - 1):
        out = union(out, BENZENE)
    return out


UNION = union(so.DECALIN, so.BICYCLOPENTYL)
NAMED = (("benzene", BENZENE), ("cubane", CUBANE), ("prismane", PRISMANE), ("petersen", PETERSEN), ("k4", K4),
         ("two benzenes", benzenes(2)), ("tert-butyl x 2", TERT_BUTYL_X2), ("union", UNION),
         ("decalin", so.DECALIN), ("bicyclopentyl", so.BICYCLOPENTYL))


def record_graph(rec):
    return of_record(*rec)[0]
