"""Oracle (test infrastructure, not product): the individualise-and-refine isomorphism test of abc-net_amd/csrc/graph_ident.hip, with
the same budgets and the same counters, so that rows and witness are comparable with the kernel bit for bit.

    identify(gp, gt, max_tries, max_rounds) -> (dict of the search columns, witness in the record's T numbering or None)
    score(mol, atoms, bonds, ...)           -> (the 11 columns of one image as a dict, witness in ORIGINAL record indices or None)
    rows(mols, records, n_valid, ...)       -> int64 [B, 11]
    map_out(mols, records, cap_atoms, ...)  -> int32 [B, cap_atoms], -1 wherever there is no witness
    brute(ga, gb)                           -> networkx is_isomorphic on the labelled multigraphs (independent of everything above)

Graphs, molecules and records are graphsim_oracle's (`of_molecule`, `of_record`), and so are `mix` and id_0: the vectorised uint64
form used for the rounds here is checked against graphsim_oracle.ids in tests/test_graphident_host.py.

The algorithm (include/abcnet_hip.h, abc_graph_identity_desc):
  sizes     atom counts and valid-bond counts differ -> different
  molecule  one path: per level, rounds of the similarity's recurrence (r counts on through the levels) until a round no longer
            raises the class count (that round is counted, at most n per level); the level's (rounds, sum of mix(id), classes) are
            recorded; not discrete: the non-singleton class of the least id VALUE is the cell, its lowest-index member is
            individualised, id = indiv(id, level)
  record    depth first: per level exactly the recorded rounds, then classes and sum must equal the record; candidates are the
            atoms whose id is the recorded cell id, in index order; a failed branch is a backtrack, which replays from level 0
  leaf      map by equal id, verify labels and the multiset of mapped bonds; verified -> same, else on with the search
  budgets   max_rounds before every round of either side, max_tries before every record-side individualisation -> undecided
"""
import numpy as np

import graphsim_oracle as so

COLUMNS = ("counted", "none", "truncated", "size_equal", "same", "different", "undecided", "levels", "tries", "backtracks", "rounds")
DEFAULT_TRIES, DEFAULT_ROUNDS = 4096, 16384      # ABC_IDENT_DEFAULT_TRIES, ABC_IDENT_DEFAULT_ROUNDS
MAX_ATOMS = 512
GOLD = 0x9E3779B97F4A7C15
U = np.uint64


def mixv(x):
    """so.mix on a uint64 array (wrapping)"""
    x = x ^ (x >> U(30))
    x = x * U(0xBF58476D1CE4E5B9)
    x = x ^ (x >> U(27))
    x = x * U(0x94D049BB133111EB)
    return x ^ (x >> U(31))


def indiv(x, level):
    """the id of the atom individualised at `level`"""
    return so.mix(so.mix(int(x)) + GOLD * (level + 1))


class _Side:
    """one graph: id_0 and the bond ends as arrays"""

    def __init__(self, graph):
        classes, _charges, bonds = graph
        self.n = len(classes)
        self.init = np.array(so.ids(graph, 0)[0], dtype=U).reshape(self.n)
        self.i = np.array([q[0] for q in bonds], dtype=np.int64)
        self.j = np.array([q[1] for q in bonds], dtype=np.int64)
        self.o = np.array([q[2] for q in bonds], dtype=U)

    def round(self, ids, r):
        acc = np.zeros(self.n, dtype=U)
        with np.errstate(over="ignore"):
            np.add.at(acc, self.i, mixv(mixv(ids[self.j]) + self.o))
            np.add.at(acc, self.j, mixv(mixv(ids[self.i]) + self.o))
            return mixv(mixv(ids + U(r)) + acc)


def _classes(ids):
    return len(np.unique(ids))


def _sum(ids):
    with np.errstate(over="ignore"):
        return int(np.sum(mixv(ids), dtype=U)) if len(ids) else 0


class _Undecided(Exception):
    pass


def _verify(gp, gt, idp, idt):
    """the witness (molecule atom -> record atom, T numbering) when mapping by equal id preserves every label and every bond"""
    where = {}
    for t, e in enumerate(idt.tolist()):
        where.setdefault(e, []).append(t)
    m = []
    for a, e in enumerate(idp.tolist()):
        ts = where.get(e, [])
        if len(ts) != 1 or gp[0][a] != gt[0][ts[0]] or gp[1][a] != gt[1][ts[0]]:
            return None
        m.append(ts[0])
    key = lambda i, j, o: (min(i, j), max(i, j), o)
    if sorted(key(m[i], m[j], o) for i, j, o in gp[2]) != sorted(key(i, j, o) for i, j, o in gt[2]):
        return None
    return m


def identify(gp, gt, max_tries=DEFAULT_TRIES, max_rounds=DEFAULT_ROUNDS):
    out = dict(size_equal=0, same=0, different=0, undecided=0, levels=0, tries=0, backtracks=0, rounds=0)
    n = len(gp[0])
    if n != len(gt[0]) or len(gp[2]) != len(gt[2]):
        out["different"] = 1
        return out, None
    out["size_equal"] = 1
    P, T = _Side(gp), _Side(gt)

    def step(side, ids, r):
        if out["rounds"] >= max_rounds:
            raise _Undecided
        out["rounds"] += 1
        return side.round(ids, r)

    witness = None
    try:
        # ---- the molecule's one path
        idp, r, level = P.init.copy(), 0, 0
        rec_rounds, rec_sum, rec_classes, rec_cell = [], [], [], []
        prev = _classes(idp)
        while True:
            k = 0
            while True:
                r += 1
                k += 1
                idp = step(P, idp, r)
                c = _classes(idp)
                if c <= prev or k >= n:
                    break
                prev = c
            rec_rounds.append(k)
            rec_sum.append(_sum(idp))
            rec_classes.append(c)
            if c == n:
                break
            vals, counts = np.unique(idp, return_counts=True)
            cell = vals[counts > 1][0]
            rec_cell.append(cell)
            if level + 1 >= n:                       # (only colliding hashes can get here)
                raise _Undecided
            v = int(np.flatnonzero(idp == cell)[0])
            idp[v] = U(indiv(idp[v], level))
            level += 1
            prev = c + 1
        out["levels"] = levels = level

        # ---- the record's search
        choice, nxt = [0] * (levels + 1), [0] * (levels + 1)

        def refine(ids, r, k):
            for _ in range(rec_rounds[k]):
                r += 1
                ids = step(T, ids, r)
            return ids, r

        def replay(upto):
            ids, r = T.init.copy(), 0
            for k in range(upto + 1):
                ids, r = refine(ids, r, k)
                if k < upto:
                    ids[choice[k]] = U(indiv(ids[choice[k]], k))
            return ids, r

        matches = lambda ids, k: _classes(ids) == rec_classes[k] and _sum(ids) == rec_sum[k]
        idt, r = replay(0)
        level, ok = 0, matches(idt, 0)
        while True:
            if ok and level == levels:
                witness = _verify(gp, gt, idp, idt)
                if witness is not None:
                    out["same"] = 1
                    break
                ok = False
            if ok:
                cand = np.flatnonzero(idt == rec_cell[level])
                cand = cand[cand >= nxt[level]]
                if len(cand):
                    if out["tries"] >= max_tries:
                        raise _Undecided
                    out["tries"] += 1
                    v = int(cand[0])
                    choice[level], nxt[level] = v, v + 1
                    idt[v] = U(indiv(idt[v], level))
                    level += 1
                    nxt[level] = 0
                    idt, r = refine(idt, r, level)
                    ok = matches(idt, level)
                    continue
            if level == 0:
                out["different"] = 1
                break
            out["backtracks"] += 1
            level -= 1
            idt, r = replay(level)
            ok = True
    except _Undecided:
        out["undecided"] = 1
        witness = None
    return out, witness


def _t_of(atoms, bonds):
    """the original indices of the record atoms some valid bond row names, in index order (of_record's numbering)"""
    n = len(np.asarray(atoms).reshape(-1, 4))
    rows = [tuple(int(v) for v in q) for q in np.asarray(bonds).reshape(-1, 3)]
    return sorted({e for i, j, _ in rows if 0 <= i < n and 0 <= j < n and i != j for e in (i, j)})


def score(mol, atoms, bonds, max_tries=DEFAULT_TRIES, max_rounds=DEFAULT_ROUNDS):
    out = dict.fromkeys(COLUMNS, 0)
    out["counted"] = 1
    if mol is None:
        out["none"] = 1
        return out, None
    out["truncated"] = int(bool(so._get(mol, "truncated")))
    res, witness = identify(so.of_molecule(mol), so.of_record(atoms, bonds), max_tries, max_rounds)
    out.update(res)
    if witness is not None:
        T = _t_of(atoms, bonds)
        witness = [T[t] for t in witness]
    return out, witness


_EMPTY = (np.zeros((0, 4), dtype=np.int32), np.zeros((0, 3), dtype=np.int32))


def rows_and_maps(mols, records, cap_atoms, n_valid=None, **budgets):
    """(int64 [B, 11], int32 [B, cap_atoms]): records may be shorter than mols (the rest are empty records); rows at or past n_valid
    are zero and their maps -1"""
    B = len(mols)
    n_valid = B if n_valid is None else n_valid
    out = np.zeros((B, len(COLUMNS)), dtype=np.int64)
    maps = np.full((B, cap_atoms), -1, dtype=np.int32)
    for b in range(min(B, n_valid)):
        a, q = records[b] if b < len(records) else _EMPTY
        s, w = score(mols[b], a, q, **budgets)
        out[b] = [s[c] for c in COLUMNS]
        if w is not None:
            maps[b, :len(w)] = w
    return out, maps


def rows(mols, records, n_valid=None, **budgets):
    return rows_and_maps(mols, records, MAX_ATOMS, n_valid, **budgets)[0]


def map_out(mols, records, cap_atoms, n_valid=None, **budgets):
    return rows_and_maps(mols, records, cap_atoms, n_valid, **budgets)[1]


# ---------------------------------------------------------------------------------------------------------------- fixtures
def union(a, b):
    """the disjoint union of two records"""
    na = len(a[0])
    return list(a[0]) + list(b[0]), list(a[1]) + [(i + na, j + na, c) for i, j, c in b[1]]


# Two refinement-equal, non-isomorphic components: every atom of the first cell is a candidate, and the ones in the wrong component
# fail only after their level's rounds.  UNION_PERMUTED is so.permuted(RandomState(2), UNION), its rows committed here: against UNION
# the search takes levels 5, tries 7, backtracks 2, rounds 46.
UNION = union(so.DECALIN, so.BICYCLOPENTYL)
UNION_PERMUTED = ([(0, 0, 1, 0)] * 20,
                  [(16, 14, 1), (2, 14, 1), (18, 0, 1), (17, 1, 1), (11, 7, 1), (12, 17, 1), (19, 13, 1), (12, 4, 1), (6, 7, 1), (11, 2, 1),
                   (18, 4, 1), (19, 6, 1), (15, 13, 1), (6, 8, 1), (15, 8, 1), (16, 7, 1), (17, 9, 1), (9, 5, 1), (10, 3, 1), (0, 9, 1),
                   (10, 1, 1), (3, 5, 1)])
UNION_COUNTERS = dict(levels=5, tries=7, backtracks=2, rounds=46)


def carbon_ring(n, order=1):
    return so.record([1] * n, [(k, k + 1, order) for k in range(n - 1)] + [(0, n - 1, order)])


def carbon_chain(n):
    return so.record([1] * n, [(k, k + 1, 1) for k in range(n - 1)])


def propanes(count):
    """`count` disjoint C-C-C fragments"""
    return so.record([1] * (3 * count), [e for k in range(count) for e in ((3 * k, 3 * k + 1, 1), (3 * k + 1, 3 * k + 2, 1))])


def random_pairs(count, seed):
    """(molecule rows, record) pairs, n = 2..12: a permuted copy (k % 4 in (0, 3)), a permuted copy with one atom changed (1),
    another random graph of the same size (2)"""
    rng = np.random.RandomState(seed)
    for k in range(count):
        n = int(rng.randint(2, 13))
        a = so.random_graph(rng, n, extra=int(rng.randint(0, 4)))
        if k % 4 == 1:
            b = so.one_atom_changed(rng, so.permuted(rng, a))
        elif k % 4 == 2:
            b = so.random_graph(rng, n, extra=int(rng.randint(0, 4)))
        else:
            b = so.permuted(rng, a)
        yield so.as_mol(b), a


# ------------------------------------------------------------------------------------------------------- independent checks
def nx_graph(graph):
    """the labelled multigraph of a normalised graph (the recipe of test_graphsim_host._nx_graph)"""
    import networkx as nx
    classes, charges, bonds = graph
    g = nx.MultiGraph()
    for a, (t, c) in enumerate(zip(classes, charges)):
        g.add_node(a, label=(t, c))
    for i, j, o in bonds:
        g.add_edge(i, j, order=o)
    return g


def brute(ga, gb):
    import networkx as nx
    iso = nx.algorithms.isomorphism
    return nx.is_isomorphic(nx_graph(ga), nx_graph(gb), node_match=iso.categorical_node_match("label", None),
                            edge_match=iso.categorical_multiedge_match("order", None))
