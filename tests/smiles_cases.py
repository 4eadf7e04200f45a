"""Test infrastructure, not product: the molecules the SMILES tests share (the example table of DESIGN.md section 7, the seeded random
recipe, the graphs at the limits) as rows of the assembler's layout, and the two graphs a round trip compares."""
import networkx as nx
import numpy as np

SYMBOLS = ("C", "C", "N", "O", "P", "F", "Cl", "S", "Br", "B", "Se", "I", "H", "Si")
MAY_BE_AROMATIC = ("B", "C", "N", "O", "P", "S", "Se")


def rows_of(symbols, bonds, charges=None, implh=()):
    """symbols by name, bonds [(end 1, end 2 (1-based), order)] -> (atoms [(x, y, index, charge, hs)], bonds [(e1, e2, order, source)],
    implh); carbon gets index 1, the other symbols their only index"""
    charges = [0] * len(symbols) if charges is None else charges
    atoms = [(3 * i, 5 * i, SYMBOLS.index(s, 1), q, 0) for i, (s, q) in enumerate(zip(symbols, charges))]
    return atoms, [(e1, e2, order, k) for k, (e1, e2, order) in enumerate(bonds)], list(implh)


def ring(lo, hi, order):
    return [(i, i + 1, order) for i in range(lo, hi)] + [(hi, lo, order)]


def chain(n):
    return rows_of(["C"] * n, [(i, i + 1, 1) for i in range(1, n)])


def star(n):
    """atom 1 bonded to the n - 1 others"""
    return rows_of(["C"] * n, [(1, i, 1) for i in range(2, n + 1)])


def complete(n):
    return rows_of(["C"] * n, [(i, j, 1) for i in range(1, n + 1) for j in range(i + 1, n + 1)])


def ladder(n):
    """two chains of n atoms and a rung between every pair: every rung is open at once"""
    return rows_of(["C"] * (2 * n), [(i, i + 1, 1) for i in range(1, n)] + [(n + i, n + i + 1, 1) for i in range(1, n)]
                   + [(i, n + i, 1) for i in range(1, n + 1)])


# the table of the rule, literally
EXAMPLES = [
    ("benzene", rows_of(["C"] * 6, [(i, i % 6 + 1, 4) for i in range(1, 7)]), "c1ccccc1"),
    ("isobutane", rows_of(["C"] * 4, [(1, 2, 1), (1, 3, 1), (1, 4, 1)]), "C(C)(C)C"),
    ("acetate", rows_of(["C", "C", "O", "O"], [(1, 2, 1), (2, 3, 2), (2, 4, 1)], [0, 0, 0, -1]), "CC(=O)[O-]"),
    ("pyrrole", rows_of(["N", "C", "C", "C", "C"], ring(1, 5, 4), implh=[1]), "[nH]1cccc1"),
    ("toluene", rows_of(["C"] * 7, [(1, 2, 1)] + ring(2, 7, 4)), "Cc1ccccc1"),
    ("biphenyl", rows_of(["C"] * 12, ring(1, 6, 4) + ring(7, 12, 4) + [(1, 7, 1)]), "c1(ccccc1)-c1ccccc1"),
    ("naphthalene", rows_of(["C"] * 10, ring(1, 6, 4) + [(5, 7, 4), (7, 8, 4), (8, 9, 4), (9, 10, 4), (10, 6, 4)]), "c1cccc2c1cccc2"),
    ("spiro[2.2]pentane", rows_of(["C"] * 5, ring(1, 3, 1) + [(1, 4, 1), (4, 5, 1), (5, 1, 1)]), "C12(CC1)CC2"),
    ("silole-like ring", rows_of(["Si", "C", "C", "C", "C"], ring(1, 5, 4)), "[SiH]1:cccc:1"),
    ("cubane", rows_of(["C"] * 8, ring(1, 4, 1) + ring(5, 8, 1) + [(i, i + 4, 1) for i in range(1, 5)]), "C12C3C4C1C1C2C3C41"),
    ("three components", rows_of(["N", "C", "Cl", "Si", "H"], [(1, 2, 5), (4, 5, 1)], [1, 0, -1, 0, 0]), "[NH3+]C.[Cl-].[SiH3][H]"),
]


def random_rows(rng):
    """one graph of the seeded recipe: 1..40 atoms of any vocabulary index, charges of {0, 0, 0, 1, -1}, up to 2 n bonds with no
    pair twice, orders 1..6, ends in either orientation, rows shuffled, 0..3 implicit-H entries"""
    n = int(rng.integers(1, 41))
    atoms = [(int(rng.integers(0, 200)), int(rng.integers(0, 200)), int(rng.integers(0, 14)), int(rng.choice([0, 0, 0, 1, -1])),
              int(rng.integers(0, 3))) for _ in range(n)]
    m = min(int(rng.integers(0, 2 * n + 1)), n * (n - 1) // 2)
    pairs = set()
    while len(pairs) < m:
        i, j = (int(v) for v in rng.integers(1, n + 1, 2))
        if i != j:
            pairs.add((min(i, j), max(i, j)))
    bonds = []
    for i, j in sorted(pairs):
        if rng.integers(0, 2):
            i, j = j, i
        bonds.append((i, j, int(rng.integers(1, 7))))
    rng.shuffle(bonds)
    bonds = [(int(i), int(j), int(o), k) for k, (i, j, o) in enumerate(bonds)]
    implh = [int(v) for v in rng.integers(1, n + 1, int(rng.integers(0, 4)))]
    return atoms, bonds, implh


def graph_of_rows(rows):
    """the graph the rule reads in the rows: nodes (symbol, charge, aromatic by the rule, listed), edges with the order class"""
    atoms, bonds, implh = rows
    g = nx.Graph()
    has4 = [False] * len(atoms)
    for e1, e2, order, _ in bonds:
        cls = 1 if order in (5, 6) else order
        g.add_edge(e1 - 1, e2 - 1, cls=cls)
        if cls == 4:
            has4[e1 - 1] = has4[e2 - 1] = True
    for i, (_, _, t, q, _) in enumerate(atoms):
        g.add_node(i, symbol=SYMBOLS[t], charge=q, aromatic=SYMBOLS[t] in MAY_BE_AROMATIC and has4[i], listed=(i + 1) in implh)
    return g


def graph_of_text(parsed):
    """the graph of smiles_oracle.parse's result: nodes (symbol, charge, aromatic as written, h as written or None)"""
    atoms, bonds = parsed
    g = nx.Graph()
    for i, (symbol, aromatic, charge, h) in enumerate(atoms):
        g.add_node(i, symbol=symbol, charge=charge, aromatic=aromatic, h=h)
    for i, j, cls in bonds:
        g.add_edge(i, j, cls=cls)
    return g


def same_graph(text_graph, rows_graph):
    """an isomorphism that keeps symbol, charge, the aromatic flag and the bond class, and under which every listed atom is written
    with exactly one hydrogen"""
    def node(t, r):
        return (t["symbol"], t["charge"], t["aromatic"]) == (r["symbol"], r["charge"], r["aromatic"]) and (not r["listed"] or t["h"] == 1)
    return nx.is_isomorphic(text_graph, rows_graph, node_match=node, edge_match=lambda a, b: a["cls"] == b["cls"])


def records_of_text(parsed, class_of):
    """parse()'s result as a raster.parse_graph record: atoms int32 [n, 4] (x, y, class, charge), bonds int32 [m, 3] (i < j, order);
    class_of: symbol -> the record's atom class"""
    atoms, bonds = parsed
    a = np.array([(0, 0, class_of[s], q) for s, _, q, _ in atoms], dtype=np.int32).reshape(-1, 4)
    q = np.array(sorted((min(i, j), max(i, j), cls) for i, j, cls in bonds), dtype=np.int32).reshape(-1, 3)
    return a, q
