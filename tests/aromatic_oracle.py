"""Test infrastructure, not product: the aromaticity rule of DESIGN.md section 7 (include/abcnet_hip.h, abc_aromatic_desc) written a
second time, straight from the rule's text and over networkx's cycle enumeration (`perceive`; it shares no code with
abcnet_amd.decode), the rule's example table, and the graphs the host and GPU tests of the perception share."""
import networkx as nx
import numpy as np

from smiles_oracle import SYMBOLS, VALENCES

COLUMNS = ("status", "candidates", "cycles", "aromatic", "rows_changed", "listed")
NOT_CANDIDATE, NONE = -2, -1
RING_SYMBOLS = {"B", "C", "N", "O", "P", "S", "Se"}
CLASS = {1: 1, 2: 2, 3: 3, 4: 4, 5: 1, 6: 1}


def perceive(symbols, charges, rows):
    """symbols [n] (None: no symbol), charges [n], rows [(i, j, order code)] 0-based -> (orders [m], codes [n], counts dict)"""
    n = len(symbols)
    valid = {q: (i, j, CLASS.get(o, 0)) for q, (i, j, o) in enumerate(rows) if 0 <= i < n and 0 <= j < n and i != j}
    at = {a: [] for a in range(n)}       # atom -> [(row, other end, class)]
    for q, (i, j, c) in valid.items():
        at[i].append((q, j, c))
        at[j].append((q, i, c))
    cand = set()
    for a in range(n):
        cs, others = [c for _, _, c in at[a]], [y for _, y, _ in at[a]]
        if (symbols[a] in RING_SYMBOLS and charges[a] in (-1, 0, 1) and len(cs) in (2, 3) and not set(cs) & {0, 3} and cs.count(2) <= 1
                and len(set(others)) == len(others)):
            cand.add(a)
    G = nx.Graph()
    G.add_nodes_from(cand)
    for q, (i, j, c) in valid.items():
        if i in cand and j in cand:
            G.add_edge(i, j, row=q)
    cycles = [c for c in nx.simple_cycles(G, length_bound=7) if len(c) >= 5]
    edges = lambda c: [G[u][v]["row"] for u, v in zip(c, c[1:] + c[:1])]
    ring = set(q for c in cycles for q in edges(c))

    def e(a):
        s, z, d = symbols[a], charges[a], len(at[a])
        for q, y, c in at[a]:
            if c == 2:
                if q in ring:
                    return 1
                return 0 if symbols[y] in ("N", "O", "S", "Se") else NONE
        has4 = any(c == 4 for _, _, c in at[a])
        table = {
            "C": {0: 1 if has4 else NONE, -1: 2, 1: 0},
            "B": {0: 0, -1: NONE, 1: NONE},
            "N": {-1: 2, 1: 1 if has4 else NONE, 0: (2 if d == 3 else 1) if has4 else 2},
            "O": {0: 2, -1: NONE, 1: NONE},
        }
        return table[{"P": "N", "S": "O", "Se": "O"}.get(s, s)][z]

    codes = [e(a) if a in cand else NOT_CANDIDATE for a in range(n)]
    aromatic = [c for c in cycles if NONE not in [codes[a] for a in c] and sum(codes[a] for a in c) == 6]
    marked = set(q for c in aromatic for q in edges(c))
    orders = [4 if q in marked else o for q, (_, _, o) in enumerate(rows)]
    counts = dict(candidates=len(cand), cycles=len(cycles), aromatic=len(aromatic), rows_changed=sum(o != rows[q][2] for q, o in enumerate(orders)))
    return orders, codes, counts


def hydrogens(symbol, charge, classes):
    """the text rule's h of an unlisted atom, from smiles_oracle's own valence lists"""
    if symbol == "H" or abs(charge) > 1 or symbol not in VALENCES:
        return 0
    v = sum(3 if c == 4 else 2 * c for c in classes) // 2
    for t in VALENCES[symbol][charge]:
        if t >= v:
            return t - v
    return 0


def perceive_rows(rows):
    """rows = (atoms [(x, y, vocabulary index, charge, hs)], bonds [(end 1, end 2, order, source)] 1-based, implh) -> (rows with the
    perceived orders and the appended list, codes, counts with `listed`)"""
    atoms, bonds, implh = rows
    n = len(atoms)
    symbols = [SYMBOLS[a[2]] if 0 <= a[2] < len(SYMBOLS) else None for a in atoms]
    charges = [a[3] for a in atoms]
    orders, codes, counts = perceive(symbols, charges, [(q[0] - 1, q[1] - 1, q[2]) for q in bonds])
    new = []
    for a in range(n):
        if (a + 1) in implh:
            continue
        mine = [(CLASS.get(q[2], 0), CLASS.get(o, 0)) for q, o in zip(bonds, orders)
                if a + 1 in (q[0], q[1]) and 1 <= q[0] <= n and 1 <= q[1] <= n and q[0] != q[1]]
        if hydrogens(symbols[a], charges[a], [c for c, _ in mine]) == 1 and hydrogens(symbols[a], charges[a], [c for _, c in mine]) == 0:
            new.append(a + 1)
    counts["listed"] = len(new)
    out = (list(atoms), [(q[0], q[1], o, q[3]) for q, o in zip(bonds, orders)], list(implh) + new)
    return out, codes, counts


# ----------------------------------------------------------------------------------------------------------------- the graphs
def rows_of(symbols, bonds, charges=None, implh=()):
    """(atoms, bonds, implh) in the assembler's layout from symbols and (end 1, end 2, order) 1-based triples"""
    charges = charges or [0] * len(symbols)
    atoms = [(3 * i, 5 * i, SYMBOLS.index(s) if s != "C" else 1, q, 0) for i, (s, q) in enumerate(zip(symbols, charges))]
    return atoms, [(i, j, o, k) for k, (i, j, o) in enumerate(bonds)], list(implh)


def ring(orders, first=1):
    """the bonds i -- i + 1 of a ring whose atoms are first .. first + len(orders) - 1"""
    n = len(orders)
    return [(first + i, first + (i + 1) % n, o) for i, o in enumerate(orders)]


K5, K6, K7 = [1, 2, 1, 2, 1], [2, 1, 2, 1, 2, 1], [1, 2, 1, 2, 1, 2, 1]
# indole: the five-ring N1 C2 C3 C4(3a) C9(7a), the six-ring C4 .. C9; naphthalene: 1 .. 10 around, 5 -- 10 across (atoms 5 and 10 fused)
INDOLE_SKELETON = [(1, 2), (2, 3), (3, 4), (4, 9), (9, 1), (4, 5), (5, 6), (6, 7), (7, 8), (8, 9)]
NAPHTHALENE_SKELETON = [(i, i + 1) for i in range(1, 10)] + [(10, 1), (5, 10)]


def with_doubles(skeleton, doubles):
    return [(i, j, 2 if (i, j) in doubles or (j, i) in doubles else 1) for i, j in skeleton]


# name, rows, the expected orders (None: unchanged), the atoms appended to the list
EXAMPLES = [
    ("benzene", rows_of(["C"] * 6, ring(K6)), [4] * 6, []),
    ("pyridine", rows_of(["N"] + ["C"] * 5, ring(K6)), [4] * 6, []),
    ("pyrrole", rows_of(["N"] + ["C"] * 4, ring(K5)), [4] * 5, [1]),
    ("furan", rows_of(["O"] + ["C"] * 4, ring(K5)), [4] * 5, []),
    ("thiophene", rows_of(["S"] + ["C"] * 4, ring(K5)), [4] * 5, []),
    ("cyclopentadienyl anion", rows_of(["C"] * 5, ring(K5), [-1, 0, 0, 0, 0]), [4] * 5, [1]),
    ("tropylium", rows_of(["C"] * 7, ring(K7), [1, 0, 0, 0, 0, 0, 0]), [4] * 7, [1]),
    # N1 C2(=O7) C3=C4 C5=C6
    ("2-pyridone", rows_of(["N", "C", "C", "C", "C", "C", "O"], ring([1, 1, 2, 1, 2, 1]) + [(2, 7, 2)]), [4] * 6 + [2], [1]),
    ("indole, form 1", rows_of(["N"] + ["C"] * 8, with_doubles(INDOLE_SKELETON, {(2, 3), (4, 9), (5, 6), (7, 8)})), [4] * 10, [1]),
    ("indole, form 2", rows_of(["N"] + ["C"] * 8, with_doubles(INDOLE_SKELETON, {(2, 3), (4, 5), (6, 7), (8, 9)})), [4] * 10, [1]),
    ("naphthalene, form 1", rows_of(["C"] * 10, with_doubles(NAPHTHALENE_SKELETON, {(1, 2), (3, 4), (5, 10), (6, 7), (8, 9)})), [4] * 11, []),
    ("naphthalene, form 2", rows_of(["C"] * 10, with_doubles(NAPHTHALENE_SKELETON, {(2, 3), (4, 5), (6, 7), (8, 9), (10, 1)})), [4] * 11, []),
    ("cyclopentadiene", rows_of(["C"] * 5, ring(K5)), None, []),
    ("fulvene", rows_of(["C"] * 6, ring(K5) + [(1, 6, 2)]), None, []),
    ("p-benzoquinone", rows_of(["C"] * 6 + ["O", "O"], ring([1, 2, 1, 1, 2, 1]) + [(1, 7, 2), (4, 8, 2)]), None, []),
    ("borole", rows_of(["B"] + ["C"] * 4, ring(K5)), None, []),
    ("cyclooctatetraene", rows_of(["C"] * 8, ring([2, 1] * 4)), None, []),
    # the five-ring 1 .. 5, the seven-ring 4 5 6 .. 10
    ("azulene", rows_of(["C"] * 10, [(1, 2, 2), (2, 3, 1), (3, 4, 2), (4, 5, 1), (5, 1, 1), (5, 6, 2), (6, 7, 1), (7, 8, 2), (8, 9, 1), (9, 10, 2),
                                      (10, 4, 1)]), None, []),
    ("benzene, order 4", rows_of(["C"] * 6, ring([4] * 6)), None, []),
]


def random_rows(rng, n_min=6, n_max=40):
    """one graph of the seeded recipe: rings of 5 .. 7 atoms drawn Kekule-like or with order 4, fused or bridged at random, then
    stray bonds up to degree 4; classes 1 .. 4 and wedges; ring symbols, halogens and Si; charges; a vocabulary index outside the
    table now and then; invalid rows (an end outside 1..n, both ends on one atom, order 0 or 9) and duplicate rows; rows shuffled, ends
    in either orientation; 0 .. 3 list entries"""
    n = int(rng.integers(n_min, n_max + 1))
    pool = [1] * 16 + [0, 0, 2, 2, 2, 3, 3, 7, 7, 4, 9, 10, 5, 13, 12]
    atoms = [(int(rng.integers(0, 200)), int(rng.integers(0, 200)), int(rng.choice(pool)) if rng.integers(0, 150) else int(rng.choice([-1, 14])),
              int(rng.choice([0] * 17 + [1, -1, 2])), 0) for _ in range(n)]
    deg, pairs, bonds = [0] * (n + 1), set(), []

    def add(i, j, o, limit=4):
        if i == j or (min(i, j), max(i, j)) in pairs or deg[i] >= limit or deg[j] >= limit:
            return False
        pairs.add((min(i, j), max(i, j)))
        deg[i] += 1
        deg[j] += 1
        bonds.append((i, j, o))
        return True

    at = 1
    while at + 5 <= n and rng.integers(0, 8):
        size = int(rng.integers(5, 8))
        if at + size - 1 > n:
            break
        members = list(range(at, at + size))
        if at > 1 and rng.integers(0, 2):          # fuse with two atoms placed before, where a pair with room is found
            for _ in range(8):
                i, j = (int(v) for v in rng.integers(1, at, 2))
                if (min(i, j), max(i, j)) in pairs and deg[i] < 3 and deg[j] < 3:
                    members = [i] + members[:size - 2] + [j]
                    break
        style = int(rng.integers(0, 4))            # 0, 1: alternating; 2: order 4; 3: anything
        for k in range(len(members)):
            i, j = members[k], members[(k + 1) % len(members)]
            o = (1 + (k + style) % 2) if style < 2 else (4 if style == 2 else int(rng.choice([1, 2, 4, 5, 6])))
            add(i, j, o, limit=3)
        at = max(members) + 1 if members[0] >= at else at + size - 2
    for _ in range(int(rng.integers(0, n // 4 + 2))):
        i, j = (int(v) for v in rng.integers(1, n + 1, 2))
        add(i, j, int(rng.choice([1, 1, 1, 2, 2, 3, 4, 5, 6])))
    for _ in range(int(rng.integers(0, 3))):       # duplicate rows and invalid rows
        kind = int(rng.integers(0, 4))
        if kind == 0 and bonds:
            i, j, o = bonds[int(rng.integers(0, len(bonds)))]
            bonds.append((j, i, int(rng.choice([1, 2, 4]))))
        elif kind == 1:
            bonds.append((int(rng.integers(1, n + 1)), int(rng.choice([0, n + 1, -3])), 2))
        elif kind == 2:
            i = int(rng.integers(1, n + 1))
            bonds.append((i, i, 1))
        elif bonds:
            k = int(rng.integers(0, len(bonds)))
            bonds[k] = (bonds[k][0], bonds[k][1], int(rng.choice([0, 9])))
    order = rng.permutation(len(bonds))
    bonds = [bonds[k] if rng.integers(0, 2) else (bonds[k][1], bonds[k][0], bonds[k][2]) for k in order]
    bonds = [(int(i), int(j), int(o), k) for k, (i, j, o) in enumerate(bonds)]
    implh = [int(v) for v in rng.integers(1, n + 1, int(rng.integers(0, 4)))]
    implh = list(dict.fromkeys(implh))
    return atoms, bonds, implh


def molecule(rows):
    """the rows as a decode.Molecule, for the host form; a vocabulary index outside the table becomes the symbol "?" (no symbol)"""
    from abcnet_amd.decode import ATOM_SYMBOLS, Molecule
    atoms, bonds, implh = rows
    return Molecule([ATOM_SYMBOLS[a[2]] if 0 <= a[2] < len(ATOM_SYMBOLS) else "?" for a in atoms], [a[3] for a in atoms], [a[4] for a in atoms],
                    [a[:2] for a in atoms], [q[:2] for q in bonds], [q[2] for q in bonds], implh, [q[3] for q in bonds])


def as_record(rows):
    """the atoms and bond rows of (atoms, bonds, implh) as a raster.parse_graph record, 0-based, the rows in their order (a record
    as GraphRecords.load takes it needs i < j in range: the callers pass graphs whose rows are valid)"""
    atoms, bonds, _ = rows
    a = np.array([(x, y, t, q) for x, y, t, q, _ in atoms], dtype=np.int32).reshape(-1, 4)
    q = np.array([(min(i, j) - 1, max(i, j) - 1, o) for i, j, o, _ in bonds], dtype=np.int32).reshape(-1, 3)
    return a, q
