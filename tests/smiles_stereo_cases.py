"""Test infrastructure, not product: the molecules the stereo tests of the SMILES writer share, as rows of the assembler's layout
(atoms (x, y, vocabulary index, charge, hs), bonds (end 1, end 2 (1-based), order, source), implicit-H entries), and the moves on
rows the invariance tests make.  x is the row, y the column of the drawing."""
import numpy as np

from smiles_cases import SYMBOLS

W = 400      # the side of the canvas the moves turn and mirror


def rows(symbols, places, bonds, charges=None, implh=()):
    charges = [0] * len(symbols) if charges is None else charges
    atoms = [(x, y, SYMBOLS.index(s, 1), q, 0) for s, (x, y), q in zip(symbols, places, charges)]
    return atoms, [(e1, e2, order, k) for k, (e1, e2, order) in enumerate(bonds)], list(implh)


def worked(order=5, swapped=False):
    """the example of the rule: C (20, 20) with N above, C lower right, O lower left; the wedge C -> N, or N -> C when swapped"""
    return rows(["C", "N", "C", "O"], [(20, 20), (10, 20), (25, 29), (25, 11)], [((2, 1) if swapped else (1, 2)) + (order,), (1, 3, 1), (1, 4, 1)])


CROSS = [(50, 50), (40, 50), (50, 62), (61, 50), (50, 37)]      # a centre and its four neighbours: up, right, down, left

# (name, rows, the text the rule gives) -- the texts were worked out by hand from the rule, the tests hold all three writers to them
CASES = [
    ("the worked example", worked(5), "[C@H](N)(C)O"),
    ("the worked example, hashed", worked(6), "[C@@H](N)(C)O"),
    ("the worked example, the nitrogen's wedge", worked(5, True), "C(N)(C)O"),
    # four neighbours, the centre is the root: T = det[(-10,0,1)-(0,-13,0); (0,12,0)-(0,-13,0); (11,0,0)-(0,-13,0)]
    #   = det[(-10,13,1); (0,25,0); (11,13,0)] = 1 * (0 * 13 - 25 * 11) = -275, text order = local order: @@
    ("four neighbours, a root", rows(["C", "F", "Cl", "Br", "I"], CROSS, [(1, 2, 5), (1, 3, 1), (1, 4, 1), (1, 5, 1)]), "[C@@](F)(Cl)(Br)I"),
    # the same centre listed last: local order (1 F, 2 Cl, 3 Br, 4 I) as above, T = -275; the text names F (parent), Cl, Br, I: @@
    ("four neighbours, a parent",
     rows(["F", "Cl", "Br", "I", "C"], CROSS[1:] + CROSS[:1], [(5, 1, 5), (5, 2, 1), (5, 3, 1), (5, 4, 1)]), "F[C@@](Cl)(Br)I"),
    # a parent and a hydrogen.  Local (O, N, F, H): T = det[(-10,0,0); (5,10,1); (7,-9,0)] = -10 * (10 * 0 - 1 * -9) = -90; the text
    # names O (parent), H, N, F: H moves two places forward, an even permutation: @@
    ("a parent and a hydrogen", rows(["O", "C", "N", "F"], [(40, 50), (50, 50), (55, 60), (57, 41)], [(1, 2, 1), (2, 3, 5), (2, 4, 1)]),
     "O[C@@H](N)F"),
    ("a spiro centre at the root, two openings",
     rows(["C"] * 5, [(50, 50), (40, 44), (38, 59), (63, 41), (60, 56)], [(1, 2, 5), (2, 3, 1), (3, 1, 1), (1, 4, 1), (4, 5, 1), (1, 5, 6)]), None),
    ("a spiro centre inside: a parent, one closing, one opening, a child",
     rows(["C"] * 5, [(40, 44), (40, 56), (50, 50), (60, 44), (60, 56)], [(1, 2, 1), (2, 3, 1), (3, 1, 6), (3, 4, 1), (4, 5, 1), (5, 3, 1)]), None),
    ("a parent, an opening and two children",
     rows(["C"] * 7, [(30, 30), (40, 40), (50, 30), (50, 50), (60, 40), (40, 20), (45, 60)],
          [(1, 2, 1), (2, 3, 1), (3, 1, 1), (2, 4, 5), (4, 5, 1), (5, 2, 1), (1, 6, 1)]), None),
    ("two closings, a parent and a child",
     rows(["C"] * 5, [(30, 30), (30, 50), (50, 52), (48, 33), (64, 20)], [(1, 2, 1), (2, 3, 1), (3, 4, 1), (4, 1, 1), (4, 2, 1), (4, 5, 5)]), None),
    # norbornane, both bridgeheads: atom 1 is the root (hydrogen, two openings, a child), atom 4 has a parent, a hydrogen and two children
    ("two bridgeheads with a hydrogen each",
     rows(["C"] * 7, [(30, 50), (40, 62), (56, 61), (66, 50), (57, 38), (41, 39), (48, 53)],
          [(1, 2, 1), (2, 3, 1), (3, 4, 1), (4, 5, 1), (5, 6, 1), (6, 1, 1), (1, 7, 5), (4, 7, 5)]), None),
    ("two wedges of equal sign", rows(["C", "F", "Cl", "Br", "I"], CROSS, [(1, 2, 5), (1, 3, 1), (1, 4, 5), (1, 5, 1)]), None),
    ("two wedges of opposite sign", rows(["C", "F", "Cl", "Br", "I"], CROSS, [(1, 2, 5), (1, 3, 6), (1, 4, 1), (1, 5, 1)]), None),
    ("a charged centre", rows(["N", "C", "C", "C", "C"], CROSS, [(1, 2, 6), (1, 3, 1), (1, 4, 1), (1, 5, 1)], charges=[1, 0, 0, 0, 0]), None),
    ("a listed centre", rows(["N", "C", "C", "O"], [(20, 20), (10, 20), (25, 29), (25, 11)], [(1, 2, 5), (1, 3, 1), (1, 4, 1)], implh=[1]), None),
]

# one candidate each, which gets no mark: (name, rows, the candidate's code -- 2 flat, 3 unqualified)
LINE = [(50, 50), (40, 50), (50, 60), (50, 40)]      # the two plain neighbours and the centre in one line
REFUSALS = [
    ("flat: the plain neighbours in line with the centre", rows(["C", "N", "C", "O"], LINE, [(1, 2, 5), (1, 3, 1), (1, 4, 1)]), 2),
    # a square cross, one arm up and the opposite arm down by as much: T = -200 z1 - 200 z3 = 0
    ("flat: four neighbours, T = 0", rows(["C", "F", "Cl", "Br", "I"], [(50, 50), (40, 50), (50, 60), (60, 50), (50, 40)],
                                          [(1, 2, 5), (1, 3, 1), (1, 4, 6), (1, 5, 1)]), 2),
    ("flat: a neighbour on the centre's pixel", rows(["C", "N", "C", "O"], [(20, 20), (10, 20), (20, 20), (25, 11)], [(1, 2, 5), (1, 3, 1), (1, 4, 1)]), 2),
    ("flat: the centre at 200000", rows(["C", "N", "C", "O"], [(200000, 20), (10, 20), (25, 29), (25, 11)], [(1, 2, 5), (1, 3, 1), (1, 4, 1)]), 2),
    ("flat: a neighbour at 200000", rows(["C", "N", "C", "O"], [(20, 20), (10, 20), (25, 200000), (25, 11)], [(1, 2, 5), (1, 3, 1), (1, 4, 1)]), 2),
    ("flat: a neighbour at -1", rows(["C", "N", "C", "O"], [(20, 20), (-1, 20), (25, 29), (25, 11)], [(1, 2, 5), (1, 3, 1), (1, 4, 1)]), 2),
    ("unqualified: a double bond", rows(["C", "N", "C", "O"], [(20, 20), (10, 20), (25, 29), (25, 11)], [(1, 2, 5), (1, 3, 2), (1, 4, 1)]), 3),
    ("unqualified: d = 2", rows(["C", "N", "C"], [(20, 20), (10, 20), (25, 29)], [(1, 2, 5), (1, 3, 1)]), 3),
    ("unqualified: d = 5", rows(["P", "F", "Cl", "Br", "I", "C"], CROSS + [(58, 58)], [(1, 2, 5), (1, 3, 1), (1, 4, 1), (1, 5, 1), (1, 6, 1)]), 3),
    ("unqualified: d = 3, h = 0", rows(["N", "C", "C", "O"], [(20, 20), (10, 20), (25, 29), (25, 11)], [(1, 2, 5), (1, 3, 1), (1, 4, 1)]), 3),
    ("unqualified: d = 4, h = 1", rows(["P", "F", "Cl", "Br", "I"], CROSS, [(1, 2, 5), (1, 3, 1), (1, 4, 1), (1, 5, 1)]), 3),
    ("unqualified: d = 4, listed", rows(["C", "F", "Cl", "Br", "I"], CROSS, [(1, 2, 5), (1, 3, 1), (1, 4, 1), (1, 5, 1)], implh=[1]), 3),
    ("unqualified: the symbol H", rows(["H", "N", "C", "O"], [(20, 20), (10, 20), (25, 29), (25, 11)], [(1, 2, 5), (1, 3, 1), (1, 4, 1)]), 3),
]

# the corners of the range: T = -199999 * 150000 = -29 999 850 000, which a 32-bit product turns into +64 921 072, the other sign
WIDE = rows(["C", "N", "C", "O"], [(0, 0), (100000, 100000), (199999, 0), (0, 150000)], [(1, 2, 6), (1, 3, 1), (1, 4, 1)])
WIDE_4 = rows(["C", "F", "Cl", "Br", "I"], [(100000, 100000), (0, 0), (0, 199999), (199999, 199999), (199999, 0)],
              [(1, 2, 5), (1, 3, 1), (1, 4, 5), (1, 5, 1)])


def wedged_chain():
    """512 atoms, the capacity: a chain of 511 carbons with a methyl (atom 512) on atom 500, the wedge from atom 500 to it"""
    places = [(2 * i + (i % 3), 40 + (i * i) % 7) for i in range(511)] + [(2 * 499 + 9, 80)]
    return rows(["C"] * 512, places, [(i, i + 1, 1) for i in range(1, 511)] + [(500, 512, 6)])


def random_rows(rng):
    """one molecule of the seeded recipe, built so that centres exist: a tree of 4..24 atoms of degree <= 4 (now and then 5) with a
    few ring bonds, mostly carbon, mostly single bonds, places on a 20..W-20 grid; then wedges from atoms of degree 3 and 4 (and a
    few from anywhere), some of them spoilt on purpose: a neighbour moved onto the centre or into line with it"""
    n = int(rng.integers(4, 25))
    kinds = ["C"] * 12 + ["N", "N", "O", "S", "P", "Si", "B", "H", "F", "Cl"]
    symbols = [kinds[int(rng.integers(0, len(kinds)))] for _ in range(n)]
    charges = [int(rng.choice([0] * 10 + [1, -1])) for _ in range(n)]
    places = []
    while len(places) < n:
        xy = (int(rng.integers(20, W - 20)), int(rng.integers(20, W - 20)))
        if xy not in places:
            places.append(xy)
    degree, pairs = [0] * n, {}
    for a in range(1, n):
        limit = 5 if rng.integers(0, 12) == 0 else 4
        free = [x for x in range(a) if degree[x] < limit] or list(range(a))
        x = free[int(rng.integers(0, len(free)))]
        pairs[(x, a)] = 1
        degree[x] += 1
        degree[a] += 1
    for _ in range(int(rng.integers(0, 4))):
        a, x = (int(v) for v in rng.integers(0, n, 2))
        if a != x and (min(a, x), max(a, x)) not in pairs and degree[a] < 4 and degree[x] < 4:
            pairs[(min(a, x), max(a, x))] = 1
            degree[a] += 1
            degree[x] += 1
    for pair in pairs:
        if rng.integers(0, 12) == 0:
            pairs[pair] = int(rng.choice([2, 2, 3, 4]))
    around = [[x for pair in pairs for x in pair if a in pair and x != a] for a in range(n)]
    wedge = {}      # pair -> (end 1, order)
    for a in range(n):
        if rng.random() < (0.6 if degree[a] in (3, 4) else 0.1):
            for x in rng.permutation(around[a])[:int(rng.choice([1, 1, 1, 2]))]:
                pair = (min(a, int(x)), max(a, int(x)))
                if pairs[pair] == 1 and pair not in wedge:
                    wedge[pair] = (a, int(rng.choice([5, 6])))
            spoil = rng.random()
            plain = [x for x in around[a] if wedge.get((min(a, x), max(a, x)), (None,))[0] != a]
            if spoil < 0.08 and plain:
                places[plain[0]] = places[a]
            elif spoil < 0.2 and degree[a] == 3 and len(plain) == 2:
                (xa, ya), (x1, y1) = places[a], places[plain[0]]
                for x2, y2 in ((2 * xa - x1, 2 * ya - y1), (2 * x1 - xa, 2 * y1 - ya)):      # across the centre, else beyond the other
                    if 0 <= x2 <= W and 0 <= y2 <= W:
                        places[plain[1]] = (x2, y2)
                        break
    bonds = []
    for (a, x), order in pairs.items():
        if (a, x) in wedge:
            e1, order = wedge[(a, x)]
            e2 = x if e1 == a else a
        else:
            e1, e2 = (a, x) if rng.integers(0, 2) else (x, a)
        bonds.append((e1 + 1, e2 + 1, order))
    bonds = [bonds[i] for i in rng.permutation(len(bonds))]
    implh = [int(v) for v in rng.integers(1, n + 1, int(rng.integers(0, 3)))]
    return rows(symbols, places, bonds, charges, implh)


def random_images(seed, count):
    rng = np.random.default_rng(seed)
    return [random_rows(rng) for _ in range(count)]


# ------------------------------------------------------------------------------------------------------- moves on rows
def renumbered(image, rng):
    """the same drawing with its atoms in another order and its rows shuffled; a plain bond may turn round, a wedge may not.
    -> (rows, new_of: the new 0-based index of every old atom)"""
    atoms, bonds, implh = image
    n = len(atoms)
    new_of = [int(v) for v in rng.permutation(n)]
    out = [None] * n
    for old, new in enumerate(new_of):
        out[new] = atoms[old]
    moved = []
    for e1, e2, order, src in bonds:
        e1, e2 = new_of[e1 - 1] + 1, new_of[e2 - 1] + 1
        if order < 5 and rng.integers(0, 2):
            e1, e2 = e2, e1
        moved.append((e1, e2, order, src))
    moved = [moved[i] for i in rng.permutation(len(moved))]
    return (out, moved, [new_of[a - 1] + 1 for a in implh]), new_of


def moved(image, place=None, order=None):
    """the same rows with every place (x, y) and every bond order sent through a function"""
    atoms, bonds, implh = image
    place = place or (lambda x, y: (x, y))
    order = order or (lambda o: o)
    return ([place(a[0], a[1]) + tuple(a[2:]) for a in atoms], [(b[0], b[1], order(b[2]), b[3]) for b in bonds], list(implh))


def mirror(x, y):
    return x, W - y


def turn(x, y):
    """a quarter turn of the canvas, a proper rotation"""
    return y, W - x


def shift(x, y):
    return x + 1000, y + 77


def swap_wedges(o):
    return {5: 6, 6: 5}.get(o, o)
