"""Test infrastructure, not product: the molecules the double-bond tests of the SMILES writer share, as rows of the assembler's
layout (smiles_stereo_cases.rows), the seeded recipe and the moves on a 0..60 canvas."""
import numpy as np

from smiles_stereo_cases import rows

W = 60      # the side of the canvas of the seeded recipe


def chain_rows(symbols, places, orders):
    return rows(list(symbols), places, [(i + 1, i + 2, o) for i, o in enumerate(orders)])


BUTENE = [(10, 10), (20, 20), (20, 30), (30, 40)]
HEXADIENE = [(10, 0), (20, 10), (20, 20), (30, 30), (30, 40), (40, 50)]
HEXADIENE_EZ = HEXADIENE[:5] + [(20, 50)]
RING_6 = [(0, 10), (10, 0), (20, 0), (30, 10), (20, 20), (10, 20)]
CENTRE = (["C", "N", "C", "O"], [(20, 20), (10, 20), (25, 29), (25, 11)], [(1, 2, 5), (1, 3, 1), (1, 4, 1)])      # the tetrahedral example


def with_propenyl(last):
    symbols, places, bonds = CENTRE
    return rows(symbols + ["C", "C"], places + [(35, 35), last], bonds + [(3, 5, 2), (5, 6, 1)])


# (name, rows, the text of the rule, the codes of the bond rows) -- the texts were worked out by hand from the rule
CASES = [
    ("trans-2-butene", chain_rows("CCCC", BUTENE, (1, 2, 1)), "C/C=C/C", [0, -1, 0]),
    ("cis-2-butene", chain_rows("CCCC", BUTENE[:3] + [(10, 40)], (1, 2, 1)), "C/C=C\\C", [0, 1, 0]),
    ("trans, numbered from the middle", rows(list("CCCC"), [(20, 20), (20, 30), (10, 10), (30, 40)], [(1, 2, 2), (1, 3, 1), (2, 4, 1)]),
     "C(=C/C)\\C", [-1, 0, 0]),
    ("(E,E)-hexadiene", chain_rows("CCCCCC", HEXADIENE, (1, 2, 1, 2, 1)), "C/C=C/C=C/C", [0, -1, 0, -1, 0]),
    ("(E,Z)-hexadiene", chain_rows("CCCCCC", HEXADIENE_EZ, (1, 2, 1, 2, 1)), "C/C=C/C=C\\C", [0, -1, 0, 1, 0]),
    ("(E,Z)-hexadiene, renumbered", chain_rows("CCCCCC", HEXADIENE_EZ[::-1], (1, 2, 1, 2, 1)), "C/C=C\\C=C\\C", [0, 1, 0, -1, 0]),
    ("tetrasubstituted", rows(["F", "C", "Cl", "C", "Br", "I"], [(10, 10), (20, 20), (30, 10), (20, 30), (10, 40), (30, 40)],
                              [(1, 2, 1), (2, 3, 1), (2, 4, 2), (4, 5, 1), (4, 6, 1)]), "F/C(/Cl)=C(\\Br)/I", [0, 0, 1, 0, 0]),
    ("oxime", chain_rows("CCNO", BUTENE, (1, 2, 1)), "C/C=N/O", [0, -1, 0]),
    ("two butenes, cis then trans", rows(list("CCCCCCCC"), BUTENE[:3] + [(10, 40)] + [(x + 30, y) for x, y in BUTENE],
                                         [(1, 2, 1), (2, 3, 2), (3, 4, 1), (5, 6, 1), (6, 7, 2), (7, 8, 1)]),
     "C/C=C\\C.C/C=C/C", [0, 1, 0, 0, -1, 0]),
    ("exocyclic, unsymmetric ring", rows(list("CCCNCCCC"), RING_6 + [(10, 30), (20, 40)],
                                         [(1, 2, 1), (2, 3, 1), (3, 4, 1), (4, 5, 1), (5, 6, 1), (6, 1, 1), (6, 7, 2), (7, 8, 1)]),
     "C1CCNC/C/1=C\\C", [0, 0, 0, 0, 0, 0, -1, 0]),
    ("isobutenyl", rows(list("CCCCC"), [(10, 10), (20, 20), (30, 10), (20, 30), (30, 40)], [(1, 2, 1), (2, 3, 1), (2, 4, 2), (4, 5, 1)]),
     "CC(C)=CC", [0, 0, 4, 0]),
    ("cyclohexene", rows(list("CCCCCC"), RING_6, [(1, 2, 2), (2, 3, 1), (3, 4, 1), (4, 5, 1), (5, 6, 1), (6, 1, 1)]),
     "C1=CCCCC1", [3, 0, 0, 0, 0, 0]),
    ("collinear 2-butene", chain_rows("CCCC", [(10, 10), (10, 20), (10, 30), (10, 40)], (1, 2, 1)), "CC=CC", [0, 2, 0]),
]
# the tetrahedral example with a propenyl group: (rows, text with both options, tetrahedral only, double bonds only)
BOTH = [
    (with_propenyl((35, 45)), "[C@H](N)(/C=C/C)O", "[C@H](N)(C=CC)O", "C(N)(/C=C/C)O"),
    (with_propenyl((45, 29)), "[C@H](N)(/C=C\\C)O", "[C@H](N)(C=CC)O", "C(N)(/C=C\\C)O"),
]
# placed by hand: (name, rows, the code of the one class-2 row)
FLAT_CASES = [
    ("an end at 200000", chain_rows("CCCC", [(10, 10), (200000, 20), (20, 30), (30, 40)], (1, 2, 1)), 2),
    ("a substituent at -1", chain_rows("CCCC", [(-1, 10), (20, 20), (20, 30), (30, 40)], (1, 2, 1)), 2),
    ("a substituent at 199999, in range", chain_rows("CCCC", [(199999, 0), (20, 20), (20, 30), (0, 199999)], (1, 2, 1)), -1),
    ("both ends on one pixel", chain_rows("CCCC", [(10, 10), (20, 20), (20, 20), (30, 40)], (1, 2, 1)), 2),
    ("a substituent on its end's pixel", chain_rows("CCCC", [(20, 20), (20, 20), (20, 30), (30, 40)], (1, 2, 1)), 2),
    ("two substituents of one end on one side", rows(list("CCNCC"), [(10, 10), (20, 20), (10, 15), (20, 30), (30, 40)],
                                                     [(1, 2, 1), (2, 3, 1), (2, 4, 2), (4, 5, 1)]), 2),
    # the corners of the range: 199999 * 199999 = 39 999 600 001, which a 32-bit product turns into another number
    ("the corners of the range", chain_rows("CCCC", [(0, 199999), (0, 0), (199999, 199999), (199999, 0)], (1, 2, 1)), -1),
]


def random_rows(rng):
    """one molecule of the seeded recipe: a tree of 4..14 atoms of degree <= 3 over C N O, now and then a run of double bonds along a
    path, up to two extra single bonds, places anywhere on the 0..W canvas; a few are spoilt on purpose (an atom moved into line
    with a double bond, or out of the range)"""
    n = int(rng.integers(4, 15))
    kinds = ["C"] * 7 + ["N", "N", "O"]
    symbols = [kinds[int(rng.integers(0, len(kinds)))] for _ in range(n)]
    places = []
    while len(places) < n:
        xy = (int(rng.integers(0, W + 1)), int(rng.integers(0, W + 1)))
        if xy not in places:
            places.append(xy)
    degree, pairs = [0] * n, {}
    for a in range(1, n):
        free = [x for x in range(a) if degree[x] < 3] or list(range(a))
        x = free[int(rng.integers(max(0, len(free) - 3), len(free)))]      # (near the end: long chains)
        pairs[(x, a)] = 1
        degree[x] += 1
        degree[a] += 1
    has_double = [False] * n
    for (x, a) in list(pairs):
        if not has_double[x] and not has_double[a] and rng.random() < 0.4:
            pairs[(x, a)] = 2
            has_double[x] = has_double[a] = True
    for _ in range(int(rng.integers(0, 3))):
        a, x = sorted(int(v) for v in rng.integers(0, n, 2))
        if a != x and (a, x) not in pairs and degree[a] < 3 and degree[x] < 3:
            pairs[(a, x)] = 1
            degree[a] += 1
            degree[x] += 1
    spoil = rng.random()
    doubles = [p for p, o in pairs.items() if o == 2]
    if doubles and spoil < 0.06:
        a, b = doubles[0]
        others = [x for p in pairs for x in p if a in p and x not in (a, b)]
        if others:
            (xa, ya), (xb, yb) = places[a], places[b]
            for spot in ((2 * xa - xb, 2 * ya - yb), (2 * xb - xa, 2 * yb - ya)):      # on the line through the double bond
                if spot not in places and 0 <= min(spot) and max(spot) <= W:
                    places[others[0]] = spot
                    break
    elif doubles and spoil < 0.09:
        a = doubles[0][int(rng.integers(0, 2))]
        places[a] = (places[a][0], 200000) if rng.integers(0, 2) else (-1 - int(rng.integers(0, 5)), places[a][1])
    bonds = [((a, x) if rng.integers(0, 2) else (x, a)) + (order,) for (a, x), order in pairs.items()]
    bonds = [(e1 + 1, e2 + 1, o) for e1, e2, o in (bonds[i] for i in rng.permutation(len(bonds)))]
    implh = [int(v) for v in rng.integers(1, n + 1, int(rng.integers(0, 2)))]
    return rows(symbols, places, bonds, None, implh)


def random_images(seed, count):
    rng = np.random.default_rng(seed)
    return [random_rows(rng) for _ in range(count)]


def in_canvas(image):
    return all(0 <= a[0] <= W and 0 <= a[1] <= W for a in image[0])


# ------------------------------------------------------------------------------------------------------- moves on rows
def mirror(x, y):
    return W - x, y


def quarter_turn(x, y):
    return y, W - x


def shift(x, y):
    return x + 1000, y + 77


def zigzag_polyene(n):
    """n carbons (n even) on a zigzag, bonds 1 2 1 2 ... 1: n / 2 - 1 conjugated double bonds, all trans, one group (the most a chain
    of n atoms holds: every end needs a substituent, so a double bond at the chain's end is no candidate)"""
    places = [(10 * (i % 2) + 20, 10 * i) for i in range(n)]
    return rows(["C"] * n, places, [(i + 1, i + 2, 2 if i % 2 == 1 else 1) for i in range(n - 1)])


def butenes(count):
    """count separate 2-butenes in one image, cis and trans by turns"""
    symbols, places, bonds = [], [], []
    for k in range(count):
        at = 4 * k
        places += [(10, 50 * k), (20, 50 * k + 10), (20, 50 * k + 20), (10 if k % 2 == 0 else 30, 50 * k + 30)]
        bonds += [(at + 1, at + 2, 1), (at + 2, at + 3, 2), (at + 3, at + 4, 1)]
    return rows(["C"] * (4 * count), places, bonds)
