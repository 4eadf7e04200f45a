"""Test infrastructure, not product: the strings the SMILES reader's tests share.  TABLE is derived by hand from the reading rule of
DESIGN.md section 7 ("Reading a SMILES"), not from any implementation: string -> atoms, bonds, the atom classes in order, the sorted
bond orders, the charges in order (classes: raster.ATOM_VOCAB, -1 outside it)."""
import numpy as np

OK, EMPTY, TOO_LONG, SYNTAX, TRUNCATED, DUPLICATE = 0, 1, 2, 3, 4, 5
MAX_BYTES = 4096
C, N, O, P, F, CL, S, BR, B, SE, I, H, SI, X = 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, -1


def _row(text, classes, orders, charges=None):
    return text, len(classes), len(orders), list(classes), sorted(orders), [0] * len(classes) if charges is None else list(charges)


TABLE = [
    _row("CC(=O)Oc1ccccc1C(=O)O", [C, C, O, O] + [C] * 6 + [C, O, O], [1] * 5 + [2] * 2 + [4] * 6),
    _row("Cn1cnc2c1c(=O)n(C)c(=O)n2C", [C, N, C, N, C, C, C, O, N, C, C, O, N, C], [1] * 3 + [2] * 2 + [4] * 10),
    _row("[Na+].[O-]c1ccccc1", [X, O] + [C] * 6, [1] + [4] * 6, [1, -1, 0, 0, 0, 0, 0, 0]),
    _row("C[C@H](N)C(=O)O", [C, C, N, C, O, O], [1, 1, 1, 2, 1]),
    _row("F/C=C\\F", [F, C, C, F], [1, 2, 1]),
    _row("C1CCCCC=1", [C] * 6, [1] * 5 + [2]),
    _row("C=1CCCCC1", [C] * 6, [1] * 5 + [2]),
    _row("C=1CCCCC=1", [C] * 6, [1] * 5 + [2]),
    _row("c1ccccc1c1ccccc1", [C] * 12, [4] * 13),
    _row("c1ccccc1-c1ccccc1", [C] * 12, [4] * 12 + [1]),
    _row("C%12CC%12", [C] * 3, [1] * 3),
    _row("C0CC0", [C] * 3, [1] * 3),
    _row("C1CC1C1CC1", [C] * 6, [1] * 7),
    _row("[13CH4]", [C], []),
    _row("[2H]O[2H]", [H, O, H], [1, 1]),
    _row("[Fe+2]", [X], [], [2]),
    _row("[Fe++]", [X], [], [2]),
    _row("[O--]", [O], [], [-2]),
    _row("[nH]1cccc1", [N, C, C, C, C], [4] * 5),
    _row("[se]1cccc1", [SE, C, C, C, C], [4] * 5),
    _row("[SiH]1:cccc:1", [SI, C, C, C, C], [4] * 5),
    _row("[C@@](F)(Cl)(Br)I", [C, F, CL, BR, I], [1] * 4),
    _row("*C", [X, C], [1]),
    _row("[CH3:7][OH]", [C, O], [1]),
    # the examples of the writer's rule (the SMILES paragraph; smiles_cases.EXAMPLES)
    _row("c1ccccc1", [C] * 6, [4] * 6),
    _row("C(C)(C)C", [C] * 4, [1] * 3),
    _row("CC(=O)[O-]", [C, C, O, O], [1, 2, 1], [0, 0, 0, -1]),
    _row("Cc1ccccc1", [C] * 7, [1] + [4] * 6),
    _row("c1(ccccc1)-c1ccccc1", [C] * 12, [4] * 12 + [1]),
    _row("c1cccc2c1cccc2", [C] * 10, [4] * 11),
    _row("C12(CC1)CC2", [C] * 5, [1] * 6),
    _row("C12C3C4C1C1C2C3C41", [C] * 8, [1] * 12),
    _row("[NH3+]C.[Cl-].[SiH3][H]", [N, C, CL, SI, H], [1, 1], [1, 0, -1, 0, 0]),
    # a few more corners of the rule
    _row("[C@TH1](F)(Cl)(Br)I", [C, F, CL, BR, I], [1] * 4),
    _row("C#N", [C, N], [3]),
    _row("[Cu+2].[O-]S(=O)(=O)[O-]", [X, O, S, O, O, O], [1, 2, 2, 1], [2, -1, 0, 0, 0, -1]),
    _row("[as]1cccc1", [X, C, C, C, C], [4] * 5),
    _row("C1.C1", [C, C], [1]),
    _row("c1ccccc1C", [C] * 7, [4] * 6 + [1]),
    _row("Cc1ccccc1", [C] * 7, [1] + [4] * 6),
    _row("[N-15]", [N], [], [-15]),
    _row("ClCBr", [CL, C, BR], [1, 1]),
]
# rows given in full: the three spellings of one ring closure are ONE record, bonds in the order of the byte that completes them
CYCLOHEXENE = ([(0, 0, C, 0)] * 6, [(0, 1, 1), (1, 2, 1), (2, 3, 1), (3, 4, 1), (4, 5, 1), (0, 5, 2)])
FULL_ROWS = {"C1CCCCC=1": CYCLOHEXENE, "C=1CCCCC1": CYCLOHEXENE, "C=1CCCCC=1": CYCLOHEXENE,
             "C12(CC1)CC2": ([(0, 0, C, 0)] * 5, [(0, 1, 1), (1, 2, 1), (0, 2, 1), (0, 3, 1), (3, 4, 1), (0, 4, 1)]),
             "[Na+].[O-]c1ccccc1": ([(0, 0, X, 1), (0, 0, O, -1)] + [(0, 0, C, 0)] * 6,
                                    [(1, 2, 1), (2, 3, 4), (3, 4, 4), (4, 5, 4), (5, 6, 4), (6, 7, 4), (2, 7, 4)])}

REFUSED = [(s, SYNTAX) for s in ("C(", "C)", "C(C", "C1CC", "C=", "=C", "C==C", "C()C", "C((C))C", "C=1CC#1", "C11", "CC.=C", "C$C", "C>>O",
                                 "[C", "C]", "[]", "C%1C", "C%(100)CC%(100)", "c1ccccc1 benzene", "[C+16]",
                                 # further corners: a number behind `)`, a dot without an atom on a side, charges, a bare symbol
                                 "C(C)1CC1", ".C", "C.", "C..C", "[C+-]", "[C++++]", "[si]", "[C:]", "[[C]]", "C\tC", "C\xe9", "Cl.l", "(C)", "1CC1",
                                 "C(.C)", "C(=)C", "C-(C)C", "[CH3", "C[", "%12", "C%1", "C/=C", "[C@@@H]", "[HH2+123]")]
REFUSED += [("C12CCC12", DUPLICATE), ("C1C1", DUPLICATE), ("C1CC1.C2CC=2.C3C3", DUPLICATE), ("", EMPTY), ("C" * (MAX_BYTES + 1), TOO_LONG)]


def truncated(max_atoms):
    return "C" * (max_atoms + 1)


def mutated(count, seed=20260401):
    """`count` seeded strings: a table entry (or a refusal) with 1..3 bytes deleted, doubled or swapped with their neighbour; most are
    refusals, some still read"""
    rng = np.random.default_rng(seed)
    base = [row[0] for row in TABLE] + [s for s, _ in REFUSED if 0 < len(s) < 64]
    out = []
    while len(out) < count:
        s = list(base[int(rng.integers(len(base)))])
        for _ in range(int(rng.integers(1, 4))):
            if not s:
                break
            k, op = int(rng.integers(len(s))), int(rng.integers(3))
            if op == 0:
                del s[k]
            elif op == 1:
                s.insert(k, s[k])
            elif k + 1 < len(s):
                s[k], s[k + 1] = s[k + 1], s[k]
        out.append("".join(s))
    return out


def as_rows(status, atoms, bonds):
    """a reader's result in one comparable form"""
    return int(status), [tuple(int(v) for v in r) for r in np.asarray(atoms).reshape(-1, 4)], [tuple(int(v) for v in r) for r in np.asarray(bonds).reshape(-1, 3)]
