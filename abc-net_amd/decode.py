"""The assembled molecule of one image (img2smiles2.py:193-311, computed on the device by csrc/assemble.hip) and the mol block
the reference writes from it (generate_smiles.py:18-105).  Pure host string work: RDKit is not a dependency; the caller hands
`Molecule.molblock()` to `Chem.MolFromMolBlock` exactly as generate_smiles.py:115 does.  `Molecule.smiles()` writes a SMILES without
RDKit, by this project's own text rule: not RDKit's canonical string.
"""
from __future__ import annotations

import numpy as np

# utils.py:12-13 inverted, with index 0 decoded as carbon (img2smiles2.py:24-25)
ATOM_SYMBOLS = ("C", "C", "N", "O", "P", "F", "Cl", "S", "Br", "B", "Se", "I", "H", "Si")
N_OMEGA = 60


def omega_table():
    """float64 [2, 60]: cos and sin of the bin angles of img2smiles2.py:160, computed as the reference computes them (numpy on the
    host).  The device reads this table and never calls a trigonometric function."""
    omega = [k * (np.pi / 30) + np.pi / 60 - np.pi / 2 for k in range(N_OMEGA)]
    # (scalar calls, as the reference makes them: numpy's array loops may take a vectorised path that rounds differently)
    return np.array([[np.cos(o) for o in omega], [np.sin(o) for o in omega]], dtype=np.float64)


class Molecule:
    """symbols [n] str, charges [n] int in {0, 1, -1}, hs [n] int, positions [n][2] int (row, column on the head-map grid),
    bonds [m][2] 1-based atom indices, orders [m] int 1..6 (4 aromatic, 5 / 6 the wedge codes), implicit_hs: 1-based indices of the
    atoms that get an implicit hydrogen; sources [m]: the index of the bond candidate every bond came from; truncated: a device
    list overflowed its capacity (the molecule is then built from the truncated lists)."""

    __slots__ = ("symbols", "charges", "hs", "positions", "bonds", "orders", "implicit_hs", "sources", "truncated")

    def __init__(self, symbols, charges, hs, positions, bonds, orders, implicit_hs, sources=None, truncated=False):
        self.symbols = [str(s) for s in symbols]
        self.charges = [int(c) for c in charges]
        self.hs = [int(h) for h in hs]
        self.positions = [[int(p[0]), int(p[1])] for p in positions]
        self.bonds = [[int(b[0]), int(b[1])] for b in bonds]
        self.orders = [int(o) for o in orders]
        self.implicit_hs = [int(i) for i in implicit_hs]
        self.sources = None if sources is None else [int(s) for s in sources]
        self.truncated = bool(truncated)

    @classmethod
    def from_device_rows(cls, atoms, bonds, implh, truncated=False):
        """atoms int [n, 5] (x, y, vocabulary index, charge value, hs), bonds int [m, 4] (end 1, end 2, order, source candidate),
        implh int [k]: the rows abc_assemble_graphs writes"""
        atoms, bonds = np.asarray(atoms).reshape(-1, 5), np.asarray(bonds).reshape(-1, 4)
        return cls([ATOM_SYMBOLS[t] for t in atoms[:, 2].tolist()], atoms[:, 3].tolist(), atoms[:, 4].tolist(), atoms[:, :2].tolist(),
                   bonds[:, :2].tolist(), bonds[:, 2].tolist(), np.asarray(implh).reshape(-1).tolist(), bonds[:, 3].tolist(), truncated)

    def __eq__(self, other):
        return isinstance(other, Molecule) and all(getattr(self, k) == getattr(other, k) for k in
                                                   ("symbols", "charges", "hs", "positions", "bonds", "orders", "implicit_hs"))

    def __repr__(self):
        return "Molecule(%d atoms, %d bonds, %d implicit H%s)" % (len(self.symbols), len(self.bonds), len(self.implicit_hs),
                                                                  ", truncated" if self.truncated else "")

    def sdf2smiles_args(self):
        """the six arguments of img2smiles2.py:313-315, with the reference's types (fresh lists: sdf2smiles rewrites the positions)"""
        return (list(self.symbols), [list(b) for b in self.bonds], list(self.charges), list(self.orders),
                [list(p) for p in self.positions], list(self.implicit_hs))

    def molblock(self):
        """the text generate_smiles.py:18-105 builds, byte for byte"""
        out = ["\n     RDKit\n\n", "%3d%3d  0  0  0  0  0  0  0  0999 V2000\n" % (len(self.symbols), len(self.bonds))]
        tail = "0  0  0  0  0  0  0  0  0  0  0  0\n"
        for sym, (px, py) in zip(self.symbols, self.positions):
            x, y = px / 60 - 1, py / 60 - 1
            # the reference's four format strings: a negative coordinate is written after three blanks, the others after four
            fx = "   {:2.4f}".format(x) if x < 0 else "    {:.4f}".format(x)
            fy = "   {:2.4f}".format(y) if y < 0 else "    {:.4f}".format(y)
            out.append("%s%s    0.0000 %s%s" % (fx, fy, sym.ljust(4), tail))
        for (b, e), order in zip(self.bonds, self.orders):
            if order <= 4:
                kind, stereo = order, 0
            else:
                kind, stereo = 1, (1 if order == 5 else 6)
            out.append("%3d%3d%3d%3d\n" % (b, e, kind, stereo))
        charged = [(i + 1, c) for i, c in enumerate(self.charges) if c != 0]
        out.append("M  CHG%3d%s\n" % (len(charged), "".join("%4d%4d" % ic for ic in charged)))
        n = len(self.implicit_hs)
        if n > 0:
            out.append("M  STY  %d%s\n" % (n, "".join("   %d DAT" % (k + 1) for k in range(n))))
            out.append("M  SLB  %d%s\n" % (n, "".join("   %d   %d" % (k + 1, k + 1) for k in range(n))))
            for k, a in enumerate(self.implicit_hs):
                out.append("M  SAL   %d  1  %d  \n" % (k + 1, a))
                out.append("M  SDT   %d MRV_IMPLICIT_H    \n" % (k + 1))
                out.append("M  SDD   %d     0.0000    0.0000    DA    ALL  1       1    \n" % (k + 1))
                out.append("M  SED   %d IMPL_H1\n" % (k + 1))
        out.append("M  END\n$$$$")
        return "".join(out)

    def smiles(self, stereo=False):
        """a deterministic, valid SMILES of this graph by the text rule of DESIGN.md section 7 (the host form and the oracle of
        csrc/smiles.hip, integers only): NOT the canonical string RDKit prints; hs is not read.  stereo=False: wedges are single
        bonds, no mark is written and the positions are not read.  stereo=True: the tetrahedral centres the wedge rows and the
        positions decide (stereo_centres) are written as `@` / `@@` in a bracket token; nothing else of the text changes.
        ValueError for a row the rule refuses and for more than 99 ring bonds open at once."""
        return self._smiles(bool(stereo))[0]

    def stereo_centres(self):
        """one code per atom by the stereo rule of DESIGN.md section 7: 0 no candidate, +1 / -1 the local parity s(a) of a marked
        centre, 2 flat, 3 unqualified (abc_smiles_stereo_desc.stereo_out).  ValueError as smiles()."""
        return self._smiles(True)[1]

    def _smiles(self, stereo):
        n = len(self.symbols)
        for i, (s, c) in enumerate(zip(self.symbols, self.charges)):
            if s not in ATOM_SYMBOLS:
                raise ValueError("Molecule.smiles: atom %d has symbol %r, which the vocabulary does not hold" % (i + 1, s))
            if not -15 <= c <= 15:
                raise ValueError("Molecule.smiles: atom %d has charge %d, outside -15..15" % (i + 1, c))
        adj, pairs = [[] for _ in range(n)], set()
        for k, ((e1, e2), order) in enumerate(zip(self.bonds, self.orders)):
            if not 1 <= order <= 6:
                raise ValueError("Molecule.smiles: bond row %d has order %d, outside 1..6" % (k, order))
            if not (1 <= e1 <= n and 1 <= e2 <= n):
                raise ValueError("Molecule.smiles: bond row %d has an end outside 1..%d: (%d, %d)" % (k, n, e1, e2))
            if e1 == e2:
                raise ValueError("Molecule.smiles: bond row %d has both ends on atom %d" % (k, e1))
            if (min(e1, e2), max(e1, e2)) in pairs:
                raise ValueError("Molecule.smiles: bond row %d is a second row for the atom pair (%d, %d)" % (k, e1, e2))
            pairs.add((min(e1, e2), max(e1, e2)))
            cls = 1 if order >= 5 else order
            adj[e1 - 1].append((e2 - 1, cls))
            adj[e2 - 1].append((e1 - 1, cls))
        for row in adj:
            row.sort()
        listed = [False] * n
        for a in self.implicit_hs:
            if 1 <= a <= n:
                listed[a - 1] = True
        aromatic = [s in _SMILES_AROMATIC and any(cls == 4 for _, cls in row) for s, row in zip(self.symbols, adj)]

        def bond_symbol(u, v, cls):
            both = aromatic[u] and aromatic[v]
            return (("-" if both else ""), "=", "#", ("" if both else ":"))[cls - 1]

        def hydrogens(a):
            s, c = self.symbols[a], self.charges[a]
            if listed[a]:
                return 1
            if s == "H" or abs(c) > 1:
                return 0
            v = sum(3 if cls == 4 else 2 * cls for _, cls in adj[a]) // 2
            return next((t - v for t in _SMILES_VALENCES[s][c + 1] if t >= v), 0)

        def token(a, mark=""):
            s, c = self.symbols[a], self.charges[a]
            sym = s.lower() if aromatic[a] else s
            if c == 0 and not listed[a] and s in _SMILES_BARE and not mark:
                return sym
            h = hydrogens(a)
            charge = "" if c == 0 else ("+" if c > 0 else "-") + ("" if abs(c) == 1 else "%d" % abs(c))
            return "[" + sym + mark + ("" if h == 0 else ("H" if h == 1 else "H%d" % h)) + charge + "]"

        # stereo: the code of every atom (0 none, +1 / -1 the local parity, 2 flat, 3 unqualified)
        centre = [0] * n
        if stereo:
            up = {}      # (end 1, end 2) of a wedge row, 0-based -> the elevation of end 2 seen from end 1
            for (e1, e2), order in zip(self.bonds, self.orders):
                if order >= 5:
                    up[(e1 - 1, e2 - 1)] = 1 if order == 5 else -1
            for a in sorted({e1 for e1, _ in up}):
                d, h = len(adj[a]), hydrogens(a)
                if self.symbols[a] == "H" or any(cls != 1 for _, cls in adj[a]) or (d, h) not in ((4, 0), (3, 1)):
                    centre[a] = 3
                    continue
                xa, ya = self.positions[a]
                rows = [(self.positions[j][0] - xa, self.positions[j][1] - ya, up.get((a, j), 0)) for j, _ in adj[a]]
                in_range = all(0 <= v <= 199999 for j in [a] + [j for j, _ in adj[a]] for v in self.positions[j])
                if not in_range or any(r[0] == 0 and r[1] == 0 for r in rows):
                    centre[a] = 2
                    continue
                if d == 3:
                    rows.append((0, 0, 0))
                (a1, a2, a3), (b1, b2, b3), (c1, c2, c3) = ([u - v for u, v in zip(r, rows[3])] for r in rows[:3])
                t = a1 * (b2 * c3 - b3 * c2) - a2 * (b1 * c3 - b3 * c1) + a3 * (b1 * c2 - b2 * c1)
                centre[a] = 2 if t == 0 else (1 if t > 0 else -1)

        # the walk, with the tree's parent pointers as its stack: the rank, the parent and the brackets of every atom
        rank, parent, order, cursor = [-1] * n, [-1] * n, [], [0] * n
        last_child, opens_branch, closes = [-1] * n, [False] * n, [0] * n
        for root in range(n):
            if rank[root] >= 0:
                continue
            rank[root] = len(order)
            order.append(root)
            cur = root
            while cur >= 0:
                if cursor[cur] == len(adj[cur]):
                    cur = parent[cur]
                    continue
                y = adj[cur][cursor[cur]][0]
                cursor[cur] += 1
                if rank[y] < 0:
                    if last_child[cur] >= 0:      # the child before this one was not the last: it stands in a branch, which
                        opens_branch[last_child[cur]] = True      # ends behind the atom visited last
                        closes[len(order) - 1] += 1
                    last_child[cur], parent[y], rank[y] = y, cur, len(order)
                    order.append(y)
                    cur = y
        # a neighbour that is neither the parent nor a child is the other end of a ring bond: the lower rank opened it
        free, number, out = [True] * 100, {}, []
        for p, a in enumerate(order):
            ring = sorted((rank[y], y, cls) for y, cls in adj[a] if y != parent[a] and parent[y] != a)
            digits, closed = [], []
            for r, y, cls in ring:
                if r < p:
                    k = number.pop((y, a))
                    closed.append(k)
                    digits.append(bond_symbol(y, a, cls))
                else:
                    k = next((i for i in range(1, 100) if free[i]), 0)
                    if k == 0:
                        raise ValueError("Molecule.smiles: more than 99 ring bonds are open at atom %d (the ring limit)" % (a + 1))
                    free[k] = False
                    number[(a, y)] = k
                digits.append("%d" % k if k < 10 else "%%%d" % k)
            for k in closed:
                free[k] = True
            if parent[a] < 0:
                lead = "." if p > 0 else ""
            else:
                lead = ("(" if opens_branch[a] else "") + bond_symbol(parent[a], a, next(cls for y, cls in adj[a] if y == parent[a]))
            mark = ""
            if centre[a] in (1, -1):
                # the neighbours as the text names them: parent, hydrogen, ring numbers as written, children in scan order; the
                # hydrogen is the last of the local order (n stands for it)
                named = ([parent[a]] if parent[a] >= 0 else []) + ([n] if len(adj[a]) == 3 else []) + [y for _, y, _ in ring] \
                    + [y for y, _ in adj[a] if parent[y] == a]
                swaps = sum(named[i] > named[j] for i in range(4) for j in range(i + 1, 4))
                mark = "@" if centre[a] * (-1 if swaps & 1 else 1) > 0 else "@@"
            out.append(lead + token(a, mark) + "".join(digits) + ")" * closes[p])
        return "".join(out), centre


# the text rule's classes: the symbols written without brackets, the ones that may be aromatic, and OUR valence
# lists by charge -1 | 0 | +1 (an isoelectronic shift; no agreement with RDKit's valence model is claimed)
_SMILES_BARE = frozenset(("B", "C", "N", "O", "P", "S", "F", "Cl", "Br", "I"))
_SMILES_AROMATIC = frozenset(("B", "C", "N", "O", "P", "S", "Se"))
_HALOGEN = ((), (1,), (2, 4, 6))
_SMILES_VALENCES = {"B": ((4,), (3,), (2,)), "C": ((3,), (4,), (3,)), "N": ((2,), (3,), (4,)), "O": ((1,), (2,), (3,)),
                    "F": ((), (1,), (2,)), "Si": ((3, 5), (4,), (3,)), "P": ((2, 4, 6), (3, 5), (4,)), "S": ((1,), (2, 4, 6), (3, 5)),
                    "Se": ((1,), (2, 4, 6), (3, 5)), "Cl": _HALOGEN, "Br": _HALOGEN, "I": _HALOGEN, "H": ((), (), ())}
