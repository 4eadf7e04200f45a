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

    def smiles(self, stereo=False, canonical=False, aromatize=False, double_bonds=False, isomeric=False):
        """isomeric=True: canonical(isomeric=True) written with both marks -- the canonical ISOMERIC form: equal strings if and only
        if the stereo graphs are equal ("The isomeric order"), unless canonical_order(isomeric=True)'s status
        says UNDECIDED or COLLISION.  A complete form of its own: stereo=, double_bonds= and canonical= are each refused with it;
        aromatize=True is allowed (the stereo elements are perceived on the perceived rows).
        aromatize=True: aromatized().smiles(stereo, canonical, double_bonds=...) -- the aromatic rings are perceived first
        (perceive_aromatic).
        A deterministic, valid SMILES of this graph by the text rule of DESIGN.md section 7 (the host form and the oracle of
        csrc/smiles.hip, integers only): NOT the canonical string RDKit prints; hs is not read.  stereo=False: wedges are single
        bonds, no mark is written and the positions are not read.  stereo=True: the tetrahedral centres the wedge rows and the
        positions decide (stereo_centres) are written as `@` / `@@` in a bracket token; nothing else of the text changes.
        double_bonds=True: the single bonds at every double bond the positions decide (double_bond_codes: +1 / -1) are written as
        `/` or `\\` in place of their empty symbol; nothing else of the text changes, and the two marks are independent.
        canonical=True: canonical().smiles() -- the same rule on the canonical atom order, so equal graphs give equal strings (not
        RDKit's canonical string either; refused with stereo=True or double_bonds=True: wedge ownership and the drawn geometry are
        not in the invariant).
        ValueError for a row the rule refuses and for more than 99 ring bonds open at once."""
        if isomeric:
            if stereo or double_bonds or canonical:
                raise ValueError("Molecule.smiles: isomeric=True already is canonical=True, stereo=True and double_bonds=True in one "
                                 "(the canonical order that reads the stereo elements); give it alone, or with aromatize=True")
            return (self.aromatized() if aromatize else self).canonical(isomeric=True)._smiles(True, True)[0]
        if aromatize:
            return self.aromatized().smiles(stereo=stereo, canonical=canonical, double_bonds=double_bonds)
        if canonical:
            if stereo or double_bonds:
                raise ValueError("Molecule.smiles: canonical=True with stereo=True or double_bonds=True is not covered (the canonical "
                                 "order does not read wedge ownership or positions)")
            return self.canonical()._smiles(False)[0]
        return self._smiles(bool(stereo), bool(double_bonds))[0]

    def canon_graph(self):
        """(classes, charges, bonds [(i, j, order class)] 0-based, tags) as csrc/graph_canon.hip reads the rows: every atom takes
        part, a row with an end outside 1..n or both ends on one atom is skipped, a wedge is a single bond, a pair listed twice
        counts twice; tag 1 for an atom implicit_hs lists"""
        n = len(self.symbols)
        classes = [canon_atom_class(ATOM_SYMBOLS.index(s)) if s in ATOM_SYMBOLS else 0 for s in self.symbols]
        bonds = [(e1 - 1, e2 - 1, canon_bond_class(o)) for (e1, e2), o in zip(self.bonds, self.orders)
                 if 1 <= e1 <= n and 1 <= e2 <= n and e1 != e2]
        tags = [0] * n
        for a in self.implicit_hs:
            if 1 <= a <= n:
                tags[a - 1] = 1
        return classes, list(self.charges), bonds, tags

    def canonical_order(self, max_tries=None, max_rounds=None, isomeric=False):
        """(rank, stats, key): rank[a] the canonical position of atom a, the CANON_COLUMNS of the search as a dict, the two hash
        words of abc_canon_desc.key -- canonical_labelling on canon_graph().  isomeric=True: the search reads stereo_elements(self)
        as its third key (the host form of abc_canonical_order_stereo) and a fourth value is returned, the STEREO_SEARCH_COLUMNS
        as a list (abc_canon_stereo_desc.stereo_search)."""
        g = self.canon_graph()
        tries = CANON_DEFAULT_TRIES if max_tries is None else max_tries
        rounds = CANON_DEFAULT_ROUNDS if max_rounds is None else max_rounds
        if isomeric:
            rank, st, traces, search = canonical_labelling(g, tries, rounds, stereo=stereo_elements(self)[0])
        else:
            rank, st, traces = canonical_labelling(g, tries, rounds)
        if self.truncated:
            st["status"] |= CANON_TRUNCATED
        key = canon_key(g, rank, traces)
        return (rank, st, key, search) if isomeric else (rank, st, key)

    def canonical(self, max_tries=None, max_rounds=None, isomeric=False):
        """this molecule on its canonical atom order (the host form of abc_canonical_order's canonical rows): atom rows moved to
        their rank; both ends of every bond renumbered in place (end 1 stays end 1); the valid rows first, ascending by (lower end,
        higher end, original row), the rows the graph skips after them verbatim; implicit_hs renumbered, the entries in 1..n ascending,
        the others after them verbatim.  Two molecules with the same graph (classes, charges, order classes, listed atoms) give the
        same symbols, charges, bonds and implicit_hs, whatever their rows' order -- unless a budget ran out (canonical_order's
        status).  isomeric=True: on canonical_order(isomeric=True); two molecules with the same STEREO graph then give the same
        stereo_centres() and double_bond_codes() too, which are the stereo word of the chosen leaf by construction."""
        rank = self.canonical_order(max_tries, max_rounds, isomeric)[0]
        n = len(rank)
        at = sorted(range(n), key=lambda a: rank[a])
        valid, rest = [], []
        for q, (e1, e2) in enumerate(self.bonds):
            if 1 <= e1 <= n and 1 <= e2 <= n and e1 != e2:
                f1, f2 = rank[e1 - 1] + 1, rank[e2 - 1] + 1
                valid.append((min(f1, f2), max(f1, f2), q, [f1, f2]))
            else:
                rest.append((q, [e1, e2]))
        rows = [(q, ends) for _, _, q, ends in sorted(valid)] + rest
        listed = sorted(rank[a - 1] + 1 for a in self.implicit_hs if 1 <= a <= n) + [a for a in self.implicit_hs if not 1 <= a <= n]
        return Molecule([self.symbols[a] for a in at], [self.charges[a] for a in at], [self.hs[a] for a in at],
                        [self.positions[a] for a in at], [ends for _, ends in rows], [self.orders[q] for q, _ in rows], listed,
                        None if self.sources is None else [self.sources[q] for q, _ in rows], self.truncated)

    def aromatic_perception(self):
        """(molecule, stats, codes): this molecule with the bonds of every aromatic cycle set to order 4 (perceive_aromatic on the
        rows as csrc/aromatic.hip reads them: the host form of abc_perceive_aromatic's molecule side), the AROMATIC_COLUMNS of the
        pass as a dict, and the code of every atom (AROM_NOT_CANDIDATE, AROM_NONE or its electrons).  Only orders and implicit_hs
        change: an atom implicit_hs does not list whose hydrogen count by the text rule (text_hydrogens) is 1 on these rows and 0 on
        the perceived ones is appended, the new entries ascending -- pyrrole stays [nH]1cccc1."""
        n = len(self.symbols)
        rows = [(e1 - 1, e2 - 1, o) for (e1, e2), o in zip(self.bonds, self.orders)]
        orders, codes, st = perceive_aromatic((self.symbols, self.charges, rows))
        before, after = [[] for _ in range(n)], [[] for _ in range(n)]
        for (i, j, o), o2 in zip(rows, orders):
            if 0 <= i < n and 0 <= j < n and i != j:
                for a in (i, j):
                    before[a].append(canon_bond_class(o))
                    after[a].append(canon_bond_class(o2))
        listed = {a - 1 for a in self.implicit_hs}
        new = [a + 1 for a in range(n) if a not in listed and before[a] != after[a]
               and text_hydrogens(self.symbols[a], self.charges[a], before[a]) == 1
               and text_hydrogens(self.symbols[a], self.charges[a], after[a]) == 0]
        st["listed"] = len(new)
        if self.truncated:
            st["status"] |= 2
        m = Molecule(self.symbols, self.charges, self.hs, self.positions, self.bonds, orders, self.implicit_hs + new, self.sources, self.truncated)
        return m, st, codes

    def aromatized(self):
        """aromatic_perception()[0]: what every stage downstream takes in place of this molecule"""
        return self.aromatic_perception()[0]

    def stereo_centres(self):
        """one code per atom by the stereo rule of DESIGN.md section 7: 0 no candidate, +1 / -1 the local parity s(a) of a marked
        centre, 2 flat, 3 unqualified (abc_smiles_stereo_desc.stereo_out).  ValueError as smiles()."""
        return self._smiles(True)[1]

    def double_bond_codes(self):
        """one code per bond row by the double-bond rule of DESIGN.md section 7: 0 not a candidate, +1 / -1 a marked double bond
        (the lowest-index substituents of its two ends on one side / on opposite sides), 2 flat, 3 on a cycle, 4 an end with twin
        leaves (abc_smiles_ez_desc.ez_out).  ValueError as smiles()."""
        return self._smiles(False, True)[2]

    def _smiles(self, stereo, double_bonds=False):
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
            return text_hydrogens(s, c, [cls for _, cls in adj[a]])

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
        low = [0] * n      # double bonds: the least rank a subtree reaches by one ring bond (a tree bond to c is a bridge iff low[c] == rank[c])
        for root in range(n):
            if rank[root] >= 0:
                continue
            rank[root] = low[root] = len(order)
            order.append(root)
            cur = root
            while cur >= 0:
                if cursor[cur] == len(adj[cur]):
                    if parent[cur] >= 0:
                        low[parent[cur]] = min(low[parent[cur]], low[cur])
                    cur = parent[cur]
                    continue
                y = adj[cur][cursor[cur]][0]
                cursor[cur] += 1
                if rank[y] >= 0 and y != parent[cur]:
                    low[cur] = min(low[cur], rank[y])
                if rank[y] < 0:
                    if last_child[cur] >= 0:      # the child before this one was not the last: it stands in a branch, which
                        opens_branch[last_child[cur]] = True      # ends behind the atom visited last
                        closes[len(order) - 1] += 1
                    last_child[cur], parent[y], rank[y] = y, cur, len(order)
                    low[y] = len(order)
                    order.append(y)
                    cur = y

        # double bonds: the code of every bond row (0 none, +1 / -1 marked, 2 flat, 3 ring, 4 twin); of a marked one both ends are kept:
        # end atom -> [partner, {substituent: side}, u (0: not fixed yet)]
        ez_codes, end = [0] * len(self.bonds), {}
        if double_bonds:
            def leaf(s):
                return len(adj[s]) == 1, self.symbols[s], self.charges[s], listed[s]

            for k, ((e1, e2), o) in enumerate(zip(self.bonds, self.orders)):
                if o != 2:
                    continue
                a, b = min(e1, e2) - 1, max(e1, e2) - 1
                subs = {e: [s for s, _ in adj[e] if s != p] for e, p in ((a, b), (b, a))}
                if not all(self.symbols[e] in ("C", "N") and len(adj[e]) in (2, 3) and all(cls == 1 for s, cls in adj[e] if s != p)
                           for e, p in ((a, b), (b, a))):
                    continue
                child = b if parent[b] == a else (a if parent[a] == b else -1)
                if child < 0 or low[child] != rank[child]:
                    ez_codes[k] = 3
                    continue
                if any(len(subs[e]) == 2 and leaf(subs[e][0])[0] and leaf(subs[e][0]) == leaf(subs[e][1]) for e in (a, b)):
                    ez_codes[k] = 4
                    continue
                pos = self.positions
                dx, dy = pos[b][0] - pos[a][0], pos[b][1] - pos[a][1]
                side = {e: [dx * (pos[s][1] - pos[e][1]) - dy * (pos[s][0] - pos[e][0]) for s in subs[e]] for e in (a, b)}
                side = {e: [(t > 0) - (t < 0) for t in ts] for e, ts in side.items()}
                if (any(not 0 <= v <= 199999 for j in [a, b] + subs[a] + subs[b] for v in pos[j])
                        or any(t == 0 for e in (a, b) for t in side[e]) or any(len(side[e]) == 2 and side[e][0] == side[e][1] for e in (a, b))):
                    ez_codes[k] = 2
                    continue
                ez_codes[k] = 1 if side[a][0] == side[b][0] else -1
                end[a], end[b] = [b, dict(zip(subs[a], side[a])), 0], [a, dict(zip(subs[b], side[b])), 0]

        def direction(first, second):
            """the symbol of a class-1 bond read first -> second, None where no marked double bond claims it.  The first symbol met
            of a group of double bonds joined by shared single bonds fixes the group's orientation: it is "/"."""
            claims = [(e, s, sign) for e, s, sign in ((first, second, 1), (second, first, -1)) if e in end]
            if not claims:
                return None
            e, s, sign = claims[0]
            if end[e][2] == 0:
                end[e][2] = end[end[e][0]][2] = sign * end[e][1][s]
                todo = [e]
                while todo:
                    x = todo.pop()
                    for x in (x, end[x][0]):
                        for t, side_t in end[x][1].items():
                            if t in end and end[t][2] == 0:
                                end[t][2] = end[end[t][0]][2] = -end[x][2] * side_t * end[t][1][x]
                                todo.append(t)
            ups = {sign * end[e][2] * end[e][1][s] for e, s, sign in claims}
            assert len(ups) == 1, "the two readings of the bond (%d, %d) disagree" % (first + 1, second + 1)
            return "/" if ups == {1} else "\\"

        # a neighbour that is neither the parent nor a child is the other end of a ring bond: the lower rank opened it
        free, number, out = [True] * 100, {}, []
        for p, a in enumerate(order):
            if parent[a] < 0:
                lead = "." if p > 0 else ""
            else:
                cls = next(cls for y, cls in adj[a] if y == parent[a])
                lead = ("(" if opens_branch[a] else "") + ((cls == 1 and direction(parent[a], a)) or bond_symbol(parent[a], a, cls))
            ring = sorted((rank[y], y, cls) for y, cls in adj[a] if y != parent[a] and parent[y] != a)
            digits, closed = [], []
            for r, y, cls in ring:
                if r < p:
                    k = number.pop((y, a))
                    closed.append(k)
                    digits.append((cls == 1 and direction(a, y)) or bond_symbol(y, a, cls))      # (the closer bears the symbol)
                else:
                    k = next((i for i in range(1, 100) if free[i]), 0)
                    if k == 0:
                        raise ValueError("Molecule.smiles: more than 99 ring bonds are open at atom %d (the ring limit)" % (a + 1))
                    free[k] = False
                    number[(a, y)] = k
                digits.append("%d" % k if k < 10 else "%%%d" % k)
            for k in closed:
                free[k] = True
            mark = ""
            if centre[a] in (1, -1):
                # the neighbours as the text names them: parent, hydrogen, ring numbers as written, children in scan order; the
                # hydrogen is the last of the local order (n stands for it)
                named = ([parent[a]] if parent[a] >= 0 else []) + ([n] if len(adj[a]) == 3 else []) + [y for _, y, _ in ring] \
                    + [y for y, _ in adj[a] if parent[y] == a]
                swaps = sum(named[i] > named[j] for i in range(4) for j in range(i + 1, 4))
                mark = "@" if centre[a] * (-1 if swaps & 1 else 1) > 0 else "@@"
            out.append(lead + token(a, mark) + "".join(digits) + ")" * closes[p])
        return "".join(out), centre, ez_codes


# ------------------------------------------------------------------------------------------------- the canonical atom order
# The host form of csrc/graph_canon.hip (the contract: include/abcnet_hip.h, abc_canon_desc): an
# individualise-and-refine search over EVERY branch that keeps the least leaf, with the device's budgets and counters, so that order,
# stats, key and certificate are comparable with the kernel word for word.  Integers only (uint64, wrapping).
CANON_COLUMNS = ("status", "leaves", "tries", "rounds", "levels_max", "pruned_trace", "pruned_orbit", "automorphisms", "improved")
CANON_EMPTY, CANON_TRUNCATED, CANON_UNDECIDED, CANON_COLLISION = 1, 2, 4, 8
CANON_DEFAULT_TRIES, CANON_DEFAULT_ROUNDS, CANON_ORBIT_LEVELS = 4096, 16384, 8
_M64 = (1 << 64) - 1
_GOLD, _CANON_TAG, _CANON_BOND = 0x9E3779B97F4A7C15, 0xD6E8FEB86659FD93, 0xC2B2AE3D27D4EB4F
_U = np.uint64


def _mix(x):
    """the splitmix64 finaliser (csrc/graph_ids.hpp)"""
    x &= _M64
    x ^= x >> 30
    x = (x * 0xBF58476D1CE4E5B9) & _M64
    x ^= x >> 27
    x = (x * 0x94D049BB133111EB) & _M64
    return x ^ (x >> 31)


def _mixv(x):
    x = x ^ (x >> _U(30))
    x = x * _U(0xBF58476D1CE4E5B9)
    x = x ^ (x >> _U(27))
    x = x * _U(0x94D049BB133111EB)
    return x ^ (x >> _U(31))


def canon_atom_class(t):
    """the class of a vocabulary index (csrc/mol_rows.hpp, atom_class): outside 0..13 -> 0, index 0 -> carbon"""
    t = int(t)
    return 0 if t < 0 or t > 13 else (1 if t == 0 else t)


def canon_bond_class(c):
    """the order class of a bond code (csrc/graph_ids.hpp, bond_class): a wedge is a single bond"""
    c = int(c)
    return 1 if c in (5, 6) else (c if 1 <= c <= 4 else 0)


def canon_leaf_hash(graph, rank):
    """h of a leaf: the wrapping sum, over the atoms, of mix(mix(mix(mix(rank + 1) + class + 1) + charge) + tag) and, over the valid
    rows, of mix(mix((lower rank << 32 | higher rank) + 0xC2B2AE3D27D4EB4F) + order class)"""
    classes, charges, bonds, tags = graph
    h = 0
    for a in range(len(classes)):
        h += _mix(_mix(_mix(_mix(rank[a] + 1) + classes[a] + 1) + (charges[a] & _M64)) + tags[a])
    for i, j, o in bonds:
        lo, hi = min(rank[i], rank[j]), max(rank[i], rank[j])
        h += _mix(_mix(((lo << 32) | hi) + _CANON_BOND) + o)
    return h & _M64


def canon_key(graph, rank, traces):
    """(h, mix(mix(mix(n) + m) + sum over the levels l of mix(mix(mix(mix(l + 1) + rounds) + classes) + sum))): a HASH of the
    relabelled graph, equal for equal graphs"""
    t = sum(_mix(_mix(_mix(_mix(l + 1) + k) + c) + s) for l, (k, c, s) in enumerate(traces)) & _M64
    return canon_leaf_hash(graph, rank), _mix(_mix(_mix(len(graph[0])) + len(graph[2])) + t)


def canon_certificate(graph, rank):
    """the relabelled graph itself: n, m, the packed word (charge << 5 | tag << 4 | class, as int32) of the atom at every rank, then
    the (lower rank, higher rank, order class) triples in ascending order"""
    classes, charges, bonds, tags = graph
    n = len(classes)
    at = [0] * n
    for a in range(n):
        w = ((charges[a] << 5) | (tags[a] << 4) | classes[a]) & 0xFFFFFFFF
        at[rank[a]] = w - (1 << 32) if w >> 31 else w
    tri = sorted((min(rank[i], rank[j]), max(rank[i], rank[j]), o) for i, j, o in bonds)
    return [n, len(bonds)] + at + [v for t in tri for v in t]


class _CanonStop(Exception):
    def __init__(self, bit):
        self.bit = bit


def stereo_word(stereo, rank):
    """the STEREO WORD of a leaf: one byte per canonical position, centre part | double-bond part << 2, each 0 none, 1 for +1, 2 for
    -1.  Centre part of the atom at the position: s(a) times the sign of the permutation that sorts its neighbours by rank (the
    hydrogen stays last).  Double-bond part, at the lower-RANK end: the bond's code times f(a) f(b), f(e) = -1 iff end e has two
    substituents and the lower-ranked one is not the lower-indexed one -- "lowest-rank substituents together / opposite".
    stereo: the element table of stereo_elements."""
    word = [0] * len(rank)
    for a, row in enumerate(stereo):
        if row[0] in (1, -1):
            nb = [rank[j] for j in row[1:5] if j >= 0]
            swaps = sum(nb[i] > nb[j] for i in range(len(nb)) for j in range(i + 1, len(nb)))
            word[rank[a]] |= 1 if row[0] * (-1 if swaps & 1 else 1) > 0 else 2
        if row[5] in (1, -1):
            v = row[5]
            for lo, hi in ((row[8], row[9]), (row[10], row[11])):
                if hi >= 0 and rank[lo] > rank[hi]:
                    v = -v
            word[min(rank[a], rank[row[7]])] |= (1 if v > 0 else 2) << 2
    return word


def canonical_labelling(graph, max_tries=CANON_DEFAULT_TRIES, max_rounds=CANON_DEFAULT_ROUNDS, stereo=None):
    """graph = (classes [n], charges [n], bonds [(i, j, order class)] 0-based, tags [n]) -> (rank [n], stats dict over CANON_COLUMNS,
    traces [(rounds, classes, sum)] of the chosen leaf).  rank[a] is the canonical position of atom a: the ranks of the least leaf
    under (trace_0, trace_1, .., h) of the search tree, certain unless the status says UNDECIDED (a budget ran out: the best leaf so
    far, or the identity order before any leaf) or COLLISION (two 64-bit sums collided; the best leaf so far).
    stereo (None: the plain search, as ever): the element table of stereo_elements.  The order of the leaves becomes (traces, h,
    stereo_word), the word compared exactly, position by position; a leaf of equal h is mapped onto the best and verified as ever,
    then: words equal -- an automorphism of the STEREO graph, merged and jumped as ever; word smaller -- the leaf becomes the best,
    nothing is merged; greater -- a normal backtrack.  Only automorphisms that keep the stereo prune.  A fourth value is then
    returned: [leaves of equal h and unequal word, stereo improvements, stereo automorphisms, 0] (STEREO_SEARCH_COLUMNS)."""
    classes, charges, bonds, tags = graph
    n = len(classes)
    st = dict.fromkeys(CANON_COLUMNS, 0)
    if n == 0:
        return ([], st, []) if stereo is None else ([], st, [], [0, 0, 0, 0])
    bi = np.array([q[0] for q in bonds], dtype=np.int64)
    bj = np.array([q[1] for q in bonds], dtype=np.int64)
    bo = np.array([q[2] for q in bonds], dtype=_U)
    deg = [0] * n
    for i, j, _ in bonds:
        deg[i] += 1
        deg[j] += 1
    init = []
    for a in range(n):
        e = _mix(_mix(_mix(classes[a] + 1) + (charges[a] & _M64)) + deg[a])
        init.append(_mix(e + _CANON_TAG * tags[a]) if tags[a] else e)
    init = np.array(init, dtype=_U)

    def one_round(ids, r):
        if st["rounds"] >= max_rounds:
            raise _CanonStop(CANON_UNDECIDED)
        st["rounds"] += 1
        acc = np.zeros(n, dtype=_U)
        with np.errstate(over="ignore"):
            np.add.at(acc, bi, _mixv(_mixv(ids[bj]) + bo))
            np.add.at(acc, bj, _mixv(_mixv(ids[bi]) + bo))
            return _mixv(_mixv(ids + _U(r)) + acc)

    def individualise(ids, v, level):
        ids[v] = _U(_mix(_mix(int(ids[v])) + _GOLD * (level + 1)))

    def automorphism(ids, best_ids):
        """the map by equal id, or None unless it keeps every label and the multiset of the bonds"""
        where = {e: y for y, e in enumerate(best_ids.tolist())}
        gamma = [where.get(e, -1) for e in ids.tolist()]
        if any(y < 0 or (classes[x], charges[x], tags[x]) != (classes[y], charges[y], tags[y]) for x, y in enumerate(gamma)):
            return None
        key = lambda i, j, o: (min(i, j), max(i, j), o)
        if sorted(key(gamma[i], gamma[j], o) for i, j, o in bonds) != sorted(key(i, j, o) for i, j, o in bonds):
            return None
        return gamma

    def merge(parent, gamma):
        """x ~ gamma(x): a union-find whose root is the least atom of the orbit, left flat"""
        def find(x):
            while parent[x] != x:
                x = parent[x]
            return x
        for x, y in enumerate(gamma):
            x, y = find(x), find(y)
            if x != y:
                parent[max(x, y)] = min(x, y)
        for x in range(n):
            parent[x] = find(x)

    cur = [(0, 0, 0)] * n                               # the trace of every level of the current path
    cell, cell_max, choice, nxt = [0] * n, [0] * n, [0] * n, [0] * n
    orbit = [list(range(n)) for _ in range(CANON_ORBIT_LEVELS + 1)]
    best = None                                         # (traces, choices, ids, h, rank[, word]) of the least leaf so far
    search = [0, 0, 0, 0]                               # stereo: STEREO_SEARCH_COLUMNS
    less_from = None                                    # the level at which the path became less than the best; None: equal so far
    try:
        ids, r, level = init.copy(), 0, 0
        prev = len(np.unique(ids))
        mode, target = "refine", -1
        while True:
            if mode == "refine":
                k = 0
                while True:
                    r += 1
                    k += 1
                    ids = one_round(ids, r)
                    c = len(np.unique(ids))
                    if c <= prev or k >= n:
                        break
                    prev = c
                with np.errstate(over="ignore"):
                    trace = (k, c, int(np.sum(_mixv(ids), dtype=_U)))
                cur[level] = trace
                st["levels_max"] = max(st["levels_max"], level)
                mode, target = "back", level - 1
                if best is not None and less_from is None:
                    if trace > best[0][level]:
                        st["pruned_trace"] += 1
                        continue
                    if trace < best[0][level]:
                        less_from = level
                if c == n:
                    st["leaves"] += 1
                    order = np.argsort(ids, kind="stable")
                    rank = [0] * n
                    for k2, a in enumerate(order.tolist()):
                        rank[a] = k2
                    h = canon_leaf_hash(graph, rank)
                    word = None if stereo is None else stereo_word(stereo, rank)
                    if best is None or less_from is not None or h < best[3]:
                        st["improved"] += best is not None
                        best, less_from = (cur[:level + 1], choice[:level], ids.copy(), h, rank, word), None
                    elif h == best[3]:
                        gamma = automorphism(ids, best[2])
                        if gamma is None:
                            raise _CanonStop(CANON_COLLISION)
                        if word != best[5]:
                            search[0] += 1
                            if word < best[5]:
                                search[1] += 1
                                st["improved"] += 1
                                best = (cur[:level + 1], choice[:level], ids.copy(), h, rank, word)
                            continue
                        search[2] += stereo is not None
                        st["automorphisms"] += 1
                        target = next(l for l in range(level) if choice[l] != best[1][l])
                        for l in range(min(target, CANON_ORBIT_LEVELS) + 1):
                            merge(orbit[l], gamma)
                    continue
                if level + 1 >= n:                       # (only colliding hashes can get here)
                    raise _CanonStop(CANON_COLLISION)
                vals, counts = np.unique(ids, return_counts=True)
                cell[level] = vals[counts > 1][0]
                cell_max[level] = int(np.flatnonzero(ids == cell[level])[-1])
                nxt[level] = 0
                if level <= CANON_ORBIT_LEVELS:
                    orbit[level] = list(range(n))
                mode = "child"
            if mode == "child":
                v = None
                for a in np.flatnonzero(ids == cell[level]).tolist():
                    if a < nxt[level]:
                        continue
                    if level <= CANON_ORBIT_LEVELS and orbit[level][a] != a:
                        st["pruned_orbit"] += 1
                        continue
                    v = a
                    break
                if v is None:
                    mode, target = "back", level - 1
                    continue
                if st["tries"] >= max_tries:
                    raise _CanonStop(CANON_UNDECIDED)
                st["tries"] += 1
                choice[level], nxt[level] = v, v + 1
                individualise(ids, v, level)
                prev = cur[level][1] + 1
                level += 1
                mode = "refine"
                continue
            # back: to the nearest level at or above `target` that still has an atom of its cell to try, its ids rebuilt by replay
            while target >= 0 and nxt[target] > cell_max[target]:
                target -= 1
            if target < 0:
                break
            level = target
            if less_from is not None and less_from > level:
                less_from = None
            ids, r = init.copy(), 0
            for k in range(level + 1):
                for _ in range(cur[k][0]):
                    r += 1
                    ids = one_round(ids, r)
                if k < level:
                    individualise(ids, choice[k], k)
            mode = "child"
    except _CanonStop as stop:
        st["status"] |= stop.bit
    out = (list(range(n)), st, []) if best is None else (best[4], st, best[0])
    return out if stereo is None else out + (search,)


# ------------------------------------------------------------------------------------------------- the stereo elements
# The host form of csrc/stereo.hip (the contract: include/abcnet_hip.h, abc_stereo_desc; the layout: contract.STEREO_ELEMENT):
# what the two stereo rules decide, as a table the canonical search can read.
STEREO_W = 12
STEREO_NONE_ROW = (0, -1, -1, -1, -1, 0, -1, -1, -1, -1, -1, -1)
STEREO_STATS_COLUMNS = ("centres", "double_bonds", "flat", "status")
STEREO_SEARCH_COLUMNS = ("unequal", "improved", "automorphisms", "reserved")
STEREO_BAD_ROW = 4      # ABC_TEXT_BAD_ROW


def stereo_elements(mol):
    """(table [n][STEREO_W], stats [4]) of a Molecule, from its stereo_centres() and double_bond_codes().  Per atom row: [0] the
    centre code (0, +1 / -1, 2 flat, 3 unqualified); [1..4] for a +1 / -1 centre its neighbours' 0-based rows ascending, the
    hydrogen of a three-neighbour centre as -1 in the last place, else -1; [5] for the lower-index end of a candidate double bond the
    code of that bond row (+1 / -1, 2, 3, 4), else 0; [6..11] for a +1 / -1 bond: the bond row, the partner, this end's one or two
    substituents ascending (-1 for none), the partner's likewise, else -1.  stats: marked centres, marked double bonds, flat (both
    kinds), status (1 EMPTY is the device's alone; 2 truncated; STEREO_BAD_ROW a row the writer refuses: the table is then all
    STEREO_NONE_ROW).  (The writer's ring limit, which the perception does not have, is a refusal here too.)"""
    n = len(mol.symbols)
    status = 2 if mol.truncated else 0
    try:
        _, centre, ez = mol._smiles(True, True)
    except ValueError:
        return [list(STEREO_NONE_ROW) for _ in range(n)], [0, 0, 0, status | STEREO_BAD_ROW]
    adj = [[] for _ in range(n)]
    for e1, e2 in mol.bonds:
        adj[e1 - 1].append(e2 - 1)
        adj[e2 - 1].append(e1 - 1)
    table = [list(STEREO_NONE_ROW) for _ in range(n)]
    for a, c in enumerate(centre):
        table[a][0] = c
        if c in (1, -1):
            table[a][1:5] = (sorted(adj[a]) + [-1])[:4]
    for k, c in enumerate(ez):
        if c == 0:
            continue
        a, b = min(mol.bonds[k]) - 1, max(mol.bonds[k]) - 1
        table[a][5] = c
        if c in (1, -1):
            subs = [(sorted(s for s in adj[e] if s != p) + [-1])[:2] for e, p in ((a, b), (b, a))]
            table[a][6:12] = [k, b] + subs[0] + subs[1]
    flat = sum(c == 2 for c in centre) + sum(c == 2 for c in ez)
    return table, [sum(c in (1, -1) for c in centre), sum(c in (1, -1) for c in ez), flat, status]


# the text rule's classes: the symbols written without brackets, the ones that may be aromatic, and OUR valence
# lists by charge -1 | 0 | +1 (an isoelectronic shift; no agreement with RDKit's valence model is claimed)
_SMILES_BARE = frozenset(("B", "C", "N", "O", "P", "S", "F", "Cl", "Br", "I"))
_SMILES_AROMATIC = frozenset(("B", "C", "N", "O", "P", "S", "Se"))
_HALOGEN = ((), (1,), (2, 4, 6))
_SMILES_VALENCES = {"B": ((4,), (3,), (2,)), "C": ((3,), (4,), (3,)), "N": ((2,), (3,), (4,)), "O": ((1,), (2,), (3,)),
                    "F": ((), (1,), (2,)), "Si": ((3, 5), (4,), (3,)), "P": ((2, 4, 6), (3, 5), (4,)), "S": ((1,), (2, 4, 6), (3, 5)),
                    "Se": ((1,), (2, 4, 6), (3, 5)), "Cl": _HALOGEN, "Br": _HALOGEN, "I": _HALOGEN, "H": ((), (), ())}


def text_hydrogens(symbol, charge, classes):
    """the hydrogen count h of an UNLISTED atom by the text rule (csrc/text_hydrogens.hpp): classes = the order
    classes of its bonds; v = (3 per class-4 bond + 2 * class per other bond) // 2; h = t - v for the first t >= v of the valence list
    of the symbol at this charge, else 0; 0 for H and for a charge outside -1..1"""
    if symbol == "H" or abs(charge) > 1 or symbol not in _SMILES_VALENCES:
        return 0
    v = sum(3 if cls == 4 else 2 * cls for cls in classes) // 2
    return next((t - v for t in _SMILES_VALENCES[symbol][charge + 1] if t >= v), 0)


# ------------------------------------------------------------------------------------------------- aromaticity perception
# The host form of csrc/aromatic.hip (the contract: include/abcnet_hip.h, abc_aromatic_desc): the rule is this
# project's own, a function of the graph alone, integers only; codes and stats are comparable with the kernel word for word.
AROMATIC_COLUMNS = ("status", "candidates", "cycles", "aromatic", "rows_changed", "listed")
AROM_NOT_CANDIDATE, AROM_NONE = -2, -1
_AROM_LONE_PAIR = frozenset(("O", "S", "Se"))


def perceive_aromatic(graph):
    """graph = (symbols [n] (None or a string outside the vocabulary: no symbol), charges [n], rows [(i, j, order code)] with 0-based
    ends as they are listed, any integers) -> (orders [m], codes [n], stats dict over AROMATIC_COLUMNS; `status` and `listed` are
    the caller's).  A row is valid when both ends are in 0..n-1 and differ; orders[q] is 4 for a row on an aromatic cycle and the
    row's own code otherwise; codes[a] is AROM_NOT_CANDIDATE, AROM_NONE or the electrons e(a)."""
    symbols, charges, rows = graph
    n = len(symbols)
    at = [[] for _ in range(n)]          # per atom: (neighbour, order class, row)
    for q, (i, j, o) in enumerate(rows):
        if 0 <= i < n and 0 <= j < n and i != j:
            cls = canon_bond_class(o)
            at[i].append((j, cls, q))
            at[j].append((i, cls, q))

    def candidate(a):
        cls = [c for _, c, _ in at[a]]
        return (symbols[a] in _SMILES_AROMATIC and -1 <= charges[a] <= 1 and len(at[a]) in (2, 3) and 0 not in cls and 3 not in cls
                and cls.count(2) <= 1 and len({y for y, _, _ in at[a]}) == len(at[a]))

    cand = [candidate(a) for a in range(n)]

    def cycles():
        """every candidate cycle once, as its atoms: from its least atom, the second atom below the last"""
        for s in range(n):
            if not cand[s]:
                continue
            stack = [(s, iter(at[s]))]
            path = [s]
            while stack:
                step = next(stack[-1][1], None)
                if step is None:
                    stack.pop()
                    path.pop()
                    continue
                v = step[0]
                if v == s:
                    if len(path) >= 5 and path[1] < path[-1]:
                        yield list(path)
                    continue
                if v < s or not cand[v] or v in path or len(path) == 7:
                    continue
                path.append(v)
                stack.append((v, iter(at[v])))

    def rows_of(cycle):
        return [next(q for y, _, q in at[u] if y == v) for u, v in zip(cycle, cycle[1:] + cycle[:1])]

    found = list(cycles())
    ring = {q for c in found for q in rows_of(c)}

    def electrons(a):
        s, c, d = symbols[a], charges[a], len(at[a])
        double = [(y, q) for y, cls, q in at[a] if cls == 2]
        if double:
            y, q = double[0]
            return 1 if q in ring else (0 if symbols[y] in ("N",) or symbols[y] in _AROM_LONE_PAIR else AROM_NONE)
        has4 = any(cls == 4 for _, cls, _ in at[a])
        if s == "C":
            return (2, (1 if has4 else AROM_NONE), 0)[c + 1]
        if s == "B":
            return 0 if c == 0 else AROM_NONE
        if s in ("N", "P"):
            return (2, ((2 if d == 3 else 1) if has4 else 2), (1 if has4 else AROM_NONE))[c + 1]
        return 2 if c == 0 else AROM_NONE

    codes = [electrons(a) if cand[a] else AROM_NOT_CANDIDATE for a in range(n)]
    aromatic = [c for c in found if all(codes[a] >= 0 for a in c) and sum(codes[a] for a in c) == 6]
    marked = {q for c in aromatic for q in rows_of(c)}
    orders = [4 if q in marked else o for q, (_, _, o) in enumerate(rows)]
    st = dict.fromkeys(AROMATIC_COLUMNS, 0)
    st.update(candidates=sum(cand), cycles=len(found), aromatic=len(aromatic), rows_changed=sum(o != o2 for (_, _, o), o2 in zip(rows, orders)))
    return orders, codes, st


# ---------------------------------------------------------------------------------------------------------- the SMILES reader
# enum abc_smiles_read_status: the status word of abc_read_smiles, exactly one value per string, in order of priority
READ_OK, READ_EMPTY, READ_TOO_LONG, READ_SYNTAX, READ_TRUNCATED, READ_DUPLICATE = 0, 1, 2, 3, 4, 5
READ_STATUS_NAMES = ("OK", "EMPTY", "TOO_LONG", "SYNTAX", "TRUNCATED", "DUPLICATE")
MAX_SMILES_READ_BYTES = 4096     # ABC_MAX_SMILES_READ_BYTES
READ_STATS_COLUMNS = ("bytes", "atoms", "bonds", "ring_bonds")
_READ_BARE = {b"B": 9, b"C": 1, b"N": 2, b"O": 3, b"P": 4, b"S": 7, b"F": 5, b"I": 11}
_READ_ORDER = {b"-": 1, b"/": 1, b"\\": 1, b"=": 2, b"#": 3, b":": 4}
_EMPTY_RECORD = (np.zeros((0, 4), dtype=np.int32), np.zeros((0, 3), dtype=np.int32))


def smiles_bytes(text):
    """the bytes of one string as the reader takes them: bytes as they are, a str in ASCII with `?` (a syntax error) for every
    character outside it"""
    if isinstance(text, (bytes, bytearray)):
        return bytes(text)
    if not isinstance(text, str):
        raise ValueError("a SMILES string must be a str (or its bytes), got %s" % type(text).__name__)
    return text.encode("ascii", "replace")


def _read_class(symbol):
    """the record's atom class of a symbol with its first letter in upper case: the raster.ATOM_VOCAB index, -1 outside it"""
    return ATOM_SYMBOLS.index(symbol, 1) if symbol in ATOM_SYMBOLS[1:] else -1


def _read_bracket(s, i):
    """the bracket atom whose `[` stands at s[i] -> (end, class, charge, aromatic), or None"""
    def digits(k):
        while s[k:k + 1].isdigit():
            k += 1
        return k

    def upper(k):
        return b"A" <= s[k:k + 1] <= b"Z"

    k = digits(i + 1)                                    # isotope
    if s[k:k + 1] == b"*":
        symbol, aromatic, k = "*", False, k + 1
    elif upper(k):
        n = 2 if b"a" <= s[k + 1:k + 2] <= b"z" else 1
        symbol, aromatic, k = s[k:k + n].decode(), False, k + n
    elif s[k:k + 2] in (b"se", b"as", b"te"):
        symbol, aromatic, k = s[k:k + 2].decode().capitalize(), True, k + 2
    elif s[k:k + 1] in (b"b", b"c", b"n", b"o", b"p", b"s") and k < len(s):
        symbol, aromatic, k = s[k:k + 1].decode().upper(), True, k + 1
    else:
        return None
    if s[k:k + 1] == b"@":                               # chirality: @ or @@, then a class such as TH1
        k += 2 if s[k + 1:k + 2] == b"@" else 1
        if upper(k) and upper(k + 1) and s[k + 2:k + 3].isdigit():
            k = digits(k + 2)
    if s[k:k + 1] == b"H":                               # hydrogens
        k += 2 if s[k + 1:k + 2].isdigit() else 1
    charge = 0
    if s[k:k + 1] in (b"+", b"-"):
        sign = s[k:k + 1]
        unit = 1 if sign == b"+" else -1
        k += 1
        if s[k:k + 1].isdigit():
            e = k + 2 if s[k + 1:k + 2].isdigit() else k + 1
            charge, k = unit * int(s[k:e]), e
        else:
            n = 1
            while n < 3 and s[k:k + 1] == sign:
                n, k = n + 1, k + 1
            charge = unit * n
        if not -15 <= charge <= 15:
            return None
    if s[k:k + 1] == b":":                               # atom class
        if not s[k + 1:k + 2].isdigit():
            return None
        k = digits(k + 1)
    if s[k:k + 1] != b"]":
        return None
    return k + 1, _read_class(symbol), charge, aromatic


def parse_smiles(text, max_atoms=None, max_bonds=None):
    """One SMILES string read into a graph record by the reading rule of DESIGN.md section 7 (the host form and the reference of
    csrc/smiles_read.hip; a stated subset of OpenSMILES, no claim about what RDKit accepts): -> (status, atoms int32 [n, 4]
    (0, 0, class, charge), bonds int32 [m, 3] (i < j, order)), status one of READ_*; every status but READ_OK comes with an empty
    record.  Sequential: one pass with the previous atom, the pending bond symbol, the branch stack and the open ring numbers."""
    s = smiles_bytes(text)
    if len(s) == 0:
        return (READ_EMPTY,) + _EMPTY_RECORD
    if len(s) > MAX_SMILES_READ_BYTES:
        return (READ_TOO_LONG,) + _EMPTY_RECORD
    syntax = (READ_SYNTAX,) + _EMPTY_RECORD
    atoms, aromatic, bonds = [], [], []
    prev, pending, stack, rings = None, 0, [], {}
    need_atom, after_close = True, False          # after the start, `(` and `.`; between `)` and the next atom
    i = 0
    while i < len(s):
        c = s[i:i + 1]
        atom = None                               # (end, class, charge, aromatic)
        if c == b"[":
            atom = _read_bracket(s, i)
            if atom is None:
                return syntax
        elif s[i:i + 2] in (b"Cl", b"Br"):
            atom = (i + 2, 6 if c == b"C" else 8, 0, False)
        elif c in _READ_BARE:
            atom = (i + 1, _READ_BARE[c], 0, False)
        elif c in (b"b", b"c", b"n", b"o", b"p", b"s"):
            atom = (i + 1, _READ_BARE[c.upper()], 0, True)
        elif c == b"*":
            atom = (i + 1, -1, 0, False)
        if atom is not None:
            a = len(atoms)
            atoms.append((0, 0, atom[1], atom[2]))
            aromatic.append(atom[3])
            if prev is not None:
                bonds.append((prev, a, pending or (4 if aromatic[prev] and atom[3] else 1)))
            prev, pending, need_atom, after_close, i = a, 0, False, False, atom[0]
        elif c in _READ_ORDER:
            if prev is None or pending:
                return syntax
            pending, i = _READ_ORDER[c], i + 1
        elif c.isdigit() or c == b"%":
            if c == b"%":
                if not (s[i + 1:i + 2].isdigit() and s[i + 2:i + 3].isdigit()):
                    return syntax
                number, i = int(s[i + 1:i + 3]), i + 3
            else:
                number, i = int(c), i + 1
            if prev is None or need_atom or after_close:      # a number is attached to the atom token before it
                return syntax
            if number in rings:
                first, symbol = rings.pop(number)
                if first == prev or (symbol and pending and symbol != pending):
                    return syntax
                bonds.append((first, prev, symbol or pending or (4 if aromatic[first] and aromatic[prev] else 1)))
            else:
                rings[number] = (prev, pending)
            pending = 0
        elif c == b"(":
            if prev is None or pending or need_atom:
                return syntax
            stack.append(prev)
            need_atom, i = True, i + 1
        elif c == b")":
            if not stack or pending or need_atom:
                return syntax
            prev, after_close, i = stack.pop(), True, i + 1
        elif c == b".":
            if stack or pending or need_atom:
                return syntax
            prev, need_atom, i = None, True, i + 1
        else:
            return syntax
    if stack or pending or need_atom or rings:
        return syntax
    if (max_atoms is not None and len(atoms) > max_atoms) or (max_bonds is not None and len(bonds) > max_bonds):
        return (READ_TRUNCATED,) + _EMPTY_RECORD
    if len({(i, j) for i, j, _ in bonds}) != len(bonds):
        return (READ_DUPLICATE,) + _EMPTY_RECORD
    return READ_OK, np.array(atoms, dtype=np.int32).reshape(-1, 4), np.array(bonds, dtype=np.int32).reshape(-1, 3)
