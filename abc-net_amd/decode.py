"""The assembled molecule of one image (img2smiles2.py:193-311, computed on the device by csrc/assemble.hip) and the mol block
the reference writes from it (generate_smiles.py:18-105).  Pure host string work: RDKit is not a dependency; the caller hands
`Molecule.molblock()` to `Chem.MolFromMolBlock` exactly as generate_smiles.py:115 does.
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
