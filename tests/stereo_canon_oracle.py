"""Test infrastructure, not product: "the same stereo graph", decided WITHOUT the canonical search and without the element table
("The isomeric order").  stereo_isomorphic(m1, m2) enumerates the isomorphisms of the graph part with networkx
and tests each against the definition on the two DRAWINGS:

  * a marked centre goes onto a marked centre, and the signed volume of its neighbours, taken in m1 in any order and in m2 in the
    order of their images, has the same sign (the hydrogen of a three-neighbour centre stands on the centre in both);
  * a marked double bond goes onto a marked double bond, and two substituents, one of each end, that lie on one side of the bond
    have images that lie on one side.

Which atoms and bonds are MARKED comes from the second transcriptions of the two rules (smiles_stereo_oracle, smiles_ez_oracle),
not from decode; volume and side are computed here, from positions and wedge rows."""
import networkx as nx

import smiles_ez_oracle as Z
import smiles_stereo_oracle as S


def rows_of(m):
    """a decode.Molecule as the (atoms, bonds, implh) rows the oracles read"""
    from abcnet_amd.decode import ATOM_SYMBOLS
    atoms = [(p[0], p[1], ATOM_SYMBOLS.index(s, 1) if s == "C" else ATOM_SYMBOLS.index(s), c, h)
             for p, s, c, h in zip(m.positions, m.symbols, m.charges, m.hs)]
    return atoms, [(e1, e2, o, k) for k, ((e1, e2), o) in enumerate(zip(m.bonds, m.orders))], list(m.implicit_hs)


class Drawing:
    """what the definition reads of one molecule"""

    def __init__(self, m):
        self.m = m
        atoms, bonds, implh = rows_of(m)
        centres = S.write(atoms, bonds, implh)[2]
        codes = Z.write(atoms, bonds, implh, tetrahedral=False)[1]
        n = len(m.symbols)
        self.marked_centres = {a for a in range(n) if centres[a] in (1, -1)}
        self.marked_bonds = {frozenset((e1 - 1, e2 - 1)) for (e1, e2), c in zip(m.bonds, codes) if c in (1, -1)}
        self.around = [[] for _ in range(n)]
        self.up = {}                   # (owner, other end) of a wedge row -> the elevation of the other end
        for (e1, e2), o in zip(m.bonds, m.orders):
            self.around[e1 - 1].append(e2 - 1)
            self.around[e2 - 1].append(e1 - 1)
            if o >= 5:
                self.up[(e1 - 1, e2 - 1)] = 1 if o == 5 else -1
        classes, charges, edges, tags = m.canon_graph()
        self.graph = nx.Graph()
        for a in range(n):
            self.graph.add_node(a, label=(classes[a], charges[a], tags[a]))
        for i, j, o in edges:
            self.graph.add_edge(i, j, order=o)

    def volume_sign(self, a, named):
        """the sign of the signed volume of centre a's neighbours in the order `named` (three: the hydrogen, on the centre, is last)"""
        xa, ya = self.m.positions[a]
        pts = [(self.m.positions[j][0] - xa, self.m.positions[j][1] - ya, self.up.get((a, j), 0)) for j in named]
        if len(pts) == 3:
            pts.append((0, 0, 0))
        (a1, a2, a3), (b1, b2, b3), (c1, c2, c3) = ([u - v for u, v in zip(p, pts[3])] for p in pts[:3])
        t = a1 * (b2 * c3 - b3 * c2) - a2 * (b1 * c3 - b3 * c1) + a3 * (b1 * c2 - b2 * c1)
        return (t > 0) - (t < 0)

    def side(self, a, b, s):
        """the side of atom s of the line from a to b"""
        pos = self.m.positions
        t = (pos[b][0] - pos[a][0]) * (pos[s][1] - pos[a][1]) - (pos[b][1] - pos[a][1]) * (pos[s][0] - pos[a][0])
        return (t > 0) - (t < 0)


def keeps_stereo(d1, d2, phi):
    """does the isomorphism phi of the graph parts (atom of d1 -> atom of d2) keep every stereo element"""
    if {phi[a] for a in d1.marked_centres} != d2.marked_centres:
        return False
    if {frozenset(phi[e] for e in bond) for bond in d1.marked_bonds} != d2.marked_bonds:
        return False
    for a in d1.marked_centres:
        named = d1.around[a]
        if d1.volume_sign(a, named) != d2.volume_sign(phi[a], [phi[j] for j in named]):
            return False
    for bond in d1.marked_bonds:
        a, b = sorted(bond)
        for s in d1.around[a]:
            for t in d1.around[b]:
                if s == b or t == a:
                    continue
                together = d1.side(a, b, s) == d1.side(a, b, t)
                if together != (d2.side(phi[a], phi[b], phi[s]) == d2.side(phi[a], phi[b], phi[t])):
                    return False
    return True


def stereo_isomorphic(m1, m2):
    """are the stereo graphs of two decode.Molecule equal: some isomorphism of the graph parts keeps every stereo element"""
    d1, d2 = Drawing(m1), Drawing(m2)
    if len(d1.marked_centres) != len(d2.marked_centres) or len(d1.marked_bonds) != len(d2.marked_bonds):
        return False
    matcher = nx.isomorphism.GraphMatcher(d1.graph, d2.graph, node_match=lambda u, v: u["label"] == v["label"],
                                          edge_match=lambda u, v: u["order"] == v["order"])
    return any(keeps_stereo(d1, d2, phi) for phi in matcher.isomorphisms_iter())
