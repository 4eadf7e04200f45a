"""The aromaticity rule where no GPU is needed: decode.perceive_aromatic / Molecule.aromatized(), the host form
of csrc/aromatic.hip, against the rule's example table, against the second implementation of tests/aromatic_oracle.py, under
renumbering, over every Kekule structure of eight skeletons, and through the SMILES reader back to the perceived graph.  Integers and
strings: every comparison is exact."""
import ctypes as C
import os
import sys

import networkx as nx
import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import abcnet_amd  # noqa: E402,F401
from abcnet_amd import _lib as L  # noqa: E402
from abcnet_amd import decode as D  # noqa: E402
import aromatic_oracle as A  # noqa: E402
import smiles_oracle as O  # noqa: E402
from smiles_cases import graph_of_rows, graph_of_text, same_graph  # noqa: E402


molecule = A.molecule


def perceived(rows):
    """(rows, codes, stats) by the host form, in the oracle's layout"""
    m, st, codes = molecule(rows).aromatic_perception()
    atoms, bonds, _ = rows
    return (list(atoms), [(q[0], q[1], o, q[3]) for q, o in zip(bonds, m.orders)], m.implicit_hs), codes, st


@pytest.fixture(scope="module")
def random_graphs():
    rng = np.random.default_rng(22)
    return [A.random_rows(rng) for _ in range(2000)]


def test_the_example_table_exactly():
    assert len(A.EXAMPLES) == 19
    for name, rows, orders, listed in A.EXAMPLES:
        (_, bonds, implh), codes, st = perceived(rows)
        want = [q[2] for q in rows[1]] if orders is None else orders
        assert [q[2] for q in bonds] == want, name
        assert implh == rows[2] + listed and st["listed"] == len(listed), name
        assert st["rows_changed"] == sum(o != q[2] for o, q in zip(want, rows[1])), name
    by_name = {name: perceived(rows) for name, rows, _, _ in A.EXAMPLES}
    assert by_name["azulene"][2]["cycles"] == 2 and by_name["azulene"][2]["aromatic"] == 0       # sums 5 and 7; the envelope has 10 atoms
    assert by_name["benzene, order 4"][2] == dict(status=0, candidates=6, cycles=1, aromatic=1, rows_changed=0, listed=0)
    assert by_name["naphthalene, form 1"][2]["aromatic"] == 2 and by_name["pyrrole"][1] == [2, 1, 1, 1, 1]
    assert by_name["cyclopentadiene"][1] == [D.AROM_NONE, 1, 1, 1, 1] and by_name["cyclooctatetraene"][2]["cycles"] == 0


def test_random_graphs_equal_the_oracle(random_graphs):
    seen = dict.fromkeys(A.COLUMNS[1:] + ("none", "not_aromatic"), 0)
    for rows in random_graphs:
        got, codes, st = perceived(rows)
        want, want_codes, counts = A.perceive_rows(rows)
        assert got == want and codes == want_codes, rows
        assert {k: st[k] for k in counts} == counts, rows
        for k in counts:
            seen[k] += counts[k] > 0
        seen["none"] += A.NONE in codes
        seen["not_aromatic"] += counts["cycles"] > counts["aromatic"]
    # the recipe reaches every part of the rule: aromatic and other cycles, NONE atoms, changed rows, listed atoms
    assert min(seen.values()) >= 20, seen


def test_renumbering_rows_and_ends_do_not_matter(random_graphs):
    rng = np.random.default_rng(5)
    for rows in random_graphs[:400]:
        atoms, bonds, implh = rows
        n = len(atoms)
        new = [int(v) for v in rng.permutation(n)]       # atom a becomes atom new[a]
        where = lambda e: new[e - 1] + 1 if 1 <= e <= n else e
        atoms2 = [None] * n
        for a in range(n):
            atoms2[new[a]] = atoms[a]
        perm = [int(k) for k in rng.permutation(len(bonds))]
        bonds2 = [(where(bonds[k][1]), where(bonds[k][0]), bonds[k][2], bonds[k][3]) if rng.integers(0, 2) else
                  (where(bonds[k][0]), where(bonds[k][1]), bonds[k][2], bonds[k][3]) for k in perm]
        (_, out, listed), codes, st = perceived(rows)
        (_, out2, listed2), codes2, st2 = perceived((atoms2, bonds2, [where(e) for e in implh]))
        assert [q[2] for q in out2] == [out[k][2] for k in perm]
        assert set(listed2) == {where(e) for e in listed} and st2 == st
        assert [codes2[new[a]] for a in range(n)] == codes


# the skeletons: (symbols, bonds (1-based), the atoms that are NOT sp2 -- a pyrrole-type N keeps its lone pair out of the matching)
def _fused(symbols, bonds, lone=()):
    return symbols, bonds, set(lone)


SKELETONS = {
    "benzene": _fused(["C"] * 6, [(i, i % 6 + 1) for i in range(1, 7)]),
    "naphthalene": _fused(["C"] * 10, A.NAPHTHALENE_SKELETON),
    "anthracene": _fused(["C"] * 14, [(i, i + 1) for i in range(1, 14)] + [(14, 1), (3, 12), (5, 10)]),
    "phenanthrene": _fused(["C"] * 14, [(i, i + 1) for i in range(1, 14)] + [(14, 1), (5, 14), (8, 13)]),
    # pyrene: the rim 1 .. 14 and the two inner atoms 15, 16
    "pyrene": _fused(["C"] * 16, [(i, i + 1) for i in range(1, 14)] + [(14, 1), (15, 16), (15, 1), (15, 5), (16, 8), (16, 12)]),
    "quinoline": _fused(["N"] + ["C"] * 9, A.NAPHTHALENE_SKELETON),
    "indole": _fused(["N"] + ["C"] * 8, A.INDOLE_SKELETON, lone=[1]),
    # carbazole: N1, the five-ring N1 C2 C7 C8 C13, the six-rings C2 .. C7 and C8 .. C13
    "carbazole": _fused(["N"] + ["C"] * 12, [(1, 2), (2, 7), (7, 8), (8, 13), (13, 1), (2, 3), (3, 4), (4, 5), (5, 6), (6, 7), (8, 9), (9, 10),
                                               (10, 11), (11, 12), (12, 13)], lone=[1]),
}


def kekule_structures(bonds, lone):
    """every perfect matching of the sp2 atoms, as a set of double bonds"""
    g = nx.Graph([b for b in bonds if b[0] not in lone and b[1] not in lone])

    def extend(graph):
        if graph.number_of_nodes() == 0:
            yield frozenset()
            return
        a = min(graph.nodes)
        for y in list(graph[a]):
            rest = graph.copy()
            rest.remove_nodes_from([a, y])
            for m in extend(rest):
                yield m | {(a, y)}
    return list(extend(g))


@pytest.mark.parametrize("name", sorted(SKELETONS))
def test_every_kekule_structure_gives_one_output(name):
    symbols, bonds, lone = SKELETONS[name]
    forms = kekule_structures(bonds, lone)
    assert len(forms) == {"benzene": 2, "naphthalene": 3, "anthracene": 4, "phenanthrene": 5, "pyrene": 6, "quinoline": 3, "indole": 2,
                          "carbazole": 4}[name]
    outs = []
    for doubles in forms:
        rows = A.rows_of(symbols, A.with_doubles(bonds, doubles))
        (_, out, listed), _, _ = perceived(rows)
        assert [q[2] for q in out] == [4] * len(bonds), (name, sorted(doubles))
        assert listed == sorted(lone)
        outs.append((out, listed))
    assert all(o == outs[0] for o in outs)
    assert len({molecule(A.rows_of(symbols, A.with_doubles(bonds, f))).smiles(canonical=True, aromatize=True) for f in forms}) == 1


def test_listing_keeps_the_hydrogen_count_of_b_c_n_o(random_graphs):
    """h by the text rule, atom by atom, before and after: the listing is exactly what keeps it for the atoms whose bare token has no h.

    Asserted for every B C N O atom whose INPUT rows hold an even number of class-4 rows, i.e. whose bond order sum s2 / 2 is a whole
    number before the pass.  With an odd number the text rule's v = s2 // 2 is the floor of a half: a neutral carbon drawn with one
    class-4 and one class-1 row (a ring drawn half in each style) has v = 5 // 2 = 2 and h = 2 before, v = 3 and h = 1 after, and no
    list entry can keep a count of 2 (an entry means exactly one hydrogen).  The `h = 2` was the floor's, not the drawing's: `c` is
    written bare either way.  Those atoms are counted below and must exist, so the limit stays visible."""
    checked = halves = 0
    for rows in random_graphs + [r for _, r, _, _ in A.EXAMPLES]:
        before, after = molecule(rows), molecule(rows).aromatized()

        def h(m, a):
            if a + 1 in m.implicit_hs:
                return 1
            n = len(m.symbols)
            cls = [D.canon_bond_class(o) for (i, j), o in zip(m.bonds, m.orders) if a + 1 in (i, j) and 1 <= i <= n and 1 <= j <= n and i != j]
            return D.text_hydrogens(m.symbols[a], m.charges[a], cls)
        for a, s in enumerate(before.symbols):
            if s not in ("B", "C", "N", "O"):
                continue
            n = len(before.symbols)
            fours = sum(o == 4 for (i, j), o in zip(before.bonds, before.orders) if a + 1 in (i, j) and 1 <= i <= n and 1 <= j <= n and i != j)
            if fours % 2:
                halves += h(before, a) != h(after, a)
                continue
            assert h(before, a) == h(after, a), (rows, a)
            checked += before.orders != after.orders
    assert checked > 1000 and halves > 0


def test_the_text_of_the_perceived_rows_reads_back_as_the_perceived_graph(random_graphs):
    written = 0
    for rows in random_graphs[:600] + [r for _, r, _, _ in A.EXAMPLES]:
        out, _, _ = perceived(rows)
        try:
            text = molecule(out).smiles()
        except (ValueError, KeyError):       # (a row the text rule refuses: the recipe has invalid and duplicate rows on purpose)
            continue
        assert text == molecule(rows).smiles(aromatize=True)
        assert same_graph(graph_of_text(O.parse(text)), graph_of_rows(out)), text
        written += 1
    assert written >= 100
    texts = {name: molecule(rows).smiles(aromatize=True) for name, rows, _, _ in A.EXAMPLES}
    assert texts["benzene"] == "c1ccccc1" == texts["benzene, order 4"] and texts["pyrrole"] == "[nH]1cccc1"
    assert texts["furan"] == "o1cccc1" and texts["pyridine"] == "n1ccccc1" and texts["cyclopentadiene"] == "C1C=CC=C1"
    assert molecule(A.EXAMPLES[0][1]).smiles() == "C1=CC=CC=C1"


def test_binding_mirrors_the_header():
    header = open(os.path.join(os.path.dirname(L.LIB_PATH), "..", "include", "abcnet_hip.h")).read()
    assert "ABC_AROM_NCOL = %d" % len(L.AROMATIC_COLUMNS) in header
    assert "ABC_AROM_NOT_CANDIDATE = %d" % L.AROM_NOT_CANDIDATE in header and "ABC_AROM_NONE = %d" % L.AROM_NONE in header
    assert D.AROMATIC_COLUMNS == L.AROMATIC_COLUMNS == A.COLUMNS and (D.AROM_NOT_CANDIDATE, D.AROM_NONE) == (L.AROM_NOT_CANDIDATE, L.AROM_NONE)
    for name in ("abc_perceive_aromatic", "abc_aromatic_desc_size"):
        assert name in L.SYMBOLS and name + "(" in header
    assert (L.AromaticDesc, "abc_aromatic_desc_size") in L.SELF_SIZED_SINCE and L.AromaticDesc not in L._STRUCTS
    assert [f for f, _ in L.AromaticDesc._fields_][:7] == [f for f, _ in L.CanonDesc._fields_][:7]


def test_launcher_refuses_before_it_touches_a_device():
    if not os.path.exists(L.LIB_PATH):
        pytest.skip("libabcnet_hip.so is not built")
    lib = L.load()
    assert lib.abc_aromatic_desc_size() == C.sizeof(L.AromaticDesc)

    def desc(**fields):
        d = L.AromaticDesc()
        base = dict(mol_counts=1 << 20, mol_atoms=2 << 20, mol_bonds=3 << 20, mol_implh=4 << 20, B=2, cap_atoms=512, cap_mol_bonds=2048,
                    stats=5 << 20, out_counts=8 << 20, out_atoms=9 << 20, out_bonds=10 << 20, out_implh=11 << 20)
        for k, v in dict(base, **fields).items():       # (addresses that are never dereferenced: the refusals come first)
            setattr(d, k, v)
        return d
    rec = dict(mol_counts=None, mol_atoms=None, mol_bonds=None, mol_implh=None, out_counts=None, out_atoms=None, out_bonds=None, out_implh=None,
               rec_counts=1 << 20, rec_atoms=2 << 20, rec_bonds=3 << 20, max_atoms=8, max_bonds=8, out_rec_bonds=6 << 20)
    for code, fields, text in ((-2, dict(cap_atoms=513), "512"), (-2, dict(rec, max_atoms=513), "512"), (-1, dict(stats=None), "null"),
                               (-1, dict(out_atoms=2 << 20), "overlaps"), (-1, dict(out_bonds=(3 << 20) + 16), "overlaps"),
                               (-1, dict(code_out=(5 << 20) + 8), "overlap"), (-1, dict(out_implh=None), "all four"),
                               (-1, dict(rec_counts=12 << 20), "one side"), (-1, dict(mol_counts=None), "one side"), (-1, dict(B=0), "empty"),
                               (-1, dict(rec, out_rec_bonds=3 << 20), "overlaps"), (-1, dict(rec, out_rec_bonds=None), "out_rec_bonds"),
                               (-1, dict(rec, out_counts=8 << 20), "out_rec_bonds")):
        assert lib.abc_perceive_aromatic(C.byref(desc(**fields)), None) == code, fields
        assert text in lib.abc_last_error().decode(), (fields, lib.abc_last_error())
    assert lib.abc_perceive_aromatic(None, None) == -1 and lib.abc_last_error().decode() == "perceive_aromatic: null descriptor"


def test_runner_and_ops_refuse_on_the_host():
    from abcnet_amd.infer import STAGES, InferenceRunner, launch_order
    from abcnet_amd.ops import AromaticityPerceiver
    from molrows import Heads
    order = launch_order()
    assert STAGES["aromatizer"] == STAGES["record_aromatizer"] == "aromatize" and sorted(order) == sorted(STAGES)
    assert order.index("assembler") + 1 == order.index("aromatizer") == order.index("record_aromatizer") - 1 == order.index("canonicalizer") - 2
    assert [a for a in order if "aromatizer" not in a] == [a for a in STAGES if "aromatizer" not in a]
    with pytest.raises(ValueError, match="aromatize=True.*assemble=True"):
        InferenceRunner(Heads(), 2, 64, 64, aromatize=True)
    with pytest.raises(ValueError, match="one side"):
        AromaticityPerceiver()
    with pytest.raises(ValueError, match="GraphRecords"):
        AromaticityPerceiver(records="records")
