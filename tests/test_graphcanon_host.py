"""CPU tier of the canonical atom order: the pruned search (decode.canonical_labelling, the host form of csrc/graph_canon.hip) against
brute force over the whole tree, against renumbering, against networkx and through the SMILES reader; the binding and the launcher's
refusals (which need no device)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import abcnet_amd  # noqa: E402,F401
from abcnet_amd import _lib as L  # noqa: E402
from abcnet_amd import decode as D  # noqa: E402
from abcnet_amd.decode import ATOM_SYMBOLS, Molecule  # noqa: E402
import graphcanon_oracle as co  # noqa: E402
import graphident_oracle as io  # noqa: E402
import graphsim_oracle as so  # noqa: E402
import smiles_oracle as O  # noqa: E402
from smiles_cases import graph_of_rows, graph_of_text, random_rows, same_graph  # noqa: E402


def _against_brute(graph, what):
    res = co.canon(graph)
    key, cert = co.brute(graph)
    assert res["stats"]["status"] == 0, (what, res["stats"])
    assert res["cert"] == cert and co.leaf_key(res) == key, (what, res["stats"])
    return res


# ------------------------------------------------------------------------------------------------------- pruning is sound
def test_pruned_search_equals_brute_force_on_every_small_connected_graph():
    """every connected graph of 1..6 atoms (networkx's atlas: 1 + 1 + 2 + 6 + 21 + 112), plain and with two seeded assignments of
    classes, charges and orders each: the least leaf of the pruned search is the least leaf of the whole tree"""
    import networkx as nx
    rng = np.random.RandomState(21)
    count = trace_pruned = 0
    for g in nx.graph_atlas_g():
        n = g.number_of_nodes()
        if n < 1 or n > 6 or not nx.is_connected(g):
            continue
        count += 1
        edges = sorted(g.edges())
        for variant in range(3):
            classes = [1] * n if variant == 0 else [int(rng.choice([1, 1, 2, 3])) for _ in range(n)]
            charges = [0] * n if variant == 0 else [int(rng.choice([0, 0, 0, 1])) for _ in range(n)]
            bonds = [(i, j, 1 if variant == 0 else int(rng.choice([1, 1, 2, 4]))) for i, j in edges]
            tags = [0] * n if variant < 2 else [int(rng.rand() < 0.2) for _ in range(n)]
            res = _against_brute((classes, charges, bonds, tags), (edges, variant))
            trace_pruned += res["stats"]["pruned_trace"]
    assert count == 143


@pytest.mark.parametrize("name, rec", co.NAMED)
def test_pruned_search_equals_brute_force_on_the_named_cases(name, rec):
    res = _against_brute(co.record_graph(rec), name)
    if name == "benzene":
        assert res["stats"]["leaves"] <= 4 and res["stats"]["pruned_orbit"] >= 1 and res["stats"]["automorphisms"] >= 1
    # and a renumbered copy is the same relabelled graph
    assert co.canon(co.record_graph(so.permuted(np.random.RandomState(3), rec)))["cert"] == res["cert"]


def test_a_trace_that_is_greater_drops_the_branch_and_one_that_is_less_replaces_the_best():
    """the identity suite's union of decalin and bicyclopentyl: its first cell holds atoms of both components, so sibling branches have
    different traces -- the search prunes by trace or finds a better leaf, and still ends where brute force does"""
    seen = dict(pruned_trace=0, improved=0)
    rng = np.random.RandomState(17)
    for _ in range(12):
        res = _against_brute(co.record_graph(so.permuted(rng, co.UNION)), "union")
        for k in seen:
            seen[k] += res["stats"][k]
    assert seen["pruned_trace"] >= 1 and seen["improved"] >= 1, seen


def test_refinement_alone_is_not_enough():
    """decalin and bicyclopentyl are refinement-equal (the similarity's refine_equal is 1): their certificates differ"""
    a, b = co.canon(co.record_graph(so.DECALIN)), co.canon(co.record_graph(so.BICYCLOPENTYL))
    assert so.refine_equal(so.of_record(*so.DECALIN), so.of_record(*so.BICYCLOPENTYL)) == 1
    assert a["cert"] != b["cert"] and a["cert"][:2] == b["cert"][:2]


# --------------------------------------------------------------------------------------------------------------- renumbering
def _renumbered(rng, rows):
    """the rows of smiles_cases.random_rows with the atoms renumbered and the bond rows in another order (orientation kept)"""
    atoms, bonds, implh = rows
    n = len(atoms)
    perm = rng.permutation(n)                           # old index -> new index
    new_atoms = [None] * n
    for old, new in enumerate(perm):
        new_atoms[int(new)] = atoms[old]
    new_bonds = [(int(perm[bonds[k][0] - 1]) + 1, int(perm[bonds[k][1] - 1]) + 1, bonds[k][2], bonds[k][3]) for k in rng.permutation(len(bonds))]
    listed = [int(perm[a - 1]) + 1 for a in implh]
    return new_atoms, new_bonds, [listed[k] for k in rng.permutation(len(listed))]


def _invariant(mol):
    """what of a canonical Molecule the graph decides.  Positions, hs, the source column and WHICH end of a row is end 1 belong to
    the drawing: end 1 stays end 1 (the wedge's owner), so between two atoms an automorphism swaps the row may stand either way; and
    a wedge is a single bond of the graph, so of two rows an automorphism swaps either may carry the wedge code"""
    return mol.symbols, mol.charges, [sorted(q) for q in mol.bonds], [D.canon_bond_class(o) for o in mol.orders], mol.implicit_hs


def test_renumbering_changes_neither_certificate_nor_rows_nor_text():
    """500 seeded graphs of the SMILES suite's recipe, 3 renumberings each"""
    rng = np.random.default_rng(5)
    rs = np.random.RandomState(5)
    texts = {}
    for k in range(500):
        rows = random_rows(rng)
        mol = Molecule.from_device_rows(*rows)
        base = mol.canonical()
        cert = D.canon_certificate(mol.canon_graph(), mol.canonical_order()[0])
        text = mol.smiles(canonical=True)
        assert text == base.smiles() and mol.canonical_order()[1]["status"] == 0
        assert same_graph(graph_of_text(O.parse(text)), graph_of_rows(rows)), text           # read back: the input graph
        for _ in range(3):
            other = Molecule.from_device_rows(*_renumbered(rs, rows))
            assert D.canon_certificate(other.canon_graph(), other.canonical_order()[0]) == cert, k
            assert _invariant(other.canonical()) == _invariant(base), k
            assert other.smiles(canonical=True) == text, k
        texts.setdefault(text, set()).add(tuple(cert))
    assert all(len(c) == 1 for c in texts.values())       # one string, one graph


def test_canonical_is_idempotent_and_keeps_what_the_graph_skips():
    mol = Molecule(["N", "C", "C", "O"], [0, 0, 1, 0], [1, 0, 2, 0], [[5, 6], [7, 8], [9, 10], [11, 12]],
                   [[4, 3], [9, 1], [3, 3], [2, 3], [1, 2], [0, 2]], [2, 1, 1, 5, 1, 3], [3, 7, 0, 3], sources=[10, 11, 12, 13, 14, 15])
    can = mol.canonical()
    assert _invariant(can.canonical()) == _invariant(can)
    assert can.bonds[3:] == [[9, 1], [3, 3], [0, 2]] and can.orders[3:] == [1, 1, 3] and can.sources[3:] == [11, 12, 15]
    assert can.implicit_hs[2:] == [7, 0] and can.implicit_hs[0] == can.implicit_hs[1]
    assert sorted(zip(can.symbols, can.charges, can.hs, map(tuple, can.positions))) == sorted(zip(mol.symbols, mol.charges, mol.hs, map(tuple, mol.positions)))
    wedge = [q for q, o in zip(can.bonds, can.orders) if o == 5][0]
    assert can.symbols[wedge[0] - 1] == "C" and can.charges[wedge[0] - 1] == 0      # end 1 stays end 1: the wedge keeps its owner
    with pytest.raises(ValueError, match="stereo"):
        mol.smiles(stereo=True, canonical=True)


# ------------------------------------------------------------------------------------------------------------------ networkx
def test_certificates_are_equal_exactly_where_networkx_finds_an_isomorphism():
    """the 2000 pairs of the identity suite (classes, charges, orders, repeated pairs), none UNDECIDED under the default budgets"""
    same = 0
    for k, (mol, rec) in enumerate(io.random_pairs(2000, seed=11)):
        gp, (gt, _) = co.of_molecule(mol), co.of_record(*rec)
        a, b = co.canon(gp), co.canon(gt)
        assert a["stats"]["status"] == 0 and b["stats"]["status"] == 0, k
        iso = io.brute(gp[:3], gt[:3])
        assert (a["cert"] == b["cert"]) == iso, k
        assert not iso or a["key"] == b["key"], k
        same += iso
    assert 800 <= same <= 1200


# ---------------------------------------------------------------------------------------------------------------------- tags
def test_a_listed_atom_is_part_of_the_graph():
    """N-C(=O)-N, the two nitrogens automorphic: listing either gives the same text, another text than listing neither"""
    def urea(implh):
        return Molecule(["N", "C", "O", "N"], [0] * 4, [0] * 4, [[0, 0]] * 4, [[1, 2], [2, 3], [2, 4]], [1, 2, 1], implh)
    first, second, neither, both = (urea(l).smiles(canonical=True) for l in ([1], [4], [], [4, 1]))
    assert first == second and first != neither and both != first and both != neither
    assert first.count("[NH]") == 1 and both.count("[NH]") == 2 and "[" not in neither
    ranks = urea([4]).canonical_order()[0], urea([1]).canonical_order()[0]
    assert ranks[0][3] == ranks[1][0] and ranks[0][0] == ranks[1][3]          # the listed nitrogen takes the same place
    # with all tags 0 id_0 is the identity's, bit for bit
    g = co.record_graph(co.UNION)
    assert co._id0(g) == so.ids(g[:3], 0)[0] and co._id0(g[:3] + ([1] + [0] * 19,))[1:] == co._id0(g)[1:]


# ----------------------------------------------------------------------------------------------------------------- budgets
def test_budgets_end_undecided_with_a_valid_order():
    g = co.record_graph(co.benzenes(2))
    full = co.canon(g)
    for budgets, leaves in ((dict(max_tries=1), 0), (dict(max_rounds=1), 0), (dict(max_tries=4), 1), (dict(max_rounds=30), None)):
        res = co.canon(g, **budgets)
        assert res["stats"]["status"] == co.UNDECIDED and sorted(res["rank"]) == list(range(12)), budgets
        assert leaves is None or res["stats"]["leaves"] == leaves
        if res["stats"]["leaves"] == 0:
            assert res["rank"] == list(range(12))
    assert full["stats"]["status"] == 0 and full["stats"]["tries"] <= 32


def test_the_worst_cases_at_capacity_under_the_default_budgets():
    """the counts beside ABC_CANON_DEFAULT_TRIES / _ROUNDS (include/abcnet_hip.h)"""
    ring, chain = co.canon(co.record_graph(io.carbon_ring(512))), co.canon(co.record_graph(io.carbon_chain(512)))
    assert ring["stats"]["status"] == 0 and ring["stats"]["tries"] <= 9 and ring["stats"]["rounds"] <= 2471 and ring["stats"]["pruned_orbit"] >= 500
    assert chain["stats"]["status"] == 0 and (chain["stats"]["tries"], chain["stats"]["rounds"]) == (2, 1008)
    for rec in (io.propanes(170), co.benzenes(64)):
        res = co.canon(co.record_graph(rec))
        assert res["stats"]["status"] == co.UNDECIDED and res["stats"]["leaves"] >= 1 and sorted(res["rank"]) == list(range(len(rec[0])))
        assert res["stats"]["rounds"] == co.DEFAULT_ROUNDS


# ---------------------------------------------------------------------------------------------------------------- the binding
def test_binding_mirrors_the_header():
    header = open(os.path.join(os.path.dirname(L.LIB_PATH), "..", "include", "abcnet_hip.h")).read()
    for name, value in (("ABC_CANON_DEFAULT_TRIES", L.CANON_DEFAULT_TRIES), ("ABC_CANON_DEFAULT_ROUNDS", L.CANON_DEFAULT_ROUNDS),
                        ("ABC_CANON_ORBIT_LEVELS", L.CANON_ORBIT_LEVELS), ("ABC_CANON_NCOL", len(L.CANON_COLUMNS)),
                        ("ABC_CANON_UNDECIDED", L.CANON_UNDECIDED), ("ABC_CANON_COLLISION", L.CANON_COLLISION)):
        assert "%s = %d" % (name, value) in header, name
    assert (D.CANON_DEFAULT_TRIES, D.CANON_DEFAULT_ROUNDS, D.CANON_ORBIT_LEVELS) == (L.CANON_DEFAULT_TRIES, L.CANON_DEFAULT_ROUNDS, L.CANON_ORBIT_LEVELS)
    assert D.CANON_COLUMNS == L.CANON_COLUMNS and (L.CanonDesc, "abc_canon_desc_size") in L.SELF_SIZED_SINCE
    assert [f for f, _ in L.CanonDesc._fields_][:7] == ["mol_counts", "mol_atoms", "mol_bonds", "mol_implh", "rec_atoms", "rec_bonds", "rec_counts"]


def test_launcher_refuses_before_it_touches_a_device():
    if not os.path.exists(L.LIB_PATH):
        pytest.skip("libabcnet_hip.so is not built")
    lib = L.load()
    assert lib.abc_canon_desc_size() == C.sizeof(L.CanonDesc)

    def desc(**fields):
        d = L.CanonDesc()
        base = dict(mol_counts=1 << 20, mol_atoms=2 << 20, mol_bonds=3 << 20, mol_implh=4 << 20, B=2, cap_atoms=512, cap_mol_bonds=2048,
                    order=5 << 20, stats=6 << 20, key=7 << 20)       # (addresses that are never dereferenced: the refusals come first)
        for k, v in dict(base, **fields).items():
            setattr(d, k, v)
        return d
    rows = dict(out_counts=8 << 20, out_atoms=9 << 20, out_bonds=10 << 20, out_implh=11 << 20)
    for code, fields, text in ((-2, dict(cap_atoms=513), "512"), (-2, dict(rows, cap_mol_bonds=4097), "4096"), (-1, dict(stats=None), "null"),
                               (-1, dict(rows, out_atoms=2 << 20), "overlaps"), (-1, dict(order=(1 << 20) + 8), "overlaps"),
                               (-1, dict(rows, out_bonds=None), "four"), (-1, dict(rec_counts=12 << 20), "one side"),
                               (-1, dict(mol_counts=None), "one side"), (-1, dict(B=0), "empty"), (-1, dict(max_rounds=-1), "max_rounds"),
                               (-2, dict(mol_counts=None, rec_counts=1 << 20, rec_atoms=2 << 20, rec_bonds=3 << 20, max_atoms=513, max_bonds=8), "512"),
                               (-1, dict(rows, mol_counts=None, rec_counts=1 << 20, rec_atoms=2 << 20, rec_bonds=3 << 20, max_atoms=8, max_bonds=8), "molecule side")):
        assert lib.abc_canonical_order(C.byref(desc(**fields)), None) == code, fields
        assert text in lib.abc_last_error().decode(), (fields, lib.abc_last_error())
    assert lib.abc_canonical_order(None, None) == -1 and lib.abc_last_error().decode() == "canonical_order: null descriptor"


def test_runner_refuses_the_flag_without_smiles_and_with_stereo():
    from abcnet_amd.infer import STAGES, InferenceRunner
    from molrows import Heads
    stages = list(STAGES)
    assert STAGES["canonicalizer"] == "smiles_canonical" and stages.index("canonicalizer") == stages.index("assembler") + 1 < stages.index("smiler")
    for kw in (dict(smiles=True, smiles_stereo=True), dict(smiles=False), dict()):
        with pytest.raises(ValueError, match="smiles_canonical"):
            InferenceRunner(Heads(), 2, 64, 64, assemble=True, smiles_canonical=True, **kw)
