"""The environment similarity, host half (no GPU): the two oracles of tests/graphsim_oracle.py against each other and by hand, the
refusals and the C ABI of csrc/graph_sim.hip."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import abcnet_amd  # noqa: E402,F401
from abcnet_amd import _lib as L  # noqa: E402
import graphsim_oracle as so  # noqa: E402
from molrows import SCORE_DEFAULTS, SCORE_POINTERS, fake_desc, Heads as _Heads  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COL = {c: i for i, c in enumerate(so.COLUMNS)}


def _row(mol, rec):
    return dict(zip(so.COLUMNS, so.rows([mol], [rec])[0].tolist()))


def _pairs(count, seed):
    """(record, record) pairs: a random graph against a copy of it with one atom changed (even k) or another random graph of the
    same size (odd k)"""
    rng = np.random.RandomState(seed)
    for k in range(count):
        n = int(rng.randint(2, 13))
        a = so.random_graph(rng, n, extra=int(rng.randint(0, 4)))
        yield a, (so.one_atom_changed(rng, a) if k % 2 == 0 else so.random_graph(rng, n, extra=int(rng.randint(0, 4))))


def test_hashed_and_structural_environments_agree_on_random_pairs():
    """the ids decide nothing but which environments are equal: (common, pred, true) of the uint64 recurrence are those of the
    hash-free nested tuples, on 2000 seeded pairs"""
    partial = 0
    for a, b in _pairs(2000, seed=2024):
        ga, gb = so.of_record(*a), so.of_record(*b)
        hashed = so.counts(so.ids(ga), so.ids(gb))
        assert hashed == so.counts(*so.structural(ga, gb)), (a, b)
        assert so.refine_equal(ga, gb) == so.refine_equal(ga, gb, layers=so.structural)
        partial += 0 < hashed[0] < min(hashed[1:])
    assert partial > 1000                      # (most pairs are near each other, not equal and not disjoint)


def _single_mix_id1(graph):
    """id_1 with the neighbour term mixed ONCE: mix(mix(id_0[a] + 1) + sum of mix(id_0[j] + o)) -- the form the contract avoids"""
    classes, charges, bonds = graph
    id_0 = so.ids(graph, 0)[0]
    acc = [0] * len(classes)
    for i, j, o in bonds:
        acc[i] += so.mix(id_0[j] + o)
        acc[j] += so.mix(id_0[i] + o)
    return [so.mix(so.mix(id_0[a] + 1) + acc[a]) for a in range(len(classes))]


def test_swap_fixture_differs_only_with_the_doubled_mix():
    """a (C-, degree 2) atom with the neighbours {C, C-} against a (C, degree 2) atom whose two neighbours are one C- through a pair
    listed twice: with a single mix the self term and the neighbour term are one function at r = o = 1, and the two sums hold the
    same three terms"""
    tri = so.of_record(*so.record([1, 1, 1], [(0, 1, 1), (0, 2, 1), (1, 2, 1)], charges=[-1, 0, -1]))
    dbl = so.of_record(*so.record([1, 1], [(0, 1, 1), (0, 1, 1)], charges=[0, -1]))
    assert so.ids(tri, 0)[0][0] == so.ids(dbl, 0)[0][1] and so.ids(tri, 0)[0][1] == so.ids(dbl, 0)[0][0]      # all of degree 2
    assert _single_mix_id1(tri)[0] == _single_mix_id1(dbl)[0]
    assert so.ids(tri, 1)[1][0] != so.ids(dbl, 1)[1][0]
    s_tri, s_dbl = so.structural(tri, dbl, 1)
    assert s_tri[1][0] != s_dbl[1][0]


def test_mix_is_splitmix64():
    # the first outputs of the splitmix64 generator seeded with 0: mix of successive multiples of the golden-ratio increment
    assert so.mix(0x9E3779B97F4A7C15) == 0xE220A8397B1DCDAF and so.mix(2 * 0x9E3779B97F4A7C15) == 0x6E789E6AA1B965F4
    assert so.mix(0) == 0


def test_order_of_atoms_rows_and_ends_changes_no_column():
    rng = np.random.RandomState(7)
    for _ in range(50):
        a = so.random_graph(rng, int(rng.randint(3, 13)), extra=3)
        b = so.one_atom_changed(rng, a)
        want = _row(so.as_mol(b), a)
        assert want == _row(so.as_mol(so.permuted(rng, b)), a) == _row(so.as_mol(b), so.permuted(rng, a))
        assert _row(so.as_mol(so.permuted(rng, a)), a)["refine_equal"] == 1


def test_cco_against_ccn_by_hand():
    """C-C-O against C-C-N: the far carbon's radius-0 and radius-1 environments and the middle carbon's radius-0 one are common"""
    row = _row(so.mol([1, 1, 3], [(1, 2, 1), (2, 3, 1)]), so.record([1, 1, 2], [(0, 1, 1), (1, 2, 1)]))
    assert [row[c] for c in so.COLUMNS] == [1, 0, 0, 1, 0, 0, 3, 3, 12, 12, 3, 262144]
    same = _row(so.mol([1, 1, 3], [(1, 2, 1), (2, 3, 1)]), so.record([3, 1, 1], [(0, 1, 1), (1, 2, 1)]))
    assert [same[c] for c in so.COLUMNS] == [1, 0, 0, 1, 1, 1, 3, 3, 12, 12, 12, 1 << 20]


def _nx_graph(rec):
    nx = pytest.importorskip("networkx")
    classes, charges, bonds = so.of_record(*rec)
    g = nx.MultiGraph()
    for a, (t, c) in enumerate(zip(classes, charges)):
        g.add_node(a, label=(t, c))
    for i, j, o in bonds:
        g.add_edge(i, j, order=o)
    return g


def _isomorphic(a, b):
    nx = pytest.importorskip("networkx")
    iso = nx.algorithms.isomorphism
    return nx.is_isomorphic(_nx_graph(a), _nx_graph(b), node_match=iso.categorical_node_match("label", None),
                            edge_match=iso.categorical_multiedge_match("order", None))


def test_decalin_and_bicyclopentyl_pass_refinement():
    """colour refinement is necessary for isomorphism, not sufficient: refine_equal is an upper bound"""
    row = _row(so.as_mol(so.DECALIN), so.BICYCLOPENTYL)
    assert row["refine_equal"] == 1 and row["size_equal"] == 1 and row["dice_one"] == 1
    assert (row["envs_common"], row["envs_pred"], row["envs_true"]) == (40, 40, 40) and row["dice_q20"] == 1 << 20
    ga, gb = so.of_record(*so.DECALIN), so.of_record(*so.BICYCLOPENTYL)
    assert sorted(so.ids(ga, 10)[10]) == sorted(so.ids(gb, 10)[10])
    assert not _isomorphic(so.DECALIN, so.BICYCLOPENTYL)


def test_isomorphic_implies_refine_equal():
    rng = np.random.RandomState(99)
    isomorphic = different = 0
    for k in range(240):
        a = so.random_graph(rng, int(rng.randint(2, 11)), extra=int(rng.randint(0, 3)))
        b = so.permuted(rng, a)
        if k % 4 == 3:
            b = so.one_atom_changed(rng, b)
        iso = _isomorphic(a, b)
        eq = _row(so.as_mol(b), a)["refine_equal"]
        assert eq or not iso, (a, b)
        isomorphic += iso
        different += not eq
    assert isomorphic >= 180 and different >= 40


def test_wedge_codes_fold_to_a_single_bond():
    rec = so.record([1, 2, 3], [(0, 1, 1), (1, 2, 2)])
    for code in (5, 6):
        assert _row(so.mol([1, 2, 3], [(1, 2, code), (2, 3, 2)]), rec)["dice_one"] == 1
        assert _row(so.mol([1, 2, 3], [(1, 2, 1), (2, 3, 2)]), so.record([1, 2, 3], [(0, 1, code), (1, 2, 2)]))["dice_one"] == 1
    assert _row(so.mol([1, 2, 3], [(1, 2, 5), (2, 3, 6)]), rec)["dice_one"] == 0
    # aromatic stays aromatic, and a code outside 1..6 is a class of its own
    assert _row(so.mol([1, 2, 3], [(1, 2, 4), (2, 3, 2)]), rec)["envs_common"] < 12
    assert _row(so.mol([1, 2, 3], [(1, 2, 9), (2, 3, 2)]), rec)["envs_common"] < 12
    assert so.bond_class(9) == so.bond_class(0) == so.bond_class(-1) == 0


def test_unknown_equals_only_unknown():
    bonds_m, bonds_r = [(1, 2, 1)], [(0, 1, 1)]
    assert _row(so.mol([99, 1], bonds_m), so.record([-1, 1], bonds_r))["dice_one"] == 1        # unknown against unknown
    assert _row(so.mol([-5, 1], bonds_m), so.record([-1, 1], bonds_r))["dice_one"] == 1
    for known in range(14):
        assert _row(so.mol([known, 1], bonds_m), so.record([-1, 1], bonds_r))["envs_common"] == 1, known   # the carbon's id_0 alone
    assert _row(so.mol([0, 1], bonds_m), so.record([1, 1], bonds_r))["dice_one"] == 1          # vocabulary index 0 reads as carbon


def test_unbonded_record_atom_is_dropped():
    rec = so.record([1, 7, 3], [(0, 2, 2)])                  # the sulphur is in no bond
    row = _row(so.mol([1, 3], [(1, 2, 2)]), rec)
    assert row["atoms_true"] == 2 and row["envs_true"] == 8 and row["dice_one"] == 1 and row["refine_equal"] == 1
    # the molecule's atoms all take part
    row = _row(so.mol([1, 3, 7], [(1, 2, 2)]), rec)
    assert row["atoms_pred"] == 3 and row["size_equal"] == 0 and row["envs_common"] == 8 and row["envs_pred"] == 12


def test_invalid_rows_are_skipped():
    good = _row(so.mol([1, 2], [(1, 2, 1)]), so.record([1, 2], [(0, 1, 1)]))
    junk = [(0, 1, 1), (1, 3, 1), (2, 2, 1), (-1, 2, 1), (1 << 30, 1, 1)]
    assert _row(so.mol([1, 2], [(1, 2, 1)] + junk), so.record([1, 2], [(0, 1, 1)])) == good
    assert _row(so.mol([1, 2], [(1, 2, 1)]), so.record([1, 2], [(0, 1, 1), (0, 2, 1), (1, 1, 1), (-1, 0, 1), (5, 0, 1)])) == good
    # a pair listed twice counts twice
    twice = _row(so.mol([1, 2], [(1, 2, 1), (2, 1, 1)]), so.record([1, 2], [(0, 1, 1)]))
    assert twice["size_equal"] == 0 and twice["envs_common"] == 0


def test_empty_and_truncated_rows():
    rec = so.record([1, 2, 3], [(0, 1, 1)])
    assert so.rows([None], [rec])[0].tolist() == [1, 1, 0, 0, 0, 0, 0, 0, 0, 8, 0, 0]
    row = _row(so.mol([1, 2], [(1, 2, 1)], truncated=True), rec)
    assert row["truncated"] == 1 and row["dice_one"] == 1
    # no atoms on either side: nothing to compare, and nothing different
    assert so.rows([so.mol([], [])], [so.record([], [])])[0].tolist() == [1, 0, 0, 1, 1, 0, 0, 0, 0, 0, 0, 0]
    assert so.rows([so.mol([1], [])] * 3, [rec], n_valid=2)[:, COL["counted"]].tolist() == [1, 1, 0]


# ---------------------------------------------------------------------------------------------------------------- refusals
@pytest.mark.parametrize("kw", [dict(), dict(assemble=True), dict(evaluate=True), dict(extract=True, evaluate=True)])
def test_score_similarity_needs_assemble_and_evaluate(kw):
    from abcnet_amd.infer import InferenceRunner
    with pytest.raises(ValueError, match="score_similarity=True.*assemble=True and evaluate=True"):
        InferenceRunner(_Heads(), 2, 64, 64, score_similarity=True, **kw)


def test_bad_shapes_are_refused_before_the_device_is_touched():
    from abcnet_amd.ops import GraphSimilarity
    z = lambda *s: torch.zeros(s, dtype=torch.int32)
    c, a, q = z(2, 4), z(2, 8, 5), z(2, 16, 4)
    for args in ((c, z(2, 8, 4), q), (c, a, z(2, 16, 3)), (z(3, 4), a, q), (z(2, 3), a, q), (c, a, z(3, 16, 4)), (c, z(2, 8), q),
                 (c, a, z(2, 0, 4)), (None, a, q)):
        with pytest.raises(ValueError):
            GraphSimilarity(*args)
    with pytest.raises(ValueError, match="512"):
        GraphSimilarity(c, z(2, 513, 5), q)
    with pytest.raises(ValueError, match="512"):
        GraphSimilarity(c, a, q, max_atoms=513)
    for kw in (dict(max_atoms=0), dict(max_bonds=0), dict(n_valid=torch.zeros(2, dtype=torch.int32)), dict(records="scorer")):
        with pytest.raises(ValueError):
            GraphSimilarity(c, a, q, **kw)
    # well-formed host tensors: there is no CPU form (the bond capacities are free)
    with pytest.raises(L.AbcNetHipError):
        GraphSimilarity(c, z(2, 512, 5), z(2, 4096, 4), max_atoms=512, max_bonds=4096)


# ---------------------------------------------------------------------------------------------------------------- the library
def test_symbols_and_descriptor_size():
    assert "abc_graph_similarity_update" in L.SYMBOLS and "abc_graph_similarity_desc_size" in L.SYMBOLS
    assert L.GraphSimilarityDesc not in L._STRUCTS
    lib = L.load()
    assert lib.abc_graph_similarity_desc_size() == C.sizeof(L.GraphSimilarityDesc)
    assert L.GRAPH_SIM_COLUMNS == so.COLUMNS and len(L.GRAPH_SIM_COLUMNS) == 12 and L.GRAPH_SIM_IDS == so.IDS
    header = open(os.path.join(ROOT, "include", "abcnet_hip.h")).read()
    assert "ABC_SIM_NCOL = 12" in header and "ABC_SIM_IDS = 2048" in header
    names = header[header.index("ABC_SIM_COUNTED"):header.index("ABC_SIM_NCOL")].replace("enum {", "").replace("= 0", "")
    assert tuple(n.strip()[len("ABC_SIM_"):].lower() for n in names.split(",") if n.strip()) == L.GRAPH_SIM_COLUMNS


def _desc(**kw):
    return fake_desc(L.GraphSimilarityDesc, SCORE_POINTERS, SCORE_DEFAULTS, **kw)


def test_launcher_refuses_bad_descriptors_on_the_host():
    lib = L.load()
    for kw, word in ((dict(B=0), b"empty"), (dict(cap_atoms=0), b"cap_atoms"), (dict(cap_atoms=513), b"cap_atoms must be 1..512"),
                     (dict(cap_mol_bonds=0), b"cap_mol_bonds"), (dict(max_atoms=0), b"max_atoms"),
                     (dict(max_atoms=513), b"max_atoms must be 1..512"), (dict(max_bonds=0), b"max_bonds"),
                     (dict(mol_counts=None), b"null"), (dict(mol_bonds=None), b"null"), (dict(rec_atoms=None), b"null"),
                     (dict(rec_counts=None), b"null"), (dict(rows=None), b"null"), (dict(totals=None), b"null")):
        assert lib.abc_graph_similarity_update(C.byref(_desc(**kw)), None) == -1, kw
        assert word in lib.abc_last_error(), (kw, lib.abc_last_error())
