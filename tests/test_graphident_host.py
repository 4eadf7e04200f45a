"""The verified isomorphism test, host half (no GPU): the oracle of tests/graphident_oracle.py against networkx and by hand, the budgets
the defaults were chosen from, the refusals and the C ABI of csrc/graph_ident.hip."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import abcnet_amd  # noqa: E402,F401
from abcnet_amd import _lib as L  # noqa: E402
import graphident_oracle as io  # noqa: E402
import graphsim_oracle as so  # noqa: E402
from molrows import SCORE_DEFAULTS, SCORE_POINTERS, fake_desc, Heads as _Heads  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COL = {c: i for i, c in enumerate(io.COLUMNS)}
WORK = ("levels", "tries", "backtracks", "rounds")


def _row(mol, rec, **budgets):
    return io.score(mol, rec[0], rec[1], **budgets)[0]


def _answer(mol, rec, **budgets):
    row = _row(mol, rec, **budgets)
    assert row["same"] + row["different"] + row["undecided"] == 1
    return "same" if row["same"] else ("different" if row["different"] else "undecided")


def _is_witness(gp, gt, m):
    """m is a bijection of the atoms that preserves class, charge and the multiset of (end, end, order class): no ids, no oracle"""
    n = len(gp[0])
    if m is None or len(m) != n or n != len(gt[0]) or sorted(m) != list(range(n)):
        return False
    if any(gp[0][a] != gt[0][m[a]] or gp[1][a] != gt[1][m[a]] for a in range(n)):
        return False
    count = {}
    for i, j, o in gt[2]:
        k = (min(i, j), max(i, j), o)
        count[k] = count.get(k, 0) + 1
    for i, j, o in gp[2]:
        k = (min(m[i], m[j]), max(m[i], m[j]), o)
        if count.get(k, 0) == 0:
            return False
        count[k] -= 1
    return not any(count.values())


# ---------------------------------------------------------------------------------------------------------------- the oracle
def test_vectorised_rounds_are_the_similaritys():
    rng = np.random.RandomState(1)
    x = rng.randint(0, 2 ** 62, size=64).astype(np.uint64) * np.uint64(4) + np.uint64(3)
    assert [so.mix(int(v)) for v in x] == io.mixv(x).tolist()
    for _ in range(10):
        g = so.of_record(*so.random_graph(rng, int(rng.randint(2, 13)), extra=3))
        side = io._Side(g)
        ids = side.init.copy()
        for r in range(1, 6):
            ids = side.round(ids, r)
            assert ids.tolist() == so.ids(g, r)[r]
    assert io.indiv(5, 0) != io.indiv(5, 1) and io.indiv(5, 0) == so.mix(so.mix(5) + io.GOLD)


def test_same_is_isomorphic_on_random_pairs():
    """2000 seeded pairs, n = 2..12: `same` <=> networkx finds an isomorphism of the labelled multigraphs, nothing is undecided, every
    witness is a label- and bond-preserving bijection, and the answer sits between the similarity's columns"""
    pytest.importorskip("networkx")
    same = different = 0
    most = dict.fromkeys(WORK, 0)
    for mol, rec in io.random_pairs(2000, seed=11):
        gp, gt = so.of_molecule(mol), so.of_record(*rec)
        res, witness = io.identify(gp, gt)
        assert res["undecided"] == 0 and res["same"] + res["different"] == 1
        assert bool(res["same"]) == io.brute(gp, gt), (mol, rec, res)
        assert (witness is not None) == bool(res["same"])
        if res["same"]:
            assert _is_witness(gp, gt, witness), (mol, rec, witness)
        sim = so.score(mol, *rec)
        assert not res["same"] or (sim["refine_equal"] and sim["dice_one"]), (mol, rec)
        assert sim["refine_equal"] or res["different"], (mol, rec)
        same += res["same"]
        different += res["different"]
        for k in WORK:
            most[k] = max(most[k], res[k])
    assert same >= 900 and different >= 900
    assert most == dict(levels=2, tries=2, backtracks=0, rounds=6)


def test_decalin_is_not_bicyclopentyl():
    """the pair refine_equal cannot separate (test_graphsim_host.test_decalin_and_bicyclopentyl_pass_refinement)"""
    assert so.score(so.as_mol(so.DECALIN), *so.BICYCLOPENTYL)["refine_equal"] == 1
    row = _row(so.as_mol(so.DECALIN), so.BICYCLOPENTYL)
    assert [row[c] for c in io.COLUMNS] == [1, 0, 0, 1, 0, 1, 0, 2, 2, 2, 20]
    row = _row(so.as_mol(so.BICYCLOPENTYL), so.DECALIN)
    assert [row[c] for c in io.COLUMNS] == [1, 0, 0, 1, 0, 1, 0, 3, 2, 2, 21]
    rng = np.random.RandomState(8)
    for rec in (so.DECALIN, so.BICYCLOPENTYL):
        for _ in range(5):
            assert _answer(so.as_mol(so.permuted(rng, rec)), rec) == "same"


def test_a_union_of_refinement_equal_components_needs_a_backtrack():
    mol = so.as_mol(io.UNION_PERMUTED)
    gp, gt = so.of_molecule(mol), so.of_record(*io.UNION)
    res, witness = io.identify(gp, gt)
    assert res["same"] == 1 and res["backtracks"] >= 1 and {k: res[k] for k in WORK} == io.UNION_COUNTERS
    assert _is_witness(gp, gt, witness) and io.brute(gp, gt)
    # a budget exit of either kind: counted, never hidden
    short = _row(mol, io.UNION, max_tries=1)
    assert [short[c] for c in io.COLUMNS] == [1, 0, 0, 1, 0, 0, 1, 5, 1, 1, 25]
    short = _row(mol, io.UNION, max_rounds=20)
    assert [short[c] for c in io.COLUMNS] == [1, 0, 0, 1, 0, 0, 1, 5, 1, 0, 20]
    assert io.score(mol, *io.UNION, max_tries=1)[1] is None
    # out of rounds on the molecule's own path: no level was finished
    assert [_row(mol, io.UNION, max_rounds=3)[c] for c in io.COLUMNS] == [1, 0, 0, 1, 0, 0, 1, 0, 0, 0, 3]
    # the two components swapped for each other's twins: refinement-equal still, and different
    twins = io.union(so.DECALIN, so.DECALIN)
    assert so.score(so.as_mol(twins), *io.UNION)["refine_equal"] == 1 and _answer(so.as_mol(twins), io.UNION) == "different"


# the symmetric worst cases the default budgets were chosen from: (record, levels, tries, backtracks, rounds)
WORST = {"a ring of 512 carbons": (io.carbon_ring(512), 2, 2, 0, 988),
         "a chain of 512 carbons": (io.carbon_chain(512), 1, 1, 0, 1008),
         "170 disjoint C-C-C": (io.propanes(170), 254, 254, 0, 1018),
         "a six-ring of order-4 bonds": (io.carbon_ring(6, order=4), 2, 2, 0, 12)}


@pytest.mark.parametrize("name", sorted(WORST))
def test_symmetric_worst_cases_stay_inside_the_default_budgets(name):
    rec, levels, tries, backtracks, rounds = WORST[name]
    for mol in (so.as_mol(rec), so.as_mol(so.permuted(np.random.RandomState(5), rec))):
        res, witness = io.identify(so.of_molecule(mol), so.of_record(*rec))
        assert res["same"] == 1 and sorted(witness) == list(range(len(rec[0])))
        assert [res[k] for k in WORK] == [levels, tries, backtracks, rounds]
    # the constants beside which these numbers are written (include/abcnet_hip.h), with room to spare
    assert 8 * tries <= io.DEFAULT_TRIES == L.IDENT_DEFAULT_TRIES and 8 * rounds <= io.DEFAULT_ROUNDS == L.IDENT_DEFAULT_ROUNDS


# ------------------------------------------------------------------------------------------------------------ the normalisation
def test_wedge_codes_fold_to_a_single_bond():
    rec = so.record([1, 2, 3], [(0, 1, 1), (1, 2, 2)])
    for code in (5, 6):
        assert _answer(so.mol([1, 2, 3], [(1, 2, code), (2, 3, 2)]), rec) == "same"
        assert _answer(so.mol([1, 2, 3], [(1, 2, 1), (2, 3, 2)]), so.record([1, 2, 3], [(0, 1, code), (1, 2, 2)])) == "same"
    assert _answer(so.mol([1, 2, 3], [(1, 2, 5), (2, 3, 6)]), rec) == "different"
    # aromatic stays aromatic, and a code outside 1..6 is a class of its own
    assert _answer(so.mol([1, 2, 3], [(1, 2, 4), (2, 3, 2)]), rec) == "different"
    assert _answer(so.mol([1, 2, 3], [(1, 2, 9), (2, 3, 2)]), rec) == "different"
    assert _answer(so.mol([1, 2, 3], [(1, 2, 9), (2, 3, 2)]), so.record([1, 2, 3], [(0, 1, -4), (1, 2, 2)])) == "same"


def test_unknown_equals_only_unknown():
    bonds_m, bonds_r = [(1, 2, 1)], [(0, 1, 1)]
    assert _answer(so.mol([99, 1], bonds_m), so.record([-1, 1], bonds_r)) == "same"
    assert _answer(so.mol([-5, 1], bonds_m), so.record([-1, 1], bonds_r)) == "same"
    for known in range(14):
        assert _answer(so.mol([known, 1], bonds_m), so.record([-1, 1], bonds_r)) == "different", known
    assert _answer(so.mol([0, 1], bonds_m), so.record([1, 1], bonds_r)) == "same"            # vocabulary index 0 reads as carbon
    # the charge counts as stored
    assert _answer(so.mol([2, 1], bonds_m, charges=[1, 0]), so.record([2, 1], bonds_r, charges=[1, 0])) == "same"
    assert _answer(so.mol([2, 1], bonds_m, charges=[1, 0]), so.record([2, 1], bonds_r, charges=[0, 1])) == "different"


def test_unbonded_record_atom_is_dropped_and_the_witness_names_original_indices():
    rec = so.record([1, 7, 3], [(0, 2, 2)])                  # the sulphur is in no bond
    row, witness = io.score(so.mol([3, 1], [(1, 2, 2)]), *rec)
    assert row["same"] == 1 and witness == [2, 0]            # (the oxygen is record atom 2, not number 1 of T)
    # the molecule's atoms all take part
    row = _row(so.mol([1, 3, 7], [(1, 2, 2)]), rec)
    assert row["size_equal"] == 0 and row["different"] == 1 and [row[k] for k in WORK] == [0, 0, 0, 0]


def test_invalid_rows_are_skipped_and_a_pair_listed_twice_counts_twice():
    junk = [(0, 1, 1), (1, 3, 1), (2, 2, 1), (-1, 2, 1), (1 << 30, 1, 1)]
    assert _answer(so.mol([1, 2], [(1, 2, 1)] + junk), so.record([1, 2], [(0, 1, 1)])) == "same"
    assert _answer(so.mol([1, 2], [(1, 2, 1)]), so.record([1, 2], [(0, 1, 1), (0, 2, 1), (1, 1, 1), (-1, 0, 1), (5, 0, 1)])) == "same"
    twice = _row(so.mol([1, 2], [(1, 2, 1), (2, 1, 1)]), so.record([1, 2], [(0, 1, 1)]))
    assert twice["size_equal"] == 0 and twice["different"] == 1
    assert _answer(so.mol([1, 2], [(1, 2, 1), (2, 1, 2)]), so.record([1, 2], [(0, 1, 2), (0, 1, 1)])) == "same"
    assert _answer(so.mol([1, 2], [(1, 2, 1), (2, 1, 1)]), so.record([1, 2], [(0, 1, 2), (0, 1, 1)])) == "different"
    # two triangles sharing nothing but their degree sequence with a doubled path: the verification is a multiset comparison
    assert _answer(so.mol([1, 1, 1], [(1, 2, 1), (2, 3, 1), (1, 3, 1)]), so.record([1, 1, 1], [(0, 1, 1), (0, 1, 1), (1, 2, 1)])) == "different"


def test_empty_truncated_n_valid_and_nothing_on_either_side():
    rec = so.record([1, 2, 3], [(0, 1, 1)])
    assert io.rows([None], [rec])[0].tolist() == [1, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0]
    row = _row(so.mol([1, 2], [(1, 2, 1)], truncated=True), rec)
    assert row["truncated"] == 1 and row["same"] == 1
    # no atoms on either side: nothing to map, and nothing different -- one round per side says so
    assert io.rows([so.mol([], [])], [so.record([], [])])[0].tolist() == [1, 0, 0, 1, 1, 0, 0, 0, 0, 0, 2]
    assert io.rows([so.mol([], [])], [so.record([1, 2], [])])[0].tolist() == [1, 0, 0, 1, 1, 0, 0, 0, 0, 0, 2]
    rows, maps = io.rows_and_maps([so.mol([1, 2], [(1, 2, 1)])] * 3, [rec, rec, rec], cap_atoms=4, n_valid=2)
    assert rows[:, COL["counted"]].tolist() == [1, 1, 0] and rows[:, COL["same"]].tolist() == [1, 1, 0]
    assert maps.tolist() == [[0, 1, -1, -1]] * 2 + [[-1] * 4]


def test_order_of_atoms_rows_and_ends_changes_no_answer():
    rng = np.random.RandomState(7)
    answers = {"same": 0, "different": 0}
    for k in range(60):
        a = so.random_graph(rng, int(rng.randint(3, 13)), extra=3)
        b = so.one_atom_changed(rng, a) if k % 2 else a
        want = _answer(so.as_mol(b), a)
        assert want == _answer(so.as_mol(so.permuted(rng, b)), a) == _answer(so.as_mol(b), so.permuted(rng, a)), (a, b)
        answers[want] += 1
    assert answers["same"] >= 30 and answers["different"] >= 25
    rng = np.random.RandomState(9)
    for _ in range(6):
        assert _answer(so.as_mol(so.permuted(rng, io.UNION)), so.permuted(rng, io.UNION)) == "same"
        assert _answer(so.as_mol(so.permuted(rng, so.DECALIN)), so.permuted(rng, so.BICYCLOPENTYL)) == "different"


# ---------------------------------------------------------------------------------------------------------------- refusals
@pytest.mark.parametrize("kw", [dict(), dict(assemble=True), dict(evaluate=True), dict(extract=True, evaluate=True)])
def test_score_identity_needs_assemble_and_evaluate(kw):
    from abcnet_amd.infer import STAGES, InferenceRunner
    with pytest.raises(ValueError, match="score_identity=True.*assemble=True and evaluate=True"):
        InferenceRunner(_Heads(), 2, 64, 64, score_identity=True, **kw)
    stages = list(STAGES)
    assert STAGES["identity"] == "score_identity" and stages.index("identity") == stages.index("similarity") + 1


def test_bad_shapes_and_budgets_are_refused_before_the_device_is_touched():
    from abcnet_amd.ops import GraphIdentity
    z = lambda *s: torch.zeros(s, dtype=torch.int32)
    c, a, q = z(2, 4), z(2, 8, 5), z(2, 16, 4)
    for args in ((c, z(2, 8, 4), q), (c, a, z(2, 16, 3)), (z(3, 4), a, q), (z(2, 3), a, q), (c, a, z(3, 16, 4)), (c, z(2, 8), q),
                 (c, a, z(2, 0, 4)), (None, a, q)):
        with pytest.raises(ValueError):
            GraphIdentity(*args)
    with pytest.raises(ValueError, match="512"):
        GraphIdentity(c, z(2, 513, 5), q)
    with pytest.raises(ValueError, match="512"):
        GraphIdentity(c, a, q, max_atoms=513)
    for kw in (dict(max_atoms=0), dict(max_bonds=0), dict(n_valid=torch.zeros(2, dtype=torch.int32)), dict(records="scorer"),
               dict(max_tries=0), dict(max_tries=-1), dict(max_rounds=0), dict(max_rounds=1 << 31)):
        with pytest.raises(ValueError):
            GraphIdentity(c, a, q, **kw)
    # well-formed host tensors: there is no CPU form (the bond capacities are free)
    with pytest.raises(L.AbcNetHipError):
        GraphIdentity(c, z(2, 512, 5), z(2, 4096, 4), max_atoms=512, max_bonds=4096, max_tries=1, max_rounds=1, witness=True)


# ---------------------------------------------------------------------------------------------------------------- the library
def test_symbols_and_descriptor_size():
    assert "abc_graph_identity_update" in L.SYMBOLS and "abc_graph_identity_desc_size" in L.SYMBOLS
    assert L.GraphIdentityDesc not in L._STRUCTS
    assert (L.GraphIdentityDesc, "abc_graph_identity_desc_size") in L.SELF_SIZED_SINCE
    assert L.GraphIdentityDesc not in [st for st, _ in L.SELF_SIZED]
    lib = L.load()
    assert lib.abc_graph_identity_desc_size() == C.sizeof(L.GraphIdentityDesc)
    assert L.GRAPH_IDENT_COLUMNS == io.COLUMNS and len(L.GRAPH_IDENT_COLUMNS) == 11
    header = open(os.path.join(ROOT, "include", "abcnet_hip.h")).read()
    assert "ABC_IDENT_NCOL = 11" in header
    assert "ABC_IDENT_DEFAULT_TRIES = %d, ABC_IDENT_DEFAULT_ROUNDS = %d" % (io.DEFAULT_TRIES, io.DEFAULT_ROUNDS) in header
    names = header[header.index("ABC_IDENT_COUNTED"):header.index("ABC_IDENT_NCOL")].replace("enum {", "").replace("= 0", "")
    assert tuple(n.strip()[len("ABC_IDENT_"):].lower() for n in names.split(",") if n.strip()) == L.GRAPH_IDENT_COLUMNS
    # the two kernels share one definition of the ids
    csrc = os.path.join(ROOT, "abc-net_amd", "csrc")
    for name in ("graph_sim.hip", "graph_ident.hip"):
        text = open(os.path.join(csrc, name)).read()
        assert '#include "graph_ids.hpp"' in text and "0xBF58476D1CE4E5B9" not in text, name
    assert "graph_ident" in open(os.path.join(ROOT, "build_hip.sh")).read()


def _desc(**kw):
    return fake_desc(L.GraphIdentityDesc, SCORE_POINTERS, SCORE_DEFAULTS, **kw)


def test_launcher_refuses_bad_descriptors_on_the_host():
    lib = L.load()
    for kw, word in ((dict(B=0), b"empty"), (dict(cap_atoms=0), b"cap_atoms"), (dict(cap_atoms=513), b"cap_atoms must be 1..512"),
                     (dict(cap_mol_bonds=0), b"cap_mol_bonds"), (dict(max_atoms=0), b"max_atoms"),
                     (dict(max_atoms=513), b"max_atoms must be 1..512"), (dict(max_bonds=0), b"max_bonds"),
                     (dict(max_tries=-1), b"max_tries"), (dict(max_rounds=-1), b"max_rounds"),
                     (dict(mol_counts=None), b"null"), (dict(mol_bonds=None), b"null"), (dict(rec_atoms=None), b"null"),
                     (dict(rec_counts=None), b"null"), (dict(rows=None), b"null"), (dict(totals=None), b"null")):
        assert lib.abc_graph_identity_update(C.byref(_desc(**kw)), None) == -1, kw
        assert word in lib.abc_last_error() and b"graph_identity" in lib.abc_last_error(), (kw, lib.abc_last_error())
