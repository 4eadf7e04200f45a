"""The score after assembly, host half (no GPU): raster.parse_graph against the brute-force oracle, the CPU closed loop through
the existing oracles, the refusals and the C ABI of csrc/graph_score.hip."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import abcnet_amd  # noqa: E402,F401
from abcnet_amd import _lib as L  # noqa: E402
from abcnet_amd.raster import parse_graph, parse_record  # noqa: E402
from abcnet_amd.synthetic import drawn_molecules, random_annotations  # noqa: E402
import graphscore_oracle as go  # noqa: E402
from molrows import SCORE_DEFAULTS, SCORE_POINTERS, fake_desc, Heads as _Heads  # noqa: E402


def _same_graph(got, want):
    atoms, bonds = got
    assert atoms.dtype == np.int32 and bonds.dtype == np.int32 and atoms.shape[1:] == (4,) and bonds.shape[1:] == (3,)
    assert atoms.tolist() == [list(a) for a in want[0]]
    assert bonds.tolist() == [list(q) for q in want[1]]


# draws as draw_augment makes them: a scale of 0.8 .. 1 per axis and non-zero integer offsets
DRAWS = [(1, 1, 0, 0), (0.8, 1.0, 7, 3), (0.93, 0.81, 11, 40), (1.0, 0.8725, 1, 99), (0.9990234375, 0.9, 64, 5)]


def _random_cases(seed):
    return [(random_annotations(12 + seed, 40, 100 * seed + k, size=400), offs) for k, offs in enumerate(DRAWS)]


@pytest.mark.parametrize("seed", [0, 1, 2, 3, 4])
def test_parse_graph_equals_the_oracle_on_random_annotations(seed):
    h = 128
    for (a, q), offs in _random_cases(seed):
        got = parse_graph(a, q, *offs, h=h)
        _same_graph(got, go.parse_graph(a, q, *offs))
        rec = parse_record(a, q, *offs, h=h)
        assert np.array_equal(got[0][:, :2], rec[0][:, :2])                   # the cells are parse_record's
        assert len(got[1]) < len(q.split(";")) - 1                             # some bond named one atom twice, or a listed pair
        assert (got[1][:, 0] < got[1][:, 1]).all() and len({(i, j) for i, j, _ in got[1].tolist()}) == len(got[1])


def test_random_annotations_cover_every_code_and_the_unknown_element():
    codes, elements = set(), set()
    for seed in range(5):
        for (a, q), offs in _random_cases(seed):
            atoms, bonds = parse_graph(a, q, *offs, h=128)
            codes |= set(bonds[:, 2].tolist())
            elements |= set(atoms[:, 2].tolist())
            if "c:" in a or "n:" in a:                                          # lower-case single letters are upper-cased
                low = [i for i, t in enumerate(a.split(";")[:-1]) if t[:2] in ("c:", "n:")]
                assert all(atoms[i, 2] == {"c": 1, "n": 2}[a.split(";")[i][0]] for i in low)
    assert codes == {1, 2, 3, 4, 5, 6} and -1 in elements and 0 not in elements


def test_parse_graph_equals_the_oracle_on_drawn_molecules():
    _x, notes = drawn_molecules(8, 512, seed=5)
    for (a, q), offs in zip(notes, DRAWS + DRAWS):
        offs = (offs[0], offs[1], offs[2] % 12, offs[3] % 12)                  # (the drawings reach the border of the canvas)
        got = parse_graph(a, q, *offs, h=128)
        _same_graph(got, go.parse_graph(a, q, *offs))
        assert np.array_equal(got[0][:, :2], parse_record(a, q, *offs, h=128)[0][:, :2])
        assert len(got[1]) == len(q.split(";")) - 1 if q else len(got[1]) == 0   # a drawing lists every pair once


def test_parse_graph_by_hand():
    atoms = "c:10,10,0;Xx:50,10,1,0;N:10,50,-1;Cl:50,50,0,2;"
    bonds = ("1:30,10,20,0,0,0;"       # (10,10) - (50,10): atoms 0, 1
             "2:30,10,-20,0,0,0;"      # the same pair from the other side: dropped
             "1:10,30,0,20,1,0;"       # stereo 1: code 5
             "1:50,30,0,20,6,1;"       # stereo 6: code 6
             "3:10,10,2,2,0,0;"        # both ends nearest to atom 0: dropped
             "4:40,30,10,20,0,0;"      # end (30,10) is as far from atom 0 as from atom 1: the first wins -> atoms 0, 3
             "1:30,30,20,20,5,0;"      # stereo 5 on the pair 0, 3: listed already, dropped
             "7:30,30,-20,20,0,0;")    # an order outside the vocabulary reads as type index 0: code 1; ends given high end first
    got = parse_graph(atoms, bonds)
    assert got[0].tolist() == [[2, 2, 1, 0], [12, 2, -1, 1], [2, 12, 2, -1], [12, 12, 6, 0]]
    assert got[1].tolist() == [[0, 1, 1], [0, 2, 5], [1, 3, 6], [0, 3, 4], [1, 2, 1]]
    _same_graph(got, go.parse_graph(atoms, bonds))
    # no atoms: every bond is dropped; no bonds: an empty [0, 3]
    assert parse_graph("", bonds)[1].shape == (0, 3) and parse_graph(atoms, "")[1].shape == (0, 3)
    with pytest.raises(ValueError):
        parse_graph("C:600,10,0;", "", h=128)


def test_cpu_closed_loop_floor():
    """annotation -> raster_oracle -> ideal logits -> nms_oracle -> decode_oracle -> assemble_oracle -> oracle score at radius 0 on
    drawn_molecules(6, 512, seed=5).  Measured: every bonded atom located, every bond matched, exact in 1 of 6 images (the other
    five: the valence repair renames chemically impossible synthetic atoms, atoms_matched 8/9, 13/21, 12/15, 10/15, 6/14)."""
    notes, records, mols, rows = go.closed_loop()
    col = {c: rows[:, i] for i, c in enumerate(go.COLUMNS)}
    print({c: v.tolist() for c, v in col.items()})
    assert len(notes) == 6 and all(m is not None for m in mols)
    assert (col["atoms_true"] > 0).all() and (col["bonds_true"] > 0).all()
    assert (col["atoms_located"] == col["atoms_true"]).all() and (col["atoms_true"] == col["atoms_pred"]).all()
    assert (col["bonds_matched"] == col["bonds_true"]).all() and (col["bonds_true"] == col["bonds_pred"]).all()
    assert (col["bonds_equal"] == 1).all() and (col["none"] == 0).all() and (col["truncated"] == 0).all()
    assert col["exact"].sum() >= 1
    # the product's records are the oracle's
    for (a, q), want in zip(notes, records):
        _same_graph(parse_graph(a, q, h=128), want)


def test_oracle_score_by_hand():
    atoms = [(2, 2, 1, 0), (12, 2, 2, 1), (2, 12, 3, 0), (40, 40, 1, 0)]      # atom 3 is in no bond: not in T
    bonds = [(0, 1, 1), (0, 2, 2)]
    mol = dict(symbols=["C", "N", "O"], charges=[0, 1, 0], positions=[[2, 2], [12, 2], [2, 12]], bonds=[[1, 2], [3, 1]], orders=[1, 2],
               truncated=False)
    s = go.score(mol, atoms, bonds)
    assert [s[c] for c in go.COLUMNS] == [1, 0, 0, 1, 1, 1, 3, 3, 3, 3, 2, 2, 2, 2]
    s = go.score(None, atoms, bonds)
    assert [s[c] for c in go.COLUMNS] == [1, 1, 0, 0, 0, 0, 3, 0, 0, 0, 2, 0, 0, 0]
    mol["positions"][1] = [13, 2]
    assert go.score(mol, atoms, bonds)["atoms_located"] == 2 and go.score(mol, atoms, bonds, radius=1)["exact"] == 1


# ---------------------------------------------------------------------------------------------------------------- refusals
@pytest.mark.parametrize("kw", [dict(), dict(assemble=True), dict(evaluate=True), dict(extract=True, evaluate=True)])
def test_score_graphs_needs_assemble_and_evaluate(kw):
    from abcnet_amd.infer import InferenceRunner
    with pytest.raises(ValueError, match="assemble=True and evaluate=True"):
        InferenceRunner(_Heads(), 2, 64, 64, score_graphs=True, **kw)


def _rows(B=2, cap_atoms=8, cap_mol_bonds=16):
    z = lambda *s: torch.zeros(s, dtype=torch.int32)
    return z(B, 4), z(B, cap_atoms, 5), z(B, cap_mol_bonds, 4)


def test_bad_shapes_are_refused_before_the_device_is_touched():
    from abcnet_amd.ops import GraphScore
    z = lambda *s: torch.zeros(s, dtype=torch.int32)
    c, a, q = _rows()
    for args in ((c, z(2, 8, 4), q), (c, a, z(2, 16, 3)), (z(3, 4), a, q), (z(2, 3), a, q), (c, a, z(3, 16, 4)), (c, z(2, 8), q),
                 (c, z(2, 2049, 5), q), (c, a, z(2, 0, 4)), (None, a, q)):
        with pytest.raises(ValueError):
            GraphScore(*args)
    for kw in (dict(max_atoms=0), dict(max_atoms=1025), dict(max_bonds=0), dict(max_bonds=1025), dict(radius=-1),
               dict(n_valid=torch.zeros(2, dtype=torch.int32))):
        with pytest.raises(ValueError):
            GraphScore(c, a, q, **kw)
    # well-formed host tensors: there is no CPU form
    with pytest.raises(L.AbcNetHipError):
        GraphScore(c, a, q)


# ---------------------------------------------------------------------------------------------------------------- the library
def test_symbols_and_descriptor_size():
    assert "abc_graph_score_update" in L.SYMBOLS and "abc_graph_score_desc_size" in L.SYMBOLS
    assert L.GraphScoreDesc not in L._STRUCTS                       # (it reports its own size, as abc_eval_desc)
    lib = L.load()
    assert lib.abc_graph_score_desc_size() == C.sizeof(L.GraphScoreDesc)
    assert L.GRAPH_SCORE_COLUMNS == go.COLUMNS and len(L.GRAPH_SCORE_COLUMNS) == 14
    header = open(os.path.join(go.ROOT, "include", "abcnet_hip.h")).read()
    assert "abc_graph_score_update" in header and "abc_graph_score_desc_size" in header


def _desc(**kw):
    return fake_desc(L.GraphScoreDesc, SCORE_POINTERS, SCORE_DEFAULTS, **kw)


def test_launcher_refuses_bad_descriptors_on_the_host():
    lib = L.load()
    for kw, word in ((dict(B=0), b"empty"), (dict(cap_atoms=0), b"cap_atoms"), (dict(cap_atoms=2049), b"cap_atoms"),
                     (dict(cap_mol_bonds=0), b"cap_mol_bonds"), (dict(max_atoms=0), b"max_atoms"), (dict(max_atoms=1025), b"max_atoms"),
                     (dict(max_bonds=0), b"max_bonds"), (dict(max_bonds=1025), b"max_bonds"), (dict(radius=-1), b"radius"),
                     (dict(mol_counts=None), b"null"), (dict(mol_bonds=None), b"null"), (dict(rec_atoms=None), b"null"),
                     (dict(rec_counts=None), b"null"), (dict(rows=None), b"null"), (dict(totals=None), b"null")):
        assert lib.abc_graph_score_update(C.byref(_desc(**kw)), None) == -1, kw
        assert word in lib.abc_last_error(), (kw, lib.abc_last_error())
