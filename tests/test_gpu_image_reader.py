"""GPU tier of the one image reader (csrc/mol_rows.hpp: mol_image / rec_image): every op that reads molecule rows on ONE hand-made
batch whose counts lie -- an EMPTY image with counts and garbage rows behind it, an image whose counts exceed the capacities -- against
decode.Molecule on the rows a reader must see."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import abcnet_amd  # noqa: E402,F401
from abcnet_amd import _lib as L  # noqa: E402
from abcnet_amd.decode import Molecule  # noqa: E402
from abcnet_amd.ops import AromaticityPerceiver, GraphCanonicalizer, GraphSimilarity, MolBlockWriter, SmilesWriter  # noqa: E402
import graphsim_oracle as so  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
CAP = 8                              # cap_atoms and cap_mol_bonds
JUNK = 99                            # no vocabulary index, no atom of an image, no bond order
EMPTY = L.MOL_EMPTY
# (x, y, vocabulary index, charge, hs) and (end 1, end 2, order, source): C-C-O; a Kekule benzene with N on atom 1 and O on atom 4
CHAIN = ([(10, 10, 1, 0, 0), (20, 14, 1, 0, 0), (30, 10, 3, 0, 0)], [(1, 2, 1, 0), (2, 3, 1, 1)], [])
RING = ([(40, 20, 1, 0, 0), (50, 26, 1, 0, 0), (50, 38, 1, 0, 0), (40, 44, 1, 0, 0), (30, 38, 1, 0, 0), (30, 26, 1, 0, 0), (40, 8, 2, 0, 0),
         (40, 56, 3, 0, 0)],
        [(1, 2, 2, 0), (2, 3, 1, 1), (3, 4, 2, 2), (4, 5, 1, 3), (5, 6, 2, 4), (6, 1, 1, 5), (1, 7, 1, 6), (4, 8, 1, 7)],
        [7, 7, 8, 7, 7, 8, 7, 7])
COUNTS = ((3, 2, 0, 0), (5, 4, 2, EMPTY), (100, 100, 100, 0))


@pytest.fixture(scope="module")
def batch():
    """(the four device tensors, [Molecule, None, Molecule]): the words no reader may see hold JUNK"""
    cnt = np.array(COUNTS, dtype=np.int32)
    atoms, bonds, implh = (np.full(s, JUNK, dtype=np.int32) for s in ((3, CAP, 5), (3, CAP, 4), (3, CAP)))
    for b, (a, q, h) in ((0, CHAIN), (2, RING)):
        atoms[b, :len(a)], bonds[b, :len(q)], implh[b, :len(h)] = a, q, h
    mols = [Molecule.from_device_rows(*CHAIN), None, Molecule.from_device_rows(*RING)]
    assert len(RING[0]) == len(RING[1]) == len(RING[2]) == CAP
    return tuple(torch.from_numpy(t).to(DEV) for t in (cnt, atoms, bonds, implh)), mols


def _run(op):
    op.run()
    torch.cuda.synchronize()
    return op


def test_the_text_writers_read_the_same_image(batch):
    rows, mols = batch
    texter = _run(MolBlockWriter(*rows))
    assert texter.molblocks() == [None if m is None else m.molblock() for m in mols] and texter.status() == [0, EMPTY, 0]
    assert "%3d%3d  0" % (CAP, CAP) in texter.molblocks()[2]
    plain, marked = _run(SmilesWriter(*rows)), _run(SmilesWriter(*rows, stereo=True, double_bonds=True))
    assert plain.smiles() == [None if m is None else m.smiles() for m in mols] and plain.status() == [0, EMPTY, 0]
    assert marked.smiles() == [None if m is None else m.smiles(stereo=True, double_bonds=True) for m in mols] and marked.status() == [0, EMPTY, 0]
    assert marked.stereo_stats()["rows"][1] == [0] * 4 and marked.double_bond_stats()["rows"][1] == [0] * 4
    assert not marked.parities()[1].any() and not marked.double_bond_codes()[1].any()
    assert marked.double_bond_codes()[2].tolist() == mols[2].double_bond_codes() and marked.parities()[2].tolist() == mols[2].stereo_centres()


def test_the_graph_ops_read_the_same_image(batch):
    rows, mols = batch
    canon = _run(GraphCanonicalizer(*rows))
    arom = _run(AromaticityPerceiver(*rows, codes=True))
    cs, orders, keys, as_, codes = canon.stats(), canon.orders(), canon.keys(), arom.stats(), arom.codes()
    assert cs[1].tolist() == (L.CANON_EMPTY,) + (0,) * (len(L.CANON_COLUMNS) - 1) and orders[1].tolist() == [-1] * CAP
    assert as_[1].tolist() == (EMPTY,) + (0,) * (len(L.AROMATIC_COLUMNS) - 1) and codes[1].tolist() == [L.AROM_NOT_CANDIDATE] * CAP
    out_c, out_a = [[t.cpu() for t in op.rows().tensors] for op in (canon, arom)]
    for b in (0, 2):
        m, n = mols[b], len(mols[b].symbols)
        rank, st, key = m.canonical_order()
        assert [int(cs[b][c]) for c in L.CANON_COLUMNS] == [st[c] for c in L.CANON_COLUMNS]
        assert orders[b].tolist() == sorted(range(n), key=lambda a: rank[a]) + [-1] * (CAP - n)
        assert [k & (1 << 64) - 1 for k in keys[b].tolist()] == list(key)
        want = m.canonical()
        assert Molecule.from_device_rows(out_c[1][b, :n], out_c[2][b, :len(m.bonds)], out_c[3][b, :len(m.implicit_hs)]) == want
        want, st, code = m.aromatic_perception()
        assert [int(as_[b][c]) for c in L.AROMATIC_COLUMNS] == [st[c] for c in L.AROMATIC_COLUMNS]
        assert codes[b].tolist() == list(code) + [L.AROM_NOT_CANDIDATE] * (CAP - n)
        assert Molecule.from_device_rows(out_a[1][b, :n], out_a[2][b, :len(m.bonds)], out_a[3][b, :len(want.implicit_hs)]) == want
    assert int(as_[2]["rows_changed"]) == 6 and int(as_[2]["aromatic"]) == 1      # (the six ring rows of image 2, all of them read)
    # the similarity against records that ARE the molecules: every environment of exactly n atoms is common
    recs = [(np.zeros((0, 4), np.int32), np.zeros((0, 3), np.int32)) if m is None else
            (np.array([a[:4] for a in im[0]], np.int32), np.array([(min(q[0], q[1]) - 1, max(q[0], q[1]) - 1, q[2]) for q in im[1]], np.int32))
            for m, im in zip(mols, (CHAIN, None, RING))]
    sim = GraphSimilarity(*rows[:3], max_atoms=CAP, max_bonds=CAP)
    sim.load(recs)
    got = _run(sim).result()["rows"]
    assert got.tolist() == so.rows(mols, recs).tolist()
    col = {c: i for i, c in enumerate(so.COLUMNS)}
    assert got[:, col["none"]].tolist() == [0, 1, 0] and got[:, col["atoms_pred"]].tolist() == [3, 0, CAP]
    assert got[:, col["dice_one"]].tolist() == [1, 0, 1] and got[:, col["refine_equal"]].tolist() == [1, 0, 1]
