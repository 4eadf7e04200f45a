"""The aromaticity perception on the device (csrc/aromatic.hip, ops.AromaticityPerceiver, InferenceRunner(aromatize=True)) against its
host form decode.Molecule.aromatic_perception / decode.perceive_aromatic, word for word: rows, implicit-H list, stats and codes.
Integers only: every comparison is torch.equal."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import abcnet_amd  # noqa: E402,F401
from abcnet_amd import _lib as L  # noqa: E402
from abcnet_amd import decode as D  # noqa: E402
from abcnet_amd.contract import GraphRecords  # noqa: E402
from abcnet_amd.ops import AromaticityPerceiver, GraphCanonicalizer, GraphIdentity, GraphScore, GraphSimilarity, SmilesWriter  # noqa: E402
import aromatic_oracle as A  # noqa: E402
from molrows import trained_unet  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
EMPTY, TRUNCATED = L.MOL_EMPTY, L.MOL_TRUNCATED
COL = {c: i for i, c in enumerate(L.AROMATIC_COLUMNS)}


def _arrays(images, cap_atoms, cap_bonds, junk):
    """images: (atoms, bonds, implh) rows, ("truncated", rows), or None (an EMPTY image whose counts lie) -> the four arrays of the
    assembler's layout; the words past the counts hold `junk`"""
    B = len(images)
    cnt = np.zeros((B, 4), dtype=np.int32)
    atoms = np.full((B, cap_atoms, 5), junk, dtype=np.int32)
    bonds = np.full((B, cap_bonds, 4), junk, dtype=np.int32)
    implh = np.full((B, cap_atoms), junk, dtype=np.int32)
    for b, im in enumerate(images):
        if im is None:
            cnt[b] = (3, 2, 1, EMPTY | TRUNCATED)
            continue
        status, rows = (TRUNCATED, im[1]) if im[0] == "truncated" else (0, im)
        a, q, h = rows
        cnt[b] = (len(a), len(q), len(h), status)
        atoms[b, :len(a)] = np.array(a, dtype=np.int32).reshape(-1, 5)
        bonds[b, :len(q)] = np.array(q, dtype=np.int32).reshape(-1, 4)
        implh[b, :len(h)] = h
    return cnt, atoms, bonds, implh


def _upload(images, cap_atoms, cap_bonds):
    """junk 1 past the counts: it would name atom 1 in a bond row and in the list"""
    return tuple(torch.from_numpy(t).to(DEV) for t in _arrays(images, cap_atoms, cap_bonds, 1))


def _expected(images, cap_atoms, cap_bonds):
    """(counts, atoms, bonds, implh, stats, codes) by the host form: zero past the counts, the counts of an EMPTY image copied"""
    out, stats, codes = [], np.zeros((len(images), len(COL)), dtype=np.int32), np.full((len(images), cap_atoms), L.AROM_NOT_CANDIDATE, dtype=np.int32)
    for b, im in enumerate(images):
        if im is None:
            out.append(None)
            stats[b, 0] = EMPTY | TRUNCATED
            continue
        rows = im[1] if im[0] == "truncated" else im
        m, st, code = A.molecule(rows).aromatic_perception()
        out.append((rows[0], [(q[0], q[1], o, q[3]) for q, o in zip(rows[1], m.orders)], m.implicit_hs))
        stats[b] = [st[c] for c in L.AROMATIC_COLUMNS]
        stats[b, 0] = TRUNCATED if im[0] == "truncated" else 0
        codes[b, :len(code)] = code
    cnt, atoms, bonds, implh = _arrays([o if o is None or images[b][0] != "truncated" else ("truncated", o) for b, o in enumerate(out)],
                                       cap_atoms, cap_bonds, 0)
    return cnt, atoms, bonds, implh, stats, codes


def _check(op, images):
    """one launch over pre-filled outputs (every word is written by every launch): everything equals the host form"""
    for t in op.rows().tensors + (op.stat, op.code):
        t.fill_(77)
    op.run()
    torch.cuda.synchronize()
    want = _expected(images, op.cap, op.cap_bonds)
    got = tuple(t.cpu() for t in op.rows().tensors + (op.stat, op.code))
    for name, g, w in zip(("mol_counts", "mol_atoms", "mol_bonds", "mol_implh", "stats", "codes"), got, want):
        bad = (g != torch.from_numpy(w)).flatten(1).any(1).nonzero().flatten().tolist()
        assert not bad, (name, bad[:8], [got[4][b].tolist() for b in bad[:4]], [want[4][b].tolist() for b in bad[:4]])
    return op.stats()


def _mol_op(images, cap_atoms, cap_bonds):
    return AromaticityPerceiver(*_upload(images, cap_atoms, cap_bonds), codes=True)


def _random(seed, count, **kw):
    rng = np.random.default_rng(seed)
    return [A.random_rows(rng, **kw) for _ in range(count)]


def _kekule_forms():
    """graphs with valid rows only (a record can hold them): the example table, and more than one ring system per image"""
    return [rows for _, rows, _, _ in A.EXAMPLES]


# --------------------------------------------------------------------------------------------------------------- against the host form
def test_the_example_table_in_one_batch():
    images = _kekule_forms()
    st = _check(_mol_op(images, 16, 16), images)
    for (name, rows, orders, listed), row in zip(A.EXAMPLES, st):
        assert row["rows_changed"] == (0 if orders is None else sum(o != q[2] for o, q in zip(orders, rows[1]))) and row["listed"] == len(listed), name
    assert st["aromatic"].sum() > 10


def test_random_graphs_equal_the_host_form():
    images = _random(31, 8, n_min=20, n_max=32)
    assert max(len(r[1]) for r in images) <= 64
    st = _check(_mol_op(images, 32, 64), images)
    assert st["cycles"].sum() > 0


def test_many_random_graphs_in_one_launch():
    """B = 256 small images: a launch costs the same, and the recipe reaches what eight graphs may miss"""
    images = _random(32, 256, n_min=6, n_max=32)
    st = _check(_mol_op(images, 32, 64), images)
    assert st["aromatic"].sum() > 0 and st["listed"].sum() > 0 and (st["cycles"] > st["aromatic"]).any()


def test_records_change_the_same_bonds_as_the_molecules():
    images = _kekule_forms()
    mol = _mol_op(images, 16, 16)
    _check(mol, images)
    records = GraphRecords(len(images), 16, 16, DEV)
    records.load([A.as_record(rows) for rows in images])
    op = AromaticityPerceiver.from_records(records, codes=True)
    op.out_bonds.fill_(77), op.stat.fill_(77), op.code.fill_(77)
    op.run()
    torch.cuda.synchronize()
    got, stats, codes = op.out_bonds.cpu().numpy(), op.stats(), op.codes().numpy()
    for b, rows in enumerate(images):
        rec_a, rec_q = A.as_record(rows)
        symbols = [D.ATOM_SYMBOLS[t] for t in rec_a[:, 2].tolist()]
        orders, code, st = D.perceive_aromatic((symbols, rec_a[:, 3].tolist(), [tuple(q) for q in rec_q.tolist()]))
        want = np.zeros((16, 3), dtype=np.int32)
        want[:len(rec_q)] = rec_q
        want[:len(rec_q), 2] = orders
        assert np.array_equal(got[b], want), b
        assert [int(stats[b][c]) for c in L.AROMATIC_COLUMNS] == [0, st["candidates"], st["cycles"], st["aromatic"], st["rows_changed"], 0]
        assert codes[b, :len(code)].tolist() == code and (codes[b, len(code):] == L.AROM_NOT_CANDIDATE).all()
        # the molecule side changed the same bonds
        assert got[b, :len(rec_q), 2].tolist() == mol.rows().tensors[2][b, :len(rec_q), 2].cpu().tolist()
    derived = op.records()
    assert isinstance(derived, GraphRecords) and derived.loaded and derived.staging.dev["bonds"] is op.out_bonds
    assert derived.staging.dev["atoms"] is records.staging.dev["atoms"]
    with pytest.raises(ValueError, match="load its source"):
        derived.load([])
    for scorer in (GraphScore, GraphSimilarity, GraphIdentity):          # the scorers and the canonicaliser accept the derived records
        s = scorer(mol.rows(), records=derived)
        assert s.d.rec_bonds == op.out_bonds.data_ptr() and s.records is derived
    assert GraphCanonicalizer.from_records(derived).d.rec_bonds == op.out_bonds.data_ptr()


# --------------------------------------------------------------------------------------------------------------------- capacity
def test_85_benzenes_at_capacity():
    """510 atoms and 510 rows in one image of capacity 512: the rows past the workgroup's 256 threads, both atoms of every thread"""
    bonds = [q for k in range(85) for q in A.ring(A.K6, first=6 * k + 1)]
    images = [A.rows_of(["C"] * 510, bonds)]
    st = _check(_mol_op(images, 512, 512), images)
    assert [int(st[0][c]) for c in L.AROMATIC_COLUMNS] == [0, 510, 85, 85, 510, 0]


def test_a_hub_of_degree_511_is_no_candidate():
    """atom 1 is bonded to every other atom, six of which are a Kekule benzene: 517 rows, the hub's degree counted past its three
    slots, the benzene perceived beside it"""
    bonds = [(1, k, 1) for k in range(2, 513)] + A.ring(A.K6, first=100)
    images = [A.rows_of(["N"] + ["C"] * 511, bonds)]
    op = _mol_op(images, 512, 520)
    st = _check(op, images)
    assert [int(st[0][c]) for c in L.AROMATIC_COLUMNS] == [0, 6, 1, 1, 6, 0]
    assert op.codes()[0, 0] == L.AROM_NOT_CANDIDATE and op.codes()[0, 99:105].tolist() == [1] * 6


def test_empty_and_truncated_images():
    benzene, pyrrole = A.EXAMPLES[0][1], A.EXAMPLES[2][1]
    images = [None, ("truncated", pyrrole), benzene, None]
    st = _check(_mol_op(images, 8, 8), images)
    assert st["status"].tolist() == [EMPTY | TRUNCATED, TRUNCATED, 0, EMPTY | TRUNCATED] and st["listed"].tolist() == [0, 1, 0, 0]


def test_a_shorter_batch_after_a_longer_one_leaves_nothing_stale():
    long = _random(33, 4, n_min=28, n_max=32)
    short = [A.EXAMPLES[2][1], None, A.rows_of([], []), A.rows_of(["C", "C"], [(1, 2, 2)])]
    up = _upload(long, 32, 64)
    op = AromaticityPerceiver(*up, codes=True)
    _check(op, long)
    for dst, src in zip(up, _upload(short, 32, 64)):
        dst.copy_(src)
    op.run()                                                            # (no refill: what the long batch left must be overwritten)
    torch.cuda.synchronize()
    want = _expected(short, 32, 64)
    for got, exp in zip(op.rows().tensors + (op.stat, op.code), want):
        assert torch.equal(got.cpu(), torch.from_numpy(exp))


def test_captured_launch_replays_on_changed_inputs():
    batches = [_random(seed, 8, n_min=12, n_max=32) for seed in (34, 35, 36)]
    up = _upload(batches[0], 32, 64)
    op = AromaticityPerceiver(*up, codes=True)
    _check(op, batches[0])
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        op.run()
    for images in batches[1:]:
        for dst, src in zip(up, _upload(images, 32, 64)):
            dst.copy_(src)
        eager = _check(op, images)
        kept = [t.clone() for t in op.rows().tensors + (op.stat, op.code)]
        for t in op.rows().tensors + (op.stat, op.code):
            t.fill_(77)
        g.replay()
        torch.cuda.synchronize()
        for t, k in zip(op.rows().tensors + (op.stat, op.code), kept):
            assert torch.equal(t, k)
        assert eager["candidates"].sum() > 0


# ----------------------------------------------------------------------------------------------------------------------- guards
def test_refusals_launch_nothing():
    lib = L.load()
    images = [A.EXAMPLES[0][1]]
    op = _mol_op(images, 16, 16)
    _check(op, images)
    outs = op.rows().tensors + (op.stat, op.code)
    before = [t.clone() for t in outs]

    def refused(code, **fields):
        d = L.AromaticDesc()
        C.memmove(C.byref(d), C.byref(op.d), C.sizeof(d))
        for k, v in fields.items():
            setattr(d, k, v)
        assert lib.abc_perceive_aromatic(C.byref(d), torch.cuda.current_stream().cuda_stream) == code, fields
    einval, eunsupported = -1, -2                                       # ABC_EINVAL, ABC_EUNSUPPORTED
    assert lib.abc_perceive_aromatic(C.byref(L.AromaticDesc()), None) == einval      # (a zeroed descriptor)
    refused(eunsupported, cap_atoms=513)
    refused(einval, stats=None)
    refused(einval, out_atoms=op.d.mol_atoms)
    refused(einval, out_bonds=op.d.mol_bonds + 16)
    refused(einval, code_out=op.d.mol_counts)
    refused(einval, out_implh=op.d.out_atoms)
    refused(einval, out_implh=None)
    refused(einval, rec_counts=op.d.mol_counts)
    torch.cuda.synchronize()
    for t, b in zip(outs, before):
        assert torch.equal(t, b)
    with pytest.raises(ValueError, match="512"):
        AromaticityPerceiver(*_upload(images, 513, 16))
    with pytest.raises(L.AbcNetHipError):
        AromaticityPerceiver(*(t.long() for t in _upload(images, 16, 16)))
    with pytest.raises(L.AbcNetHipError, match="records"):
        op.records()
    with pytest.raises(L.AbcNetHipError, match="codes"):
        AromaticityPerceiver(*_upload(images, 16, 16)).codes()


# ------------------------------------------------------------------------------------------------------------------ end to end
def test_three_drawings_of_benzene_are_one_molecule():
    """Kekule benzene, its other Kekule form and order-4 benzene: through the perceiver one canonical string, c1ccccc1, and `same`
    against the order-4 record for all three.  Without the perceiver the strings differ and the two Kekule forms are `different`."""
    images = [A.rows_of(["C"] * 6, A.ring(A.K6)), A.rows_of(["C"] * 6, A.ring(A.K6[1:] + A.K6[:1])), A.rows_of(["C"] * 6, A.ring([4] * 6))]
    up = _upload(images, 8, 8)
    records = GraphRecords(3, 8, 8, DEV)
    records.load([A.as_record(images[2])] * 3)
    col = L.GRAPH_IDENT_COLUMNS.index("same")

    def answers(rows):
        canon = GraphCanonicalizer(rows)
        writer = SmilesWriter(canon.rows())
        ident = GraphIdentity(rows, records=records, max_atoms=8, max_bonds=8)
        for op in (canon, writer, ident):
            op.run()
        torch.cuda.synchronize()
        return writer.smiles(), ident.rows[:, col].cpu().tolist()
    op = AromaticityPerceiver(*up)
    op.run()
    assert answers(op.rows()) == (["c1ccccc1"] * 3, [1, 1, 1])
    texts, same = answers(abcnet_amd.contract.MoleculeRows(*up))        # the rows as they are listed: what the perceiver is for
    assert texts == ["C1C=CC=CC=1", "C1C=CC=CC=1", "c1ccccc1"] and same == [0, 0, 1]


def test_runner_perceives_before_the_canonical_smiles(golden_dir):
    """batch 4 at 96 x 96 (the size of the runner's other tests), the trained fixture: smiles() is
    m.aromatized().smiles(canonical=True) for the runner's own molecules, eager and replayed alike; molblocks() keeps its bytes;
    with the flag off nothing moves"""
    from abcnet_amd.infer import InferenceRunner
    from abcnet_amd.synthetic import drawn_molecules
    B, S = 4, 96
    m = trained_unet(golden_dir)
    plain = InferenceRunner(m, B, S, S, use_graph=True, assemble=True, smiles=True, molblocks=True, smiles_canonical=True)
    run = InferenceRunner(m, B, S, S, use_graph=True, assemble=True, smiles=True, molblocks=True, smiles_canonical=True, aromatize=True)
    assert plain.aromatizer is None and plain._stages == ["extractor", "assembler", "canonicalizer", "texter", "smiler"]
    assert plain.canonicalizer.d.mol_atoms == plain.assembler.rows.tensors[1].data_ptr()
    assert run._stages == ["extractor", "assembler", "aromatizer", "canonicalizer", "texter", "smiler"]
    assert run.canonicalizer.d.mol_atoms == run.aromatizer.rows().tensors[1].data_ptr() == run.aromatizer.d.out_atoms
    assert run.texter.d.mol_atoms == run.assembler.rows.tensors[1].data_ptr() == run.aromatizer.d.mol_atoms
    some = False
    for seed in (40, 40, 41):                                           # eager, capture + replay, replay of another batch
        x, _ = drawn_molecules(B, S, seed=seed)
        for r in (plain, run):
            r.load_batch(x.to(DEV))
            r.step()
        torch.cuda.synchronize()
        mols = run.molecules()
        assert run.smiles() == [None if mol is None else mol.aromatized().smiles(canonical=True) for mol in mols], seed
        assert plain.smiles() == [None if mol is None else mol.smiles(canonical=True) for mol in mols], seed
        assert run.molblocks() == plain.molblocks() == [None if mol is None else mol.molblock() for mol in mols]
        st = run.aromatic_stats()
        for b, mol in enumerate(mols):
            want = dict.fromkeys(L.AROMATIC_COLUMNS, 0) if mol is None else mol.aromatic_perception()[1]
            if mol is None:
                want["status"] = EMPTY
            assert {c: int(st[b][c]) & (~TRUNCATED if c == "status" and mol is None else -1) for c in L.AROMATIC_COLUMNS} == want, (seed, b)
        some |= any(mol is not None and len(mol.symbols) > 1 for mol in mols)
    assert run._graph is not None and some
    stereo = InferenceRunner(m, B, S, S, use_graph=False, assemble=True, smiles=True, smiles_stereo=True, aromatize=True)
    stereo.load_batch(x.to(DEV))
    stereo.step()
    torch.cuda.synchronize()
    assert stereo.smiles() == [None if mol is None else mol.aromatized().smiles(stereo=True) for mol in stereo.molecules()]
