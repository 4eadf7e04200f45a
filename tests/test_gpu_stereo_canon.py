"""The canonical ISOMERIC order on the device (csrc/graph_canon.hip's second instantiation, abc_canonical_order_stereo,
ops.GraphCanonicalizer(stereo=True), InferenceRunner(smiles_isomeric=True)) against the host form
decode.Molecule.canonical_order(isomeric=True) / .smiles(isomeric=True), on the families of tests/test_stereo_canon_host.py, which
holds that host form to an oracle independent of the search.  Integers and bytes: exact."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import abcnet_amd  # noqa: E402,F401
from abcnet_amd import _lib as L  # noqa: E402
from abcnet_amd import decode as D  # noqa: E402
from abcnet_amd.ops import GraphCanonicalizer, SmilesWriter  # noqa: E402
import smiles_stereo_cases as ST  # noqa: E402
from molrows import trained_unet  # noqa: E402
from test_gpu_stereo_perceive import ONE_ATOM, expected, upload, with_status  # noqa: E402
from test_stereo_canon_host import FAMILIES, butane, molecule  # noqa: E402

DEV = "cuda"
CAP = 32
IMAGES = [im for fam in FAMILIES for im in fam]
BATCHES = [IMAGES[k:k + 16] for k in range(0, len(IMAGES), 16)]


def _signed(v):
    return v - (1 << 64) if v >> 63 else v


def host(images, cap=CAP):
    """order, stats, key, stereo_search and the canonical rows of every image by the host form, as the device lays them out"""
    B = len(images)
    order = np.full((B, cap), -1, dtype=np.int32)
    stats = np.zeros((B, len(L.CANON_COLUMNS)), dtype=np.int32)
    key = np.zeros((B, 2), dtype=np.int64)
    search = np.zeros((B, 4), dtype=np.int32)
    rows, texts = [], []
    for b, im in enumerate(images):
        m = molecule(im)
        rank, st, k, s = m.canonical_order(isomeric=True)
        for a, r in enumerate(rank):
            order[b, r] = a
        stats[b] = [st[c] for c in L.CANON_COLUMNS]
        key[b] = [_signed(k[0]), _signed(k[1])]
        search[b] = s
        mc = m.canonical(isomeric=True)
        rows.append(([(p[0], p[1], D.ATOM_SYMBOLS.index(x, 1), c, h) for p, x, c, h in zip(mc.positions, mc.symbols, mc.charges, mc.hs)],
                     [(e1, e2, o, src) for (e1, e2), o, src in zip(mc.bonds, mc.orders, mc.sources)], mc.implicit_hs, 0))
        texts.append(m.smiles(isomeric=True))
    return order, stats, key, search, rows, texts


def check(images, cap=CAP):
    up = upload([with_status(im) for im in images], cap, cap)
    plain = GraphCanonicalizer(*up)
    plain.run()
    torch.cuda.synchronize()
    before = [t.clone() for t in (plain.order, plain.stat, plain.key) + plain.out.tensors]
    op = GraphCanonicalizer(*up, stereo=True)
    for t in (op.order, op.stat, op.key, op.search) + op.out.tensors:
        t.fill_(77)
    op.run()
    w = SmilesWriter(op.rows(), stereo=True, double_bonds=True)
    w.run()
    torch.cuda.synchronize()
    order, stats, key, search, rows, texts = host(images, cap)
    assert torch.equal(op.order.cpu(), torch.from_numpy(order))
    assert torch.equal(op.stat.cpu(), torch.from_numpy(stats))
    assert torch.equal(op.key.cpu(), torch.from_numpy(key))
    assert torch.equal(op.search.cpu(), torch.from_numpy(search))
    assert [tuple(r) for r in op.stereo_search().tolist()] == [tuple(r) for r in search.tolist()]
    want = upload(rows, cap, cap)
    got = op.rows().tensors
    n_atoms, n_bonds, n_listed = (up[0][:, k].tolist() for k in range(3))
    assert torch.equal(got[0], up[0])
    for b in range(len(images)):      # (past the counts the device writes zeros, the upload junk)
        assert torch.equal(got[1][b, :n_atoms[b]], want[1][b, :n_atoms[b]]) and not got[1][b, n_atoms[b]:].any()
        assert torch.equal(got[2][b, :n_bonds[b]], want[2][b, :n_bonds[b]]) and not got[2][b, n_bonds[b]:].any()
        assert torch.equal(got[3][b, :n_listed[b]], want[3][b, :n_listed[b]]) and not got[3][b, n_listed[b]:].any()
    assert w.smiles() == texts
    # the plain canonicaliser of the same rows: untouched by the stereo one, and bit-identical when run again
    for t, was in zip((plain.order, plain.stat, plain.key) + plain.out.tensors, before):
        assert torch.equal(t, was)
    plain.run()
    torch.cuda.synchronize()
    for t, was in zip((plain.order, plain.stat, plain.key) + plain.out.tensors, before):
        assert torch.equal(t, was)
    assert torch.equal(op.key, plain.key)      # all leaves of equal h relabel to one graph
    return op, texts


def test_canonical_order_stereo_is_exported_and_separates_enantiomers():
    """fails on the parent: the library has no abc_canonical_order_stereo"""
    assert hasattr(L.load(), "abc_canonical_order_stereo")
    rng = np.random.default_rng(3)
    images = [ST.worked(5), ST.worked(6), ST.renumbered(ST.worked(5), rng)[0], ST.moved(ST.worked(5), ST.mirror), butane(5, 5), butane(6, 6),
              butane(5, 6), butane(6, 5), ONE_ATOM]
    op, texts = check(images)
    assert texts[0] == texts[2] and texts[1] == texts[3] and texts[0] != texts[1]
    assert texts[4] == texts[5] and len({texts[4], texts[6], texts[7]}) == 3
    assert op.stereo_elements().shape == (len(images), CAP, L.STEREO_W)


@pytest.mark.parametrize("k", range(len(BATCHES)))
def test_families_equal_the_host_form(k):
    check(BATCHES[k])


def test_a_second_run_overwrites_every_word_and_is_capturable():
    first, second = BATCHES[0][:8], BATCHES[-2][:7] + [ONE_ATOM]
    up = upload([with_status(im) for im in first], CAP, CAP)
    op = GraphCanonicalizer(*up, stereo=True)
    w = SmilesWriter(op.rows(), stereo=True, double_bonds=True)
    op.run()
    w.run()
    torch.cuda.synchronize()
    assert w.smiles() == host(first)[5]
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, capture_error_mode="thread_local"):
        op.run()
        w.run()
    for dst, src in zip(up, upload([with_status(im) for im in second], CAP, CAP)):
        dst.copy_(src)
    for t in (op.order, op.stat, op.key, op.search, op.perceiver.table, op.perceiver.stat):
        t.fill_(77)
    g.replay()
    torch.cuda.synchronize()
    order, stats, key, search, _, texts = host(second)
    assert torch.equal(op.order.cpu(), torch.from_numpy(order)) and torch.equal(op.stat.cpu(), torch.from_numpy(stats))
    assert torch.equal(op.key.cpu(), torch.from_numpy(key)) and torch.equal(op.search.cpu(), torch.from_numpy(search))
    assert w.smiles() == texts
    table, table_stats = expected([with_status(im) for im in second], CAP)
    assert torch.equal(op.stereo_elements(), table) and torch.equal(op.perceiver.stat.cpu(), table_stats)


def test_refusals():
    from abcnet_amd.contract import GraphRecords
    lib = L.load()
    up = upload([with_status(ST.worked(5))], 16, 16)
    op = GraphCanonicalizer(*up, stereo=True)
    op.run()
    torch.cuda.synchronize()
    before = [t.clone() for t in (op.order, op.stat, op.key, op.search)]

    def refused(code, **fields):
        d = L.CanonStereoDesc()
        C.memmove(C.byref(d), C.byref(op.d), C.sizeof(d))
        for k, v in fields.items():
            setattr(d, k, v)
        assert lib.abc_canonical_order_stereo(C.byref(d), torch.cuda.current_stream().cuda_stream) == code, fields

    einval, eunsupported = -1, -2
    assert lib.abc_canonical_order_stereo(C.byref(L.CanonStereoDesc()), None) == einval
    refused(einval, elements=None)
    refused(einval, stereo_search=None)
    refused(einval, rec_counts=op.d.mol_counts)                                      # both sides
    refused(einval, mol_counts=None, rec_counts=op.d.mol_counts, rec_atoms=op.d.mol_atoms, rec_bonds=op.d.mol_bonds, max_atoms=16, max_bonds=16)
    refused(einval, stereo_search=op.d.elements)
    refused(einval, order=op.d.elements)
    refused(eunsupported, cap_atoms=513)
    torch.cuda.synchronize()
    for t, was in zip((op.order, op.stat, op.key, op.search), before):
        assert torch.equal(t, was)
    with pytest.raises(ValueError, match="molecule side"):
        GraphCanonicalizer(records=GraphRecords(1, 16, 16, torch.device(DEV)), stereo=True)
    with pytest.raises(L.AbcNetHipError, match="stereo=True"):
        GraphCanonicalizer(*up).stereo_search()


def test_runner_writes_isomeric_smiles(golden_dir):
    """batch 4 at 96 x 96, the trained fixture the canonical GPU tests use: smiles() is m.smiles(isomeric=True) of the runner's own
    molecules, eager and replayed alike, with aromatize=True as well; the runner without the flag has the bytes it had"""
    from abcnet_amd.infer import InferenceRunner
    from abcnet_amd.synthetic import drawn_molecules
    B, S = 4, 96
    m = trained_unet(golden_dir)
    plain = InferenceRunner(m, B, S, S, use_graph=True, assemble=True, smiles=True, smiles_canonical=True)
    run = InferenceRunner(m, B, S, S, use_graph=True, assemble=True, smiles=True, smiles_isomeric=True)
    arom = InferenceRunner(m, B, S, S, use_graph=True, assemble=True, smiles=True, smiles_isomeric=True, aromatize=True)
    assert run._stages == ["extractor", "assembler", "canonicalizer", "smiler"] and run.canonicalizer.stereo and not plain.canonicalizer.stereo
    assert arom._stages == ["extractor", "assembler", "aromatizer", "canonicalizer", "smiler"]
    assert run.smiler.stereo and run.smiler.double_bonds and run.smiler.d.mol_atoms == run.canonicalizer.rows().tensors[1].data_ptr()
    some = False
    for seed in (40, 40, 41):                                       # eager, capture + replay, replay of another batch
        x, _ = drawn_molecules(B, S, seed=seed)
        for r in (plain, run, arom):
            r.load_batch(x.to(DEV))
            r.step()
        torch.cuda.synchronize()
        mols = run.molecules()
        assert run.smiles() == [None if mol is None else mol.smiles(isomeric=True) for mol in mols], seed
        assert arom.smiles() == [None if mol is None else mol.smiles(isomeric=True, aromatize=True) for mol in mols], seed
        assert plain.smiles() == [None if mol is None else mol.smiles(canonical=True) for mol in mols], seed
        st = run.canonical_stats()
        assert [int(s) for s in st["status"]] == [L.CANON_EMPTY if mol is None else (L.CANON_TRUNCATED if mol.truncated else 0) for mol in mols]
        assert torch.equal(run.canonical_keys(), plain.canonical_keys())
        search = run.stereo_search()
        assert [tuple(r) for r in search.tolist()] == [(0, 0, 0, 0) if mol is None else tuple(mol.canonical_order(isomeric=True)[3]) for mol in mols]
        some |= any(mol is not None and len(mol.symbols) > 1 for mol in mols)
    assert run._graph is not None and some
    with pytest.raises(L.AbcNetHipError, match="smiles_isomeric"):
        plain.stereo_search()
