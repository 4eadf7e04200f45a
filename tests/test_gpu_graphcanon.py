"""The canonical atom order on the device (csrc/graph_canon.hip, ops.GraphCanonicalizer, InferenceRunner(smiles_canonical=True))
against the oracle (tests/graphcanon_oracle.py; the search is decode.canonical_labelling, held to brute force and to networkx in
tests/test_graphcanon_host.py): order, stats, key, certificate and the canonical rows are compared with torch.equal -- the chosen leaf,
every work counter and every word of the relabelled graph.

Measured on an MI355X (device events around one launch of B = 1, test_the_worst_cases_at_capacity prints them): the ring of 512 carbons
5.27 ms (5 tries, 1483 rounds), the chain of 512 carbons 3.43 ms (2 tries, 1008 rounds), 170 disjoint C-C-C 32.6 ms (UNDECIDED: the
16384 rounds of the default budget, 32 leaves).  The whole file takes 6 s."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import abcnet_amd  # noqa: E402,F401
from abcnet_amd import _lib as L  # noqa: E402
from abcnet_amd.contract import GraphRecords  # noqa: E402
from abcnet_amd.ops import GraphCanonicalizer, GraphIdentity, SmilesWriter  # noqa: E402
import graphcanon_oracle as co  # noqa: E402
import graphident_oracle as io  # noqa: E402
import graphsim_oracle as so  # noqa: E402
from molrows import records_to_numpy, trained_unet, upload_molecules  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
COL = {c: i for i, c in enumerate(co.COLUMNS)}


def _upload(mols, cap_atoms, cap_mol_bonds):
    """molrows.upload_molecules plus the implicit-H list of mol["implh"] (junk 5 past the count, which would name an atom)"""
    cnt, atoms, bonds = upload_molecules(mols, cap_atoms, cap_mol_bonds, junk_bond=(1, 2, 3, 0))
    implh = np.full((len(mols), cap_atoms), 5, dtype=np.int32)
    for b, m in enumerate(mols):
        listed = [] if m is None else list(m.get("implh", ()))
        implh[b, :len(listed)] = listed
        cnt[b, 2] = len(listed)
    return cnt, atoms, bonds, torch.from_numpy(implh).to(DEV)


def _mol_op(mols, cap_atoms=64, cap_mol_bonds=96, **kw):
    return GraphCanonicalizer(*_upload(mols, cap_atoms, cap_mol_bonds), cert=True, **kw)


def _norm(rec):
    """the record with the lower atom of every row first, as GraphRecords.load wants it (raster.parse_graph writes it so)"""
    return rec[0], [(min(i, j), max(i, j), o) for i, j, o in rec[1]]


def _rec_op(recs, max_atoms=64, max_bonds=96, **kw):
    records = GraphRecords(len(recs), max_atoms, max_bonds, DEV)
    records.load(records_to_numpy(recs))
    return GraphCanonicalizer.from_records(records, cert=True, **kw)


def _check(op, images, mols=None, **budgets):
    """one launch over pre-filled outputs: order, stats, key and cert equal the oracle's; with `mols`, the canonical rows too"""
    want = co.outputs(images, op.cap, op.cap_bonds, **budgets)
    for t in (op.order, op.stat, op.key, op.cert) + (op.out.tensors if op.out is not None else ()):
        t.fill_(77)                                                    # (every word is written by every launch)
    op.run()
    torch.cuda.synchronize()
    rows = [dict(zip(co.COLUMNS, r)) for r in op.stat.cpu().tolist()]
    for name, got, exp in zip(("stats", "order", "key", "cert"), (op.stat, op.order, op.key, op.cert), (want[1], want[0], want[2], want[3])):
        bad = (got.cpu() != torch.from_numpy(exp)).flatten(1).any(1).nonzero().flatten().tolist()
        assert not bad, (name, bad[:8], [rows[b] for b in bad[:4]], [dict(zip(co.COLUMNS, want[1][b].tolist())) for b in bad[:4]])
    if mols is not None:
        exp = [co.canonical_rows(m, op.cap, op.cap_bonds, **budgets) for m in mols]
        for k, name in enumerate(("mol_counts", "mol_atoms", "mol_bonds", "mol_implh")):
            assert torch.equal(op.rows().tensors[k].cpu(), torch.from_numpy(np.stack([e[k] for e in exp]))), name
    return rows


def _pairs():
    pairs = list(io.random_pairs(256, seed=11))
    return [m for m, _ in pairs], [r for _, r in pairs]


# ------------------------------------------------------------------------------------------------------------- random graphs
def test_random_graphs_equal_the_oracle_in_one_launch():
    """the first 256 of the identity suite's pairs, B = 256, cap_atoms = cap_mol_bonds = 16: the molecules on the molecule side (every
    fourth with a listed atom), the records on the records side"""
    mols, recs = _pairs()
    mols = [dict(m, implh=[1 + b % len(m["atoms"])]) if b % 4 == 0 else m for b, m in enumerate(mols)]
    rows = _check(_mol_op(mols, 16, 16), [co.molecule_image(m) for m in mols], mols)
    assert not any(r["status"] for r in rows) and sum(r["automorphisms"] > 0 for r in rows) >= 1
    rows = _check(_rec_op(recs, 16, 16), [co.record_image(r) for r in recs])
    assert not any(r["status"] for r in rows)


def test_certificates_agree_with_the_identity():
    """on the 256 pairs the molecule's certificate equals the record's exactly where GraphIdentity says `same`"""
    mols, recs = _pairs()
    up = _upload(mols, 16, 16)
    records = GraphRecords(len(recs), 16, 16, DEV)
    records.load(records_to_numpy(recs))
    cm, cr = GraphCanonicalizer(*up[:3], cert=True, rows=False), GraphCanonicalizer.from_records(records, cert=True)
    ident = GraphIdentity(*up[:3], records=records)
    for op in (cm, cr, ident):
        op.run()
    torch.cuda.synchronize()
    same = ident.rows.cpu()[:, L.GRAPH_IDENT_COLUMNS.index("same")].bool()
    equal = (cm.certificates() == cr.certificates()).all(1)
    assert torch.equal(equal, same) and 100 <= int(same.sum()) <= 200
    assert torch.equal((cm.keys() == cr.keys()).all(1) | ~same, torch.ones_like(same))      # (equal graphs: equal keys)


# ------------------------------------------------------------------------------------------------------------ hand-made rows
def test_hand_made_rows_equal_the_oracle():
    """the identity test's rows -- ends out of range, a loop, int32 extremes, a vocabulary index of -(1 << 31), an unknown class, a
    pair listed twice, an EMPTY image, a TRUNCATED one, zero atoms without EMPTY -- and n = 1, n = 2; both sides"""
    from test_gpu_graphident import _cases
    cases = _cases()
    mols = [m for _, m, _ in cases] + [so.mol([6], []), so.mol([7, 6], [(2, 1, 1)]), so.mol([6, 6, 2], [(1, 2, 1), (2, 3, 1)]) | dict(implh=[3, 0, 99, 1, 3])]
    names = [name for name, _, _ in cases] + ["n = 1", "n = 2", "listed atoms and junk entries"]
    rows = dict(zip(names, _check(_mol_op(mols), [co.molecule_image(m) for m in mols], mols)))
    assert rows["no molecule"] == dict(dict.fromkeys(co.COLUMNS, 0), status=co.EMPTY | co.TRUNCATED)
    assert rows["truncated"]["status"] == co.TRUNCATED and rows["nothing on either side"] == dict.fromkeys(co.COLUMNS, 0)
    assert rows["n = 1"]["leaves"] == 1 and rows["n = 1"]["tries"] == 0 and rows["n = 2"]["leaves"] == 1
    assert all(r["status"] & ~co.TRUNCATED == 0 or name == "no molecule" for name, r in rows.items())
    recs = [r for _, _, r in cases]
    _check(_rec_op(recs), [co.record_image(r) for r in recs])


def test_record_rows_may_hold_any_int32():
    """load() refuses such records; hand-made device rows may hold them, and junk past the counts"""
    rec = so.record([1, 2, 3, 6, 7], [(0, 1, 1), (1, 2, 2), (2, 3, 4)])
    bad = [(0, 5, 1), (2, 2, 1), (-1, 1, 1), (1 << 30, 0, 1), (3, -(1 << 31), 1), (3, 1, 9)]      # the last one is valid, ends swapped
    op = _rec_op([rec, rec], 8, 16)
    torch.cuda.synchronize()
    d_atoms, d_bonds, d_cnt = op.records.staging.dev.values()
    d_atoms.fill_(11)
    d_bonds[:] = torch.tensor([0, 4, 1], dtype=torch.int32, device=DEV)
    for b in range(2):
        d_atoms[b, :5] = torch.tensor(rec[0], dtype=torch.int32, device=DEV)
    d_bonds[0, :3] = torch.tensor(rec[1], dtype=torch.int32, device=DEV)
    d_bonds[1, :9] = torch.tensor(bad[:3] + rec[1] + bad[3:], dtype=torch.int32, device=DEV)
    d_cnt.copy_(torch.tensor([[5, 5], [3, 9]], dtype=torch.int32, device=DEV))
    _check(op, [co.record_image(rec), co.record_image((rec[0], bad[:3] + rec[1] + bad[3:]))])
    d_cnt.copy_(torch.tensor([[5, 1 << 30], [3, -7]], dtype=torch.int32, device=DEV))         # counts past the capacities are clamped
    _check(op, [co.record_image(rec), co.record_image((d_atoms[1].cpu().numpy(), np.zeros((0, 3), np.int32)))])


# ----------------------------------------------------------------------------------------------------------------- symmetry
SYMMETRIC = [("benzene", co.BENZENE), ("cubane", co.CUBANE), ("petersen", co.PETERSEN), ("hub", co.HUB), ("two benzenes", co.benzenes(2)),
             ("union", co.UNION)]


def test_symmetric_graphs_equal_the_oracle():
    rng = np.random.RandomState(4)
    recs = [_norm(r) for _, r in SYMMETRIC] + [_norm(so.permuted(rng, r)) for _, r in SYMMETRIC]
    mols = [so.as_mol(r) for r in recs]
    rows = _check(_mol_op(mols), [co.molecule_image(m) for m in mols], mols)
    assert rows[0]["leaves"] <= 4 and rows[0]["pruned_orbit"] >= 1 and all(r["automorphisms"] >= 1 and not r["status"] for r in rows)
    assert rows[3]["levels_max"] == 36 and rows[3]["tries"] > 1000      # the hub: orbits of ten spokes, far below the orbit levels
    op = _rec_op(recs)
    _check(op, [co.record_image(r) for r in recs])
    cert = op.certificates()
    assert torch.equal(cert[:6], cert[6:])                            # a renumbered copy: the same relabelled graph


def _check_stereo(mols, cap_atoms=64, cap_mol_bonds=96, **budgets):
    """abc_canonical_order_stereo on molecules without a stereo element: the element table is all none, order, stats, key, certificate
    and rows are those of the plain search (_check) and the stereo_search row is the host form's; returns (rows, stereo_search rows)"""
    from abcnet_amd import decode as D
    op = GraphCanonicalizer(*_upload(mols, cap_atoms, cap_mol_bonds), cert=True, stereo=True, **budgets)
    op.search.fill_(77)
    rows = _check(op, [co.molecule_image(m) for m in mols], mols, **budgets)
    table = op.stereo_elements()
    for b, m in enumerate(mols):
        assert table[b, :len(m["atoms"])].tolist() == [list(D.STEREO_NONE_ROW)] * len(m["atoms"]), b
    search = op.search.cpu().tolist()
    tries, rounds = budgets.get("max_tries", D.CANON_DEFAULT_TRIES), budgets.get("max_rounds", D.CANON_DEFAULT_ROUNDS)
    assert search == [D.canonical_labelling(co.of_molecule(m), tries, rounds, stereo=[D.STEREO_NONE_ROW] * len(m["atoms"]))[3] for m in mols]
    return rows, search


# a budget that runs out AFTER a best leaf exists, inside a replay or a later level: the order written is the best leaf so far
LATE = [(dict(max_tries=3), 8, dict(leaves=2, tries=3, rounds=17, automorphisms=1)), (dict(max_rounds=12), 6, dict(leaves=2, rounds=12))]


@pytest.mark.parametrize("budgets, ring, want", [(dict(max_tries=1), 0, dict(leaves=0)), (dict(max_rounds=1), 0, dict(leaves=0))] + LATE,
                         ids=["budgets0", "budgets1", "budgets2", "budgets3"])      # (the ids the first two cases have always had)
def test_tiny_budgets_end_undecided(budgets, ring, want):
    """benzene (ring 0), or under a LATE budget its ring of carbons, beside a pair that needs one round and no try: a budget is an
    image's own, and the order is the oracle's -- the identity order before any leaf, the best leaf so far after one (those on both
    sides)"""
    first = co.BENZENE if ring == 0 else _norm(io.carbon_ring(ring))
    recs = [first, so.record([1, 2], [(0, 1, 1)])]
    mols = [so.as_mol(first), so.mol([1, 2], [(1, 2, 1)])]
    sides = [_check(_mol_op(mols, **budgets), [co.molecule_image(m) for m in mols], mols, **budgets)]
    if ring:
        sides.append(_check(_rec_op(recs, **budgets), [co.record_image(r) for r in recs], **budgets))
    for rows in sides:
        assert rows[0]["status"] == co.UNDECIDED and {k: rows[0][k] for k in want} == want
        assert rows[1]["status"] == 0 and rows[1]["leaves"] == 1 and rows[1]["rounds"] == 1


@pytest.mark.parametrize("budgets, ring, want", LATE)
def test_late_budgets_end_undecided_in_the_stereo_search(budgets, ring, want):
    """the same two rings through abc_canonical_order_stereo with an element table that is all none, each beside the image that
    finishes: the plain search's answer, and the one automorphism is a stereo automorphism"""
    mols = [so.as_mol(_norm(io.carbon_ring(ring))), so.mol([1, 2], [(1, 2, 1)])]
    rows, search = _check_stereo(mols, **budgets)
    assert rows[0]["status"] == co.UNDECIDED and {k: rows[0][k] for k in want} == want and search[0] == [0, 0, 1, 0]
    assert rows[1]["status"] == 0 and rows[1]["leaves"] == 1 and rows[1]["rounds"] == 1 and search[1] == [0, 0, 0, 0]


@pytest.mark.parametrize("name, rec", [("ring", io.carbon_ring(512)), ("chain", io.carbon_chain(512)), ("propanes", io.propanes(170))])
def test_the_worst_cases_at_capacity(name, rec):
    """512 atoms, every atom like every other, under the default budgets: compared with the oracle whichever way they come out (the
    ring and the chain are decided; 170 disjoint C-C-C run out of rounds); one launch of B = 1 each, its device time printed"""
    rec = _norm(so.permuted(np.random.RandomState(5), rec))
    op = _rec_op([rec], 512, 512)
    rows = _check(op, [co.record_image(rec)])
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    op.run()
    e1.record()
    torch.cuda.synchronize()
    print(name, rows[0], "%.2f ms" % e0.elapsed_time(e1))
    assert (rows[0]["status"] == 0) == (name != "propanes") and rows[0]["rounds"] >= 900


def test_more_molecule_rows_than_threads():
    """a ring of 257 carbons on the MOLECULE side: 257 bond rows, the smallest number at which the round's loop over the molecule rows
    past the workgroup's 256 threads runs (the other molecule-side cases stay below it, the 512-atom cases are records)"""
    mol = so.as_mol(_norm(so.permuted(np.random.RandomState(5), io.carbon_ring(257))))
    op = _mol_op([mol], 512, 512)
    rows = _check(op, [co.molecule_image(mol)], [mol])
    assert rows[0]["status"] == 0 and rows[0]["leaves"] == 3 and rows[0]["tries"] == 5 and rows[0]["rounds"] == 700
    assert op.rows().tensors[0].cpu().tolist() == [[257, 257, 0, 0]]
    # the same rows through the stereo entry, the element table all none: the same order, key and stats
    rows, search = _check_stereo([mol], 512, 512)
    assert rows[0]["status"] == 0 and rows[0]["leaves"] == 3 and rows[0]["tries"] == 5 and rows[0]["rounds"] == 700
    assert search == [[0, 0, 2, 0]]


# --------------------------------------------------------------------------------------------------------- renumbered uploads
def _renumbered(rng, rec):
    """the same graph with its atoms renumbered and its bond rows in another order; every row keeps its orientation"""
    atoms, bonds = rec
    perm = rng.permutation(len(atoms))                  # old index -> new index
    new_atoms = [None] * len(atoms)
    for old, new in enumerate(perm):
        new_atoms[new] = atoms[old]
    return new_atoms, [(int(perm[bonds[k][0]]), int(perm[bonds[k][1]]), bonds[k][2]) for k in rng.permutation(len(bonds))]


def test_renumbered_uploads_give_the_same_rows_and_text():
    """two numberings of the same molecules: the canonical rows are equal word for word (positions apart: every atom sits at (0, 0)
    here), and SmilesWriter on them packs the same bytes"""
    rng = np.random.RandomState(8)
    recs = [so.random_graph(rng, int(rng.randint(2, 25)), extra=int(rng.randint(0, 4))) for _ in range(40)] + [r for _, r in SYMMETRIC]
    # (the text rule takes one row per pair, classes it knows and small charges)
    recs = [([(x, y, 1 if t < 0 else t, c) for x, y, t, c in a], list({(min(i, j), max(i, j)): (i, j, o) for i, j, o in q}.values())) for a, q in recs]
    ops, texts = [], []
    for k in range(2):
        mols = [so.as_mol(_renumbered(rng, r)) if k else so.as_mol(r) for r in recs]
        op = _mol_op(mols)
        _check(op, [co.molecule_image(m) for m in mols], mols)
        w = SmilesWriter(op.rows())
        w.run()
        torch.cuda.synchronize()
        ops.append(op)
        texts.append((w.text.cpu(), w.index.cpu(), w.smiles()))
    # counts, atoms and the implicit-H list word for word; the bond rows in the same places with the same atoms and order -- the source
    # column is the original row, and WHICH end is end 1 belongs to the drawing (end 1 stays end 1, the wedge's owner: between two atoms
    # an automorphism swaps the row may stand either way; a wedge code is the drawing's too: the graph holds its order class)
    for k in (0, 1, 3):
        assert torch.equal(ops[0].rows().tensors[k], ops[1].rows().tensors[k])
    a, b = ops[0].rows().tensors[2].cpu(), ops[1].rows().tensors[2].cpu()
    fold = lambda o: torch.where(o >= 5, torch.ones_like(o), o)
    assert torch.equal(a[..., :2].sort(-1).values, b[..., :2].sort(-1).values) and torch.equal(fold(a[..., 2]), fold(b[..., 2]))
    assert torch.equal(ops[0].certificates(), ops[1].certificates())
    assert torch.equal(texts[0][0], texts[1][0]) and torch.equal(texts[0][1], texts[1][1]) and texts[0][2] == texts[1][2]
    assert len(set(texts[0][2])) == len({tuple(c) for c in ops[0].certificates().tolist()})      # equal strings iff equal graphs


def test_a_shorter_batch_after_a_longer_one_leaves_nothing_stale():
    rng = np.random.RandomState(9)
    long = [so.as_mol(so.random_graph(rng, 20, extra=3)) for _ in range(4)]
    short = [so.as_mol(so.random_graph(rng, 3, extra=0)), None, so.mol([], []), so.as_mol(so.random_graph(rng, 2, extra=0))]
    up = _upload(long, 32, 32)
    op = GraphCanonicalizer(*up, cert=True)
    _check(op, [co.molecule_image(m) for m in long], long)
    for dst, src in zip(up, _upload(short, 32, 32)):
        dst.copy_(src)
    for t in (op.order, op.stat, op.key, op.cert) + op.out.tensors:
        t.fill_(77)
    op.run()
    torch.cuda.synchronize()
    want = co.outputs([co.molecule_image(m) for m in short], 32, 32)
    for got, exp in zip((op.order, op.stat, op.key, op.cert), want):
        assert torch.equal(got.cpu(), torch.from_numpy(exp))
    exp = [co.canonical_rows(m, 32, 32) for m in short]
    for k in range(4):
        assert torch.equal(op.rows().tensors[k].cpu(), torch.from_numpy(np.stack([e[k] for e in exp])))


# ------------------------------------------------------------------------------------------------------------------- guards
def test_refusals_launch_nothing():
    lib = L.load()
    mols = [so.as_mol(co.BENZENE)]
    op = _mol_op(mols, 16, 16)
    _check(op, [co.molecule_image(m) for m in mols], mols)
    before = [t.clone() for t in (op.order, op.stat, op.key, op.cert) + op.out.tensors]

    def refused(code, **fields):
        d = L.CanonDesc()
        C.memmove(C.byref(d), C.byref(op.d), C.sizeof(d))
        for k, v in fields.items():
            setattr(d, k, v)
        assert lib.abc_canonical_order(C.byref(d), torch.cuda.current_stream().cuda_stream) == code, fields
    einval, eunsupported = -1, -2                                       # ABC_EINVAL, ABC_EUNSUPPORTED
    codes = {lib.abc_canonical_order(C.byref(L.CanonDesc()), None)}                    # (a zeroed descriptor: ABC_EINVAL)
    assert codes == {einval}
    refused(eunsupported, cap_atoms=513)
    refused(eunsupported, cap_mol_bonds=4097)
    refused(einval, stats=None)
    refused(einval, out_atoms=op.d.mol_atoms)
    refused(einval, out_bonds=op.d.mol_bonds + 16)
    refused(einval, order=op.d.mol_counts)
    refused(einval, out_implh=None)
    refused(einval, rec_counts=op.d.mol_counts)
    refused(einval, max_tries=-1)
    torch.cuda.synchronize()
    for t, b in zip((op.order, op.stat, op.key, op.cert) + op.out.tensors, before):
        assert torch.equal(t, b)
    with pytest.raises(ValueError, match="512"):
        GraphCanonicalizer(*_upload(mols, 513, 16))
    with pytest.raises(ValueError, match="4096"):
        GraphCanonicalizer(*_upload(mols, 16, 4097))
    GraphCanonicalizer(*_upload(mols, 16, 4097), rows=False)
    with pytest.raises(ValueError, match="one side"):
        GraphCanonicalizer()
    with pytest.raises(L.AbcNetHipError):
        GraphCanonicalizer(*(t.long() for t in _upload(mols, 16, 16)))
    with pytest.raises(L.AbcNetHipError, match="rows"):
        _rec_op([_norm(co.BENZENE)]).rows()


# ------------------------------------------------------------------------------------------------------------------ the runner
def test_runner_writes_canonical_smiles(golden_dir):
    """batch 4 at 96 x 96 (the size of the runner's other tests), the trained fixture: smiles() is m.smiles(canonical=True) for the
    runner's own molecules, eager and replayed from the captured graph alike; the flag adds one launch and moves nothing else"""
    from abcnet_amd.infer import InferenceRunner
    from abcnet_amd.synthetic import drawn_molecules
    from molrows import Heads
    B, S = 4, 96
    m = trained_unet(golden_dir)
    plain = InferenceRunner(m, B, S, S, use_graph=True, assemble=True, smiles=True, molblocks=True)
    run = InferenceRunner(m, B, S, S, use_graph=True, assemble=True, smiles=True, molblocks=True, smiles_canonical=True)
    assert plain.canonicalizer is None and "canonicalizer" not in plain._stages
    assert run._stages == ["extractor", "assembler", "canonicalizer", "texter", "smiler"]
    assert run.smiler.d.mol_atoms == run.canonicalizer.rows().tensors[1].data_ptr() and run.texter.d.mol_atoms == run.assembler.rows.tensors[1].data_ptr()
    texts, some = [], False
    for seed in (40, 40, 40, 41):                                       # eager, capture + replay, replay again, replay of another batch
        x, _ = drawn_molecules(B, S, seed=seed)
        for r in (plain, run):
            r.load_batch(x.to(DEV))
            r.step()
        torch.cuda.synchronize()
        mols = run.molecules()
        got = run.smiles()
        assert got == [None if mol is None else mol.smiles(canonical=True) for mol in mols], seed
        assert run.molblocks() == plain.molblocks() and plain.smiles() == [None if mol is None else mol.smiles() for mol in mols]
        st = run.canonical_stats()
        assert [int(s) for s in st["status"]] == [L.CANON_EMPTY if mol is None else (L.CANON_TRUNCATED if mol.truncated else 0) for mol in mols]
        keys = run.canonical_keys()
        assert keys.shape == (B, 2) and all(tuple(keys[b].tolist()) == tuple(co._signed(k) for k in mol.canonical_order()[2])
                                            for b, mol in enumerate(mols) if mol is not None)
        some |= any(mol is not None and len(mol.symbols) > 1 for mol in mols)
        texts.append((run.smiler.text.cpu().clone(), run.smiler.index.cpu().clone()))
    assert run._graph is not None and some
    assert torch.equal(texts[1][0], texts[2][0]) and torch.equal(texts[1][1], texts[2][1])       # replayed twice: the same bytes
    assert torch.equal(texts[0][0], texts[1][0]) and torch.equal(texts[0][1], texts[1][1])       # eager and replayed: the same bytes
    for kw in (dict(smiles_stereo=True, smiles=True), dict(smiles=False)):
        with pytest.raises(ValueError, match="smiles_canonical"):
            InferenceRunner(Heads(), B, S, S, assemble=True, smiles_canonical=True, **kw)
