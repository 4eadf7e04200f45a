"""The environment similarity on the device (csrc/graph_sim.hip, ops.GraphSimilarity, InferenceRunner(score_similarity=True))
against the oracle (tests/graphsim_oracle.py).  Every comparison is integer-exact, and the fingerprint ids themselves (ids_out) are
compared bit for bit."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import abcnet_amd  # noqa: E402,F401
from abcnet_amd import _lib as L  # noqa: E402
from abcnet_amd.contract import GraphRecords  # noqa: E402
from abcnet_amd.ops import GraphScore, GraphSimilarity  # noqa: E402
from abcnet_amd.raster import parse_graph  # noqa: E402
from abcnet_amd.synthetic import drawn_molecules  # noqa: E402
import graphsim_oracle as so  # noqa: E402
from molrows import for_score_oracle, records_to_numpy, trained_unet, upload_molecules  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
COL = {c: i for i, c in enumerate(so.COLUMNS)}


def _upload(mols, cap_atoms, cap_mol_bonds):
    return upload_molecules(mols, cap_atoms, cap_mol_bonds, junk_bond=(1, 2, 3, 0))      # (a junk row that would be a valid bond)


_records = records_to_numpy


def _op(mols, recs, cap_atoms=64, cap_mol_bonds=96, max_atoms=64, max_bonds=96, n_valid=None):
    gs = GraphSimilarity(*_upload(mols, cap_atoms, cap_mol_bonds), max_atoms=max_atoms, max_bonds=max_bonds, n_valid=n_valid, debug_ids=True)
    gs.load(_records(recs))
    return gs


def _check(gs, mols, recs, n_valid=None):
    """one launch: rows and ids against the oracle; returns the rows as dicts"""
    gs.run()
    torch.cuda.synchronize()
    res = gs.result()
    want = so.rows(mols, recs, n_valid)
    assert res["rows"].tolist() == want.tolist(), [dict(zip(so.COLUMNS, r)) for r in res["rows"].tolist()]
    ids = gs.ids.cpu().numpy().view(np.uint64)
    nv = len(mols) if n_valid is None else n_valid
    assert np.array_equal(ids[:nv], so.ids_out(mols, recs, n_valid)[:nv])
    return res, [dict(zip(so.COLUMNS, r)) for r in res["rows"].tolist()]


# ------------------------------------------------------------------------------------------------------------ hand-made rows
def _cases():
    ring = so.record([1, 2, 3, 6], [(0, 1, 1), (1, 2, 2), (2, 3, 4), (0, 3, 5)], charges=[0, 1, -1, 0])
    ring_mol = so.as_mol(ring)
    edit = lambda atoms=None, bonds=None, **kw: dict(
        atoms=[(atoms or {}).get(i, a) for i, a in enumerate(ring_mol["atoms"])],
        bonds=[(bonds or {}).get(i, q) for i, q in enumerate(ring_mol["bonds"])], truncated=kw.get("truncated", False))
    hub = so.record([2] + [1] * 40, [(0, k, 1 + k % 4) for k in range(1, 41)])
    rng = np.random.RandomState(3)
    big = so.random_graph(rng, 30, extra=5)
    junk_rows = [(0, 1, 1), (1, 5, 1), (2, 2, 1), (-1, 2, 1), (1 << 30, 1, 1), (-(1 << 31), 3, 1), (3, (1 << 31) - 1, 1)]
    return [
        ("identical", ring_mol, ring),
        ("C-C-O against C-C-N", so.mol([1, 1, 3], [(1, 2, 1), (2, 3, 1)]), so.record([1, 1, 2], [(0, 1, 1), (1, 2, 1)])),
        ("swap", so.as_mol(so.record([1, 1, 1], [(0, 1, 1), (0, 2, 1), (1, 2, 1)], charges=[-1, 0, -1])),
         so.record([1, 1], [(0, 1, 1), (0, 1, 1)], charges=[0, -1])),
        ("decalin against bicyclopentyl", so.as_mol(so.DECALIN), so.BICYCLOPENTYL),
        ("wedges fold", edit(bonds={0: (1, 2, 6), 3: (1, 4, 1)}), ring),
        ("unknown against unknown", so.mol([99, 1], [(1, 2, 1)]), so.record([-1, 1], [(0, 1, 1)])),
        ("unknown against known", so.mol([13, 1], [(1, 2, 1)]), so.record([-1, 1], [(0, 1, 1)])),
        ("negative vocabulary index", so.mol([-(1 << 31), 1], [(1, 2, 1)]), so.record([-1, 1], [(0, 1, 1)])),
        ("unbonded record atom", so.mol([1, 3], [(1, 2, 2)]), so.record([1, 7, 3], [(0, 2, 2)])),
        ("type 0 on a carbon", edit(atoms={0: (0, 0, 0, 0)}), ring),
        ("aromatic against single", edit(bonds={0: (1, 2, 4)}), ring),
        ("wrong charge", edit(atoms={1: (0, 0, 2, 0)}), ring),
        ("large charges", so.mol([1, 2], [(1, 2, 1)], charges=[-(1 << 31), (1 << 31) - 1]),
         so.record([1, 2], [(0, 1, 1)], charges=[-(1 << 31), (1 << 31) - 1])),
        ("pair listed twice", so.mol([1, 2], [(1, 2, 1), (2, 1, 1)]), so.record([1, 2], [(0, 1, 1)])),
        ("pair listed twice on both sides", so.mol([1, 2], [(1, 2, 1), (2, 1, 2)]), so.record([1, 2], [(0, 1, 2), (0, 1, 1)])),
        ("hub of degree 40", so.as_mol(so.permuted(rng, hub)), hub),
        ("hub with one order changed", so.as_mol((hub[0], [(0, 1, 3)] + hub[1][1:])), hub),
        ("no molecule", None, ring),
        ("truncated", dict(ring_mol, bonds=ring_mol["bonds"][:2], truncated=True), ring),
        ("invalid rows", dict(ring_mol, bonds=junk_rows[:4] + ring_mol["bonds"] + junk_rows[4:]), ring),
        ("empty record", ring_mol, so.record([], [])),
        ("nothing on either side", so.mol([], []), so.record([1, 2], [])),
        ("permuted copy", so.as_mol(so.permuted(rng, big)), big),
        ("one atom changed", so.as_mol(so.permuted(rng, so.one_atom_changed(rng, big))), big),
    ]


def test_hand_made_rows_equal_the_oracle():
    cases = _cases()
    assert len(cases) == 24
    got = {}
    for lo in (0, 8, 16):                                             # three batches of B = 8
        part = cases[lo:lo + 8]
        mols, recs = [m for _, m, _ in part], [r for _, _, r in part]
        res, rows = _check(_op(mols, recs), mols, recs)
        assert [res[c] for c in so.COLUMNS] == so.rows(mols, recs).sum(0).tolist()
        got.update({name: rows[i] for i, (name, _, _) in enumerate(part)})
    # what the cases are there for, spelled out (the oracle and the kernel could share a misreading)
    row = lambda name: [got[name][c] for c in so.COLUMNS]
    full = 1 << 20
    assert row("identical") == [1, 0, 0, 1, 1, 1, 4, 4, 16, 16, 16, full]
    assert row("type 0 on a carbon") == row("wedges fold") == row("identical")
    assert row("C-C-O against C-C-N") == [1, 0, 0, 1, 0, 0, 3, 3, 12, 12, 3, 262144]
    assert row("decalin against bicyclopentyl") == [1, 0, 0, 1, 1, 1, 10, 10, 40, 40, 40, full]
    # the id_0 of C and of C-, and the radius-1 environment of the triangle's C: two C- through single bonds, as a pair listed twice
    assert got["swap"]["envs_common"] == 3 and got["swap"]["size_equal"] == 0
    assert row("unknown against unknown") == row("negative vocabulary index") == [1, 0, 0, 1, 1, 1, 2, 2, 8, 8, 8, full]
    assert row("unknown against known") == [1, 0, 0, 1, 0, 0, 2, 2, 8, 8, 1, full // 8]
    assert row("unbonded record atom") == row("large charges") == row("unknown against unknown")
    # a four-ring, every atom within two bonds of every other.  A changed bond: id_0 reads no order, so all four survive, and id_1
    # of the two atoms away from it.  A changed atom: id_0 of the other three, and id_1 of the one opposite
    assert row("aromatic against single") == [1, 0, 0, 1, 0, 0, 4, 4, 16, 16, 6, 6 * full // 16]
    assert row("wrong charge") == [1, 0, 0, 1, 0, 0, 4, 4, 16, 16, 4, 4 * full // 16]
    assert row("pair listed twice") == [1, 0, 0, 0, 0, 0, 2, 2, 8, 8, 0, 0]
    assert row("pair listed twice on both sides") == [1, 0, 0, 1, 1, 1, 2, 2, 8, 8, 8, full]
    assert row("hub of degree 40") == [1, 0, 0, 1, 1, 1, 41, 41, 164, 164, 164, full]
    # (the hub's id_1 .. id_3 and the changed leaf's, and id_2, id_3 of the 39 other leaves)
    assert got["hub with one order changed"]["refine_equal"] == 0 and got["hub with one order changed"]["envs_common"] == 164 - 6 - 78
    assert row("no molecule") == [1, 1, 0, 0, 0, 0, 0, 0, 0, 16, 0, 0]
    assert got["truncated"]["truncated"] == 1 and got["truncated"]["size_equal"] == 0 and got["truncated"]["atoms_pred"] == 4
    assert row("invalid rows") == row("identical")
    assert row("empty record") == [1, 0, 0, 0, 0, 0, 4, 0, 16, 0, 0, 0]
    assert row("nothing on either side") == [1, 0, 0, 1, 1, 0, 0, 0, 0, 0, 0, 0]
    assert got["permuted copy"]["refine_equal"] == got["permuted copy"]["dice_one"] == 1 and got["permuted copy"]["atoms_true"] == 30
    assert got["one atom changed"]["refine_equal"] == 0 and 0 < got["one atom changed"]["envs_common"] < 120


def test_record_rows_may_hold_any_int32():
    """load() refuses such records; hand-made device rows may hold them, and junk past the counts"""
    rec = so.record([1, 2, 3, 6, 7], [(0, 1, 1), (1, 2, 2), (2, 3, 4)])
    bad = [(0, 5, 1), (2, 2, 1), (-1, 1, 1), (1 << 30, 0, 1), (3, -(1 << 31), 1), (3, 1, 9)]      # the last one is valid, ends swapped
    mols = [so.mol([1, 2, 3, 6], [(1, 2, 1), (2, 3, 2), (3, 4, 4)])] * 2              # (the record's sulphur is in no bond)
    gs = _op(mols, [rec, rec], cap_atoms=8, cap_mol_bonds=8, max_atoms=8, max_bonds=16)
    torch.cuda.synchronize()
    d_atoms, d_bonds, d_cnt = gs.records.staging.dev.values()
    d_atoms.fill_(11)
    d_bonds[:] = torch.tensor([0, 4, 1], dtype=torch.int32, device=DEV)            # (junk that would be a valid row)
    for b in range(2):
        d_atoms[b, :5] = torch.tensor(rec[0], dtype=torch.int32, device=DEV)
    d_bonds[0, :3] = torch.tensor(rec[1], dtype=torch.int32, device=DEV)
    d_bonds[1, :9] = torch.tensor(bad[:3] + rec[1] + bad[3:], dtype=torch.int32, device=DEV)
    d_cnt.copy_(torch.tensor([[5, 5], [3, 9]], dtype=torch.int32, device=DEV))
    recs = [rec, (rec[0], bad[:3] + rec[1] + bad[3:])]
    _res, rows = _check(gs, mols, recs)
    assert rows[0]["dice_one"] == 1 and rows[0]["atoms_true"] == 4
    assert rows[1]["atoms_true"] == 4 and rows[1]["size_equal"] == 0 and 0 < rows[1]["envs_common"] < 16
    # counts past the capacities are clamped
    d_cnt.copy_(torch.tensor([[5, 1 << 30], [3, -7]], dtype=torch.int32, device=DEV))
    want = so.rows(mols, [rec, (d_atoms[1].cpu().numpy(), np.zeros((0, 3), np.int32))])
    gs.run()
    torch.cuda.synchronize()
    assert gs.result()["rows"].tolist() == want.tolist() and want[1, COL["atoms_true"]] == 0


# ------------------------------------------------------------------------------------------------------------------- shapes
def _ring(n, changed=None):
    classes = [1 + k % 3 for k in range(n)]
    if changed is not None:
        classes[changed] = 7
    return so.record(classes, [(k, k + 1, 1 + k % 2) for k in range(n - 1)] + [(0, n - 1, 1)])


def test_sizes_where_the_loops_turn():
    """257 atoms (one over a pass of 256 threads), 512 (the capacity, 64 refinement rounds), 1 atom without a bond; B = 4"""
    rng = np.random.RandomState(5)
    chain = so.record([1 + k % 2 for k in range(257)], [(k, k + 1, 1) for k in range(256)])
    chain_mol = so.as_mol(so.permuted(rng, (chain[0][:256] + [(0, 0, 3, 0)], chain[1])))
    mols = [chain_mol, so.as_mol(so.permuted(rng, _ring(512, changed=300))), so.mol([6], []), so.as_mol(so.permuted(rng, _ring(512)))]
    recs = [chain, _ring(512), so.record([6], []), _ring(512)]
    gs = _op(mols, recs, cap_atoms=512, cap_mol_bonds=512, max_atoms=512, max_bonds=512)
    _res, rows = _check(gs, mols, recs)
    assert rows[0]["atoms_pred"] == 257 and rows[0]["size_equal"] == 1 and rows[0]["refine_equal"] == 0
    assert rows[0]["envs_common"] == 4 * 257 - (1 + 2 + 3 + 4)                    # the changed end atom is seen from up to 3 bonds away
    assert rows[1]["atoms_true"] == 512 and rows[1]["envs_true"] == 2048 and rows[1]["size_equal"] == 1 and rows[1]["refine_equal"] == 0
    assert rows[1]["envs_common"] == 2048 - (1 + 3 + 5 + 7)
    assert [rows[2][c] for c in so.COLUMNS] == [1, 0, 0, 0, 0, 0, 1, 0, 4, 0, 0, 0]    # (an unbonded record atom is not in T)
    assert rows[3]["refine_equal"] == 1 and rows[3]["dice_one"] == 1 and rows[3]["envs_common"] == 2048


def test_bond_rows_are_not_bounded_by_the_workgroup():
    """cap_mol_bonds 2048 with 600 valid rows on 300 atoms, a record of 600 bonds"""
    rng = np.random.RandomState(6)
    atoms = [(0, 0, int(rng.randint(1, 14)), int(rng.choice([0, 0, 1, -1]))) for _ in range(300)]
    pairs = [(k, k + 1) for k in range(299)] + [(0, 299)]
    while len(pairs) < 600:
        i, j = sorted(int(v) for v in rng.choice(300, size=2, replace=False))
        pairs.append((i, j))
    rec = (atoms, [(i, j, int(rng.randint(1, 7))) for i, j in pairs])
    near = (atoms, rec[1][:599] + [(rec[1][599][0], rec[1][599][1], 1 + rec[1][599][2] % 4)])
    mols = [so.as_mol(so.permuted(rng, rec)), so.as_mol(so.permuted(rng, near))]
    gs = _op(mols, [rec, rec], cap_atoms=320, cap_mol_bonds=2048, max_atoms=300, max_bonds=1024)
    _res, rows = _check(gs, mols, [rec, rec])
    assert rows[0]["refine_equal"] == 1 and rows[0]["envs_common"] == 1200
    assert rows[1]["refine_equal"] == 0 and rows[1]["size_equal"] == 1 and 0 < rows[1]["envs_common"] < 1200


# --------------------------------------------------------------------------------------------------------- calls and sharing
def test_n_valid_totals_and_reset():
    cases = _cases()[:8]
    mols, recs = [m for _, m, _ in cases], [r for _, _, r in cases]
    nv = torch.full((1,), 5, dtype=torch.int32, device=DEV)
    gs = _op(mols, recs, n_valid=nv)
    gs.rows.fill_(9)                                                  # (overwritten by every call, the rows past n_valid too)
    ref = so.rows(mols, recs, n_valid=5)
    assert (ref[5:] == 0).all() and ref[:5, 0].tolist() == [1] * 5
    for call in (1, 2, 3):
        res, _rows = _check(gs, mols, recs, n_valid=5)
        assert [res[c] for c in so.COLUMNS] == (call * ref.sum(0)).tolist()
    assert res["counted"] == 15 and res["similarity"] == res["dice_q20"] / 2.0 ** 20 / 15
    # n_valid is read on the device: another value, the same descriptor; out-of-range values are clamped
    for n, counted in ((8, 8), (0, 0), (-3, 0), (99, 8)):
        gs.reset()
        nv.fill_(n)
        res, _rows = _check(gs, mols, recs, n_valid=counted)
        assert res["counted"] == counted
    gs.reset()
    res = gs.result()
    assert all(res[c] == 0 for c in so.COLUMNS) and np.isnan(res["similarity"])


@pytest.mark.parametrize("made_by", ["the scorer", "the caller"])
def test_records_are_shared_with_a_graph_score(made_by):
    """one load, both ops right; who did not make the records stages nothing and refuses a load of its own.  The records are the
    scorer's, taken from it, or a GraphRecords built directly and handed to both."""
    import graphscore_oracle as go
    cases = _cases()[:4]
    mols, recs = [m for _, m, _ in cases], [r for _, _, r in cases]
    rows = _upload(mols, 16, 32)
    if made_by == "the scorer":
        scorer = GraphScore(*rows, max_atoms=16, max_bonds=24, radius=0)
        sim = GraphSimilarity(*rows, records=scorer, debug_ids=True)
        loader, refusers = scorer, [sim]
    else:
        loader = GraphRecords(len(mols), 16, 24, DEV)
        scorer = GraphScore(*rows, radius=0, records=loader)
        sim = GraphSimilarity(*rows, records=loader, debug_ids=True)
        assert scorer.records is loader and (scorer.max_atoms, scorer.max_bonds) == (16, 24) and not scorer.loaded
        refusers = [scorer, sim]
    # (one GraphRecords, so one staging and one set of device buffers: nothing is staged twice)
    assert sim.records is scorer.records and (sim.max_atoms, sim.max_bonds) == (16, 24) and not sim.loaded
    assert sim.d.rec_atoms == scorer.d.rec_atoms == scorer.records.staging.dev["atoms"].data_ptr()
    for op in refusers:
        with pytest.raises(ValueError, match="scorer"):
            op.load(_records(recs))
    loader.load(_records(recs))
    assert sim.loaded and scorer.loaded
    scorer.run()
    _check(sim, mols, recs)
    for_score = [for_score_oracle(m, go.ATOM_SYMBOLS) for m in mols]
    assert scorer.result()["rows"].tolist() == go.rows(for_score, recs, 0).tolist()
    with pytest.raises(ValueError, match="512"):
        GraphSimilarity(*rows, records=GraphScore(*rows, max_atoms=513, max_bonds=24))
    with pytest.raises(ValueError):
        GraphSimilarity(*_upload(mols[:3], 16, 32), records=scorer)
    with pytest.raises(L.AbcNetHipError):
        GraphSimilarity(*(t.long() for t in rows))


# ------------------------------------------------------------------------------------------------------------------ the runner
def test_runner_grades_its_own_molecules(golden_dir):
    """the twin of test_runner_scores_its_own_molecules: batch 4 at 96 x 96, a short batch of 3 through SampleBuilder, three steps
    (eager, capture + replay, replay), the trained fixture; beside it the same runner without the flag, whose "molecules" must
    not move, and one with the flag alone, which stages the records itself"""
    from abcnet_amd.augment import SampleBuilder, draw_augment
    from abcnet_amd.infer import InferenceRunner
    B, S, n = 4, 96, 3
    h = S // 4
    m = trained_unet(golden_dir)
    kw = dict(use_graph=True, assemble=True, evaluate=True)
    plain = InferenceRunner(m, B, S, S, score_graphs=True, **kw)
    run = InferenceRunner(m, B, S, S, score_graphs=True, score_similarity=True, **kw)
    solo = InferenceRunner(m, B, S, S, score_similarity=True, **kw)
    assert plain.similarity is None and run.similarity.records is run.scorer.records is run.records and run.similarity.keep[3] is run.n_valid
    assert run.similarity.ids is None and solo.scorer is None and solo.similarity.records is solo.records is not None
    builders = [SampleBuilder(r, amount=0.1, max_src=(S, S), sparse=True, max_atoms=64, max_bonds=64) for r in (plain, run, solo)]
    for r in (run, solo):
        with pytest.raises(L.AbcNetHipError, match="no graph records"):
            r.step()
    total = np.zeros(len(so.COLUMNS), dtype=np.int64)
    some_molecule = False
    for step in range(3):
        x, notes = drawn_molecules(n, S, seed=40 + step)
        srcs = [((1.0 - x[b, 0].numpy()) * 255).astype(np.uint8) for b in range(n)]       # dark ink on white
        for sb, r in zip(builders, (plain, run, solo)):
            sb.load(srcs, [a for a, _ in notes], [q for _, q in notes], np.random.RandomState(step))
            sb.run()
            r.step()
        torch.cuda.synchronize()
        rs = np.random.RandomState(step)
        graphs = [parse_graph(a, q, *draw_augment(rs, 0.1, srcs[b].shape, S)[1], h=h) for b, (a, q) in enumerate(notes)]
        mols = run.molecules()
        some_molecule |= any(mol is not None for mol in mols[:n])
        want = so.rows(mols, graphs, n_valid=n)
        ev, ev_plain, ev_solo = run.evaluation(), plain.evaluation(), solo.evaluation()
        res = ev["similarity"]
        print(step, [None if mol is None else (len(mol.symbols), len(mol.bonds)) for mol in mols], res["rows"].tolist())
        assert res["rows"].tolist() == want.tolist(), step
        total += want.sum(0)
        assert [res[c] for c in so.COLUMNS] == total.tolist(), step
        assert res["similarity"] == total[COL["dice_q20"]] / 2.0 ** 20 / total[COL["counted"]]
        # the flag moves nothing else, and the op that stages its own records says the same
        assert "similarity" not in ev_plain and "molecules" not in ev_solo
        assert ev["molecules"]["rows"].tolist() == ev_plain["molecules"]["rows"].tolist()
        assert [ev["molecules"][c] for c in L.GRAPH_SCORE_COLUMNS] == [ev_plain["molecules"][c] for c in L.GRAPH_SCORE_COLUMNS]
        assert ev_solo["similarity"]["rows"].tolist() == want.tolist() and ev_solo["similarity"]["dice_q20"] == total[COL["dice_q20"]]
    assert run._graph is not None and solo._graph is not None and total[COL["counted"]] == 3 * n
    assert some_molecule, "every molecule of every step is None: the similarity of these weights says nothing"
    run.reset_evaluation()
    res = run.evaluation()
    assert all(res["similarity"][c] == 0 for c in so.COLUMNS) and all(res["molecules"][c] == 0 for c in L.GRAPH_SCORE_COLUMNS)
