"""The verified isomorphism test on the device (csrc/graph_ident.hip, ops.GraphIdentity, InferenceRunner(score_identity=True)) against
the oracle (tests/graphident_oracle.py): rows, totals and the witness table are compared with torch.equal -- answers, work counters
and every word of the bijection.

Measured on an MI355X (device events around one launch of B = 1, test_the_longest_cases_inside_the_default_budgets prints them): the
ring of 512 carbons 2.34 ms (988 rounds), the chain of 512 carbons 2.39 ms (1008 rounds), 170 disjoint C-C-C 3.43 ms (254 levels,
1018 rounds).  (With the class count as a quadratic sweep instead of the LDS table they took 16.8, 16.8 and 34.7 ms.)"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import abcnet_amd  # noqa: E402,F401
from abcnet_amd import _lib as L  # noqa: E402
from abcnet_amd.contract import GraphRecords  # noqa: E402
from abcnet_amd.ops import GraphIdentity, GraphScore, GraphSimilarity  # noqa: E402
from abcnet_amd.raster import parse_graph  # noqa: E402
from abcnet_amd.synthetic import drawn_molecules  # noqa: E402
import graphident_oracle as io  # noqa: E402
import graphsim_oracle as so  # noqa: E402
from molrows import records_to_numpy, trained_unet, upload_molecules  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
COL = {c: i for i, c in enumerate(io.COLUMNS)}
SIM = {c: i for i, c in enumerate(so.COLUMNS)}


def _upload(mols, cap_atoms, cap_mol_bonds):
    return upload_molecules(mols, cap_atoms, cap_mol_bonds, junk_bond=(1, 2, 3, 0))      # (a junk row that would be a valid bond)


def _op(mols, recs, cap_atoms=64, cap_mol_bonds=96, max_atoms=64, max_bonds=96, n_valid=None, witness=True, **budgets):
    gi = GraphIdentity(*_upload(mols, cap_atoms, cap_mol_bonds), max_atoms=max_atoms, max_bonds=max_bonds, n_valid=n_valid, witness=witness,
                       **budgets)
    gi.load(records_to_numpy(recs))
    return gi


def _check(gi, mols, recs, n_valid=None, calls=1, **budgets):
    """one launch: rows, totals and witness against the oracle with torch.equal; returns the rows as dicts"""
    want_rows, want_map = io.rows_and_maps(mols, recs, gi.cap_atoms, n_valid, **budgets)
    gi.reset()
    if gi.map is not None:
        gi.map.fill_(77)                                              # (written entirely by every launch)
    for _ in range(calls):
        gi.run()
    torch.cuda.synchronize()
    assert torch.equal(gi.rows.cpu(), torch.from_numpy(want_rows).int()), [dict(zip(io.COLUMNS, r)) for r in gi.rows.cpu().tolist()]
    assert torch.equal(gi.totals.cpu(), torch.from_numpy(calls * want_rows.sum(0)))
    if gi.map is not None:
        assert torch.equal(gi.map.cpu(), torch.from_numpy(want_map))
    return [dict(zip(io.COLUMNS, r)) for r in want_rows.tolist()]


# --------------------------------------------------------------------------------------------------------------- random pairs
def test_random_pairs_equal_the_oracle_in_one_launch():
    """the first 256 of the host suite's pairs (there held to networkx), B = 256"""
    pairs = list(io.random_pairs(256, seed=11))
    mols, recs = [m for m, _ in pairs], [r for _, r in pairs]
    rows = _check(_op(mols, recs, cap_atoms=16, cap_mol_bonds=16, max_atoms=16, max_bonds=16), mols, recs)
    assert sum(r["same"] for r in rows) >= 100 and sum(r["different"] for r in rows) >= 100 and not any(r["undecided"] for r in rows)


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
        ("decalin against bicyclopentyl", so.as_mol(so.DECALIN), so.BICYCLOPENTYL),
        ("decalin permuted", so.as_mol(so.permuted(rng, so.DECALIN)), so.DECALIN),
        ("bicyclopentyl permuted", so.as_mol(so.permuted(rng, so.BICYCLOPENTYL)), so.BICYCLOPENTYL),
        ("the union that backtracks", so.as_mol(io.UNION_PERMUTED), io.UNION),
        ("twin decalins against the union", so.as_mol(io.union(so.DECALIN, so.DECALIN)), io.UNION),
        ("wedges fold", edit(bonds={0: (1, 2, 6), 3: (1, 4, 1)}), ring),
        ("unknown against unknown", so.mol([99, 1], [(1, 2, 1)]), so.record([-1, 1], [(0, 1, 1)])),
        ("unknown against known", so.mol([13, 1], [(1, 2, 1)]), so.record([-1, 1], [(0, 1, 1)])),
        ("negative vocabulary index", so.mol([-(1 << 31), 1], [(1, 2, 1)]), so.record([-1, 1], [(0, 1, 1)])),
        ("unbonded record atom", so.mol([3, 1], [(1, 2, 2)]), so.record([1, 7, 3], [(0, 2, 2)])),
        ("type 0 on a carbon", edit(atoms={0: (0, 0, 0, 0)}), ring),
        ("aromatic against single", edit(bonds={0: (1, 2, 4)}), ring),
        ("wrong charge", edit(atoms={1: (0, 0, 2, 0)}), ring),
        ("large charges", so.mol([1, 2], [(1, 2, 1)], charges=[-(1 << 31), (1 << 31) - 1]),
         so.record([1, 2], [(0, 1, 1)], charges=[-(1 << 31), (1 << 31) - 1])),
        ("pair listed twice", so.mol([1, 2], [(1, 2, 1), (2, 1, 1)]), so.record([1, 2], [(0, 1, 1)])),
        ("pair listed twice on both sides", so.mol([1, 2], [(1, 2, 1), (2, 1, 2)]), so.record([1, 2], [(0, 1, 2), (0, 1, 1)])),
        ("pair listed twice with other orders", so.mol([1, 2], [(1, 2, 1), (2, 1, 1)]), so.record([1, 2], [(0, 1, 2), (0, 1, 1)])),
        ("hub of degree 40", so.as_mol(so.permuted(rng, hub)), hub),
        ("hub with one order changed", so.as_mol((hub[0], [(0, 1, 3)] + hub[1][1:])), hub),
        ("no molecule", None, ring),
        ("truncated", dict(ring_mol, truncated=True), ring),
        ("invalid rows", dict(ring_mol, bonds=junk_rows[:4] + ring_mol["bonds"] + junk_rows[4:]), ring),
        ("empty record", ring_mol, so.record([], [])),
        ("nothing on either side", so.mol([], []), so.record([1, 2], [])),
        ("a six-ring of order-4 bonds", so.as_mol(so.permuted(rng, io.carbon_ring(6, order=4))), io.carbon_ring(6, order=4)),
        ("permuted copy", so.as_mol(so.permuted(rng, big)), big),
        ("one atom changed", so.as_mol(so.permuted(rng, so.one_atom_changed(rng, big))), big),
    ]


def test_hand_made_rows_equal_the_oracle():
    cases = _cases()
    mols, recs = [m for _, m, _ in cases], [r for _, _, r in cases]
    rows = _check(_op(mols, recs), mols, recs)
    got = {name: rows[i] for i, (name, _, _) in enumerate(cases)}
    # what the cases are there for, spelled out (the oracle and the kernel could share a misreading)
    answer = lambda name: [got[name][c] for c in ("size_equal", "same", "different", "undecided")]
    for name in ("identical", "decalin permuted", "bicyclopentyl permuted", "the union that backtracks", "wedges fold", "unknown against unknown",
                 "negative vocabulary index", "unbonded record atom", "type 0 on a carbon", "large charges", "pair listed twice on both sides",
                 "hub of degree 40", "truncated", "invalid rows", "nothing on either side", "a six-ring of order-4 bonds", "permuted copy"):
        assert answer(name) == [1, 1, 0, 0], name
    for name in ("decalin against bicyclopentyl", "twin decalins against the union", "unknown against known", "aromatic against single",
                 "wrong charge", "pair listed twice with other orders", "hub with one order changed", "one atom changed"):
        assert answer(name) == [1, 0, 1, 0], name
    for name in ("pair listed twice", "empty record"):
        assert answer(name) == [0, 0, 1, 0] and [got[name][c] for c in ("levels", "tries", "backtracks", "rounds")] == [0] * 4, name
    assert [got["no molecule"][c] for c in io.COLUMNS] == [1, 1] + [0] * 9
    assert got["truncated"]["truncated"] == 1
    assert {k: got["the union that backtracks"][k] for k in io.UNION_COUNTERS} == io.UNION_COUNTERS
    assert got["decalin against bicyclopentyl"]["backtracks"] == 2


@pytest.mark.parametrize("budgets, want", [(dict(max_tries=1), [1, 0, 0, 1, 0, 0, 1, 5, 1, 1, 25]),
                                           (dict(max_rounds=20), [1, 0, 0, 1, 0, 0, 1, 5, 1, 0, 20]),
                                           (dict(max_rounds=3), [1, 0, 0, 1, 0, 0, 1, 0, 0, 0, 3]),
                                           (dict(max_rounds=24), [1, 0, 0, 1, 0, 0, 1, 5, 1, 1, 24]),
                                           (dict(max_rounds=33), [1, 0, 0, 1, 0, 0, 1, 5, 3, 2, 33])])
def test_tiny_budgets_end_undecided(budgets, want):
    """the backtracking fixture beside a pair that needs one round per side and no try: a budget is an image's own.  The last two end
    inside the record's search after a backtrack (graphident_oracle.identify: 23 rounds are run when the first backtrack comes, the
    third try is made by round 31, the fourth at 35): 24 one round into the replay behind the first backtrack, 33 in the rounds of a
    level behind the second"""
    mols, recs = [so.as_mol(io.UNION_PERMUTED), so.mol([1, 2], [(1, 2, 1)])], [io.UNION, so.record([2, 1], [(0, 1, 1)])]
    rows = _check(_op(mols, recs, **budgets), mols, recs, **budgets)
    assert [rows[0][c] for c in io.COLUMNS] == want
    assert [rows[1][c] for c in io.COLUMNS] == [1, 0, 0, 1, 1, 0, 0, 0, 0, 0, 2]


# ------------------------------------------------------------------------------------------------------------------- shapes
def _with_bonds(rng, n, m):
    """n atoms in a ring and chords up to m bond rows"""
    atoms = [(0, 0, int(rng.randint(1, 14)), int(rng.choice([0, 0, 1, -1]))) for _ in range(n)]
    pairs = [(k, k + 1) for k in range(n - 1)] + [(0, n - 1)]
    while len(pairs) < m:
        i, j = sorted(int(v) for v in rng.choice(n, size=2, replace=False))
        pairs.append((i, j))
    return atoms, [(i, j, int(rng.randint(1, 7))) for i, j in pairs]


def test_sizes_where_the_loops_turn():
    """255 / 256 / 257 valid bond rows (a pass of 256 threads), a row past them changed, 1 and 2 atoms; B = 7"""
    rng = np.random.RandomState(6)
    recs, mols = [], []
    for m in (255, 256, 257):
        rec = _with_bonds(rng, 200, m)
        recs.append(rec)
        mols.append(so.as_mol(so.permuted(rng, rec)))
    last = recs[2][1][256]
    near = (recs[2][0], recs[2][1][:256] + [(last[0], last[1], 1 + last[2] % 4)])
    recs += [recs[2], so.record([6], []), so.record([6, 7], [(0, 1, 1)]), so.record([6, 7], [(0, 1, 1)])]
    mols += [so.as_mol(so.permuted(rng, near)), so.mol([6], []), so.mol([7, 6], [(2, 1, 1)]), so.mol([7, 7], [(2, 1, 1)])]
    rows = _check(_op(mols, recs, cap_atoms=200, cap_mol_bonds=300, max_atoms=200, max_bonds=257), mols, recs)
    assert [r["same"] for r in rows] == [1, 1, 1, 0, 0, 1, 0] and [r["different"] for r in rows] == [0, 0, 0, 1, 1, 0, 1]
    assert rows[3]["size_equal"] == 1 and rows[4]["size_equal"] == 0      # (an unbonded record atom is not in T: one atom against none)


@pytest.mark.parametrize("name, rec", [("ring", io.carbon_ring(512)), ("chain", io.carbon_chain(512)), ("propanes", io.propanes(170))])
def test_the_longest_cases_inside_the_default_budgets(name, rec):
    """512 atoms (the capacity), every atom like every other: the most rounds (ring, chain) and the most levels and tries (170
    disjoint C-C-C) the defaults were chosen from; one launch of B = 1 each, its time printed"""
    mol = so.as_mol(so.permuted(np.random.RandomState(5), rec))
    gi = _op([mol], [rec], cap_atoms=512, cap_mol_bonds=512, max_atoms=512, max_bonds=512)
    rows = _check(gi, [mol], [rec])
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    gi.run()
    e1.record()
    torch.cuda.synchronize()
    print(name, rows[0], "%.2f ms" % e0.elapsed_time(e1))
    assert rows[0]["same"] == 1 and rows[0]["rounds"] >= 900 and rows[0]["tries"] in (1, 2, 254)


def test_bond_rows_are_not_bounded_by_the_workgroup():
    """cap_mol_bonds 2048 with 600 valid rows on 300 atoms, a record of 600 bonds: the verification counts rows past the threads"""
    rng = np.random.RandomState(6)
    rec = _with_bonds(rng, 300, 600)
    near = (rec[0], rec[1][:599] + [(rec[1][599][0], rec[1][599][1], 1 + rec[1][599][2] % 4)])
    mols = [so.as_mol(so.permuted(rng, rec)), so.as_mol(so.permuted(rng, near))]
    rows = _check(_op(mols, [rec, rec], cap_atoms=320, cap_mol_bonds=2048, max_atoms=300, max_bonds=1024), mols, [rec, rec])
    assert rows[0]["same"] == 1 and rows[1]["different"] == 1 and rows[1]["size_equal"] == 1


# --------------------------------------------------------------------------------------------------------- calls and sharing
def test_witness_off_changes_nothing_and_totals_accumulate():
    cases = _cases()[:8]
    mols, recs = [m for _, m, _ in cases], [r for _, _, r in cases]
    nv = torch.full((1,), 5, dtype=torch.int32, device=DEV)
    with_map, without = _op(mols, recs, n_valid=nv), _op(mols, recs, n_valid=nv, witness=False)
    assert without.map is None and without.d.map_out is None and with_map.map.shape == (8, 64)
    for gi in (with_map, without):
        gi.rows.fill_(9)                                              # (overwritten by every call, the rows past n_valid too)
        _check(gi, mols, recs, n_valid=5, calls=3)
    assert torch.equal(with_map.rows, without.rows) and torch.equal(with_map.totals, without.totals)
    res = with_map.result()
    assert res["counted"] == 15 and res["share_same"] == res["same"] / 15 and res["share_undecided"] == 0.0
    assert (with_map.map[5:] == -1).all()
    # n_valid is read on the device: another value, the same descriptor; out-of-range values are clamped
    for n, counted in ((8, 8), (0, 0), (-3, 0), (99, 8)):
        nv.fill_(n)
        _check(with_map, mols, recs, n_valid=counted)
        assert with_map.result()["counted"] == counted
    with_map.reset()
    res = with_map.result()
    assert all(res[c] == 0 for c in io.COLUMNS) and np.isnan(res["share_same"]) and np.isnan(res["share_undecided"])


def test_record_rows_may_hold_any_int32():
    """load() refuses such records; hand-made device rows may hold them, and junk past the counts"""
    rec = so.record([1, 2, 3, 6, 7], [(0, 1, 1), (1, 2, 2), (2, 3, 4)])
    bad = [(0, 5, 1), (2, 2, 1), (-1, 1, 1), (1 << 30, 0, 1), (3, -(1 << 31), 1), (3, 1, 9)]      # the last one is valid, ends swapped
    mols = [so.mol([1, 2, 3, 6], [(1, 2, 1), (2, 3, 2), (3, 4, 4)])] * 2              # (the record's sulphur is in no bond)
    gi = _op(mols, [rec, rec], cap_atoms=8, cap_mol_bonds=8, max_atoms=8, max_bonds=16)
    torch.cuda.synchronize()
    d_atoms, d_bonds, d_cnt = gi.records.staging.dev.values()
    d_atoms.fill_(11)
    d_bonds[:] = torch.tensor([0, 4, 1], dtype=torch.int32, device=DEV)            # (junk that would be a valid row)
    for b in range(2):
        d_atoms[b, :5] = torch.tensor(rec[0], dtype=torch.int32, device=DEV)
    d_bonds[0, :3] = torch.tensor(rec[1], dtype=torch.int32, device=DEV)
    d_bonds[1, :9] = torch.tensor(bad[:3] + rec[1] + bad[3:], dtype=torch.int32, device=DEV)
    d_cnt.copy_(torch.tensor([[5, 5], [3, 9]], dtype=torch.int32, device=DEV))
    recs = [rec, (rec[0], bad[:3] + rec[1] + bad[3:])]
    rows = _check(gi, mols, recs)
    assert rows[0]["same"] == 1 and rows[1]["size_equal"] == 0 and rows[1]["different"] == 1
    # counts past the capacities are clamped
    d_cnt.copy_(torch.tensor([[5, 1 << 30], [3, -7]], dtype=torch.int32, device=DEV))
    rows = _check(gi, mols, [rec, (d_atoms[1].cpu().numpy(), np.zeros((0, 3), np.int32))])
    assert rows[0]["same"] == 1 and rows[1]["size_equal"] == 0 and rows[1]["different"] == 1


def test_records_are_shared_with_a_graph_score_and_a_similarity():
    """one GraphRecords, one load, three ops on the same launch inputs: same <= refine_equal row by row, same => dice_one, and
    exact => same (the positional lower bound)"""
    pairs = list(io.random_pairs(32, seed=12))
    cases = _cases()[:8]
    mols, recs = [m for m, _ in pairs] + [m for _, m, _ in cases], [r for _, r in pairs] + [r for _, _, r in cases]
    rows = _upload(mols, 24, 32)
    records = GraphRecords(len(mols), 24, 32, DEV)
    scorer = GraphScore(*rows, radius=0, records=records)
    sim = GraphSimilarity(*rows, records=records)
    ident = GraphIdentity(*rows, records=records, witness=True)
    taken = GraphIdentity(*rows, records=sim)                         # (a scorer's records are taken)
    assert ident.records is sim.records is scorer.records is taken.records is records and (ident.max_atoms, ident.max_bonds) == (24, 32)
    assert ident.d.rec_atoms == sim.d.rec_atoms == records.staging.dev["atoms"].data_ptr() and not ident.loaded
    with pytest.raises(ValueError, match="scorer"):
        ident.load(records_to_numpy(recs))
    records.load(records_to_numpy(recs))
    assert ident.loaded
    for op in (scorer, sim, taken):
        op.run()
    _check(ident, mols, recs)
    torch.cuda.synchronize()
    r_id, r_sim, r_gs = ident.rows.cpu().numpy(), sim.rows.cpu().numpy(), scorer.rows.cpu().numpy()
    assert np.array_equal(r_id, taken.rows.cpu().numpy())
    same = r_id[:, COL["same"]]
    assert (same <= r_sim[:, SIM["refine_equal"]]).all() and (same <= r_sim[:, SIM["dice_one"]]).all()
    assert (r_sim[:, SIM["refine_equal"]] + r_id[:, COL["different"]] + r_id[:, COL["none"]] >= 1).all()
    assert (r_gs[:, L.GRAPH_SCORE_COLUMNS.index("exact")] <= same).all()
    assert np.array_equal(r_id[:, COL["size_equal"]], r_sim[:, SIM["size_equal"]])
    assert same.sum() >= 10 and (r_sim[:, SIM["refine_equal"]] - same).sum() >= 1      # (decalin against bicyclopentyl is in there)
    with pytest.raises(ValueError, match="512"):
        GraphIdentity(*rows, records=GraphScore(*rows, max_atoms=513, max_bonds=24))
    with pytest.raises(ValueError):
        GraphIdentity(*_upload(mols[:3], 24, 32), records=records)
    with pytest.raises(L.AbcNetHipError):
        GraphIdentity(*(t.long() for t in rows))


# ------------------------------------------------------------------------------------------------------------------ the runner
def _as_record(mol):
    """an assembled molecule (decode.Molecule) as the graph record that says the same"""
    atoms = [(p[0], p[1], so.ATOM_SYMBOLS.index(s), c) for p, s, c in zip(mol.positions, mol.symbols, mol.charges)]
    bonds = [(min(q) - 1, max(q) - 1, o) for q, o in zip(mol.bonds, mol.orders)]
    return np.array(atoms, dtype=np.int32).reshape(-1, 4), np.array(bonds, dtype=np.int32).reshape(-1, 3)


def test_runner_identifies_its_own_molecules(golden_dir):
    """batch 4 at 96 x 96 (the size of test_runner_grades_its_own_molecules), a short batch of 3 through SampleBuilder, the trained
    fixture: an eager step and its replay from the captured graph say the same, every step equals the oracle, the flag moves no other
    result, and each image's own molecule fed back as its record is `same`"""
    from abcnet_amd.augment import SampleBuilder, draw_augment
    from abcnet_amd.infer import InferenceRunner
    B, S, n = 4, 96, 3
    h = S // 4
    m = trained_unet(golden_dir)
    kw = dict(use_graph=True, assemble=True, evaluate=True, score_similarity=True)
    plain = InferenceRunner(m, B, S, S, **kw)
    run = InferenceRunner(m, B, S, S, score_identity=True, **kw)
    solo = InferenceRunner(m, B, S, S, use_graph=True, assemble=True, evaluate=True, score_identity=True)
    assert plain.identity is None and run.identity.records is run.similarity.records is run.records and run.identity.keep[3] is run.n_valid
    assert run.identity.map is None and run._stages.index("identity") == run._stages.index("similarity") + 1
    assert solo.wants_graph_records and solo.similarity is None and solo.identity.records is solo.records is not None
    builders = [SampleBuilder(r, amount=0.1, max_src=(S, S), sparse=True, max_atoms=64, max_bonds=64) for r in (plain, run, solo)]
    for r in (run, solo):
        with pytest.raises(L.AbcNetHipError, match="no graph records"):
            r.step()
    total = np.zeros(len(io.COLUMNS), dtype=np.int64)
    tables, some_molecule = [], False
    for step, seed in enumerate((40, 40, 41)):                          # eager, capture + replay of the same batch, replay of another
        x, notes = drawn_molecules(n, S, seed=seed)
        srcs = [((1.0 - x[b, 0].numpy()) * 255).astype(np.uint8) for b in range(n)]       # dark ink on white
        for sb, r in zip(builders, (plain, run, solo)):
            sb.load(srcs, [a for a, _ in notes], [q for _, q in notes], np.random.RandomState(seed))
            sb.run()
            r.step()
        torch.cuda.synchronize()
        rs = np.random.RandomState(seed)
        graphs = [parse_graph(a, q, *draw_augment(rs, 0.1, srcs[b].shape, S)[1], h=h) for b, (a, q) in enumerate(notes)]
        mols = run.molecules()
        some_molecule |= any(mol is not None for mol in mols[:n])
        want = io.rows(mols, graphs, n_valid=n)
        ev, ev_plain = run.evaluation(), plain.evaluation()
        res = ev["identity"]
        print(step, [None if mol is None else (len(mol.symbols), len(mol.bonds)) for mol in mols], res["rows"].tolist())
        assert res["rows"].tolist() == want.tolist() and (res["rows"][n:] == 0).all(), step
        total += want.sum(0)
        assert [res[c] for c in io.COLUMNS] == total.tolist(), step
        assert res["share_same"] == total[COL["same"]] / total[COL["counted"]] and res["undecided"] == 0
        tables.append(res["rows"])
        # the flag moves nothing else
        assert "identity" not in ev_plain and ev["similarity"]["rows"].tolist() == ev_plain["similarity"]["rows"].tolist()
        assert [ev["similarity"][c] for c in so.COLUMNS] == [ev_plain["similarity"][c] for c in so.COLUMNS]
        assert (res["rows"][:, COL["same"]] <= ev["similarity"]["rows"][:, SIM["refine_equal"]]).all()
        ev_solo = solo.evaluation()
        assert "similarity" not in ev_solo and ev_solo["identity"]["rows"].tolist() == want.tolist()
        assert [ev_solo["identity"][c] for c in io.COLUMNS] == total.tolist()
    assert run._graph is not None and total[COL["counted"]] == 3 * n
    assert np.array_equal(tables[0], tables[1])                        # eager and replayed: identical
    assert some_molecule, "every molecule of every step is None: the identity of these weights says nothing"
    # each image's own molecule as its record: the replayed graph reads the new records and finds every one the same
    own = [_as_record(mol) if mol is not None else (np.zeros((0, 4), np.int32), np.zeros((0, 3), np.int32)) for mol in run.molecules()[:n]]
    run.reset_evaluation()
    run.load_graphs(own)
    run.step()
    res = run.evaluation()["identity"]
    assert res["counted"] == n and res["same"] == res["counted"] - res["none"] and res["different"] == res["undecided"] == 0
    assert res["same"] >= 1
    run.reset_evaluation()
    res = run.evaluation()
    assert all(res["identity"][c] == 0 for c in io.COLUMNS) and all(res["similarity"][c] == 0 for c in so.COLUMNS)
