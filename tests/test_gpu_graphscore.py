"""The score after assembly on the device (csrc/graph_score.hip, ops.GraphScore, InferenceRunner(score_graphs=True)) against the
brute-force oracle (tests/graphscore_oracle.py).  Every comparison is integer-exact."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import abcnet_amd  # noqa: E402,F401
from abcnet_amd import _lib as L  # noqa: E402
from abcnet_amd.ops import GraphAssembler, GraphScore, PeakExtractor, nms_peaks  # noqa: E402
from abcnet_amd.raster import TargetRasterizer, parse_graph, parse_record  # noqa: E402
from abcnet_amd.synthetic import drawn_molecules  # noqa: E402
import graphscore_oracle as go  # noqa: E402
from molrows import for_score_oracle, records_to_numpy, trained_unet, upload_molecules  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
COL = {c: i for i, c in enumerate(go.COLUMNS)}


# ------------------------------------------------------------------------------------------------------------ hand-made rows
def _mol(atoms, bonds, truncated=False):
    """atoms [(x, y, vocabulary index, charge)], bonds [(end 1, end 2 (1-based), order)]: the rows the assembler would store"""
    return dict(atoms=[tuple(a) for a in atoms], bonds=[tuple(q) for q in bonds], truncated=truncated)


def _for_oracle(m):
    return for_score_oracle(m, go.ATOM_SYMBOLS)


def _upload(mols, cap_atoms, cap_mol_bonds):
    return upload_molecules(mols, cap_atoms, cap_mol_bonds, junk_bond=(1, 1, 1, 1))


# the annotated graph of most cases: a four-ring C - N+ - O- - Cl and one atom no bond names (not in T)
REC = ([(5, 5, 1, 0), (10, 5, 2, 1), (10, 12, 3, -1), (5, 12, 6, 0), (20, 20, 1, 0)], [(0, 1, 1), (1, 2, 2), (2, 3, 4), (0, 3, 5)])
ATOMS = [(5, 5, 1, 0), (10, 5, 2, 1), (10, 12, 3, -1), (5, 12, 6, 0)]
BONDS = [(1, 2, 1), (3, 2, 2), (3, 4, 4), (4, 1, 5)]               # (the assembler stores the ends in either order)
NO_REC = ([], [])


def _edit(atoms=None, bonds=None, **kw):
    a, q = list(ATOMS), list(BONDS)
    for i, v in (atoms or {}).items():
        a[i] = v
    for i, v in (bonds or {}).items():
        q[i] = v
    return _mol(a, q, **kw)


def _cases():
    tie_rec = ([(10, 5, 1, 0), (30, 30, 2, 0), (32, 30, 3, 0), (50, 50, 1, 0)], [(0, 3, 1), (1, 2, 2)])
    # (9,5) and (11,5) are one cell from annotated (10,5): the lower row is its nearest; (31,30) is one cell from annotated
    # (30,30) and (32,30): the lower record index is its nearest; (50,50) sits exactly
    tie_mol = _mol([(9, 5, 1, 0), (11, 5, 1, 0), (31, 30, 2, 0), (50, 50, 1, 0)], [(1, 4, 1), (2, 4, 1), (3, 4, 2)])
    twin_rec = ([(5, 5, 1, 0), (10, 5, 2, 0), (5, 5, 3, 0), (10, 12, 1, 0)], [(0, 1, 1), (2, 3, 1)])      # atoms 0 and 2 share a cell
    twin_mol = _mol([(5, 5, 1, 0), (10, 5, 2, 0), (10, 12, 1, 0)], [(1, 2, 1), (1, 3, 1)])
    unknown_rec = ([(5, 5, -1, 0), (10, 5, 0, 0)], [(0, 1, 1)])     # an element outside the vocabulary; index 0 reads as carbon
    unknown_mol = _mol([(5, 5, 13, 0), (10, 5, 1, 0)], [(1, 2, 1)])
    return [
        ("identical", _edit(), REC),
        ("wrong element", _edit(atoms={1: (10, 5, 3, 1)}), REC),
        ("wrong charge", _edit(atoms={1: (10, 5, 2, 0)}), REC),
        ("type 0 on a carbon", _edit(atoms={0: (5, 5, 0, 0)}), REC),
        ("missing bond", _mol(ATOMS, BONDS[:2] + BONDS[3:]), REC),
        ("spurious bond", _mol(ATOMS, BONDS + [(1, 3, 1)]), REC),
        ("wrong order", _edit(bonds={1: (3, 2, 1)}), REC),
        ("one cell off", _edit(atoms={2: (11, 12, 3, -1)}), REC),
        ("ties in both directions", tie_mol, tie_rec),
        ("two annotated atoms in one cell", twin_mol, twin_rec),
        ("no molecule", None, REC),
        ("truncated", _mol(ATOMS, BONDS[:2], truncated=True), REC),
        ("empty record", _edit(), NO_REC),
        ("empty record, empty molecule", _mol([], []), NO_REC),
        ("an atom on the unbonded annotated atom", _mol(ATOMS + [(20, 20, 1, 0)], BONDS + [(5, 1, 1)]), REC),
        ("unknown element", unknown_mol, unknown_rec),
    ]


def _score(mols, recs, radius, cap_atoms=32, cap_mol_bonds=64, max_atoms=32, max_bonds=32, n_valid=None):
    gs = GraphScore(*_upload(mols, cap_atoms, cap_mol_bonds), max_atoms=max_atoms, max_bonds=max_bonds, radius=radius, n_valid=n_valid)
    gs.load(records_to_numpy(recs))
    return gs


@pytest.mark.parametrize("radius", [0, 1])
def test_hand_made_rows_equal_the_oracle(radius):
    cases = _cases()
    assert len(cases) == 16
    got = {}
    for lo in (0, 8):                                                 # two batches of B = 8
        part = cases[lo:lo + 8]
        gs = _score([m for _, m, _ in part], [r for _, _, r in part], radius)
        gs.run()
        torch.cuda.synchronize()
        res = gs.result()
        rows = res["rows"]
        ref = go.rows([_for_oracle(m) for _, m, _ in part], [r for _, _, r in part], radius)
        for i, (name, _, _) in enumerate(part):
            assert rows[i].tolist() == ref[i].tolist(), (name, radius, dict(zip(go.COLUMNS, rows[i].tolist())))
            got[name] = dict(zip(go.COLUMNS, rows[i].tolist()))
        assert [res[c] for c in go.COLUMNS] == ref.sum(0).tolist()
    # what the cases are there for, spelled out (the oracle and the kernel could share a misreading)
    row = lambda name: [got[name][c] for c in go.COLUMNS]
    assert row("identical") == [1, 0, 0, 1, 1, 1, 4, 4, 4, 4, 4, 4, 4, 4]
    assert row("type 0 on a carbon") == row("identical")
    assert row("wrong element") == [1, 0, 0, 0, 0, 1, 4, 4, 4, 3, 4, 4, 4, 4] == row("wrong charge")
    assert row("missing bond") == [1, 0, 0, 0, 1, 0, 4, 4, 4, 4, 4, 3, 3, 3]
    assert row("spurious bond") == [1, 0, 0, 0, 1, 0, 4, 4, 4, 4, 4, 5, 4, 4]
    assert row("wrong order") == [1, 0, 0, 0, 1, 0, 4, 4, 4, 4, 4, 4, 4, 3]
    assert row("one cell off") == ([1, 0, 0, 1, 1, 1, 4, 4, 4, 4, 4, 4, 4, 4] if radius else [1, 0, 0, 0, 0, 0, 4, 4, 3, 3, 4, 4, 2, 2])
    assert row("no molecule") == [1, 1, 0, 0, 0, 0, 4, 0, 0, 0, 4, 0, 0, 0]
    assert row("truncated") == [1, 0, 1, 0, 1, 0, 4, 4, 4, 4, 4, 2, 2, 2]
    assert row("empty record") == [1, 0, 0, 0, 0, 0, 0, 4, 0, 0, 0, 4, 0, 0]
    assert row("empty record, empty molecule") == [1, 0, 0, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0, 0]
    assert row("an atom on the unbonded annotated atom") == [1, 0, 0, 0, 0, 0, 4, 5, 4, 4, 4, 5, 4, 4]
    assert row("unknown element") == [1, 0, 0, 0, 0, 1, 2, 2, 2, 1, 1, 1, 1, 1]
    # radius 0: of the tie case only (50,50) is located; radius 1: (10,5) <-> row 0 and (30,30) <-> row 2, never rows 1 / (32,30)
    assert row("ties in both directions") == ([1, 0, 0, 0, 0, 0, 4, 4, 3, 3, 2, 3, 1, 1] if radius else [1, 0, 0, 0, 0, 0, 4, 4, 1, 1, 2, 3, 0, 0])
    # the lower record index owns the shared cell: atom 2 is never located, its bond never paired
    assert row("two annotated atoms in one cell") == [1, 0, 0, 0, 0, 0, 4, 3, 3, 3, 2, 2, 1, 1]


def _grid_case(seed):
    """256 annotated atoms on a 16 x 16 grid of pitch 5 with 256 bonds, against 300 molecule atoms: the grid in another order,
    moved by up to two cells, and 44 strays"""
    rng = np.random.RandomState(seed)
    cell = [(5 + 5 * i, 5 + 5 * j) for i in range(16) for j in range(16)]
    rec_atoms = [(x, y, int(rng.randint(1, 14)), int(rng.choice([0, 0, 1, -1]))) for x, y in cell]
    pairs = [(16 * i + j, 16 * i + j + 1) for i in range(16) for j in range(15)] + [(16 * i, 16 * i + 16) for i in range(15)] + [(15, 31)]
    rec_bonds = [(i, j, int(rng.randint(1, 7))) for i, j in pairs]
    assert len(rec_atoms) == 256 and len(rec_bonds) == 256
    perm = rng.permutation(300)                                         # molecule row of grid atom k: perm[k]; strays: perm[256:]
    matoms = [None] * 300
    for k, (x, y, e, c) in enumerate(rec_atoms):
        dx, dy = (int(v) for v in rng.choice([0, 0, 0, 1, -1, 2, -2], size=2))
        e2 = e if rng.rand() < 0.9 else int(rng.randint(0, 14))
        matoms[perm[k]] = (x + dx, y + dy, e2, c if rng.rand() < 0.9 else 0)
    for r in perm[256:]:
        matoms[r] = (int(rng.randint(0, 90)), int(rng.randint(0, 90)), 1, 0)
    mbonds = []
    for i, j, code in rec_bonds:
        if rng.rand() < 0.05:
            continue
        e = (int(perm[i]) + 1, int(perm[j]) + 1)
        mbonds.append((e if rng.rand() < 0.5 else e[::-1]) + (code if rng.rand() < 0.9 else 1 + code % 6,))
    for _ in range(40):
        i, j = (int(v) for v in rng.choice(300, size=2, replace=False))
        mbonds.append((i + 1, j + 1, 1))
    return _mol(matoms, mbonds), (rec_atoms, rec_bonds)


@pytest.mark.parametrize("radius", [0, 1, 2])
def test_strided_loops_on_a_perturbed_grid(radius):
    """more atoms and bonds than the workgroup has threads, two images"""
    cases = [_grid_case(11), _grid_case(12)]
    mols, recs = [m for m, _ in cases], [r for _, r in cases]
    assert all(len(m["atoms"]) == 300 and len(m["bonds"]) > 256 for m in mols)
    gs = _score(mols, recs, radius, cap_atoms=320, cap_mol_bonds=320, max_atoms=256, max_bonds=256)
    gs.run()
    torch.cuda.synchronize()
    rows = gs.result()["rows"]
    ref = go.rows([_for_oracle(m) for m in mols], recs, radius)
    print(radius, rows.tolist())
    assert rows.tolist() == ref.tolist()
    located = rows[:, COL["atoms_located"]]
    assert (located > 0).all() and (located < 256).all() and (rows[:, COL["bonds_matched"]] < rows[:, COL["bonds_paired"]]).all()


def test_n_valid_totals_and_reset():
    cases = _cases()[:8]
    mols, recs = [m for _, m, _ in cases], [r for _, _, r in cases]
    nv = torch.full((1,), 5, dtype=torch.int32, device=DEV)
    gs = _score(mols, recs, 1, n_valid=nv)
    gs.rows.fill_(9)                                                  # (overwritten by every call, the rows past n_valid too)
    ref = go.rows([_for_oracle(m) for m in mols], recs, 1, n_valid=5)
    assert (ref[5:] == 0).all() and ref[:5, 0].tolist() == [1] * 5
    for call in (1, 2, 3):
        gs.run()
        torch.cuda.synchronize()
        res = gs.result()
        assert res["rows"].tolist() == ref.tolist()
        assert [res[c] for c in go.COLUMNS] == (call * ref.sum(0)).tolist()
    assert res["counted"] == 15 and res["share_exact"] == res["exact"] / 15
    assert res["share_atoms"] == res["atoms_matched"] / res["atoms_true"] and res["share_bonds"] == res["bonds_matched"] / res["bonds_true"]
    # n_valid is read on the device: another value, the same descriptor; out-of-range values are clamped
    for n, counted in ((8, 8), (0, 0), (-3, 0), (99, 8)):
        gs.reset()
        nv.fill_(n)
        gs.run()
        torch.cuda.synchronize()
        res = gs.result()
        assert res["counted"] == counted and res["rows"].tolist() == go.rows([_for_oracle(m) for m in mols], recs, 1, n_valid=counted).tolist()
    gs.reset()
    res = gs.result()
    assert all(res[c] == 0 for c in go.COLUMNS) and np.isnan(res["share_exact"])


def test_load_pads_and_refuses():
    mols = [_edit()] * 4
    gs = _score(mols, [REC, REC], 0, max_atoms=8, max_bonds=4)        # two records for four images: the others are empty
    gs.run()
    torch.cuda.synchronize()
    assert gs.result()["rows"].tolist() == go.rows([_for_oracle(m) for m in mols], [REC, REC], 0).tolist()
    a, q = np.array(REC[0], dtype=np.int32), np.array(REC[1], dtype=np.int32)
    for bad in ([(np.zeros((9, 4), np.int32), q)], [(a, np.concatenate([q, q]))], [(a, q)] * 5, [(a[:, :3], q)], [(a, q[:, :2])],
                [(a, np.array([[1, 0, 1]], np.int32))], [(a, np.array([[0, 5, 1]], np.int32))], [(a, np.array([[2, 2, 1]], np.int32))]):
        with pytest.raises(ValueError):
            gs.load(bad)
    gs.reset()
    gs.run()                                                            # the refused loads left the staged records alone
    torch.cuda.synchronize()
    assert gs.result()["exact"] == 2
    with pytest.raises(L.AbcNetHipError):
        GraphScore(*(t.cpu() for t in _upload(mols, 32, 64)))
    with pytest.raises(L.AbcNetHipError):
        GraphScore(*(t.long() for t in _upload(mols, 32, 64)))


# --------------------------------------------------------------------------------------------------------- device closed loop
def test_device_closed_loop_equals_the_cpu_chain():
    """annotation records -> TargetRasterizer -> ideal logits (torch ops) -> nms_peaks -> PeakExtractor -> GraphAssembler -> GraphScore
    on the six molecules of the host test: the rows of the CPU chain through the oracles"""
    notes, records, _mols, want = go.closed_loop()
    B, h = len(notes), go.CLOSED_LOOP["size"] // 4
    rz = TargetRasterizer(B, h, max_atoms=64, max_bonds=64)
    rz.load([parse_record(a, q, h=h) for a, q in notes])
    lg = [t.contiguous() for t in go.ideal_logits(rz.run())]
    am, bm, _rho, _om = nms_peaks(lg[0], lg[4], lg[6], lg[7])
    ex = PeakExtractor(lg, am, bm, cap_atoms=512, cap_bonds=16384)
    ex.run()
    asm = GraphAssembler.from_extractor(ex, cap_mol_bonds=2048)
    asm.run()
    gs = GraphScore.from_assembler(asm, max_atoms=64, max_bonds=64, radius=0)
    gs.load([parse_graph(a, q, h=h) for a, q in notes])
    gs.run()
    torch.cuda.synchronize()
    res = gs.result()
    assert res["rows"].tolist() == want.tolist()
    assert res["exact"] == int(want[:, COL["exact"]].sum()) >= 1 and res["counted"] == B
    # and the oracle on the device's own molecules says the same
    assert go.rows(asm.molecules(), records, 0).tolist() == want.tolist()


# ------------------------------------------------------------------------------------------------------------------ the runner
def test_runner_scores_its_own_molecules(golden_dir):
    """batch 4 at 96 x 96 -- drawn_molecules has one atom and no bond at 64, and an 80 x 80 input has a 20 x 20 map, no multiple
    of the 32-pixel groups of SampleBuilder's sparse rasteriser -- a short batch of 3 through SampleBuilder, three steps (eager,
    capture + replay, replay).  Weights: the trained fixture."""
    from abcnet_amd.augment import SampleBuilder, draw_augment
    from abcnet_amd.infer import InferenceRunner
    B, S, n, radius = 4, 96, 3, 1
    h = S // 4
    m = trained_unet(golden_dir)
    plain = InferenceRunner(m, B, S, S, use_graph=True, assemble=True, evaluate=True)
    assert plain.scorer is None and "molecules" not in plain.evaluation()
    with pytest.raises(L.AbcNetHipError):
        plain.load_graphs([])
    run = InferenceRunner(m, B, S, S, use_graph=True, assemble=True, evaluate=True, score_graphs=True, score_radius=radius)
    assert run.scorer.radius == radius and run.scorer.keep[3] is run.n_valid
    sb = SampleBuilder(run, amount=0.1, max_src=(S, S), sparse=True, max_atoms=64, max_bonds=64)
    with pytest.raises(L.AbcNetHipError, match="no graph records"):
        run.step()
    total = np.zeros(len(go.COLUMNS), dtype=np.int64)
    some_molecule = False
    for step in range(3):
        x, notes = drawn_molecules(n, S, seed=40 + step)
        assert all(q for _, q in notes)                                # every drawing has bonds at this size
        srcs = [((1.0 - x[b, 0].numpy()) * 255).astype(np.uint8) for b in range(n)]       # dark ink on white
        rs_a, rs_b = np.random.RandomState(step), np.random.RandomState(step)
        sb.load(srcs, [a for a, _ in notes], [q for _, q in notes], rs_a)
        sb.run()
        run.step()
        torch.cuda.synchronize()
        graphs = [parse_graph(a, q, *draw_augment(rs_b, 0.1, srcs[b].shape, S)[1], h=h) for b, (a, q) in enumerate(notes)]
        assert all(len(q) > 0 for _, q in graphs) and int(run.n_valid) == n
        mols = run.molecules()
        some_molecule |= any(mol is not None for mol in mols[:n])
        want = go.rows(mols, graphs, radius, n_valid=n)
        res = run.evaluation()["molecules"]
        print(step, [None if mol is None else (len(mol.symbols), len(mol.bonds)) for mol in mols], res["rows"].tolist())
        assert res["rows"].tolist() == want.tolist(), step
        total += want.sum(0)
        assert [res[c] for c in go.COLUMNS] == total.tolist(), step
    assert run._graph is not None and total[COL["counted"]] == 3 * n
    assert some_molecule, "every molecule of every step is None: the score of these weights says nothing"
    run.reset_evaluation()
    res = run.evaluation()
    assert all(res["molecules"][c] == 0 for c in go.COLUMNS) and sum(res[k].sum() for k in ("atom_type", "bond_type")) == 0
