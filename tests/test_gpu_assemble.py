"""GPU parity: device-side graph assembly (abc_assemble_graphs, through the C ABI) against the molecules produced by the
reference text itself (img2smiles2.py:193-311, tests/golden/assemble_128.npz) and against the oracle (tests/assemble_oracle.py,
pinned to those goldens) -- exact: integer work plus float64 decisions that are reproducible bit for bit.  No tolerance anywhere."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import abcnet_amd  # noqa: E402,F401
from abcnet_amd.decode import Molecule  # noqa: E402
from abcnet_amd.ops import GraphAssembler, PeakExtractor, nms_peaks  # noqa: E402
from abcnet_amd.synthetic import correlated_logits, drawn_molecules, synthetic_images, synthetic_targets  # noqa: E402
import assemble_oracle as ao  # noqa: E402
from molrows import assemble_golden, filled_unet, trained_unet  # noqa: E402

DEV = "cuda"


def _upload(lists, cap_atoms, cap_bonds, counts=None):
    """hand-made lists [(atoms [n,5], bonds [m,4], rho [m])] as device tensors of the extractor's layout"""
    B = len(lists)
    cnt = torch.zeros(B, 4, dtype=torch.int32)
    atoms, bonds = torch.zeros(B, cap_atoms, 5, dtype=torch.int32), torch.zeros(B, cap_bonds, 4, dtype=torch.int32)
    rho = torch.zeros(B, cap_bonds, dtype=torch.float32)
    for b, (a, c, r) in enumerate(lists):
        n, m = len(a), len(c)
        atoms[b, :n] = torch.as_tensor(np.asarray(a).reshape(-1, 5), dtype=torch.int32)
        bonds[b, :m] = torch.as_tensor(np.asarray(c).reshape(-1, 4), dtype=torch.int32)
        rho[b, :m] = torch.as_tensor(np.asarray(r, dtype=np.float32))
        cnt[b] = torch.tensor([n, n, max(m, 1), m] if counts is None else counts[b], dtype=torch.int32)
    return cnt.to(DEV), atoms.to(DEV), bonds.to(DEV), rho.to(DEV)


def _mol(o):
    """the oracle's dict as a Molecule (None stays None)"""
    if o is None:
        return None
    return Molecule(o["symbols"], o["charges"], o["hs"], o["positions"], o["bonds"], o["orders"], o["implicit_hs"], o["sources"], o["truncated"])


def _same(got, want, what=""):
    assert (got is None) == (want is None), what
    if want is not None:
        assert got == want and got.sources == want.sources and got.truncated == want.truncated, what


def test_every_golden_case_on_the_device(golden_dir):
    cases = assemble_golden(golden_dir)
    asm = GraphAssembler(*_upload([(c["atoms"], c["bonds"], c["rho"]) for _, c in cases], 128, 2048))
    asm.run()
    torch.cuda.synchronize()
    mols = asm.molecules()
    cnt = asm.mol_counts.cpu().numpy()
    for b, (name, c) in enumerate(cases):
        m = mols[b]
        assert m is not None and not m.truncated, name
        assert cnt[b].tolist() == [len(c["symbols"]), len(c["bond2atom_index_final"]), len(c["atom_implicit_hs_list"]), 0], name
        assert m.symbols == c["symbols"].tolist() and m.charges == c["charges"].tolist() and m.hs == c["hs"].tolist(), name
        assert m.positions == c["positions"].tolist(), name
        assert m.bonds == c["bond2atom_index_final"].tolist() and m.orders == c["bonds_property_list_final"].tolist(), name
        assert m.implicit_hs == c["atom_implicit_hs_list"].tolist(), name
        assert m.molblock() == str(c["molblock"]), name
        # which candidate every bond came from: the arg-min arrays of the reference, seen through the edge filter
        i1, i2 = c["atom_index1"], c["atom_index2"]
        first = {}
        for i in range(len(i1)):
            if i1[i] != i2[i]:
                first.setdefault((min(i1[i], i2[i]), max(i1[i], i2[i])), i)
        assert m.sources == sorted(first.values()), name


def test_bond_peaks_without_a_surviving_candidate_give_an_empty_molecule():
    """the one input the reference does not define (its np.flip raises on the empty array): bond peaks exist, no candidate survived
    the bin rule.  Here: zero atoms, zero bonds, not None -- the same as "no bond survives the edge filter".  Checked against the
    oracle only; beside it an image without atom peaks and one without bond peaks (both None)."""
    a = np.array([[10, 10, 1, 0, 0], [30, 30, 2, 0, 1]])
    none = (np.zeros((0, 4)), np.zeros(0))
    lists = [(a, *none), (a, *none), (np.zeros((0, 5)), np.array([[20, 20, 7, 0]]), np.array([5.0]))]
    counts = [[2, 2, 3, 0], [2, 2, 0, 0], [0, 0, 1, 1]]
    asm = GraphAssembler(*_upload(lists, 8, 8, counts))
    asm.run()
    torch.cuda.synchronize()
    mols = asm.molecules()
    want = [_mol(ao.assemble_counts(counts[b], *lists[b], 8, 8, 8)) for b in range(3)]
    assert want[0] is not None and want[0].symbols == [] and want[0].bonds == [] and want[1] is None and want[2] is None
    for b in range(3):
        _same(mols[b], want[b], b)
    assert mols[0].molblock() == Molecule([], [], [], [], [], [], []).molblock()
    assert asm.mol_counts.cpu()[:, 3].tolist() == [0, ao.EMPTY, ao.EMPTY]


def _extract(lg, **caps):
    d = [t.to(DEV).contiguous() for t in lg]
    am, bm, _rho, _om = nms_peaks(d[0], d[4], d[6], d[7])
    ex = PeakExtractor(d, am, bm, **caps)
    ex.run()
    return ex


def _oracle_on_lists(lists, cap_atoms, cap_bonds, cap_mol_bonds):
    return [_mol(ao.assemble_counts(l["counts"], l["atoms"].numpy(), l["bonds"].numpy(), l["rho"].numpy(), cap_atoms, cap_bonds,
                                    cap_mol_bonds, vectorised=True)) for l in lists]


@pytest.mark.parametrize("B,h,noise", [(1, 32, 0.5), (3, 96, 1.5), (2, 128, 2.5)])
def test_extractor_to_assembler_other_shapes_and_dense_peaks(B, h, noise):
    """the inputs of test_extract_other_shapes_and_dense_peaks: an image with no atom peak (None), rows of zero omega logits, noisy maps
    with hundreds to thousands of atoms and tens of thousands of candidates; the oracle runs on the extractor's own lists"""
    tg = synthetic_targets(B, h, seed=5)
    lg = correlated_logits(tg, seed=31, centre_noise=noise)
    lg[0][0].fill_(-5.0)
    lg[7][:, :, ::3, :] = 0.0
    ex = _extract(lg, cap_atoms=2048, cap_bonds=65536)
    asm = GraphAssembler.from_extractor(ex, cap_mol_bonds=65536)
    asm.run()
    torch.cuda.synchronize()
    mols, lists = asm.molecules(), ex.lists()
    want = _oracle_on_lists(lists, 2048, 65536, 65536)
    assert mols[0] is None and lists[0]["counts"][0] == 0
    for j in range(B):
        _same(mols[j], want[j], j)
        assert mols[j] is None or not mols[j].truncated, lists[j]["counts"]
    if B > 1:
        assert max(len(m.bonds) for m in mols if m is not None) > 100


def test_truncation_is_reported(golden_dir):
    tg = synthetic_targets(1, 64, seed=5)
    lg = correlated_logits(tg, seed=31, centre_noise=2.5)
    ex = _extract(lg, cap_atoms=8, cap_bonds=16)
    asm = GraphAssembler.from_extractor(ex)
    asm.run()
    torch.cuda.synchronize()
    m, l = asm.molecules()[0], ex.lists()[0]
    assert l["truncated"] and m is not None and m.truncated
    # the molecule of the kept prefixes (the extractor's own test holds those prefixes to the reference's)
    _same(m, _oracle_on_lists([l], 8, 16, asm.cap_mol_bonds)[0])
    full = _extract(lg, cap_atoms=2048, cap_bonds=65536).lists()[0]
    assert torch.equal(l["atoms"], full["atoms"][:len(l["atoms"])]) and len(l["atoms"]) <= 8
    # cap_mol_bonds hit: the first bonds of the reference's list, and the flag
    c = dict(assemble_golden(golden_dir))["decode_128_image1"]
    asm = GraphAssembler(*_upload([(c["atoms"], c["bonds"], c["rho"])], 64, 2048), cap_mol_bonds=40)
    asm.run()
    torch.cuda.synchronize()
    m = asm.molecules()[0]
    assert m.truncated and len(m.bonds) == 40 and m.orders == c["bonds_property_list_final"].tolist()[:40]
    _same(m, _mol(ao.assemble_counts([54, 54, 1222, 1222], c["atoms"], c["bonds"], c["rho"], 64, 2048, 40)))


def _stage_by_stage(lists, cap_atoms, cap_bonds):
    """the candidate lists a runner returned, uploaded again and assembled by a launch of its own"""
    asm = GraphAssembler(*_upload([(l["atoms"], l["bonds"], l["rho"]) for l in lists], cap_atoms, cap_bonds,
                                  counts=[l["counts"] for l in lists]))
    asm.run()
    torch.cuda.synchronize()
    return asm.molecules()


def test_inference_runner_with_assembly():
    """eval forward + NMS + extraction + assembly in one captured graph, replayed == the stages run one by one; and assemble=True leaves
    the candidate lists and the masks bit-identical to a runner built without it"""
    from abcnet_amd.infer import InferenceRunner
    m = filled_unet(dropout_p=0.0)
    run = InferenceRunner(m, 2, 128, 128, use_graph=True, assemble=True)
    plain = InferenceRunner(m, 2, 128, 128, use_graph=True, extract=True)
    assert run.extractor is not None and plain.assembler is None
    with pytest.raises(Exception):
        plain.molecules()
    for seed in (7, 8, 9):
        x = synthetic_images(2, 128, seed=seed).to(DEV)
        for r in (run, plain):
            r.load_batch(x)
            r.step()
        torch.cuda.synchronize()
        got, lists, lists0 = run.molecules(), run.candidates(), plain.candidates()
        for a, b in zip(lists, lists0):
            assert torch.equal(a["atoms"], b["atoms"]) and torch.equal(a["bonds"], b["bonds"]) and torch.equal(a["rho"], b["rho"])
            assert a["counts"] == b["counts"]
        assert torch.equal(run.atom_mask, plain.atom_mask) and torch.equal(run.bond_mask, plain.bond_mask)
        assert torch.equal(run.rho_abs, plain.rho_abs) and torch.equal(run.omega_mask, plain.omega_mask)
        one_by_one = _stage_by_stage(lists, run.extractor.cap_atoms, run.extractor.cap_bonds)
        want = _oracle_on_lists(lists, run.extractor.cap_atoms, run.extractor.cap_bonds, run.assembler.cap_mol_bonds)
        for j in range(2):
            _same(got[j], one_by_one[j], (seed, j))
            _same(got[j], want[j], (seed, j))
    assert run._graph is not None


@pytest.mark.parametrize("fp8", [False, True])
def test_decode_and_fp8_runners_give_the_same_molecules(fp8):
    """the assembly reads lists, not maps: with decode=True (bf16 and e4m3 graphs) the molecules are those of the runner that stores
    every map, and both are the oracle's on the runner's own candidates"""
    from abcnet_amd.infer import InferenceRunner
    m = filled_unet("bf16")
    run = InferenceRunner(m, 2, 128, 128, use_graph=True, fold_bn=True, fp8=fp8, assemble=True)
    dec = InferenceRunner(m, 2, 128, 128, use_graph=True, fold_bn=True, fp8=fp8, assemble=True, decode=True)
    assert dec.decode and not run.decode
    for seed in (7, 8):
        x = synthetic_images(2, 128, seed=seed).to(DEV)
        for r in (run, dec):
            r.load_batch(x)
            r.step()
        torch.cuda.synchronize()
        got = run.molecules()
        want = _oracle_on_lists(run.candidates(), run.extractor.cap_atoms, run.extractor.cap_bonds, run.assembler.cap_mol_bonds)
        for j, (a, b) in enumerate(zip(got, dec.molecules())):
            _same(a, b, (seed, j))
            _same(a, want[j], (seed, j))


def test_trained_fixture_molecules_equal_the_oracle(golden_dir):
    """the frozen trained network on drawn molecules at 512 x 512 (what config 5 runs on in practice: clean peaks, a handful of
    candidates per bond): device molecules == oracle on the runner's own candidates.  How many graphs equal the drawn annotation
    is reported by profiles/tools/assemble_step.py, not asserted."""
    from abcnet_amd.infer import InferenceRunner
    m = trained_unet(golden_dir)
    B = 16
    x, _notes = drawn_molecules(B, 512, seed=777)
    run = InferenceRunner(m, B, 512, 512, use_graph=True, assemble=True)
    run.load_batch(x.to(DEV))
    for _ in range(2):                      # the second step is the graph replay
        run.step()
    torch.cuda.synchronize()
    got, lists = run.molecules(), run.candidates()
    want = _oracle_on_lists(lists, run.extractor.cap_atoms, run.extractor.cap_bonds, run.assembler.cap_mol_bonds)
    for j in range(B):
        _same(got[j], want[j], j)
    real = [g for g in got if g is not None]
    assert real and all(g.molblock().endswith("M  END\n$$$$") for g in real)
