"""GPU parity of the extractor's omega rule (abc_extract_desc.omega_rule through ops.PeakExtractor / InferenceRunner): rule
"peaks" -- the candidates img2smiles.py:139 and img2smiles3.py:140 walk -- against the lists the reference text produced
(tests/golden/decode3_128.npz) and the oracle (tests/extract_rule_oracle.py), bit for bit; rule "raw" against today's oracle."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import abcnet_amd  # noqa: E402,F401
from abcnet_amd import _lib as L  # noqa: E402
from abcnet_amd.ops import PeakExtractor, nms_peaks  # noqa: E402
from abcnet_amd.synthetic import correlated_logits, synthetic_images, synthetic_targets  # noqa: E402
from oracle import decode_oracle  # noqa: E402
import assemble_oracle as ao  # noqa: E402
import extract_rule_oracle as ero  # noqa: E402

DEV = "cuda"
HEADS = [1, 14, 3, 2, 1, 360, 60, 60]


def _run(lg, rule, **caps):
    d = [t.to(DEV).contiguous() for t in lg]
    am, bm, rho, om = nms_peaks(d[0], d[4], d[6], d[7])
    ex = PeakExtractor(d, am, bm, omega_rule=rule, **caps)
    assert ex.omega_rule == rule
    ex.run()
    torch.cuda.synchronize()
    return ex.lists(), (am.cpu(), bm.cpu(), rho.cpu(), om.cpu())


def _oracle(lg, nms, j, rule, **kw):
    am, bm, rho, _ = nms
    return ero.extract(am[j, 0], bm[j, 0], lg[1][j], lg[2][j], lg[3][j], lg[5][j], rho[j], lg[7][j], rule, **kw)


def _same_lists(g, want, what=""):
    atoms, bonds, rhos = want
    assert torch.equal(g["atoms"].long(), atoms), what
    assert torch.equal(g["bonds"].long(), bonds), what
    assert torch.equal(g["rho"], rhos), what
    assert g["counts"][1] == len(atoms) and g["counts"][3] == len(bonds), what


def _same_golden(g, gold, p):
    assert np.array_equal(g["atoms"].numpy(), gold[p + "atoms"]), p
    assert np.array_equal(g["bonds"][:, :2].numpy(), gold[p + "bond_pos"]), p
    assert np.array_equal(g["bonds"][:, 2].numpy(), gold[p + "bond_bin"]) and np.array_equal(g["bonds"][:, 3].numpy(), gold[p + "bond_type"]), p
    assert np.array_equal(g["rho"].numpy(), gold[p + "bond_rho"]), p
    omega = g["bonds"][:, 2].numpy().astype(np.float64) * (np.pi / 30) + np.pi / 60 - np.pi / 2
    r = g["rho"].numpy().astype(np.float64)
    assert np.array_equal(np.stack([r * np.cos(omega), r * np.sin(omega)], 1).reshape(-1, 2), gold[p + "bond_delta"]), p


def test_peak_rule_matches_golden_and_oracle(golden_dir):
    """the seeded maps of decode_128.npz, and the hand-made omega rows (bins 0 / 29 / 30 / 59, the wrap between 59 and 0, a plateau,
    -1 exactly and just above, a peak of exactly 0, an all-equal row, peaks that lose to or tie with their opposite, no peak above -1)
    at bond peaks of a 2 x 32 x 32 map"""
    gold = np.load(os.path.join(golden_dir, "decode3_128.npz"))
    tg = synthetic_targets(2, 128, seed=3)
    seeded = correlated_logits(tg, seed=29, centre_noise=0.5)
    for tag, lg in (("s", seeded), ("h", ero.hand_made_maps(gold, 32))):
        got, nms = _run(lg, "peaks")
        for j in range(2):
            assert not got[j]["truncated"]
            _same_golden(got[j], gold, "%s%d_" % (tag, j))
            _same_lists(got[j], _oracle(lg, nms, j, "peaks"), (tag, j))
    assert got[1]["counts"][2] == 1 and got[1]["counts"][3] == 0        # a bond peak without a candidate


@pytest.fixture(scope="module")
def odd_maps():
    """seeded noise at 3 x 40 x 24, every map quantised to quarters: ties between neighbouring bins, plateaus and exact zeros"""
    g = torch.Generator().manual_seed(53)
    return [torch.round(torch.randn((3, c, 40, 24), generator=g) * 2 * 4) / 4 for c in HEADS]


@pytest.mark.parametrize("rule", ["raw", "peaks"])
def test_odd_shape_both_rules(odd_maps, rule):
    got, nms = _run(odd_maps, rule, cap_atoms=2048, cap_bonds=65536)
    om = nms[3]
    assert (odd_maps[7] == 0).any() and int(nms[1].sum()) > 100
    for j in range(3):
        g = got[j]
        assert not g["truncated"], g["counts"]
        _same_lists(g, _oracle(odd_maps, nms, j, rule), (rule, j))
        assert len(g["bonds"]) > 0
        if rule == "peaks":      # a subset of the NMS kernel's omega mask at the same pixels, bit for bit
            b = g["bonds"].long()
            assert bool((om[j][b[:, 2], b[:, 0], b[:, 1]] == 1).all())
    if rule == "raw":
        want = [decode_oracle.extract(nms[0][j, 0], nms[1][j, 0], odd_maps[1][j], odd_maps[2][j], odd_maps[3][j], odd_maps[5][j], nms[2][j],
                                      odd_maps[7][j]) for j in range(3)]
        for j in range(3):
            _same_lists(got[j], want[j], j)


def test_dense_bond_peaks_past_the_limit_and_truncation():
    """every pixel of a 72 x 72 map is a bond peak (5184 > 4096): the candidates are those of the first 4096 peaks in raster order,
    counts[2] is the true number of peaks; with a small cap_bonds the list is the prefix and counts[3] still the true total"""
    g = torch.Generator().manual_seed(59)
    lg = [torch.round(torch.randn((1, c, 72, 72), generator=g) * 2 * 4) / 4 for c in HEADS]
    lg[4].fill_(0.0)
    got, nms = _run(lg, "peaks", cap_atoms=2048, cap_bonds=65536)
    assert int(nms[1].sum()) == 72 * 72
    want = _oracle(lg, nms, 0, "peaks", max_bond_peaks=4096)
    g0 = got[0]
    assert g0["counts"][2] == 72 * 72 and g0["truncated"]
    assert len(want[1]) < 65536
    _same_lists(g0, want, "dense")
    small, _ = _run(lg, "peaks", cap_atoms=2048, cap_bonds=64)
    s0 = small[0]
    assert s0["truncated"] and len(s0["bonds"]) == 64
    assert torch.equal(s0["bonds"].long(), want[1][:64]) and torch.equal(s0["rho"], want[2][:64])
    assert s0["counts"][3] == len(want[1]) and s0["counts"][2] == 72 * 72


def _runner_maps(run):
    """the maps a decode-mode runner holds, in the oracle's form: the bond-type planes as the one-hot of the stored arg-max map"""
    lg = [None if t is None else t.cpu() for t in run.logits]
    B, _, h, w = lg[7].shape
    lg[5] = torch.nn.functional.one_hot(run.btype_idx.cpu().long(), 6).permute(0, 4, 1, 2, 3).reshape(B, 360, h, w).float()
    return lg, (run.atom_mask.cpu(), run.bond_mask.cpu(), run.rho_abs.cpu(), run.omega_mask.cpu())


def _mol(o):
    from abcnet_amd.decode import Molecule
    if o is None:
        return None
    return Molecule(o["symbols"], o["charges"], o["hs"], o["positions"], o["bonds"], o["orders"], o["implicit_hs"], o["sources"], o["truncated"])


def test_inference_runner_with_either_rule():
    """decode-mode runners with assembly, one per rule, on the same seeded model and input: candidates() == the oracle of the rule on
    the runner's own masks and maps, molecules() == the assembly oracle on those candidates"""
    from abcnet_amd.infer import InferenceRunner
    from abcnet_amd.unet import UNet
    from oracle import unet_oracle as uo
    m = UNet(1, uo.HEADS, dtype="bf16")
    m.load_state_dict(uo.filled_state("unet", 1, uo.HEADS, seed=0))
    m = m.to(DEV)
    x = synthetic_images(2, 64, seed=7).to(DEV)
    total = {}
    for rule in ("peaks", "raw"):
        run = InferenceRunner(m, 2, 64, 64, decode=True, assemble=True, omega_rule=rule)
        assert run.omega_rule == rule and run.extractor.omega_rule == rule and run.decode
        run.load_batch(x)
        run.step()
        run.step()
        torch.cuda.synchronize()
        lists, mols = run.candidates(), run.molecules()
        lg, nms = _runner_maps(run)
        for j in range(2):
            _same_lists(lists[j], _oracle(lg, nms, j, rule), (rule, j))
            if rule == "raw":
                _same_lists(lists[j], decode_oracle.extract(nms[0][j, 0], nms[1][j, 0], lg[1][j], lg[2][j], lg[3][j], lg[5][j], nms[2][j],
                                                            lg[7][j]), j)
            l = lists[j]
            want = _mol(ao.assemble_counts(l["counts"], l["atoms"].numpy(), l["bonds"].numpy(), l["rho"].numpy(), run.extractor.cap_atoms,
                                           run.extractor.cap_bonds, run.assembler.cap_mol_bonds, vectorised=True))
            assert (mols[j] is None) == (want is None), (rule, j)
            if want is not None:
                assert mols[j] == want and mols[j].sources == want.sources and mols[j].truncated == want.truncated, (rule, j)
        total[rule] = sum(len(l["bonds"]) for l in lists)
    assert total["peaks"] > 0 and total["raw"] > 0


def test_unknown_rule_and_cpu_tensors_fail_loudly():
    tg = synthetic_targets(1, 32, seed=5)
    lg = correlated_logits(tg, seed=31)
    d = [t.to(DEV).contiguous() for t in lg]
    am, bm, _, _ = nms_peaks(d[0], d[4], d[6], d[7])
    with pytest.raises(ValueError, match="omega_rule"):
        PeakExtractor(d, am, bm, omega_rule="mask")
    with pytest.raises(L.AbcNetHipError):
        PeakExtractor(lg, lg[0], lg[4], omega_rule="peaks")
    ex = PeakExtractor(d, am, bm, omega_rule="peaks")
    ex.d.omega_rule = 2
    with pytest.raises(L.AbcNetHipError, match="omega_rule"):
        ex.run()
