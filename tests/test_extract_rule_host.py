"""CPU side of the extractor's omega rule (abc_extract_desc.omega_rule, ops.PeakExtractor(omega_rule=...)): the oracle of both
rules against the lists the reference text itself produced (img2smiles3.py:63-81,114-194: tests/golden/decode3_128.npz, written by
tests/golden/make_golden_decode3.py), the conditions that golden has to meet, the binding, and the refusals that come before
the device is touched."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import abcnet_amd  # noqa: E402,F401
from abcnet_amd import _lib as L  # noqa: E402
from abcnet_amd.synthetic import correlated_logits, synthetic_targets  # noqa: E402
from oracle import decode_oracle, nms_oracle  # noqa: E402
import extract_rule_oracle as ero  # noqa: E402

# the candidate bins every hand-made row has to give under the peak rule
HAND_EXPECT = {"bin_0": [0], "bin_29": [29], "bin_30": [30], "bin_59": [59], "wrap_59_over_0": [59], "wrap_0_over_59": [0],
               "plateau": [10, 11], "minus_one": [20], "zero_peak": [7], "all_equal": list(range(30)), "loses_to_opposite": [40],
               "tie_with_opposite": [15], "no_candidate": []}


@pytest.fixture(scope="module")
def gold(golden_dir):
    return dict(np.load(os.path.join(golden_dir, "decode3_128.npz")))


@pytest.fixture(scope="module")
def seeded():
    tg = synthetic_targets(2, 128, seed=3)
    lg = correlated_logits(tg, seed=29, centre_noise=0.5)
    return lg, nms_oracle.nms(lg[0], lg[4], lg[6], lg[7])


def _extract(lg, nms, j, rule, **kw):
    am, bm, rho, _ = nms
    return ero.extract(am[j, 0], bm[j, 0], lg[1][j], lg[2][j], lg[3][j], lg[5][j], rho[j], lg[7][j], rule, **kw)


def _check_image(gold, p, atoms, bonds, rhos):
    assert np.array_equal(atoms.numpy(), gold[p + "atoms"])
    assert np.array_equal(bonds[:, :2].numpy(), gold[p + "bond_pos"]) and np.array_equal(bonds[:, 2].numpy(), gold[p + "bond_bin"])
    assert np.array_equal(bonds[:, 3].numpy(), gold[p + "bond_type"])
    assert np.array_equal(rhos.numpy(), gold[p + "bond_rho"])
    # the reference's bonds_delta_list (img2smiles3.py:161-165), bit for bit
    omega = bonds[:, 2].numpy().astype(np.float64) * (np.pi / 30) + np.pi / 60 - np.pi / 2
    r = rhos.numpy().astype(np.float64)
    assert np.array_equal(np.stack([r * np.cos(omega), r * np.sin(omega)], 1).reshape(-1, 2), gold[p + "bond_delta"])


def test_oracle_matches_the_reference_lists_on_the_seeded_maps(gold, seeded, golden_dir):
    lg, nms = seeded
    gold2 = np.load(os.path.join(golden_dir, "decode_128.npz"))
    for j in range(2):
        assert np.array_equal(gold["s%d_atoms" % j], gold2["atoms%d" % j])          # the maps of decode_128.npz
        _check_image(gold, "s%d_" % j, *_extract(lg, nms, j, "peaks"))


def test_oracle_matches_the_reference_lists_on_the_hand_made_rows(gold):
    lg = ero.hand_made_maps(gold, 32)
    nms = nms_oracle.nms(lg[0], lg[4], lg[6], lg[7])
    assert int(nms[1].sum()) == len(gold["hand_names"])
    for j in range(2):
        _check_image(gold, "h%d_" % j, *_extract(lg, nms, j, "peaks"))


def test_raw_rule_is_the_decode_oracle(seeded):
    lg, (am, bm, rho, _) = seeded
    for j in range(2):
        want = decode_oracle.extract(am[j, 0], bm[j, 0], lg[1][j], lg[2][j], lg[3][j], lg[5][j], rho[j], lg[7][j])
        for got in (_extract(lg, seeded[1], j, "raw"), _extract(lg, seeded[1], j, "raw", max_bond_peaks=1 << 20)):
            assert all(torch.equal(a, b) for a, b in zip(got, want))
    with pytest.raises(ValueError, match="omega_rule"):
        _extract(lg, seeded[1], 0, "mask")


def test_golden_meets_its_conditions(gold, seeded):
    lg, (am, bm, rho, _) = seeded
    for j in range(2):
        peaks = bm[j, 0].nonzero(as_tuple=False).tolist()
        differ = sum(ero.kept_bins(lg[7][j, :, x, y].tolist(), "raw") != ero.kept_bins(lg[7][j, :, x, y].tolist(), "peaks") for x, y in peaks)
        assert differ >= 1 and differ == int(gold["s%d_differ" % j])        # the two rules part on every seeded image
        assert len(peaks) > 0 and len(gold["s%d_bond_bin" % j]) > 0          # and the peak rule leaves candidates
    names = gold["hand_names"].tolist()
    assert set(names) == set(HAND_EXPECT)
    rows = {n: gold["hand_omega"][i].tolist() for i, n in enumerate(names)}
    for i, name in enumerate(names):
        b, x, y = gold["hand_bond_pos"][i].tolist()
        assert max(x, y) < 32
        at = (gold["h%d_bond_pos" % b] == [x, y]).all(1)
        assert gold["h%d_bond_bin" % b][at].tolist() == HAND_EXPECT[name], name          # what the reference text gave
    assert {0, 29, 30, 59} <= set(gold["h0_bond_bin"].tolist())
    assert ero.omega_peak_bins(rows["plateau"]) == [10, 11] and rows["plateau"][10] == rows["plateau"][11]
    v = gold["hand_omega"][names.index("minus_one")]
    assert v[5] == np.float32(-1.0) and v[20] == np.nextafter(np.float32(-1.0), np.float32(0.0))
    assert v[4] < v[5] > v[6] and ero.omega_peak_bins(v.tolist()) == [20]
    assert rows["zero_peak"][7] == 0.0 and ero.kept_bins(rows["zero_peak"], "peaks") == [7] and 7 not in ero.kept_bins(rows["zero_peak"], "raw")
    assert len(set(rows["all_equal"])) == 1 and ero.omega_peak_bins(rows["all_equal"]) == list(range(60))
    assert ero.kept_bins(rows["all_equal"], "peaks") == list(range(30))
    assert ero.omega_peak_bins(rows["loses_to_opposite"]) == [10, 40]
    assert ero.omega_peak_bins(rows["tie_with_opposite"]) == [15, 45]
    # an image with a bond peak and atoms but no candidate: the assembler's "no surviving candidate" input
    assert ero.omega_peak_bins(rows["no_candidate"]) == [] and max(rows["no_candidate"]) <= -1
    assert len(gold["h1_bond_bin"]) == 0 and len(gold["h1_atoms"]) > 0 and (gold["hand_bond_pos"][:, 0] == 1).sum() == 1


def test_extract_desc_carries_the_rule():
    names = [f[0] for f in L.ExtractDesc._fields_]
    assert names[-2:] == ["btype_idx", "omega_rule"] and dict(L.ExtractDesc._fields_)["omega_rule"] is C.c_int32
    assert (L.OMEGA_RAW, L.OMEGA_PEAKS) == (0, 1) and L.ExtractDesc().omega_rule == L.OMEGA_RAW
    assert L._STRUCTS.index(L.ExtractDesc) == 17
    assert L.load().abc_sizeof(17) == C.sizeof(L.ExtractDesc)
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "abcnet_hip.h")).read()
    assert "enum abc_omega_rule { ABC_OMEGA_RAW = 0, ABC_OMEGA_PEAKS = 1 }" in hdr


def test_launcher_refuses_an_unknown_rule_on_the_host():
    lib = L.load()
    d = L.ExtractDesc()
    for f in ("atom_mask", "bond_mask", "types", "charges", "hs", "btypes", "rho", "omega", "counts", "atoms", "bonds", "bond_rho", "work",
              "work_masks"):
        setattr(d, f, 256)                              # never dereferenced: the refusal comes first
    d.B, d.h, d.w, d.cap_atoms, d.cap_bonds = 2, 32, 32, 512, 16384
    for rule in (2, -1, 7):
        d.omega_rule = rule
        assert lib.abc_extract_peaks(C.byref(d), None) == -1, rule          # ABC_EINVAL, before any launch
        assert b"omega_rule" in lib.abc_last_error()


def test_python_refuses_an_unknown_rule_name():
    from abcnet_amd.infer import InferenceRunner
    from abcnet_amd.ops import OMEGA_RULES, PeakExtractor
    from abcnet_amd.unet import UNet
    assert OMEGA_RULES == {"raw": 0, "peaks": 1}
    lg = [torch.zeros(1, c, 8, 8) for c in (1, 14, 3, 2, 1, 360, 60, 60)]
    for bad in ("mask", "PEAKS", 1, None):
        with pytest.raises(ValueError, match="omega_rule"):
            PeakExtractor(lg, lg[0], lg[4], omega_rule=bad)
        with pytest.raises(ValueError, match="omega_rule"):
            InferenceRunner(UNet(1, [1, 14, 3, 2, 1, 360, 60, 60]), 2, 64, 64, extract=True, omega_rule=bad)
