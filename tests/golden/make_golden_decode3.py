"""Golden of the candidate extraction under the omega PEAK rule (needs the reference checkout: it reads the reference's text;
what it writes travels, the reference does not).

  decode3_128.npz   img2smiles3.py:63-81 (NMS and the circular 3-tap omega peak mask) and :114-194 (the candidate loops, which
                    walk `bond_omega_img2[:, x, y].nonzero()`, :140) executed from the reference text on
                      * the seeded head maps of decode_128.npz (2 x 128 x 128; the atom lists must equal that file's, which shows
                        the maps are the same), and
                      * hand-made omega rows, one per edge of the rule, placed at bond peaks inside the top-left 32 x 32 cells of a
                        2 x 128 x 128 map (the reference text hard-codes 128; tests/extract_rule_oracle.hand_made_maps rebuilds
                        the maps at any size from the stored rows).
                    Stored per image (s0, s1: seeded; h0, h1: hand-made): atoms (x, y, type, charge, hs), bond_pos, bond_type and
                    bond_delta exactly as the reference lists hold them, and bond_bin / bond_rho: the omega bin and |rho| of every
                    candidate, from tests/extract_rule_oracle.extract(..., "peaks") and checked here against the reference's lists
                    (positions and types equal, rho * cos / sin of the bin angle equal to bonds_delta_list bit for bit).  For the
                    hand-made cases also the inputs: hand_names, hand_bond_pos (image, x, y), hand_omega / hand_rho / hand_btypes
                    rows, hand_atom_pos and the atom-head rows.

The hand-made rows (baseline -3: below the mask's -1 threshold and non-zero):
  bin_0, bin_29, bin_30, bin_59   one peak at that bin: a surviving candidate at each
  wrap_59_over_0, wrap_0_over_59  bins 0 and 59 are neighbours: the lower of the two is no peak
  plateau                         two equal neighbouring maxima, both in the mask, both candidates
  minus_one                       a local maximum of exactly -1 (not in the mask) and one just above -1 (a candidate)
  zero_peak                       a peak of exactly 0: a candidate under this rule, skipped by img2smiles2.py's `.nonzero()`
  all_equal                       every bin is a peak; bins 0..29 survive the opposite test (`<`), bins 30..59 do not (`<=`): 30
  loses_to_opposite               a peak in the mask whose opposite direction is higher: only the opposite one is a candidate
  tie_with_opposite               a peak at bin 45 equal to its opposite bin 15: 15 stays (`<`), 45 goes (`<=`)
  no_candidate (alone in image 1) local maxima at -2, none above -1: the mask is empty, so the image has a bond peak and no
                                  candidate -- the assembler's "bond peaks without a surviving candidate" input.
A row whose mask is NOT empty always keeps a candidate, so "no candidate" can only be made with an empty mask: a global maximum
M > -1 is in the mask; if some global maximum lies in bins 0..29 it survives (`<` against values that are not larger); otherwise
all of them lie in 30..59, and one of them is dropped only by an opposite bin of the same value -- bins 31..59 have their
opposites in 0..29 (excluded), bin 30 has 0 (excluded) and 59, and bin 59's opposites 28 and 29 are excluded, so 59 stays.

    python tests/golden/make_golden_decode3.py
"""
import contextlib
import io
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from make_golden import PRED_NAMES, REF, slice_text  # noqa: E402

import extract_rule_oracle as ero  # noqa: E402

I2S3 = os.path.join(REF, "img2smiles3.py")
BASE = -3.0


def run_reference(lg):
    """img2smiles3.py:63-81 and :114-194 on the 8 head maps [B, c, 128, 128]; per image None (the reference's `continue`: no key
    point) or its seven lists.  The loop slice sits inside `for j in range(B)` and uses `continue`: it is executed wrapped in that
    loop; the vocabulary look-ups are identity maps here."""
    B = lg[0].shape[0]
    ns = {"torch": torch, "np": np}
    for n, v in zip(PRED_NAMES, lg):
        ns[n] = v.clone()
    ns["imgs"] = torch.zeros(B, 1, 512, 512)
    exec(slice_text(I2S3, 63, 81), ns)

    class _Ident(dict):
        def __missing__(self, k):
            return k
    ns["atom_type_devocab"], ns["atom_charge_devocab"] = _Ident(), _Ident()
    ns["results"] = []
    ns["collected"] = {}
    body = slice_text(I2S3, 114, 194)
    src = "for j in range(%d):\n" % B + "".join("    " + l if l.strip() else l for l in body.splitlines(True))
    src += ("\n    collected[j] = (atoms_position_list, atoms_type_list, atoms_charge_list, atoms_hs_list, bonds_position_list, "
            "bonds_property_list, bonds_delta_list)\n")
    with contextlib.redirect_stdout(io.StringIO()):
        exec(src, ns)
    return [ns["collected"].get(j) for j in range(B)], ns["bond_targets_pred"], ns["bond_omega_types_pred2"]


def image_arrays(lists, lg, j):
    """one image's reference lists as arrays + the bin and |rho| of every candidate from the oracle, checked against them"""
    ap, aty, ach, ahs, bp, bpr, bd = lists
    res = {"atoms": np.concatenate([np.array(ap, dtype=np.int64).reshape(-1, 2), np.array(aty, dtype=np.int64).reshape(-1, 1),
                                    np.array(ach, dtype=np.int64).reshape(-1, 1), np.array(ahs, dtype=np.int64).reshape(-1, 1)], axis=1),
           "bond_pos": np.array(bp, dtype=np.int64).reshape(-1, 2), "bond_type": np.array(bpr, dtype=np.int64),
           "bond_delta": np.array(bd, dtype=np.float64).reshape(-1, 2)}
    from oracle import nms_oracle
    am, bm, rho, _ = nms_oracle.nms(lg[0][j:j + 1], lg[4][j:j + 1], lg[6][j:j + 1], lg[7][j:j + 1])
    atoms, bonds, rhos = ero.extract(am[0, 0], bm[0, 0], lg[1][j], lg[2][j], lg[3][j], lg[5][j], rho[0], lg[7][j], "peaks")
    assert np.array_equal(atoms.numpy(), res["atoms"])
    assert np.array_equal(bonds[:, :2].numpy(), res["bond_pos"]) and np.array_equal(bonds[:, 3].numpy(), res["bond_type"])
    omega = bonds[:, 2].numpy().astype(np.float64) * (np.pi / 30) + np.pi / 60 - np.pi / 2
    r = rhos.numpy().astype(np.float64)
    assert np.array_equal(np.stack([r * np.cos(omega), r * np.sin(omega)], 1).reshape(-1, 2), res["bond_delta"])
    res["bond_bin"], res["bond_rho"] = bonds[:, 2].numpy(), rhos.numpy()
    return res


def hand_rows():
    def row(**bins):
        v = np.full(60, BASE, dtype=np.float32)
        for k, x in bins.items():
            v[int(k[1:])] = x
        return v
    just_above = np.nextafter(np.float32(-1.0), np.float32(0.0))
    rows = [
        ("bin_0", row(b0=2.0)), ("bin_29", row(b29=2.0)), ("bin_30", row(b30=2.0)), ("bin_59", row(b59=2.0)),
        ("wrap_59_over_0", row(b59=2.0, b0=1.0)), ("wrap_0_over_59", row(b0=2.0, b59=1.0)),
        ("plateau", row(b10=1.5, b11=1.5)),
        ("minus_one", row(b5=-1.0, b20=just_above)),
        ("zero_peak", row(b7=0.0)),
        ("all_equal", np.full(60, 0.25, dtype=np.float32)),
        ("loses_to_opposite", row(b10=1.0, b40=2.0)),
        ("tie_with_opposite", row(b45=1.0, b15=1.0)),
        ("no_candidate", row(b3=-2.0, b33=-2.0, b50=-2.0)),
    ]
    return rows


# what every row must give: the candidate bins under the peak rule (asserted against the reference's run below)
HAND_EXPECT = {"bin_0": [0], "bin_29": [29], "bin_30": [30], "bin_59": [59], "wrap_59_over_0": [59], "wrap_0_over_59": [0],
               "plateau": [10, 11], "minus_one": [20], "zero_peak": [7], "all_equal": list(range(30)), "loses_to_opposite": [40],
               "tie_with_opposite": [15], "no_candidate": []}


def hand_inputs():
    rows = hand_rows()
    g = torch.Generator().manual_seed(41)
    n = len(rows)
    pos = []
    for i, (name, _) in enumerate(rows):       # bond peaks 4 cells apart inside 32 x 32; the no-candidate row alone in image 1
        pos.append([1, 9, 13] if name == "no_candidate" else [0, 3 + 4 * (i // 4), 2 + 7 * (i % 4)])
    apos = [[0, 1, 1], [0, 30, 29], [0, 17, 31], [1, 5, 5], [1, 20, 11]]
    q = lambda *s: (torch.round(torch.randn(s, generator=g) * 4) / 4).numpy().astype(np.float32)   # noqa: E731
    return {"hand_names": np.array([r[0] for r in rows]), "hand_bond_pos": np.array(pos, dtype=np.int64),
            "hand_omega": np.stack([r[1] for r in rows]), "hand_rho": q(n, 60) * 3 + np.float32(0.125), "hand_btypes": q(n, 360),
            "hand_atom_pos": np.array(apos, dtype=np.int64), "hand_atom_types": q(len(apos), 14), "hand_atom_charges": q(len(apos), 3),
            "hand_atom_hs": q(len(apos), 2)}


def check_conditions(res):
    """the conditions on the golden (tests/test_extract_rule_host.py asserts them again on the committed file)"""
    names = res["hand_names"].tolist()
    pos = res["hand_bond_pos"]
    for i, name in enumerate(names):
        b, x, y = pos[i].tolist()
        at = (res["h%d_bond_pos" % b] == [x, y]).all(1)
        assert res["h%d_bond_bin" % b][at].tolist() == HAND_EXPECT[name], (name, res["h%d_bond_bin" % b][at].tolist())
        v = res["hand_omega"][i].tolist()
        assert ero.kept_bins(v, "peaks") == HAND_EXPECT[name]
    assert len(res["h1_bond_bin"]) == 0 and len(res["h1_atoms"]) > 0
    survivors = set(res["h0_bond_bin"].tolist())
    assert {0, 29, 30, 59} <= survivors
    zi = names.index("zero_peak")
    assert 7 in ero.kept_bins(res["hand_omega"][zi].tolist(), "peaks") and 7 not in ero.kept_bins(res["hand_omega"][zi].tolist(), "raw")
    mi = names.index("minus_one")
    assert res["hand_omega"][mi][5] == -1.0 and -1.0 < res["hand_omega"][mi][20] < -0.9999
    assert ero.omega_peak_bins(res["hand_omega"][names.index("plateau")].tolist()) == [10, 11]
    assert ero.omega_peak_bins(res["hand_omega"][names.index("all_equal")].tolist()) == list(range(60))
    assert ero.omega_peak_bins(res["hand_omega"][names.index("loses_to_opposite")].tolist()) == [10, 40]


def main():
    from abcnet_amd.synthetic import correlated_logits, synthetic_targets
    from oracle import decode_oracle, nms_oracle
    gold2 = np.load(os.path.join(HERE, "decode_128.npz"))
    res = {}
    # ---- the seeded maps of decode_128.npz
    tg = synthetic_targets(2, 128, seed=3)
    lg = correlated_logits(tg, seed=29, centre_noise=0.5)
    lists, bond_mask, omega_mask = run_reference(lg)
    am, bm, rho, om = nms_oracle.nms(lg[0], lg[4], lg[6], lg[7])
    assert torch.equal(bond_mask, bm) and torch.equal(omega_mask, om)
    for j in range(2):
        assert lists[j] is not None
        r = image_arrays(lists[j], lg, j)
        assert np.array_equal(r["atoms"], gold2["atoms%d" % j]), "the seeded maps are not those of decode_128.npz"
        differ = 0
        for x, y in bm[j, 0].nonzero(as_tuple=False).tolist():
            v = lg[7][j, :, x, y].tolist()
            differ += ero.kept_bins(v, "raw") != ero.kept_bins(v, "peaks")
        assert differ >= 1 and len(r["bond_bin"]) >= 1
        _, raw_bonds, _ = decode_oracle.extract(am[j, 0], bm[j, 0], lg[1][j], lg[2][j], lg[3][j], lg[5][j], rho[j], lg[7][j])
        print("seeded image %d: %d bond peaks, %d candidates under the peak rule (%d under the raw rule), %d peaks where the rules differ"
              % (j, int(bm[j].sum()), len(r["bond_bin"]), len(raw_bonds), differ))
        res["s%d_differ" % j] = np.array(differ)
        for k, v in r.items():
            res["s%d_%s" % (j, k)] = v
    # ---- the hand-made rows
    hand = hand_inputs()
    res.update(hand)
    lg = ero.hand_made_maps(hand, 128)
    lists, bond_mask, _ = run_reference(lg)
    assert int(bond_mask.sum()) == len(hand["hand_names"])          # every stored position is a bond peak, and nothing else is
    for j in range(2):
        assert lists[j] is not None
        for k, v in image_arrays(lists[j], lg, j).items():
            res["h%d_%s" % (j, k)] = v
        print("hand-made image %d: %d atoms, %d candidates" % (j, len(res["h%d_atoms" % j]), len(res["h%d_bond_bin" % j])))
    check_conditions(res)
    out = os.path.join(HERE, "decode3_128.npz")
    np.savez_compressed(out, **res)
    print("wrote", out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
