"""Goldens of the graph-assembly stage (needs the reference checkout: it reads the reference's text; what it writes travels,
the reference does not).

  assemble_128.npz   img2smiles2.py:193-311 (candidate lists -> molecule) and generate_smiles.py:18-105 (molecule -> mol block
                     text, as a function body cut before the RDKit call; RDKit is never imported) executed from the reference text
                     on candidate lists.  The vocabularies come from utils.py:12-14 and img2smiles2.py:20-28, :32-34, the bond
                     deltas from img2smiles2.py:160 and :164.  Cases: the two images of decode_128.npz (its committed lists,
                     re-derived with the bin and |rho| of every candidate and checked against it), and hand-made lists, one per
                     rule of the stage.  Stored per case: the input lists and atom_index1, atom_index2, the final atom symbols /
                     charges / hs / positions, bond2atom_index_final, bonds_property_list_final, atom_implicit_hs_list and the
                     mol block text.

    python tests/golden/make_golden_assemble.py
"""
import contextlib
import io
import math
import os
import sys
import warnings
from copy import deepcopy

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from make_golden import REF, slice_text  # noqa: E402

I2S = os.path.join(REF, "img2smiles2.py")


def reference_namespace():
    ns = {"np": np}
    exec(slice_text(os.path.join(REF, "utils.py"), 12, 14), ns)
    exec(slice_text(I2S, 20, 28), ns)
    exec(slice_text(I2S, 32, 34), ns)
    return ns


def molblock_function():
    body = slice_text(os.path.join(REF, "generate_smiles.py"), 18, 105)
    src = "def molblock(atom_list,bond_list,atom_charge_list,bond_type_list,atoms_position_list=None,atom_hs_list=[]):\n"
    src += "".join("    " + l if l.strip() else l for l in body.splitlines(True)) + "\n    return text\n"
    ns = {}
    exec(src, ns)
    return ns["molblock"]


def run_reference(base, molblock, atoms, bonds, rho):
    """the reference text on one image's lists: atoms [n, 5] (x, y, type, charge, hs indices), bonds [m, 4] (x, y, bin, type), rho f32 [m]"""
    ns = dict(base)
    delta = []
    for (x, y, k, t), r in zip(bonds.tolist(), rho.tolist()):
        one = {"np": np, "omega_index": k, "rho": float(np.float32(r))}       # (.item() of the f32 map)
        exec(slice_text(I2S, 160, 160), one)
        exec(slice_text(I2S, 164, 164), one)
        delta.append([one["delta_x"], one["delta_y"]])
    ns["bonds_position_list"] = [[x, y] for x, y, _, _ in bonds.tolist()]
    ns["bonds_property_list"] = [t for _, _, _, t in bonds.tolist()]
    ns["bonds_delta_list"] = delta
    ns["atoms_position_list"] = [[x, y] for x, y, _, _, _ in atoms.tolist()]
    ns["atoms_type_list"] = [ns["atom_type_devocab"][t] for t in atoms[:, 2].tolist()]
    ns["atoms_charge_list"] = [ns["atom_charge_devocab"][c] for c in atoms[:, 3].tolist()]
    ns["atoms_hs_list"] = atoms[:, 4].tolist()
    ns["total_nums"] = 0
    out = io.StringIO()
    with contextlib.redirect_stdout(out), warnings.catch_warnings():
        warnings.simplefilter("ignore")             # rho == 0: the reference divides 0 by 0
        exec(slice_text(I2S, 193, 311), ns)
    text = molblock(ns["atoms_type_list_final"], ns["bond2atom_index_final"], ns["atoms_charge_list_final"],
                    ns["bonds_property_list_final"], deepcopy(ns["atoms_position_list_final"]), ns["atom_implicit_hs_list"])
    return ns, delta, text, out.getvalue()


# ---- hand-made lists ---------------------------------------------------------------------------------------------------
C, N, O, F, H = 1, 2, 3, 5, 12           # vocabulary indices (utils.py:12-13)


def atom(x, y, t=C, charge=0, hs=0):
    return [x, y, t, charge, hs]


def bond(p, q, order=1):
    """a candidate at the midpoint of atoms p -> q (end 1 is p): bin of the direction, |rho| = half the length"""
    cx, cy = (p[0] + q[0]) / 2, (p[1] + q[1]) / 2
    assert cx == int(cx) and cy == int(cy), (p, q)
    dx, dy = (q[0] - p[0]) / 2, (q[1] - p[1]) / 2
    k = int(math.floor((math.atan2(dy, dx) + math.pi / 2) / (math.pi / 30))) % 60
    return [int(cx), int(cy), k, order - 1], math.hypot(dx, dy)


def case(atoms, cands):
    return (np.array(atoms, dtype=np.int32).reshape(-1, 5), np.array([c[0] for c in cands], dtype=np.int32).reshape(-1, 4),
            np.array([c[1] for c in cands], dtype=np.float32))


def star(n, centre_type=F, charge=0, order=1):
    """a centre with n neighbours 20 px away in the 8 compass directions"""
    dirs = [(20, 0), (14, 14), (0, 20), (-14, 14), (-20, 0), (-14, -14), (0, -20), (14, -14)][:n]
    a = [atom(60, 60, centre_type, charge)] + [atom(60 + dx, 60 + dy) for dx, dy in dirs]
    return case(a, [bond(a[0], q, order) for q in a[1:]])


def find_exact_tie():
    """a candidate and two atoms mirrored across its centre, perpendicular to it, whose distances tie EXACTLY in float64 at both
    ends: both arg-mins take the first atom and the candidate goes.  Searched over the bins, a few |rho| and the integer offsets
    roughly perpendicular to the bin (the mirror symmetry alone does not make the float64 sums equal: the hits are diagonal
    offsets at the 45-degree bins)"""
    import assemble_oracle as ao
    COS, SIN = ao.omega_table()
    for k in range(60):
        for r in (4.0, 5.0, 6.0, 8.0):
            dx, dy = r * COS[k], r * SIN[k]
            n = math.sqrt(dx * dx + dy * dy)
            e1x, e1y = dx / n, dy / n
            for wx in range(-8, 9):
                for wy in range(-8, 9):
                    if (wx, wy) <= (0, 0) or wx * wx + wy * wy < 32 or abs(wx * e1x + wy * e1y) > 0.2 * math.hypot(wx, wy):
                        continue
                    a, b = [64 - wx, 64 - wy], [64 + wx, 64 + wy]
                    d = []
                    for sgn in (1.0, -1.0):
                        for (ax, ay) in (a, b):
                            u, v = 64 + sgn * dx - ax, 64 + sgn * dy - ay
                            s = sgn * (u * e1x + v * e1y)
                            d.append(abs(ao.lrelu(s)) + abs((2.0 * u) * -e1y + (2.0 * v) * e1x))
                    if d[0] == d[1] and d[2] == d[3]:
                        return np.array([atom(*a), atom(*b), atom(10, 10)], dtype=np.int32), k, r
    raise RuntimeError("no exact tie found")


def hand_made():
    cases = {}
    a = [atom(20, 20), atom(20, 60)]
    cases["both_ends_one_atom"] = case(a, [([20, 22, 29, 0], 1.0), bond(a[0], a[1])])
    a = [atom(30, 30), atom(50, 70)]
    fwd, back = bond(a[0], a[1], 1), bond(a[1], a[0], 2)
    cases["repeated_pair_first_wins"] = case(a, [back, fwd, bond(a[0], a[1], 3)])
    a = [atom(30, 30), atom(70, 50), atom(90, 90)]
    cases["rho_zero"] = case(a, [([50, 40, 7, 0], 0.0), bond(a[0], a[1]), ([80, 70, 33, 1], 0.0), bond(a[1], a[2], 2)])
    atoms, k, r = find_exact_tie()
    cases["exact_tie_mirrored_atoms"] = case(atoms.tolist(), [([64, 64, k, 0], r), bond(atoms[0], atoms[2])])
    print("exact tie: atoms", atoms[:2, :2].tolist(), "bin", k, "rho", r)
    # two atoms on one pixel tie exactly whatever the candidate: the first index wins at both ends of the candidate between them
    a = [atom(40, 40), atom(40, 40), atom(80, 80)]
    cases["exact_tie_coincident_atoms"] = case(a, [bond(a[0], a[2]), bond(a[2], a[1], 2)])
    a = [atom(20, 20), atom(100, 100, N), atom(20, 60)]
    cases["isolated_atom_in_the_middle"] = case(a, [bond(a[0], a[2])])
    cases["one_atom_only"] = case([atom(64, 64, O)], [([64, 70, 29, 0], 6.0), ([60, 64, 14, 1], 4.0)])
    for n in range(2, 9):
        cases["repair_count_%d" % n] = star(n)
    cases["repair_double_bonds_on_oxygen"] = star(2, centre_type=O, order=2)         # count 4 -> C
    cases["charge_minus_enters_count"] = star(2, centre_type=O, charge=2)           # O-: 2 + 1 = 3 -> N
    cases["charge_plus_enters_count"] = star(4, centre_type=N, charge=1)            # N+: 4 - 1 = 3, stays N
    cases["uncharged_four_bonds_on_nitrogen"] = star(4, centre_type=N)              # 4 -> C
    a = [atom(20, 20, C, 0, 1), atom(20, 40, N, 0, 1), atom(40, 60, N, 0, 0), atom(60, 60, N, 0, 1), atom(80, 80, O, 0, 1)]
    cases["aromatic_implicit_h_order"] = case(a, [bond(a[2], a[3], 4), bond(a[0], a[1], 4), bond(a[1], a[2], 4), bond(a[3], a[4], 1)])
    a = [atom(30, 30), atom(30, 90, N, 1), atom(90, 30, O, 2), atom(90, 90), atom(60, 60), atom(0, 0), atom(126, 126)]
    cases["molblock_coordinate_signs"] = case(a, [bond(a[0], a[1]), bond(a[1], a[3], 5), bond(a[3], a[2], 6), bond(a[2], a[0], 2),
                                                  bond(a[0], a[4], 3), bond(a[5], a[0]), bond(a[3], a[6])])
    a = [atom(10 + 10 * i, 10 + 10 * j, [C, N, O][(i + j) % 3]) for i in range(10) for j in range(11)]
    cands = [bond(a[i * 11 + j], a[i * 11 + j + 1]) for i in range(10) for j in range(10)]
    cands += [bond(a[i * 11], a[(i + 1) * 11], 2) for i in range(0, 9, 2)]
    cases["hundred_atoms"] = case(a, cands)
    return cases


def decode_cases():
    """the two images of decode_128.npz with the bin and |rho| of every candidate (the golden stores positions, types and deltas):
    the extraction oracle on the same seeded maps, checked against the committed lists"""
    import torch  # noqa: F401
    import abcnet_amd  # noqa: F401
    from abcnet_amd.synthetic import correlated_logits, synthetic_targets
    from oracle import decode_oracle, nms_oracle
    gold = np.load(os.path.join(HERE, "decode_128.npz"))
    tg = synthetic_targets(2, 128, seed=3)
    lg = correlated_logits(tg, seed=29, centre_noise=0.5)
    am, bm, rho, _ = nms_oracle.nms(lg[0], lg[4], lg[6], lg[7])
    cases = {}
    for j in range(2):
        atoms, bonds, rhos = decode_oracle.extract(am[j, 0], bm[j, 0], lg[1][j], lg[2][j], lg[3][j], lg[5][j], rho[j], lg[7][j])
        atoms, bonds, rhos = atoms.numpy().astype(np.int32), bonds.numpy().astype(np.int32), rhos.numpy()
        assert np.array_equal(atoms, gold["atoms%d" % j]) and np.array_equal(bonds[:, :2], gold["bond_pos%d" % j])
        assert np.array_equal(bonds[:, 3], gold["bond_type%d" % j])
        cases["decode_128_image%d" % j] = (atoms, bonds, rhos, gold["bond_delta%d" % j])
    return cases


def main():
    base, molblock = reference_namespace(), molblock_function()
    cases = decode_cases()
    cases.update(hand_made())
    res = {"n": np.array(len(cases))}
    for ci, (name, c) in enumerate(cases.items()):
        atoms, bonds, rho = c[:3]
        ns, delta, text, printed = run_reference(base, molblock, atoms, bonds, rho)
        if len(c) > 3:
            assert np.array_equal(np.array(delta), c[3]), name          # the committed deltas, bit for bit
        p = "c%d_" % ci
        res[p + "name"] = np.array(name)
        res[p + "atoms"], res[p + "bonds"], res[p + "rho"] = atoms, bonds, rho
        res[p + "atom_index1"] = np.asarray(ns["atom_index1"], dtype=np.int64)
        res[p + "atom_index2"] = np.asarray(ns["atom_index2"], dtype=np.int64)
        res[p + "symbols"] = np.array(ns["atoms_type_list_final"], dtype="U8")
        res[p + "charges"] = np.array(ns["atoms_charge_list_final"], dtype=np.int64)
        res[p + "hs"] = np.array(ns["atoms_hs_list_final"], dtype=np.int64)
        res[p + "positions"] = np.array(ns["atoms_position_list_final"], dtype=np.int64).reshape(-1, 2)
        res[p + "bond2atom_index_final"] = np.array(ns["bond2atom_index_final"], dtype=np.int64).reshape(-1, 2)
        res[p + "bonds_property_list_final"] = np.array(ns["bonds_property_list_final"], dtype=np.int64)
        res[p + "atom_implicit_hs_list"] = np.array(ns["atom_implicit_hs_list"], dtype=np.int64)
        res[p + "molblock"] = np.array(text)
        nan = int(np.isnan(ns["distance1"]).any(axis=1).sum())
        print("%-34s %3d atoms %4d candidates -> %3d atoms %3d bonds %2d implicit H, %2d repairs, %d NaN rows, %d bytes of text" % (
            name, len(atoms), len(bonds), len(ns["atoms_type_list_final"]), len(ns["bond2atom_index_final"]),
            len(ns["atom_implicit_hs_list"]), len(printed.splitlines()), nan, len(text)))
    np.savez_compressed(os.path.join(HERE, "assemble_128.npz"), **res)


if __name__ == "__main__":
    main()
