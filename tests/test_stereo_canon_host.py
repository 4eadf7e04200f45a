"""The canonical ISOMERIC form on the host (decode.Molecule.smiles(isomeric=True): canonical_labelling with the stereo elements as a
third key, stereo_elements) against an oracle that is independent of the search (stereo_canon_oracle.stereo_isomorphic: every
isomorphism of the graph part, tested against the definition on the two drawings).  Strings and integers: exact."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import importlib  # noqa: E402

import abcnet_amd  # noqa: E402,F401
from abcnet_amd import decode as D  # noqa: E402
from abcnet_amd.decode import Molecule  # noqa: E402
import smiles_ez_cases as EZ  # noqa: E402
import smiles_ez_oracle as Z  # noqa: E402
import smiles_stereo_cases as ST  # noqa: E402
import smiles_stereo_oracle as S  # noqa: E402
import test_smiles_ez_host as EH  # noqa: E402
from stereo_canon_oracle import rows_of, stereo_isomorphic  # noqa: E402

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX_ATOMS = 15      # the oracle enumerates isomorphisms: under 16 atoms it is instant


def molecule(image):
    return Molecule.from_device_rows(np.asarray(image[0]).reshape(-1, 5), np.asarray(image[1]).reshape(-1, 4), image[2])


def single_wedge_swapped(image):
    """the same rows with the FIRST wedge row alone turned from 5 to 6 or back (no wedge: the same rows)"""
    atoms, bonds, implh = image
    k = next((k for k, b in enumerate(bonds) if b[2] >= 5), None)
    return atoms, [(b[0], b[1], ST.swap_wedges(b[2]) if i == k else b[2], b[3]) for i, b in enumerate(bonds)], list(implh)


def family(image, rng, mirror, turn, shift):
    """the drawing; a renumbered, turned and shifted copy (the SAME stereoisomer); its mirror image; the mirror image with the wedges
    swapped; a copy with a single wedge swapped"""
    same = ST.moved(ST.moved(ST.renumbered(image, rng)[0], turn), shift)
    return [image, same, ST.moved(image, mirror), ST.moved(image, mirror, ST.swap_wedges), single_wedge_swapped(image)]


def _families():
    rng = np.random.default_rng(2024)
    out = []
    wedge = [im for im in ST.random_images(11, 60) if len(im[0]) <= MAX_ATOMS][:16]
    wedge += [im for _, im, _ in ST.CASES] + [im for im, *_ in EZ.BOTH]
    for im in wedge:
        out.append(family(im, rng, ST.mirror, ST.turn, ST.shift))
    double = [im for im in EZ.random_images(12, 60) if EZ.in_canvas(im)][:16] + [im for _, im, _, _ in EZ.CASES]
    for im in double:
        out.append(family(im, rng, EZ.mirror, EZ.quarter_turn, EZ.shift))
    return out


FAMILIES = _families()      # (shared with tests/test_gpu_stereo_canon.py)
MARKS = re.compile(r"[/\\]|@+")


def test_isomeric_is_a_new_option():
    """fails on the parent with a TypeError: smiles() had no isomeric="""
    m = molecule(ST.worked(5))
    assert m.smiles(isomeric=True) == "[C@H](O)(N)C" and molecule(ST.worked(6)).smiles(isomeric=True) == "[C@@H](O)(N)C"


@pytest.mark.parametrize("k", range(len(FAMILIES)))
def test_equal_strings_iff_equal_stereo_graphs(k):
    mols = [molecule(im) for im in FAMILIES[k]]
    texts = [m.smiles(isomeric=True) for m in mols]
    for m in mols:
        assert m.canonical_order(isomeric=True)[1]["status"] == 0      # the default budgets decide every case
    for i in range(len(mols)):
        for j in range(i + 1, len(mols)):
            assert (texts[i] == texts[j]) == stereo_isomorphic(mols[i], mols[j]), (k, i, j, texts[i], texts[j])
    assert texts[0] == texts[1]      # the renumbered, turned and shifted copy is the same stereoisomer


def test_across_families_equal_strings_are_isomorphic():
    bucket = {}
    for fam in FAMILIES:
        for im in fam:
            m = molecule(im)
            bucket.setdefault(m.smiles(isomeric=True), []).append(m)
    shared = 0
    for mols in bucket.values():
        for i in range(1, len(mols)):
            assert stereo_isomorphic(mols[0], mols[i])
            shared += 1
    assert shared > len(FAMILIES)      # (every family shares at least the string of its first two)


@pytest.mark.parametrize("k", range(len(FAMILIES)))
def test_invariants(k):
    for im in FAMILIES[k]:
        m = molecule(im)
        text = m.smiles(isomeric=True)
        mc = m.canonical(isomeric=True)
        # the marks removed: the plain canonical text (the stereo oracles derive the marked text from the plain one, so S.write / Z.write
        # on the isomeric rows give this text from the plain text of those rows)
        atoms, bonds, implh = rows_of(mc)
        both, codes, _, _ = Z.write(atoms, bonds, implh, tetrahedral=True)
        assert both == text
        assert mc.smiles() == m.smiles(canonical=True)
        # certificate and key: the plain search's
        g = m.canon_graph()
        rank, st, key, search = m.canonical_order(isomeric=True)
        rank0, st0, key0 = m.canonical_order()
        assert key == key0 and D.canon_certificate(g, rank) == D.canon_certificate(g, rank0)
        assert search[3] == 0 and search[0] >= search[1] and st["automorphisms"] == search[2]
        # the mark readers accept the text against the isomeric rows
        _, preorder, centres, _ = S.write(atoms, bonds, implh)
        seen = S.read(Z.strip(text), *S.in_text_order(atoms, bonds, preorder))
        assert sorted(preorder[p] for p in seen) == [a for a, c in enumerate(centres) if c in (1, -1)]
        assert all(written == geometric for written, geometric in seen.values())
        EH.configurations((atoms, bonds, implh), MARKS.sub(lambda x: "" if x.group(0)[0] == "@" else x.group(0), text), codes)
        # stereo_elements agrees with stereo_centres() / double_bond_codes()
        table, stats = D.stereo_elements(m)
        assert [r[0] for r in table] == m.stereo_centres()
        ez = m.double_bond_codes()
        at = {min(b) - 1: c for b, c in zip(m.bonds, ez) if c != 0}
        assert [r[5] for r in table] == [at.get(a, 0) for a in range(len(table))]
        assert stats[:2] == [sum(c in (1, -1) for c in m.stereo_centres()), sum(c in (1, -1) for c in ez)]
        for a, r in enumerate(table):
            assert len(r) == D.STEREO_W
            if r[5] in (1, -1):
                assert sorted(m.bonds[r[6]]) == [a + 1, r[7] + 1] and m.orders[r[6]] == 2


# ------------------------------------------------------------------------------------------------------------- pinned by hand
def test_the_worked_example_and_its_enantiomer():
    rng = np.random.default_rng(5)
    up, down = molecule(ST.worked(5)).smiles(isomeric=True), molecule(ST.worked(6)).smiles(isomeric=True)
    assert up != down and Z.strip(up.replace("@", "")) == Z.strip(down.replace("@", ""))
    for _ in range(8):
        assert molecule(ST.renumbered(ST.worked(5), rng)[0]).smiles(isomeric=True) == up
        assert molecule(ST.moved(ST.renumbered(ST.worked(6), rng)[0], ST.turn)).smiles(isomeric=True) == down
    assert molecule(ST.moved(ST.worked(5), ST.mirror)).smiles(isomeric=True) == down


def butane(w2, w3):
    """2,3-disubstituted butane F-C(C)(H)-C(C)(H)-F on a zigzag: atoms C1 C2 C3 C4 F(on 2) F(on 3), a wedge from each centre to its F"""
    places = [(10, 10), (20, 20), (20, 32), (10, 42), (30, 14), (30, 38)]
    return ST.rows(["C", "C", "C", "C", "F", "F"], places, [(1, 2, 1), (2, 3, 1), (3, 4, 1), (2, 5, w2), (3, 6, w3)])


def test_butane_has_three_stereoisomers():
    a, b, meso, meso2 = (molecule(butane(*w)).smiles(isomeric=True) for w in ((5, 6), (6, 5), (5, 5), (6, 6)))
    assert len({a, b, meso}) == 3 and meso == meso2
    assert stereo_isomorphic(molecule(butane(5, 5)), molecule(butane(6, 6)))
    assert not stereo_isomorphic(molecule(butane(5, 6)), molecule(butane(6, 5)))
    # a meso drawing equals its mirror image; the chiral pair are each other's
    assert molecule(ST.moved(butane(5, 5), ST.mirror)).smiles(isomeric=True) == meso
    assert molecule(ST.moved(butane(5, 6), ST.mirror)).smiles(isomeric=True) == b


def test_hexadiene_forward_and_in_reverse():
    forward = EZ.chain_rows("CCCCCC", EZ.HEXADIENE_EZ, (1, 2, 1, 2, 1))
    reverse = EZ.chain_rows("CCCCCC", EZ.HEXADIENE_EZ[::-1], (1, 2, 1, 2, 1))
    assert molecule(forward).smiles(isomeric=True) == molecule(reverse).smiles(isomeric=True)
    assert molecule(forward).smiles(double_bonds=True) != molecule(reverse).smiles(double_bonds=True)
    ee = EZ.chain_rows("CCCCCC", EZ.HEXADIENE, (1, 2, 1, 2, 1))
    assert molecule(ee).smiles(isomeric=True) != molecule(forward).smiles(isomeric=True)


def test_a_wedge_on_a_centre_with_twin_methyls_equals_its_mirror_image():
    twin = ST.rows(["C", "N", "C", "C"], [(20, 20), (10, 20), (25, 29), (25, 11)], [(1, 2, 5), (1, 3, 1), (1, 4, 1)])
    m, mm = molecule(twin), molecule(ST.moved(twin, ST.mirror))
    assert m.stereo_centres()[0] in (1, -1)
    assert m.smiles(isomeric=True) == mm.smiles(isomeric=True) and stereo_isomorphic(m, mm)
    assert m.smiles(isomeric=True) == molecule(ST.moved(twin, None, ST.swap_wedges)).smiles(isomeric=True)


def test_without_stereo_elements_the_bytes_are_the_canonical_text():
    for im in ST.random_images(3, 30):
        plain = ST.moved(im, None, lambda o: 1 if o >= 5 else (1 if o == 2 else o))
        m = molecule(plain)
        assert m.smiles(isomeric=True) == m.smiles(canonical=True)
        rank, st, key, search = m.canonical_order(isomeric=True)
        assert (rank, st, key) == m.canonical_order() and search == [0, 0, st["automorphisms"], 0]


# ----------------------------------------------------------------------------------------------------------------- the surface
def test_refusals():
    m = molecule(ST.worked(5))
    for kw in (dict(stereo=True), dict(double_bonds=True), dict(canonical=True)):
        with pytest.raises(ValueError, match="isomeric=True already is canonical=True, stereo=True and double_bonds=True"):
            m.smiles(isomeric=True, **kw)
    with pytest.raises(ValueError, match="canonical=True with stereo=True"):      # the old refusal stays
        m.smiles(canonical=True, stereo=True)
    with pytest.raises(ValueError, match="canonical=True with stereo=True or double_bonds=True"):
        m.smiles(canonical=True, double_bonds=True)
    assert m.smiles(isomeric=True, aromatize=True) == m.aromatized().smiles(isomeric=True)
    benzene = ST.rows(["C"] * 6, EZ.RING_6, [(1, 2, 2), (2, 3, 1), (3, 4, 2), (4, 5, 1), (5, 6, 2), (6, 1, 1)])
    assert molecule(benzene).smiles(isomeric=True, aromatize=True) == "c1ccccc1"


def test_runner_flag_rule():
    infer = importlib.import_module("abcnet_amd.infer")
    flags = dict.fromkeys(("assemble", "evaluate", "score_graphs", "score_similarity", "score_identity", "molblocks", "smiles", "aromatize",
                           "smiles_stereo", "smiles_double_bonds", "smiles_canonical"), False)
    infer.check_flags(flags)      # the eleven-key dict is still what check_flags takes
    infer.check_isomeric(False, flags)
    with pytest.raises(ValueError, match="needs smiles=True"):
        infer.check_isomeric(True, flags)
    ok = dict(flags, assemble=True, smiles=True)
    infer.check_isomeric(True, ok)
    infer.check_isomeric(True, dict(ok, aromatize=True))
    for other in ("smiles_canonical", "smiles_stereo", "smiles_double_bonds"):
        with pytest.raises(ValueError, match="already is smiles_canonical, smiles_stereo and smiles_double_bonds"):
            infer.check_isomeric(True, dict(ok, **{other: True}))
    with pytest.raises(ValueError, match="smiles_canonical=True, smiles_stereo=True"):      # the old refusal still raises
        infer.check_flags(dict(ok, smiles_canonical=True, smiles_stereo=True))
    assert "smiles_isomeric" not in infer.STAGES.values() and all("smiles_isomeric" not in rule[0] for rule in infer.FLAG_NEEDS)


def test_abi_mirrors():
    from abcnet_amd import _lib as L
    from abcnet_amd import contract
    assert L.STEREO_W == 12 == len(contract.STEREO_ELEMENT) == len(L.STEREO_NONE_ROW)
    assert C.sizeof(L.CanonStereoDesc) == C.sizeof(L.CanonDesc) + 16 and C.sizeof(L.StereoDesc) == 4 * 8 + 16 + 2 * 8
    assert [f[0] for f in L.CanonStereoDesc._fields_[:len(L.CanonDesc._fields_)]] == [f[0] for f in L.CanonDesc._fields_]
    named = {fn for _, fn in L.SELF_SIZED_SINCE}
    assert {"abc_stereo_desc_size", "abc_canon_stereo_desc_size"} <= named
    assert {"abc_perceive_stereo", "abc_canonical_order_stereo"} <= set(L.SYMBOLS)
    header = open(os.path.join(_ROOT, "include", "abcnet_hip.h")).read()
    assert "enum { ABC_STEREO_W = 12 };" in header and L.STEREO_STATS_COLUMNS[3] == "status"
    lib_path = L.LIB_PATH
    if os.path.exists(lib_path):      # the library, where it is built: it reports the sizes the binding has
        lib = L.load()
        assert lib.abc_stereo_desc_size() == C.sizeof(L.StereoDesc) and lib.abc_canon_stereo_desc_size() == C.sizeof(L.CanonStereoDesc)
