"""The double-bond rule of the SMILES writer on the host: decode.Molecule.smiles(double_bonds=True) against the
rule written a second time (smiles_ez_oracle.write) and against what "/" and "\\" mean (smiles_ez_oracle.read, itself held to strings
from the literature).  No GPU.  Bytes and integers: exact."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import abcnet_amd  # noqa: E402,F401
from abcnet_amd.decode import Molecule  # noqa: E402
import smiles_ez_oracle as Z  # noqa: E402
import smiles_oracle as O  # noqa: E402
import smiles_stereo_oracle as S  # noqa: E402
from smiles_ez_cases import (BOTH, CASES, FLAT_CASES, W, butenes, in_canvas, mirror, quarter_turn, random_images, shift,  # noqa: E402
                             zigzag_polyene)
from smiles_stereo_cases import moved, renumbered  # noqa: E402

SEED, COUNT = 23, 1500      # (the recipe's seed and size: the conditions below are asserted on the ORACLE's codes alone)


def molecule(image):
    return Molecule.from_device_rows(np.asarray(image[0]).reshape(-1, 5), np.asarray(image[1]).reshape(-1, 4), image[2])


def side_of_line(image, a, b, s):
    """the drawing's own sign test, in exact integers: on which side of the line through a and b (directed a -> b) does s lie"""
    (xa, ya), (xb, yb), (xs, ys) = (tuple(image[0][k][:2]) for k in (a, b, s))
    # in the frame whose first axis is a -> b, the second coordinate of s - a is its signed distance from the line times |b - a|
    ux, uy = xb - xa, yb - ya
    across = -uy * (xs - xa) + ux * (ys - ya)
    return (across > 0) - (across < 0)


def configurations(image, text, codes):
    """{frozenset({(end, substituent), (end, substituent)}): together?} of every marked double bond, by ATOM index, as the reader sees
    the text; asserted against the drawing"""
    preorder = S.preorder_of(len(image[0]), image[1])
    marked = {tuple(sorted((r[0] - 1, r[1] - 1))) for r, c in zip(image[1], codes) if c in (1, -1)}
    out = {}
    for (i, j, x, y), word in Z.read(text).items():
        i, j, x, y = (preorder[p] for p in (i, j, x, y))
        if tuple(sorted((i, j))) not in marked:
            continue      # (an unmarked double bond between two marked ones may see a symbol at both ends: it says nothing)
        a, b = sorted((i, j))
        together = side_of_line(image, a, b, x) == side_of_line(image, a, b, y)
        assert word == ("together" if together else "opposite"), (text, i, j, x, y)
        out[frozenset(((i, x), (j, y)))] = together
    return out


def groups_start_with_a_slash(image, text, codes):
    """every group of marked double bonds joined by shared single bonds: the first of its symbols in the text is "/" -> (number of
    groups, shared single bonds, symbols at a closing digit)"""
    n, in_text = Z.bonds_in_text(text)
    preorder = S.preorder_of(n, image[1])
    marked = [tuple(sorted((r[0] - 1, r[1] - 1))) for r, c in zip(image[1], codes) if c in (1, -1)]
    end_of = {e: k for k, pair in enumerate(marked) for e in pair}
    group = list(range(len(marked)))

    def find(k):
        while group[k] != k:
            k = group[k]
        return k
    symbols, shared = [], 0
    for first, second, symbol, offset in in_text:
        if symbol in ("/", "\\"):
            owners = {end_of[e] for e in (preorder[first], preorder[second]) if e in end_of}
            assert owners, "a symbol no marked double bond claims in %r" % text
            if len(owners) == 2:
                shared += 1
                k1, k2 = (find(k) for k in owners)
                group[k1] = k2
            symbols.append((offset, symbol, next(iter(owners))))
    first_of = {}
    for offset, symbol, owner in sorted(symbols):
        first_of.setdefault(find(owner), symbol)
    assert len(first_of) == len({find(k) for k in range(len(marked))}) and set(first_of.values()) <= {"/"}, text
    at_digit = sum(text[offset + 1].isdigit() or text[offset + 1] == "%" for offset, _, _ in symbols)
    return len(first_of), shared, at_digit


def all_three(image, tetrahedral=False):
    """host form == oracle, byte for byte and code for code; stripped of its symbols the text is the plain one; the reader and the
    drawing agree; every group starts with "/".  -> (text, codes, configurations)"""
    m = molecule(image)
    text, codes = m.smiles(double_bonds=True, stereo=tetrahedral), m.double_bond_codes()
    want, want_codes, stats, _ = Z.write(*image, tetrahedral=tetrahedral)
    assert text == want and codes == want_codes
    assert stats == (sum(c in (1, -1) for c in codes), codes.count(2), codes.count(3), codes.count(4))
    assert Z.strip(text) == m.smiles(stereo=tetrahedral) and (tetrahedral or Z.strip(text) == O.write(*image))
    conf = configurations(image, text, codes)
    assert len({frozenset(e for e, _ in key) for key in conf}) == stats[0]      # every marked double bond is read back
    groups_start_with_a_slash(image, text, codes)
    return text, codes, conf


def test_the_reader_on_strings_from_the_literature():
    """OpenSMILES: F/C=C/F and its mirror image in the text are trans, F/C=C\\F cis; a branch reads from the atom in front"""
    assert Z.read("F/C=C/F") == {(1, 2, 0, 3): "opposite"}
    assert Z.read("F/C=C\\F") == {(1, 2, 0, 3): "together"}
    assert Z.read("C(/F)=C/F") == {(0, 2, 1, 3): "together"}
    assert Z.read("C(\\F)=C/F") == {(0, 2, 1, 3): "opposite"}
    assert Z.read("F\\C=C\\F") == {(1, 2, 0, 3): "opposite"} and Z.read("F\\C=C/F") == {(1, 2, 0, 3): "together"}
    # a symbol at a closing digit is read from the atom that bears it: C1 ... C/1 says atom 0 is above the closer
    assert Z.read("C1CCNC/C/1=C\\C") == {(5, 6, 4, 7): "together", (5, 6, 0, 7): "opposite"}
    assert Z.read("CC=CC") == {} and Z.strip("C/C=C\\C") == "CC=CC"


@pytest.mark.parametrize("name,image,text,codes", CASES, ids=[c[0] for c in CASES])
def test_examples_byte_for_byte(name, image, text, codes):
    got, got_codes, _ = all_three(image)
    assert got == text and got_codes == codes


def test_examples_with_tetrahedral_stereo():
    for image, both, tetrahedral, double in BOTH:
        m = molecule(image)
        assert m.smiles(stereo=True, double_bonds=True) == both == all_three(image, tetrahedral=True)[0]
        assert m.smiles(stereo=True) == tetrahedral and m.smiles(double_bonds=True) == double == all_three(image)[0]
        assert m.stereo_centres() == [-1, 0, 0, 0, 0, 0] and m.double_bond_codes() == [0, 0, 0, -1 if "/C=C/C" in both else 1, 0]


@pytest.mark.parametrize("name,image,code", FLAT_CASES, ids=[c[0] for c in FLAT_CASES])
def test_cases_placed_by_hand(name, image, code):
    text, codes, _ = all_three(image)
    assert [c for c in codes if c] == [code] and (("/" in text) == (code in (1, -1)))


def test_wide_shapes_on_the_host():
    text, codes, conf = all_three(zigzag_polyene(64))
    assert text == "C" + "/C=C" * 31 + "/C" and codes.count(-1) == 31 and len(conf) == 31
    text, codes, _ = all_three(butenes(6))
    assert text == ".".join(["C/C=C\\C", "C/C=C/C"] * 3)


@pytest.fixture(scope="module")
def seeded():
    images = random_images(SEED, COUNT)
    return images, [all_three(im) for im in images]


def test_the_seed_meets_its_conditions_by_the_oracle_alone(seeded):
    """so that the tests below cannot pass on nothing"""
    images, _ = seeded
    marked = flat = ring = twin = shared = at_digit = two_subs = n_one_sub = 0
    for image in images:
        text, codes, stats, found = Z.write(*image)
        marked, flat, ring, twin = marked + stats[0], flat + stats[1], ring + stats[2], twin + stats[3]
        _, s, d = groups_start_with_a_slash(image, text, codes)
        shared, at_digit = shared + s, at_digit + d
        for turns in found.values():
            ends = [e for e, _ in turns]
            two_subs += any(ends.count(e) == 2 for e in ends)
            n_one_sub += any(ends.count(e) == 1 and image[0][e][2] == 2 for e in ends)
    print("marked %d, flat %d, ring %d, twin %d, shared bonds %d, symbols at a closing digit %d, double bonds with a two-substituent "
          "end %d, with an N end of one substituent %d" % (marked, flat, ring, twin, shared, at_digit, two_subs, n_one_sub))
    assert marked >= 100 and min(flat, ring, twin, shared, at_digit, two_subs, n_one_sub) >= 1


def test_moves_of_the_canvas_change_nothing(seeded):
    images, results = seeded
    for image, (text, codes, _) in zip(images, results):
        if not in_canvas(image):
            continue      # (a place out of the range on purpose: a mirror image would bring it back in)
        for move in (mirror, quarter_turn, shift):
            m = molecule(moved(image, place=move))
            assert m.smiles(double_bonds=True) == text and m.double_bond_codes() == codes, move.__name__


def test_renumbering_keeps_every_configuration(seeded):
    images, results = seeded
    rng = np.random.default_rng(SEED + 1)
    kept = 0
    for image, (_, _, conf) in zip(images, results):
        again, new_of = renumbered(image, rng)
        old_of = {new: old for old, new in enumerate(new_of)}
        _, _, conf2 = all_three(again)
        assert {frozenset((old_of[e], old_of[x]) for e, x in key): v for key, v in conf2.items()} == conf
        kept += len(conf)
    assert kept >= 100


def test_off_is_the_text_of_today():
    for image in random_images(SEED, 200) + [c[1] for c in CASES]:
        m = molecule(image)
        assert m.smiles() == m.smiles(double_bonds=False) == O.write(*image) == m._smiles(False)[0]
        assert m.smiles(stereo=True) == S.write(*image)[0]


def test_canonical_is_refused():
    m = molecule(CASES[0][1])
    with pytest.raises(ValueError, match="canonical=True"):
        m.smiles(double_bonds=True, canonical=True)
    assert m.smiles(canonical=True)


def test_aromatize_marks_only_the_chain_bond_of_styrene():
    """Kekule styrene with a methyl on the chain: the ring's double bonds are on a cycle (and aromatic once perceived), the chain's is
    marked"""
    ring = [(20, 10), (10, 16), (10, 28), (20, 34), (30, 28), (30, 16)]
    image = ([(x, y, 1, 0, 0) for x, y in ring + [(20, 0), (30, -6), (30, -18)]],
             [(1, 2, 2, 0), (2, 3, 1, 1), (3, 4, 2, 2), (4, 5, 1, 3), (5, 6, 2, 4), (6, 1, 1, 5), (1, 7, 1, 6), (7, 8, 2, 7), (8, 9, 1, 8)], [])
    image = moved(image, place=lambda x, y: (x, y + 20))
    m = molecule(image)
    assert m.double_bond_codes() == [3, 0, 3, 0, 3, 0, 0, -1, 0]
    assert m.smiles(double_bonds=True) == "C1(=CC=CC=C1)/C=C/C"
    assert m.smiles(double_bonds=True, aromatize=True) == "c1(ccccc1)/C=C/C" and m.smiles(aromatize=True) == "c1(ccccc1)C=CC"
    assert m.aromatized().double_bond_codes() == [0, 0, 0, 0, 0, 0, 0, -1, 0]
