"""The tetrahedral stereo rule of the SMILES writer on the host: decode.Molecule.smiles(stereo=True) against the
rule written a second time (smiles_stereo_oracle.write) and against what the marks mean (smiles_stereo_oracle.read).  No GPU.
Bytes and integers: exact."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import abcnet_amd  # noqa: E402,F401
from abcnet_amd.decode import Molecule  # noqa: E402
import smiles_oracle as O  # noqa: E402
import smiles_stereo_oracle as S  # noqa: E402
from smiles_cases import EXAMPLES  # noqa: E402
from smiles_cases import random_rows as plain_random_rows  # noqa: E402
from smiles_stereo_cases import (CASES, REFUSALS, WIDE, WIDE_4, mirror, moved, random_images, renumbered, shift, swap_wedges,  # noqa: E402
                                 turn)

FLIPPED = {"@": "@@", "@@": "@"}


def host(image):
    m = Molecule.from_device_rows(np.asarray(image[0]).reshape(-1, 5), np.asarray(image[1]).reshape(-1, 4), image[2])
    return m.smiles(stereo=True), m.stereo_centres(), m


def all_three(image):
    """host form == oracle, byte for byte and code for code; every mark read back from the geometry.  -> (text, codes, marks by
    atom index)"""
    text, codes, m = host(image)
    want, preorder, want_codes, stats = S.write(*image)
    assert text == want and codes == want_codes
    seen = S.read(text, *S.in_text_order(image[0], image[1], preorder))
    assert sorted(preorder[p] for p in seen) == [a for a, c in enumerate(codes) if c in (1, -1)]
    for p, (written, geometric) in seen.items():
        assert written == geometric, (text, p)
    assert stats == (sum(c in (1, -1) for c in codes), codes.count(2), codes.count(3), sum(o in (5, 6) for o in m.orders))
    # the marks are all that differs from the plain text, whose graph the plain suite checks
    assert same_but_for_marks(m.smiles(), text) and O.write(*image) == m.smiles()
    return text, codes, {preorder[p]: written for p, (written, _) in seen.items()}


def same_but_for_marks(plain, marked):
    """token by token: what stands between the atoms is the same, an atom without a mark is the same, an atom with a mark is the
    plain atom in brackets with the mark behind its symbol (and the hydrogen it stands for, which a bare token does not write)"""
    spans_p, _, _, _ = S.structure(plain)
    spans_m, named, marks, _ = S.structure(marked)
    if len(spans_p) != len(spans_m):
        return False
    at_p = at_m = 0
    for (lo, hi), (mlo, mhi), mark, around in zip(spans_p, spans_m, marks, named):
        if plain[at_p:lo] != marked[at_m:mlo]:
            return False
        was, now = plain[lo:hi], marked[mlo:mhi]
        if mark and was[0] != "[":
            was = "[" + was + ("H" if S.HYDROGEN in around else "") + "]"
        if now.replace("@", "") != was:
            return False
        at_p, at_m = hi, mhi
    return plain[at_p:] == marked[at_m:]


@pytest.mark.parametrize("name,image,text", CASES, ids=[c[0] for c in CASES])
def test_cases(name, image, text):
    got, codes, marks = all_three(image)
    if text is not None:
        assert got == text
    if "nitrogen's wedge" in name:
        assert codes == [0, 3, 0, 0] and not marks
    else:
        assert len(marks) == (2 if "two bridgeheads" in name else 1) and codes.count(0) == len(codes) - len(marks)
    if "hashed" in name:
        assert codes[0] == 1
    if "opposite sign" in name or "equal sign" in name:
        assert sum(o in (5, 6) for o in host(image)[2].orders) == 2


def test_two_wedges_agree_with_each_alone():
    """F up and Br up are the same statement about the centre; F up and Cl down are not independent either: each text has one mark
    and the reader accepts it -- and hashing everything flips it"""
    for name, image, _ in CASES:
        if "two wedges" in name:
            text, _, marks = all_three(image)
            flipped = all_three(moved(image, order=swap_wedges))[2]
            assert {a: FLIPPED[m] for a, m in marks.items()} == flipped, name


@pytest.mark.parametrize("name,image,code", REFUSALS, ids=[c[0] for c in REFUSALS])
def test_refusals(name, image, code):
    text, codes, marks = all_three(image)
    assert codes[0] == code and codes[1:] == [0] * (len(codes) - 1) and not marks
    assert "@" not in text and text == host(image)[2].smiles()


def test_the_corners_of_the_range_need_64_bits():
    for image in (WIDE, WIDE_4):
        text, codes, marks = all_three(image)
        assert codes[0] in (1, -1) and len(marks) == 1
    # T of WIDE: det[(100000, 100000, -1); (199999, 0, 0); (0, 150000, 0)] = -199999 * 150000; cut to 32 bits that is +64 921 072
    t = S.det4([(100000, 100000, -1, 1), (199999, 0, 0, 1), (0, 150000, 0, 1), (0, 0, 0, 1)])
    assert t == -199999 * 150000 and (t + 2 ** 31) % 2 ** 32 - 2 ** 31 == 64921072
    assert host(WIDE)[1][0] == -1


RANDOM = random_images(41, 120)


def test_the_generator_hides_nothing():
    """conditions on the generator, checked with the oracle: centres, flat and unqualified atoms all occur"""
    with_mark = flat = unqualified = 0
    for image in RANDOM:
        _, _, codes, stats = S.write(*image)
        with_mark += stats[0] > 0
        flat += stats[1]
        unqualified += stats[2]
    print("random images: %d of %d carry a mark, %d flat atoms, %d unqualified atoms" % (with_mark, len(RANDOM), flat, unqualified))
    assert 2 * with_mark >= len(RANDOM) and flat >= 10 and unqualified >= 10


def test_random_molecules_and_their_images_under_moves():
    rng = np.random.default_rng(42)
    for k, image in enumerate(RANDOM):
        _, codes, marks = all_three(image)
        # another numbering: another walk, other permutations, and every mark is still what the drawing says
        again, new_of = renumbered(image, rng)
        _, codes2, _ = all_three(again)
        assert [abs(c) if c in (1, -1) else c for c in codes] == [abs(codes2[new_of[a]]) if codes2[new_of[a]] in (1, -1) else codes2[new_of[a]]
                                                                  for a in range(len(codes))], k
        # the mirror image, all wedges hashed, both, a quarter turn, a shift
        flipped = {a: FLIPPED[m] for a, m in marks.items()}
        assert all_three(moved(image, place=mirror))[2] == flipped, k
        assert all_three(moved(image, order=swap_wedges))[2] == flipped, k
        assert all_three(moved(image, place=mirror, order=swap_wedges))[2] == marks, k
        assert all_three(moved(image, place=turn))[2] == marks, k
        assert all_three(moved(image, place=shift))[2] == marks, k


def test_without_stereo_nothing_changes():
    for _, image, text in EXAMPLES:
        m = Molecule.from_device_rows(np.asarray(image[0]).reshape(-1, 5), np.asarray(image[1]).reshape(-1, 4), image[2])
        assert m.smiles() == m.smiles(stereo=False) == text
    rng = np.random.default_rng(43)
    for _ in range(200):      # the plain suite's recipe: wedges in either direction, any order, any symbol
        image = plain_random_rows(rng)
        m = Molecule.from_device_rows(np.asarray(image[0]).reshape(-1, 5), np.asarray(image[1]).reshape(-1, 4), image[2])
        assert m.smiles() == m.smiles(stereo=False) == O.write(*image)
        text, codes, _ = all_three(image)
        if not any(c in (1, -1) for c in codes):
            assert text == m.smiles()


def test_guards_and_binding_without_a_device():
    """the refusals come before any launch: null descriptor, null stereo_stats (ABC_EINVAL), capacities over the limits
    (ABC_EUNSUPPORTED); the helpers are host arithmetic; the mirror struct has the library's size"""
    import ctypes as C
    from abcnet_amd import _lib as L
    from molrows import Heads, fake_desc
    lib = L.load()
    assert lib.abc_smiles_stereo_desc_size() == C.sizeof(L.SmilesStereoDesc) == C.sizeof(L.SmilesDesc) + 16
    pointers = ("mol_counts", "mol_atoms", "mol_bonds", "mol_implh", "text", "index", "work", "stereo_stats")
    defaults = dict(B=2, cap_atoms=512, cap_mol_bonds=2048, cap_text=1 << 20)
    d = fake_desc(L.SmilesStereoDesc, pointers, defaults)
    assert lib.abc_smiles_stereo_text_bytes(C.byref(d)) == 14 * 512 + 7 * 2048 == lib.abc_smiles_text_bytes(C.byref(fake_desc(L.SmilesDesc, pointers[:7], defaults))) + 2 * 512
    assert lib.abc_smiles_stereo_work_ints(C.byref(d)) == 2 + 2 * (14 * 512 + 7 * 2048) // 4
    assert lib.abc_smiles_stereo_text_bytes(C.byref(fake_desc(L.SmilesStereoDesc, pointers, defaults, cap_atoms=0))) == 0
    assert lib.abc_smiles_stereo_work_ints(C.byref(fake_desc(L.SmilesStereoDesc, pointers, defaults, B=0))) == 0
    assert lib.abc_write_smiles_stereo(None, None) == -1 and b"write_smiles_stereo: null descriptor" in lib.abc_last_error()
    for fields, code, why in ((dict(stereo_stats=None), -1, b"null stereo_stats"), (dict(cap_atoms=513), -2, b"cap_atoms must be <= 512"),
                              (dict(cap_mol_bonds=4097), -2, b"cap_mol_bonds must be <= 4096"), (dict(B=0), -1, b"empty"),
                              (dict(cap_text=0), -1, b"cap_text"), (dict(cap_text=2 ** 31), -1, b"cap_text"),
                              (dict(mol_implh=None), -1, b"null molecule buffer"), (dict(work=None), -1, b"null output")):
        assert lib.abc_write_smiles_stereo(C.byref(fake_desc(L.SmilesStereoDesc, pointers, defaults, **fields)), None) == code, fields
        assert why in lib.abc_last_error(), fields
    from abcnet_amd.infer import InferenceRunner
    with pytest.raises(ValueError, match="smiles_stereo=True.*needs smiles=True"):
        InferenceRunner(Heads(), 2, 128, 128, assemble=True, smiles_stereo=True)
