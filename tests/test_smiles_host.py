"""The SMILES text rule where no GPU is needed: decode.Molecule.smiles(), the host form of csrc/smiles.hip,
against the rule's example table, against the recursive transcription of tests/smiles_oracle.py, and through that file's reader
back to the graph of the rows.  Strings and integers: every comparison is exact."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import abcnet_amd  # noqa: E402,F401
from abcnet_amd import _lib as L  # noqa: E402
from abcnet_amd.decode import ATOM_SYMBOLS, Molecule  # noqa: E402
import smiles_oracle as O  # noqa: E402
from smiles_cases import EXAMPLES, chain, complete, graph_of_rows, graph_of_text, ladder, random_rows, same_graph  # noqa: E402

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "abcnet_hip.h")


def host(rows):
    atoms, bonds, implh = rows
    return Molecule.from_device_rows(np.asarray(atoms).reshape(-1, 5), np.asarray(bonds).reshape(-1, 4), implh).smiles()


@pytest.fixture(scope="module")
def random_texts():
    """the 3000 seeded graphs of the recipe with the host form's text, once for the tests that read them"""
    rng = np.random.default_rng(20)
    out = []
    for _ in range(3000):
        rows = random_rows(rng)
        out.append((rows, host(rows)))
    return out


def test_the_example_table_literally():
    assert len(EXAMPLES) == 11
    for name, rows, text in EXAMPLES:
        assert host(rows) == text, name
        assert O.write(*rows) == text, name


def test_random_graphs_equal_the_oracle_and_read_back_as_the_rows(random_texts):
    for rows, text in random_texts:
        atoms, bonds, implh = rows
        assert text == O.write(*rows)
        # same_graph matches symbol, charge, bond class and the rule's aromatic flag, and wants h = 1 at every listed atom
        assert same_graph(graph_of_text(O.parse(text)), graph_of_rows(rows)), text


def test_listed_atoms_have_one_hydrogen_atom_by_atom():
    """the same over graphs whose atoms can be told apart (a chain of distinct symbols): atom i of the text is atom i of the rows"""
    syms = ["N", "C", "O", "S", "P", "B", "Se", "Si"]
    atoms = [(0, 0, ATOM_SYMBOLS.index(s), 0, 0) for s in syms]
    bonds = [(i, i + 1, 4 if i % 2 else 1, i) for i in range(1, len(syms))]
    for implh in ([], [1], [2, 7], [3, 3, 8], [0, 9, 5]):
        parsed, _ = O.parse(host((atoms, bonds, implh)))
        assert [s for s, _, _, _ in parsed] == syms
        for i, (_, _, _, h) in enumerate(parsed):
            if i + 1 in implh:
                assert h == 1, (implh, i)
            elif h is not None:      # a bracket atom that is not listed.  Se: s2 = 2 + 3, v = 2, valence 2; Si: s2 = 3, v = 1, valence 4
                assert syms[i] in ("Se", "Si") and h == {"Se": 0, "Si": 3}[syms[i]], (implh, i, h)


def test_ring_limit_and_the_long_chain():
    text = host(complete(19))
    assert len(text) == 797 and text == O.write(*complete(19))
    assert max(int(text[i + 1:i + 3]) for i, ch in enumerate(text) if ch == "%") == 97
    assert same_graph(graph_of_text(O.parse(text)), graph_of_rows(complete(19)))
    for rows in (complete(20), ladder(256)):
        with pytest.raises(ValueError, match="ring limit"):
            host(rows)
        with pytest.raises(O.Refused) as e:
            O.write(*rows)
        assert e.value.cause == "ring_limit"
    text = host(chain(512))
    assert text == "C" * 512 == O.write(*chain(512))


REFUSALS = [("a vocabulary index", lambda a, q: a.__setitem__(1, (0, 0, 14, 0, 0)), "vocabulary|symbol"),
            ("a charge of 16", lambda a, q: a.__setitem__(2, (0, 0, 1, 16, 0)), "charge"),
            ("a charge of -16", lambda a, q: a.__setitem__(2, (0, 0, 1, -16, 0)), "charge"),
            ("an order of 0", lambda a, q: q.__setitem__(0, (1, 2, 0, 0)), "order"),
            ("an order of 7", lambda a, q: q.__setitem__(0, (1, 2, 7, 0)), "order"),
            ("an end of 0", lambda a, q: q.__setitem__(1, (0, 3, 1, 1)), "end"),
            ("an end past n", lambda a, q: q.__setitem__(1, (2, 5, 1, 1)), "end"),
            ("both ends on one atom", lambda a, q: q.__setitem__(1, (3, 3, 1, 1)), "both ends"),
            ("a pair listed twice", lambda a, q: q.append((2, 1, 2, 3)), "second row"),
            ("a pair listed twice, the same way", lambda a, q: q.append((3, 4, 1, 3)), "second row")]


@pytest.mark.parametrize("what,spoil,match", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refused_rows(what, spoil, match):
    atoms, bonds = [(0, 0, 1, 0, 0)] * 4, [(1, 2, 1, 0), (2, 3, 2, 1), (3, 4, 1, 2)]
    assert host((atoms, bonds, [])) == "CC=CC"
    atoms, bonds = list(atoms), list(bonds)
    spoil(atoms, bonds)
    if atoms[1][2] == 14:      # (from_device_rows cannot name the symbol of index 14: the Molecule is built by hand)
        m = Molecule(["C", "Xx", "C", "C"], [0] * 4, [0] * 4, [[0, 0]] * 4, [b[:2] for b in bonds], [b[2] for b in bonds], [])
        with pytest.raises(ValueError, match=match):
            m.smiles()
    else:
        with pytest.raises(ValueError, match=match):
            host((atoms, bonds, []))
    with pytest.raises(O.Refused) as e:
        O.write(atoms, bonds, [])
    assert e.value.cause == "bad_row"


def test_an_implicit_h_entry_outside_the_atoms_is_ignored():
    atoms, bonds = [(0, 0, 2, 0, 0), (0, 0, 1, 0, 0)], [(1, 2, 1, 0)]
    assert host((atoms, bonds, [0, 3, -1, 77])) == "NC" == O.write(atoms, bonds, [0, 3, -1, 77])
    assert host((atoms, bonds, [1])) == "[NH]C"
    assert Molecule([], [], [], [], [], [], []).smiles() == "" == O.write([], [], [])


def test_charges_at_the_edges():
    for q, want in ((-15, "[C-15]C"), (15, "[C+15]C"), (2, "[C+2]C"), (-2, "[C-2]C"), (1, "[CH2+]C"), (-1, "[CH2-]C")):
        rows = ([(0, 0, 1, q, 0), (0, 0, 1, 0, 0)], [(1, 2, 1, 0)], [])
        assert host(rows) == want == O.write(*rows)
        assert O.parse(want)[0][0][2] == q


def test_text_bytes_bound_holds_the_longest_texts(random_texts):
    if not os.path.exists(L.LIB_PATH):
        pytest.skip("libabcnet_hip.so is not built")
    lib = L.load()

    def bound(cap_atoms, cap_bonds):
        d = L.SmilesDesc()
        d.cap_atoms, d.cap_mol_bonds = cap_atoms, cap_bonds
        return lib.abc_smiles_text_bytes(C.byref(d))

    assert bound(0, 8) == 0 and bound(8, 0) == 0 and bound(512, 2048) == 12 * 512 + 7 * 2048
    for (atoms, bonds, _), text in random_texts:      # every graph at capacities that just hold it
        assert bound(max(len(atoms), 1), max(len(bonds), 1)) >= len(text), text
    assert bound(19, 171) >= 797 and bound(512, 511) >= 512
    # everything at its widest at once: two-letter bracket atoms with a hydrogen count and a two-digit charge, in branches
    wide = ([(0, 0, 13, 0, 0)] + [(0, 0, 10, -15, 0)] * 40, [(1, i, 2, i) for i in range(2, 42)], list(range(1, 42)))
    assert bound(41, 40) >= len(host(wide))


def test_the_binding_mirrors_the_header():
    lib = L.load()
    header = open(HEADER).read()
    for name in ("abc_write_smiles", "abc_smiles_text_bytes", "abc_smiles_work_ints", "abc_smiles_desc_size"):
        assert name in L.SYMBOLS and name + "(" in header
    assert (L.SmilesDesc, "abc_smiles_desc_size") in L.SELF_SIZED_SINCE and L.SmilesDesc not in L._STRUCTS
    assert lib.abc_smiles_desc_size() == C.sizeof(L.SmilesDesc)
    assert "ABC_TEXT_RING_LIMIT = %d" % L.TEXT_RING_LIMIT in header and "ABC_MAX_SMILES_ATOMS = ABC_MAX_SIM_ATOMS" in header
    assert L.MAX_SMILES_ATOMS == L.MAX_SIM_ATOMS == 512
    assert not L.TEXT_RING_LIMIT & (L.TEXT_BAD_ROW | L.TEXT_OVERFLOW | L.MOL_EMPTY | L.MOL_TRUNCATED)


def test_the_launcher_refuses_what_it_cannot_hold():
    from molrows import fake_desc
    lib = L.load()
    pointers = ("mol_counts", "mol_atoms", "mol_bonds", "mol_implh", "text", "index", "work")
    defaults = dict(B=2, cap_atoms=512, cap_mol_bonds=2048, cap_text=4096)

    def refused(**kw):
        rc = lib.abc_write_smiles(C.byref(fake_desc(L.SmilesDesc, pointers, defaults, **kw)), None)
        return rc, lib.abc_last_error()

    assert lib.abc_write_smiles(C.byref(L.SmilesDesc()), None) == -1                 # B < 1
    assert lib.abc_write_smiles(C.byref(fake_desc(L.SmilesDesc, (), defaults)), None) == -1      # null pointers
    for kw, rc, word in ((dict(cap_atoms=513), -2, b"cap_atoms"), (dict(cap_mol_bonds=4097), -2, b"cap_mol_bonds"),
                         (dict(cap_atoms=0), -1, b"cap_atoms"), (dict(cap_text=0), -1, b"cap_text"), (dict(cap_text=2 ** 31), -1, b"cap_text")):
        got, msg = refused(**kw)
        assert got == rc and word in msg, kw
    d = fake_desc(L.SmilesDesc, pointers, defaults)
    assert lib.abc_smiles_work_ints(C.byref(d)) == 2 + (2 * (12 * 512 + 7 * 2048) + 3) // 4


def test_the_classes_refuse_before_any_device_work():
    import torch
    from abcnet_amd.infer import InferenceRunner
    from abcnet_amd.ops import SmilesWriter
    from molrows import Heads
    z = lambda *shape: torch.zeros(shape, dtype=torch.int32)
    c, a, q, h = z(2, 4), z(2, 8, 5), z(2, 16, 4), z(2, 8)
    for rows in ((c, a.numpy(), q, h), (c, z(2, 8, 4), q, h), (z(3, 4), a, q, h), (c, a, q, z(2, 9)), (c, z(2, 513, 5), q, z(2, 513)),
                 (c, a, z(2, 4097, 4), h)):
        with pytest.raises(ValueError, match="^SmilesWriter"):
            SmilesWriter(*rows)
    with pytest.raises(L.AbcNetHipError, match="^SmilesWriter"):      # well-formed host tensors: there is no CPU form
        SmilesWriter(c, a, q, h)
    with pytest.raises(ValueError, match="smiles=True.*assemble=True"):
        InferenceRunner(Heads(), 2, 128, 128, smiles=True)
