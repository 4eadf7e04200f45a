"""CPU side of the device graph assembly (abcnet_amd.ops.GraphAssembler, csrc/assemble.hip, abcnet_amd.decode): the oracle --
the specification of the kernel's operation order -- against the reference's goldens, arg-min arrays included; the mol block
text; the binding and the launcher's host refusals."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import abcnet_amd  # noqa: E402,F401
from abcnet_amd import _lib as L  # noqa: E402
import assemble_oracle as ao  # noqa: E402
from molrows import ASSEMBLE_DEFAULTS, ASSEMBLE_POINTERS, fake_desc, assemble_golden as cases  # noqa: E402

RULES = {"both_ends_one_atom", "repeated_pair_first_wins", "rho_zero", "exact_tie_mirrored_atoms", "exact_tie_coincident_atoms",
         "isolated_atom_in_the_middle", "one_atom_only", "charge_minus_enters_count", "charge_plus_enters_count",
         "aromatic_implicit_h_order", "molblock_coordinate_signs", "hundred_atoms"} | {"repair_count_%d" % n for n in range(2, 9)}


def test_golden_holds_the_cases_of_every_rule(golden_dir):
    by_name = dict(cases(golden_dir))
    assert RULES <= set(by_name) and {"decode_128_image0", "decode_128_image1"} <= set(by_name)
    # the figures of the two fixture images: atoms / candidates -> atoms / bonds / implicit-H entries
    for name, want in (("decode_128_image0", (59, 1154, 56, 171, 16)), ("decode_128_image1", (54, 1222, 54, 162, 11))):
        c = by_name[name]
        assert (len(c["atoms"]), len(c["bonds"]), len(c["symbols"]), len(c["bond2atom_index_final"]), len(c["atom_implicit_hs_list"])) == want
    assert len(by_name["hundred_atoms"]["symbols"]) >= 100 and len(by_name["hundred_atoms"]["bond2atom_index_final"]) >= 100
    assert len(by_name["one_atom_only"]["symbols"]) == 0
    pos = by_name["molblock_coordinate_signs"]["positions"]
    assert (pos < 60).any(0).all() and (pos > 60).any(0).all()


def test_oracle_reproduces_every_golden_case(golden_dir):
    """the proof that the operation order of tests/assemble_oracle.py (and of the kernel) IS the reference's"""
    for name, c in cases(golden_dir):
        got = ao.assemble(c["atoms"], c["bonds"], c["rho"])
        assert got["atom_index1"] == c["atom_index1"].tolist(), name
        assert got["atom_index2"] == c["atom_index2"].tolist(), name
        assert got["symbols"] == c["symbols"].tolist(), name
        assert got["charges"] == c["charges"].tolist() and got["hs"] == c["hs"].tolist(), name
        assert got["positions"] == c["positions"].tolist(), name
        assert got["bonds"] == c["bond2atom_index_final"].tolist(), name
        assert got["orders"] == c["bonds_property_list_final"].tolist(), name
        assert got["implicit_hs"] == c["atom_implicit_hs_list"].tolist(), name
        assert [ao.ATOM_SYMBOLS[t] for t in got["types"]] == got["symbols"] and not got["truncated"]


def test_array_form_of_the_oracle_has_the_same_bits(golden_dir):
    """the GPU tests use the array form on lists too long for the scalar loop"""
    for name, c in cases(golden_dir):
        assert ao.bond_ends_numpy(c["atoms"], c["bonds"], c["rho"], chunk=100) == ao.bond_ends(c["atoms"], c["bonds"], c["rho"]), name
        assert ao.assemble(c["atoms"], c["bonds"], c["rho"], vectorised=True) == ao.assemble(c["atoms"], c["bonds"], c["rho"]), name


def test_near_ties_are_the_normal_case(golden_dir):
    """the smallest gap between the best and the second-best atom on the fixture is a few ulps: why no float32 and no fused
    multiply-add may enter the distances"""
    from abcnet_amd.decode import omega_table
    c = dict(cases(golden_dir))["decode_128_image1"]
    cs = omega_table()
    r = c["rho"].astype(np.float64)
    delta = np.stack([r * cs[0][c["bonds"][:, 2]], r * cs[1][c["bonds"][:, 2]]], 1)
    e1 = delta / np.sqrt((delta ** 2).sum(-1, keepdims=True))
    d = (c["bonds"][:, None, :2] + delta[:, None]) - c["atoms"][None, :, :2]
    dist = np.abs(np.maximum((d * e1[:, None]).sum(-1), 0.5 * (d * e1[:, None]).sum(-1))) + np.abs((2 * d * np.stack([-e1[:, 1], e1[:, 0]], 1)[:, None]).sum(-1))
    s = np.sort(dist, 1)
    assert 0 < (s[:, 1] - s[:, 0]).min() < 1e-13


def _molecule(c):
    from abcnet_amd.decode import Molecule
    return Molecule(c["symbols"].tolist(), c["charges"], c["hs"], c["positions"], c["bond2atom_index_final"], c["bonds_property_list_final"],
                    c["atom_implicit_hs_list"])


def test_molblock_equals_the_reference_text(golden_dir):
    three_digit = signs = implicit = charged = 0
    for name, c in cases(golden_dir):
        m = _molecule(c)
        want = str(c["molblock"])
        assert m.molblock() == want, name
        three_digit += len(m.symbols) >= 100
        signs += "   -0." in want and "    0." in want
        implicit += "M  SED" in want
        charged += "M  CHG  0" not in want
    assert three_digit and signs and implicit and charged
    blk = str(dict(cases(golden_dir))["decode_128_image0"]["molblock"])
    assert len(blk.encode()) == 8974


def test_molecule_from_the_oracle_gives_the_same_text(golden_dir):
    from abcnet_amd.decode import Molecule
    for name, c in cases(golden_dir):
        o = ao.assemble(c["atoms"], c["bonds"], c["rho"])
        atoms = np.array([p + [t, ch, h] for p, t, ch, h in zip(o["positions"], o["types"], o["charges"], o["hs"])], dtype=np.int32).reshape(-1, 5)
        bonds = np.array([b + [k, s] for b, k, s in zip(o["bonds"], o["orders"], o["sources"])], dtype=np.int32).reshape(-1, 4)
        m = Molecule.from_device_rows(atoms, bonds, o["implicit_hs"])
        assert m == _molecule(c) and m.molblock() == str(c["molblock"]), name


def test_sdf2smiles_args_have_the_reference_types(golden_dir):
    c = dict(cases(golden_dir))["aromatic_implicit_h_order"]
    m = _molecule(c)
    syms, bonds, charges, orders, pos, implh = m.sdf2smiles_args()
    assert all(type(s) is str for s in syms) and all(type(v) is int for v in charges + orders + implh)
    assert all(type(v) is int for b in bonds for v in b) and all(type(v) is int for p in pos for v in p)
    assert implh == c["atom_implicit_hs_list"].tolist() and len(implh) == 2
    pos[0][0] = -1                                    # sdf2smiles rewrites its position argument: a copy, not the molecule's
    assert m.positions[0][0] != -1


def test_omega_table_is_the_reference_formula():
    from abcnet_amd.decode import omega_table
    t = omega_table()
    assert t.shape == (2, 60) and t.dtype == np.float64
    for k in (0, 7, 29, 30, 59):
        omega = k * (np.pi / 30) + np.pi / 60 - np.pi / 2
        assert t[0, k] == np.cos(omega) and t[1, k] == np.sin(omega)
    c, s = ao.omega_table()
    assert t[0].tolist() == c and t[1].tolist() == s


def test_assemble_desc_declared_in_binding():
    assert "abc_assemble_graphs" in L.SYMBOLS and "abc_assemble_work_ints" in L.SYMBOLS
    assert L._STRUCTS[-1] is L.AssembleDesc and L._STRUCTS.index(L.AssembleDesc) == 27
    lib = L.load()
    assert lib.abc_sizeof(27) == C.sizeof(L.AssembleDesc)
    assert lib.abc_sizeof(28) == -1


def _desc(**kw):
    return fake_desc(L.AssembleDesc, ASSEMBLE_POINTERS, ASSEMBLE_DEFAULTS, **kw)


def test_launcher_refuses_bad_descriptors_on_the_host():
    lib = L.load()
    for kw, word in ((dict(cap_atoms=0), b"cap_atoms"), (dict(cap_atoms=2049), b"cap_atoms"), (dict(cap_mol_bonds=0), b"cap_mol_bonds"),
                     (dict(cap_bonds=0), b"cap_bonds"), (dict(trig=None), b"table"), (dict(counts=None), b"null"),
                     (dict(bond_rho=None), b"null"), (dict(mol_bonds=None), b"null"), (dict(work=None), b"null"), (dict(B=0), b"empty")):
        assert lib.abc_assemble_graphs(C.byref(_desc(**kw)), None) == -1, kw
        assert word in lib.abc_last_error(), (kw, lib.abc_last_error())


def test_work_size_covers_the_pair_table():
    lib = L.load()
    # per image: one int per candidate + two tables of a power of two >= twice the distinct pairs the caps allow
    assert lib.abc_assemble_work_ints(C.byref(_desc())) == 2 * (16384 + 2 * 32768)
    assert lib.abc_assemble_work_ints(C.byref(_desc(cap_atoms=8, cap_bonds=16384))) == 2 * (16384 + 2 * 64)
    assert lib.abc_assemble_work_ints(C.byref(_desc(cap_atoms=0))) == 0


def test_no_cpu_fallback():
    import torch
    from abcnet_amd.ops import GraphAssembler
    with pytest.raises(L.AbcNetHipError):
        GraphAssembler(torch.zeros(1, 4, dtype=torch.int32), torch.zeros(1, 8, 5, dtype=torch.int32), torch.zeros(1, 16, 4, dtype=torch.int32),
                       torch.zeros(1, 16))
