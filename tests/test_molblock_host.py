"""The device mol block writer (csrc/molblock.hip, ops.MolBlockWriter) where no GPU is needed: the integer coordinate rule against
the host form's formatting over its whole domain, the per-image byte bound of abc_molblock_text_bytes against the adversarial
molecule of three capacities, the descriptor mirror and the exported symbols, and what the constructors refuse."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import abcnet_amd  # noqa: F401
from abcnet_amd import _lib as L
from abcnet_amd.decode import Molecule

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def coord_text(px):
    """the kernel's rule (put_coord of csrc/molblock.hip), integers only"""
    a = abs(px - 60) * 500
    q = (2 * a + 3) // 6
    return "%s%d.%04d" % ("   -" if px < 60 else "    ", q // 10000, q % 10000)


def test_integer_coordinate_rule_is_the_host_formatting_for_every_position():
    """every px in 0..199999: the text Molecule.molblock() puts in front of the symbol"""
    for lo in range(0, 200000, 500):
        pxs = list(range(lo, lo + 500))
        m = Molecule(["C"] * 500, [0] * 500, [0] * 500, [[p, 199999 - p] for p in pxs], [], [], [])
        lines = m.molblock().split("\n")[4:4 + 500]
        for p, line in zip(pxs, lines):
            want = coord_text(p) + coord_text(199999 - p) + "    0.0000 C   0"
            assert line.startswith(want), (p, line, want)


def adversarial(cap_atoms, cap_mol_bonds):
    n = cap_atoms
    return Molecule(["Cl"] * n, [-15] * n, [0] * n, [[199999, 199999]] * n, [[n, n - 1]] * cap_mol_bonds, [5] * cap_mol_bonds,
                    list(range(n, 0, -1)))


def _bound(cap_atoms, cap_mol_bonds):
    d = L.MolBlockDesc()
    d.cap_atoms, d.cap_mol_bonds = cap_atoms, cap_mol_bonds
    return L.load().abc_molblock_text_bytes(C.byref(d))


@pytest.mark.parametrize("caps", [(8, 8), (128, 512), (1024, 4096)])
def test_text_bytes_bounds_the_adversarial_molecule(caps):
    """all atoms Cl at 199999 with charge -15, every atom an implicit-H entry, every bond a wedge between the highest indices"""
    text = adversarial(*caps).molblock()
    bound = _bound(*caps)
    print("capacities %s: adversarial text %d bytes, bound %d" % (caps, len(text), bound))
    assert bound >= len(text)
    # and an int32 at its widest in every free column
    n, m = caps
    lo = -2 ** 31
    wide = Molecule(["Cl"] * n, [lo] * n, [0] * n, [[199999, 199999]] * n, [[lo, lo]] * m, [lo] * m, [lo] * n)
    assert bound >= len(wide.molblock())


def test_text_bytes_needs_capacities():
    assert _bound(0, 8) == 0 and _bound(8, 0) == 0 and _bound(1, 1) > 0


def test_symbols_and_descriptor_size():
    for name in ("abc_write_molblocks", "abc_molblock_text_bytes", "abc_molblock_desc_size"):
        assert name in L.SYMBOLS
    assert L.MolBlockDesc not in L._STRUCTS
    lib = L.load()
    assert lib.abc_molblock_desc_size() == C.sizeof(L.MolBlockDesc)
    header = open(os.path.join(ROOT, "include", "abcnet_hip.h")).read()
    assert "ABC_TEXT_BAD_ROW = %d" % L.TEXT_BAD_ROW in header and "ABC_TEXT_OVERFLOW = %d" % L.TEXT_OVERFLOW in header
    assert not (L.TEXT_BAD_ROW | L.TEXT_OVERFLOW) & (L.MOL_EMPTY | L.MOL_TRUNCATED)


def test_the_launcher_refuses_before_it_touches_a_device():
    lib = L.load()
    d = L.MolBlockDesc()
    assert lib.abc_write_molblocks(C.byref(d), None) != 0        # B < 1
    d.B, d.cap_atoms, d.cap_mol_bonds, d.cap_text = 2, 8, 8, 100
    assert lib.abc_write_molblocks(C.byref(d), None) != 0        # null pointers
    assert b"null" in lib.abc_last_error()
    buf = np.zeros(64, dtype=np.int32)
    for f in ("mol_counts", "mol_atoms", "mol_bonds", "mol_implh", "text", "index", "work"):
        setattr(d, f, buf.ctypes.data)
    d.cap_text = 0
    assert lib.abc_write_molblocks(C.byref(d), None) != 0 and b"cap_text" in lib.abc_last_error()
    d.cap_text = 2 ** 31
    assert lib.abc_write_molblocks(C.byref(d), None) != 0 and b"cap_text" in lib.abc_last_error()


def test_writer_validates_its_rows():
    from abcnet_amd.ops import MolBlockWriter

    def z(*shape):
        return torch.zeros(shape, dtype=torch.int32)
    c, a, q, h = z(2, 4), z(2, 8, 5), z(2, 8, 4), z(2, 8)
    with pytest.raises(ValueError):
        MolBlockWriter(c, a.numpy(), q, h)
    with pytest.raises(ValueError):
        MolBlockWriter(c, z(2, 8, 4), q, h)
    with pytest.raises(ValueError):
        MolBlockWriter(z(3, 4), a, q, h)
    with pytest.raises(ValueError):
        MolBlockWriter(c, a, q, z(2, 9))
    # well-formed host tensors: there is no CPU form
    with pytest.raises(L.AbcNetHipError):
        MolBlockWriter(c, a, q, h)


def test_runner_needs_the_assembler_for_the_text():
    from abcnet_amd.infer import InferenceRunner
    with pytest.raises(ValueError, match="assemble=True"):
        InferenceRunner(None, 2, 128, 128, molblocks=True)
