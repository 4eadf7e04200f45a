"""The stereo perception stage on the device (csrc/stereo.hip, abc_perceive_stereo, ops.StereoPerceiver) against the SMILES writer's
own codes on the same rows (the two kernels take both rules from csrc/stereo_rules.hpp, but each fills its own lists, does its own walk
and writes its own outputs: this holds them to one answer) and against the host form decode.stereo_elements.  Integers: exact, no
tolerance anywhere."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import abcnet_amd  # noqa: E402,F401
from abcnet_amd import _lib as L  # noqa: E402
from abcnet_amd import decode as D  # noqa: E402
from abcnet_amd.decode import Molecule  # noqa: E402
from abcnet_amd.ops import SmilesWriter, StereoPerceiver  # noqa: E402
import smiles_ez_cases as EZ  # noqa: E402
import smiles_stereo_cases as ST  # noqa: E402

DEV = "cuda"
EINVAL, EUNSUPPORTED = -1, -2
ONE_ATOM = ([(5, 5, 1, 0, 0)], [], [])


def upload(images, cap_atoms, cap_bonds):
    """hand-made rows [(atoms [n,5], bonds [m,4], implh [k], status)] as device tensors of the assembler's layout; the rows past the
    counts hold a pattern that must not be read (an index the vocabulary does not have, a double bond no atom has)"""
    B = len(images)
    cnt = torch.zeros(B, 4, dtype=torch.int32)
    atoms = torch.full((B, cap_atoms, 5), 77, dtype=torch.int32)
    bonds = torch.full((B, cap_bonds, 4), 2, dtype=torch.int32)
    implh = torch.full((B, cap_atoms), 77, dtype=torch.int32)
    for b, (a, q, h, status) in enumerate(images):
        a, q, h = np.asarray(a, dtype=np.int64).reshape(-1, 5), np.asarray(q, dtype=np.int64).reshape(-1, 4), np.asarray(h, dtype=np.int64).reshape(-1)
        atoms[b, :len(a)] = torch.as_tensor(a, dtype=torch.int32)
        bonds[b, :len(q)] = torch.as_tensor(q, dtype=torch.int32)
        implh[b, :len(h)] = torch.as_tensor(h, dtype=torch.int32)
        cnt[b] = torch.tensor([len(a), len(q), len(h), status], dtype=torch.int32)
    return cnt.to(DEV), atoms.to(DEV), bonds.to(DEV), implh.to(DEV)


def with_status(image, status=0):
    return tuple(image[:3]) + (status,)


def expected(images, cap_atoms):
    """(table [B, cap_atoms, STEREO_W], stats [B, 4]) by the host form"""
    table = np.tile(np.array(D.STEREO_NONE_ROW, dtype=np.int32), (len(images), cap_atoms, 1))
    stats = np.zeros((len(images), 4), dtype=np.int32)
    for b, (a, q, h, status) in enumerate(images):
        if status & L.MOL_EMPTY:
            stats[b, 3] = status & 3
        elif any(not 0 <= row[2] <= 13 for row in a):      # (from_device_rows cannot name such an atom's symbol)
            stats[b, 3] = (status & 3) | L.TEXT_BAD_ROW
        else:
            m = Molecule.from_device_rows(np.asarray(a).reshape(-1, 5), np.asarray(q).reshape(-1, 4), h, truncated=bool(status & L.MOL_TRUNCATED))
            rows, st = D.stereo_elements(m)
            if len(rows):
                table[b, :len(rows)] = np.array(rows, dtype=np.int32)
            stats[b] = st
    return torch.from_numpy(table), torch.from_numpy(stats)


def check(images, cap_atoms=32, cap_bonds=32):
    assert len(images) <= 16 and len(images[0][0]) != len(images[-1][0])
    up = upload(images, cap_atoms, cap_bonds)
    op = StereoPerceiver(*up)
    op.table.fill_(77)
    op.stat.fill_(77)
    op.run()
    w = SmilesWriter(*up, stereo=True, double_bonds=True)
    w.run()
    torch.cuda.synchronize()
    el = op.elements()
    # the writer's codes of the same rows: the centre of every atom; the code of every candidate's row, at its lower end
    assert torch.equal(el[..., 0], w.parities())
    ez, rows = w.double_bond_codes(), up[2].cpu()
    at_lower = torch.zeros_like(el[..., 5])
    for b, q in ez.nonzero().tolist():
        at_lower[b, int(rows[b, q, :2].min()) - 1] = ez[b, q]
    assert torch.equal(el[..., 5], at_lower)
    st = op.stat.cpu()
    assert st[:, 3].tolist() == w.status()
    assert torch.equal(st[:, 0], w.stats.cpu()[:, 0]) and torch.equal(st[:, 1], w.ez_stats.cpu()[:, 0])
    assert torch.equal(st[:, 2], w.stats.cpu()[:, 1] + w.ez_stats.cpu()[:, 1])
    # the whole table and the stats: the host form's
    want, want_stats = expected(images, cap_atoms)
    assert torch.equal(el, want)
    assert torch.equal(st, want_stats)
    assert [tuple(r) for r in op.stats().tolist()] == [tuple(r) for r in want_stats.tolist()]
    return el, st


def test_perceive_stereo_is_exported_and_runs():
    """fails on the parent: the library has no abc_perceive_stereo"""
    assert hasattr(L.load(), "abc_perceive_stereo")
    el, st = check([with_status(ONE_ATOM), with_status(ST.worked(5))])
    assert el[0, 0].tolist() == list(D.STEREO_NONE_ROW)
    assert el[1, 0, 0] in (1, -1) and el[1, 0, 1:].tolist() == [1, 2, 3, -1, 0] + [-1] * 6
    assert st.tolist() == [[0, 0, 0, 0], [1, 0, 0, 0]]


def test_tetrahedral_cases():
    images = [with_status(ONE_ATOM), with_status(ST.worked(5)), with_status(ST.worked(6)), with_status(ST.worked(5, True))]
    images += [with_status(im) for _, im, _ in ST.CASES[3:]]
    el, st = check(images)
    assert int(st[:, 0].sum()) >= 5
    four = el[4, 0].tolist()      # "four neighbours, a root"
    assert four[0] in (1, -1) and four[1:5] == [1, 2, 3, 4]


def test_refusals_flat_and_wide():
    images = [with_status(ONE_ATOM)] + [with_status(im) for _, im, _ in ST.REFUSALS]
    el, st = check(images)
    assert el[1:, :, 0].max(dim=1).values.tolist() == [code for _, _, code in ST.REFUSALS]
    images = [with_status(ONE_ATOM)] + [with_status(im) for _, im, _ in EZ.FLAT_CASES] + [with_status(ST.WIDE), with_status(ST.WIDE_4)]
    el, st = check(images)
    n = len(EZ.FLAT_CASES)
    assert [int(el[1 + k, :, 5][el[1 + k, :, 5] != 0][0]) for k in range(n)] == [code for _, _, code in EZ.FLAT_CASES]
    assert el[n + 1, 0, 0] in (1, -1) and el[n + 2, 0, 0] in (1, -1)      # the products near 2^40 keep their sign


def test_double_bond_cases():
    """every hand-made case of the double-bond rule: marked, ring (cyclohexene), exocyclic, twins (isobutenyl), flat; both marks"""
    images = [with_status(ONE_ATOM)] + [with_status(im) for _, im, _, _ in EZ.CASES] + [with_status(im) for im, *_ in EZ.BOTH]
    el, st = check(images)
    names = [name for name, *_ in EZ.CASES]
    assert el[1 + names.index("cyclohexene"), 0, 5] == L.EZ_RING and el[1 + names.index("isobutenyl"), 1, 5] == L.EZ_TWIN
    exo = el[1 + names.index("exocyclic, unsymmetric ring"), 5].tolist()
    assert exo[5:] == [-1, 6, 6, 0, 4, 7, -1]      # by hand: opposite, bond row 6, partner 6, substituents 0 and 4, the partner's 7


def test_seeded_molecules():
    for seed, recipe in ((21, ST.random_images), (22, EZ.random_images)):
        images = [with_status(ONE_ATOM)] + [with_status(im) for im in recipe(seed, 15)]
        check(images)


def test_rows_the_writer_refuses_and_status_bits():
    worked = ST.worked(5)
    duplicate = (worked[0], worked[1] + [(3, 1, 1, 3)], [])
    out_of_range = (worked[0], [(1, 2, 5, 0), (1, 9, 1, 1), (1, 4, 1, 2)], [])
    bad_symbol = ([(20, 20, 14, 0, 0)] + list(worked[0][1:]), worked[1], [])
    bad_order = (worked[0], [(1, 2, 7, 0), (1, 3, 1, 1), (1, 4, 1, 2)], [])
    listed_junk = (worked[0], worked[1], [0, 77, -3])
    images = [with_status(ONE_ATOM), with_status(worked, L.MOL_EMPTY | L.MOL_TRUNCATED), with_status(duplicate), with_status(worked, L.MOL_TRUNCATED),
              with_status(out_of_range), with_status(bad_symbol), with_status(bad_order), with_status(listed_junk), with_status(([], [], [])),
              with_status(EZ.CASES[0][1], L.MOL_TRUNCATED)]
    el, st = check(images)
    assert st[:, 3].tolist() == [0, 3, 4, 2, 4, 4, 4, 0, 0, 2]
    none = torch.tensor(D.STEREO_NONE_ROW, dtype=torch.int32)
    for b in (1, 2, 4, 5, 6, 8):
        assert torch.equal(el[b], none.expand(32, 12))


def long_chain():
    """a 300-atom molecule at cap_atoms 512: a zigzag chain of 299 carbons, a double bond between atoms 270 and 271, and a fluorine
    (atom 299) on a wedge from atom 280, whose rows are 298 (the wedge) and 270 (the double bond): the second atom of a thread,
    and more bond rows than threads"""
    places = [(10 * (i % 2) + 20, 10 * i) for i in range(299)] + [(45, 2800)]
    bonds = [(i + 1, i + 2, 2 if i == 270 else 1) for i in range(298)] + [(281, 300, 5)]
    return ST.rows(["C"] * 299 + ["F"], places, bonds)


def test_a_long_chain_past_one_atom_per_thread():
    image = long_chain()
    assert len(image[1]) > 256
    el, st = check([with_status(image), with_status(ONE_ATOM)], cap_atoms=512, cap_bonds=512)
    assert st[0].tolist() == [1, 1, 0, 0]
    assert el[0, 280, 0] in (1, -1) and el[0, 280, 1:5].tolist() == [279, 281, 299, -1]
    assert el[0, 270, 5] in (1, -1) and el[0, 270, 6:].tolist() == [270, 271, 269, -1, 272, -1]


def test_at_the_capacity_of_512_atoms():
    """MAX_ATOMS == 2 * ST, the last thread's second atom: the 512-carbon zigzag polyene (255 marked double bonds; the last candidate
    has its lower end at index 509 and the last atom, 511, for a substituent) and the 512-atom chain with the wedge from atom 500"""
    images = [with_status(EZ.zigzag_polyene(512)), with_status(ST.wedged_chain()), with_status(ONE_ATOM)]
    el, st = check(images, cap_atoms=512, cap_bonds=512)
    assert st[0, 1] == 255 and st[1, 0] == 1


def test_a_second_run_overwrites_every_word_and_is_capturable():
    first = [with_status(im) for im in ST.random_images(23, 8)]
    second = [with_status(ONE_ATOM), with_status(ST.worked(6)), with_status(ST.worked(5), L.MOL_EMPTY)] + [with_status(im) for im in EZ.random_images(24, 5)]
    up = upload(first, 32, 32)
    op = StereoPerceiver(*up)
    op.run()
    torch.cuda.synchronize()
    want, want_stats = expected(first, 32)
    assert torch.equal(op.elements(), want) and torch.equal(op.stat.cpu(), want_stats)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, capture_error_mode="thread_local"):
        op.run()
    for dst, src in zip(up, upload(second, 32, 32)):
        dst.copy_(src)
    g.replay()
    torch.cuda.synchronize()
    want, want_stats = expected(second, 32)
    assert torch.equal(op.elements(), want) and torch.equal(op.stat.cpu(), want_stats)


def test_refusals_launch_nothing():
    lib = L.load()
    up = upload([with_status(ST.worked(5))], 16, 16)
    op = StereoPerceiver(*up)
    op.run()
    torch.cuda.synchronize()
    before = (op.table.clone(), op.stat.clone())

    def refused(code, **fields):
        d = L.StereoDesc()
        C.memmove(C.byref(d), C.byref(op.d), C.sizeof(d))
        for k, v in fields.items():
            setattr(d, k, v)
        assert lib.abc_perceive_stereo(C.byref(d), torch.cuda.current_stream().cuda_stream) == code, fields

    assert lib.abc_perceive_stereo(C.byref(L.StereoDesc()), None) == EINVAL
    refused(EUNSUPPORTED, cap_atoms=513)
    refused(EUNSUPPORTED, cap_mol_bonds=4097)
    refused(EINVAL, mol_implh=None)
    refused(EINVAL, elements=None)
    refused(EINVAL, stats=None)
    refused(EINVAL, B=0)
    torch.cuda.synchronize()
    assert torch.equal(op.table, before[0]) and torch.equal(op.stat, before[1])
    with pytest.raises(ValueError, match="512"):
        StereoPerceiver(*upload([with_status(ONE_ATOM)], 513, 16))
