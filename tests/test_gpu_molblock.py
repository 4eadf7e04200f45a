"""GPU parity of the device mol block writer (abc_write_molblocks, ops.MolBlockWriter) against the host form
decode.Molecule.molblock(), which tests/golden/assemble_128.npz pins to the reference's own text.  Bytes and integers: exact, no
tolerance anywhere."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import abcnet_amd  # noqa: E402,F401
from abcnet_amd import _lib as L  # noqa: E402
from abcnet_amd.decode import Molecule  # noqa: E402
from abcnet_amd.ops import GraphAssembler, MolBlockWriter  # noqa: E402
from abcnet_amd.synthetic import synthetic_images  # noqa: E402
from molrows import assemble_golden, filled_unet  # noqa: E402

DEV = "cuda"
POSITIONS = (0, 59, 60, 61, 659, 660, 199999)
CHARGES = (-15, -1, 0, 1, 15)


def _rows(images, cap_atoms, cap_bonds):
    """hand-made rows [(atoms [n,5], bonds [m,4], implh [k], status)] as device tensors of the assembler's layout; the rows past
    the counts hold a pattern the writer must not read (an index the vocabulary does not have)"""
    B = len(images)
    cnt = torch.zeros(B, 4, dtype=torch.int32)
    atoms = torch.full((B, cap_atoms, 5), 77, dtype=torch.int32)
    bonds = torch.full((B, cap_bonds, 4), 77, dtype=torch.int32)
    implh = torch.full((B, cap_atoms), 77, dtype=torch.int32)
    for b, (a, q, h, status) in enumerate(images):
        a, q, h = np.asarray(a, dtype=np.int64).reshape(-1, 5), np.asarray(q, dtype=np.int64).reshape(-1, 4), np.asarray(h, dtype=np.int64).reshape(-1)
        atoms[b, :len(a)] = torch.as_tensor(a, dtype=torch.int32)
        bonds[b, :len(q)] = torch.as_tensor(q, dtype=torch.int32)
        implh[b, :len(h)] = torch.as_tensor(h, dtype=torch.int32)
        cnt[b] = torch.tensor([len(a), len(q), len(h), status], dtype=torch.int32)
    return cnt.to(DEV), atoms.to(DEV), bonds.to(DEV), implh.to(DEV)


def _oracle(images):
    return [None if s & L.MOL_EMPTY else Molecule.from_device_rows(a, q, h, truncated=bool(s & L.MOL_TRUNCATED)).molblock()
            for a, q, h, s in images]


def _molecule(rng, n, m, k, wild=True):
    atoms = np.stack([rng.choice(POSITIONS, n), rng.choice(POSITIONS, n), rng.integers(0, 14, n), rng.choice(CHARGES, n),
                      rng.integers(0, 3, n)], axis=1).reshape(-1, 5)
    ends = np.array([1, 2, max(n, 1), n + 1, 0, -3, 2 ** 31 - 1, -2 ** 31]) if wild else np.arange(1, max(n, 1) + 1)
    bonds = np.stack([rng.choice(ends, m), rng.choice(ends, m), np.arange(m) % 8 if wild else 1 + np.arange(m) % 6, np.arange(m)],
                     axis=1).reshape(-1, 4)
    implh = rng.choice(ends, k)
    return atoms, bonds, implh, 0


def _long_batch():
    """B = 6 at cap_atoms 1024: EMPTY, zero atoms and bonds, TRUNCATED, 9 and 10 implicit-H entries, 1000 atoms and bonds"""
    rng = np.random.default_rng(5)
    two = np.array([[60, 61, 6, -1, 0], [0, 199999, 10, 15, 1], [659, 660, 13, 0, 2], [59, 60, 8, 1, 0]])     # Cl, Se, Si, Br
    empty = (two, np.array([[1, 2, 1, 0]]), [1], L.MOL_EMPTY)            # (rows behind an EMPTY status are not text)
    nothing = (np.zeros((0, 5)), np.zeros((0, 4)), [], 0)
    truncated = _molecule(rng, 40, 64, 3)[:3] + (L.MOL_TRUNCATED,)
    nine, ten = _molecule(rng, 12, 8, 9), _molecule(rng, 12, 8, 10)
    big = _molecule(rng, 1000, 1000, 120)
    big[1][:8, 2] = np.arange(8)                                          # orders 0..7
    big[1][-1, :2] = (1000, 999)
    return [empty, nothing, truncated, nine, ten, big]


def _run(images, cap_atoms, cap_bonds, cap_text=None):
    w = MolBlockWriter(*_rows(images, cap_atoms, cap_bonds), cap_text=cap_text)
    w.run()
    torch.cuda.synchronize()
    return w


def _check_index(w, texts):
    idx = w.index.cpu().tolist()
    off, status = idx[:w.B + 1], idx[w.B + 1:]
    assert off[0] == 0 and all(b >= a for a, b in zip(off, off[1:]))
    assert [b - a for a, b in zip(off, off[1:])] == [0 if t is None else len(t) for t in texts]
    return off, status


def test_golden_cases_give_the_reference_text(golden_dir):
    """every case of assemble_128.npz in one batch (capacities 128 / 2048): assembler -> writer == the text the reference wrote"""
    cases = assemble_golden(golden_dir)
    B, cap_atoms, cap_bonds = len(cases), 128, 2048
    cnt = torch.zeros(B, 4, dtype=torch.int32)
    atoms, bonds = torch.zeros(B, cap_atoms, 5, dtype=torch.int32), torch.zeros(B, cap_bonds, 4, dtype=torch.int32)
    rho = torch.zeros(B, cap_bonds, dtype=torch.float32)
    for b, (_, c) in enumerate(cases):
        n, m = len(c["atoms"]), len(c["bonds"])
        atoms[b, :n] = torch.as_tensor(np.asarray(c["atoms"]).reshape(-1, 5), dtype=torch.int32)
        bonds[b, :m] = torch.as_tensor(np.asarray(c["bonds"]).reshape(-1, 4), dtype=torch.int32)
        rho[b, :m] = torch.as_tensor(np.asarray(c["rho"], dtype=np.float32))
        cnt[b] = torch.tensor([n, n, max(m, 1), m], dtype=torch.int32)
    asm = GraphAssembler(cnt.to(DEV), atoms.to(DEV), bonds.to(DEV), rho.to(DEV))
    w = MolBlockWriter.from_assembler(asm)
    assert w.cap_text == B * w.image_bytes
    asm.run()
    w.run()
    torch.cuda.synchronize()
    got = w.molblocks()
    want = [str(c["molblock"]) for _, c in cases]
    for b, (name, _) in enumerate(cases):
        assert got[b] == want[b], name
    _, status = _check_index(w, want)
    assert status == [0] * B and w.status() == status


def test_hand_made_rows_equal_the_host_form():
    images = _long_batch()
    want = _oracle(images)
    assert want[0] is None and want[1] == Molecule([], [], [], [], [], [], []).molblock()
    assert "1000" in want[5].split("\n")[3][:8] and "M  STY  10   1 DAT" in want[4] and "M  STY  9   1 DAT" in want[3]
    w = _run(images, 1024, 1024)
    got = w.molblocks()
    for b in range(len(images)):
        assert got[b] == want[b], b
    _, status = _check_index(w, want)
    assert status == [L.MOL_EMPTY, 0, L.MOL_TRUNCATED, 0, 0, 0]


def test_refused_rows():
    """a vocabulary index of 14, one of -1 and a position of 200000, each in its own image between intact ones"""
    rng = np.random.default_rng(6)
    images = [_molecule(rng, 20 + b, 18, 2) for b in range(7)]
    images[1][0][19, 2] = 14
    images[3][0][0, 2] = -1
    images[5][0][7, 1] = 200000
    want = [None if b in (1, 3, 5) else _oracle([im])[0] for b, im in enumerate(images)]
    w = _run(images, 32, 32)
    off, status = _check_index(w, want)
    assert status == [0, L.TEXT_BAD_ROW, 0, L.TEXT_BAD_ROW, 0, L.TEXT_BAD_ROW, 0] and w.status() == status
    raw = w.text[:off[-1]].cpu().numpy().tobytes()
    for b in (0, 2, 4, 6):
        assert raw[off[b]:off[b + 1]].decode("ascii") == want[b], b
    with pytest.raises(L.AbcNetHipError, match="image 1 .*BAD_ROW"):
        w.molblocks()
    # a position of -1 is refused as well; 199999 and index 13 are not
    edge = [_molecule(rng, 4, 3, 0) for _ in range(2)]
    edge[0][0][2, 0] = -1
    edge[1][0][2] = (199999, 199999, 13, 0, 0)
    w = _run(edge, 8, 8)
    assert w.status() == [L.TEXT_BAD_ROW, 0]


def test_capacity_is_a_prefix_rule():
    rng = np.random.default_rng(7)
    images = [_molecule(rng, 10 + 3 * b, 12, b % 3) for b in range(5)] + [(np.zeros((0, 5)), np.zeros((0, 4)), [], L.MOL_EMPTY)]
    want = _oracle(images)
    total = sum(len(t) for t in want[:5])
    rows = _rows(images, 32, 32)
    w = MolBlockWriter(*rows, cap_text=total + 4096)
    # the same buffers behind a smaller cap_text: everything at or beyond it must stay as it is
    w.text.fill_(0xA5)
    w.d.cap_text = total - 1
    w.run()
    torch.cuda.synchronize()
    off, status = _check_index(w, want[:4] + [None, None])
    assert status == [0, 0, 0, 0, L.TEXT_OVERFLOW, L.MOL_EMPTY | L.TEXT_OVERFLOW]
    raw = w.text.cpu().numpy()
    for b in range(4):
        assert raw[off[b]:off[b + 1]].tobytes().decode("ascii") == want[b], b
    assert off[-1] == total - len(want[4]) and (raw[off[-1]:] == 0xA5).all()
    with pytest.raises(L.AbcNetHipError, match="image 4 .*OVERFLOW"):
        w.molblocks()
    # below the first image's length: nothing is written at all
    w.text.fill_(0xA5)
    w.d.cap_text = len(want[0]) - 1
    w.run()
    torch.cuda.synchronize()
    off, status = _check_index(w, [None] * 6)
    assert off == [0] * 7 and all(s & L.TEXT_OVERFLOW for s in status) and (w.text.cpu().numpy() == 0xA5).all()
    # exactly the total: everything fits
    w.d.cap_text = total
    w.run()
    torch.cuda.synchronize()
    assert w.molblocks() == want
    with pytest.raises(ValueError, match="cap_text"):
        MolBlockWriter(*rows, cap_text=2 ** 31)
    with pytest.raises(ValueError, match="cap_text"):
        MolBlockWriter(*rows, cap_text=0)


def test_a_short_batch_after_a_long_one_shows_nothing_stale():
    long_images = _long_batch()
    cnt, atoms, bonds, implh = _rows(long_images, 1024, 1024)
    w = MolBlockWriter(cnt, atoms, bonds, implh)
    w.run()
    torch.cuda.synchronize()
    assert w.molblocks() == _oracle(long_images)
    rng = np.random.default_rng(8)
    short = [_molecule(rng, 3 + b, 2 + b, b % 2, wild=False) for b in range(6)]
    for dst, src in zip((cnt, atoms, bonds, implh), _rows(short, 1024, 1024)):
        dst.copy_(src)
    w.run()
    torch.cuda.synchronize()
    want = _oracle(short)
    assert w.molblocks() == want
    off, status = _check_index(w, want)
    assert off[-1] == sum(len(t) for t in want) and status == [0] * 6


def test_inference_runner_with_molblocks():
    """eager, captured and replayed steps (another batch before the replay): the device text is the host form's of molecules()"""
    from abcnet_amd.infer import InferenceRunner
    m = filled_unet(dropout_p=0.0)
    with pytest.raises(ValueError, match="assemble=True"):
        InferenceRunner(m, 2, 128, 128, molblocks=True)
    run = InferenceRunner(m, 2, 128, 128, use_graph=True, assemble=True, molblocks=True)
    seen = 0
    for seed in (7, 8, 9):
        run.load_batch(synthetic_images(2, 128, seed=seed).to(DEV))
        run.step()
        torch.cuda.synchronize()
        want = [mol.molblock() if mol is not None else None for mol in run.molecules()]
        assert run.molblocks() == want, seed
        seen += sum(t is not None for t in want)
    print("images with a molecule over the three steps: %d of 6" % seen)
    assert run._graph is not None
    plain = InferenceRunner(m, 2, 128, 128, use_graph=False, assemble=True)
    with pytest.raises(L.AbcNetHipError):
        plain.molblocks()
