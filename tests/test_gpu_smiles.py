"""GPU parity of the device SMILES writer (abc_write_smiles, ops.SmilesWriter) against the host form decode.Molecule.smiles(), which
tests/test_smiles_host.py holds to the rule's example table and to a second transcription of the rule.  Bytes and integers: exact,
no tolerance anywhere."""
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
from abcnet_amd.ops import GraphAssembler, GraphIdentity, SmilesWriter  # noqa: E402
from abcnet_amd.synthetic import synthetic_images  # noqa: E402
import smiles_oracle as O  # noqa: E402
from molrows import assemble_golden, filled_unet  # noqa: E402
from smiles_cases import (EXAMPLES, SYMBOLS, chain, complete, graph_of_rows, graph_of_text, random_rows, records_of_text,  # noqa: E402
                          same_graph, star)

DEV = "cuda"
NOTHING = ([], [], [])


def _rows(images, cap_atoms, cap_bonds):
    """hand-made rows [(atoms [n,5], bonds [m,4], implh [k], status)] as device tensors of the assembler's layout; the rows past
    the counts hold a pattern the writer must not read (an index the vocabulary does not have, a bond no atom has)"""
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


def _host(image):
    """the host form of one image: the text, or None (EMPTY), "bad_row" / "ring_limit" for what the rule refuses"""
    a, q, h, status = image
    if status & L.MOL_EMPTY:
        return None
    if any(not 0 <= row[2] <= 13 for row in a):      # (from_device_rows cannot name such an atom's symbol)
        return "bad_row"
    try:
        return Molecule.from_device_rows(np.asarray(a).reshape(-1, 5), np.asarray(q).reshape(-1, 4), h).smiles()
    except ValueError as e:
        return "ring_limit" if "ring limit" in str(e) else "bad_row"


def _check(w, images):
    """index, status words and bytes of the last run against the host form; returns the texts (None where none is written)"""
    want = [_host(im) for im in images]
    bits = {"bad_row": L.TEXT_BAD_ROW, "ring_limit": L.TEXT_RING_LIMIT}
    texts = [None if t in bits else t for t in want]
    idx = w.index.cpu().tolist()
    off, status = idx[:w.B + 1], idx[w.B + 1:]
    assert off[0] == 0 and [b - a for a, b in zip(off, off[1:])] == [0 if t is None else len(t) for t in texts]
    assert status == [(im[3] & (L.MOL_EMPTY | L.MOL_TRUNCATED)) | bits.get(t, 0) for im, t in zip(images, want)] and w.status() == status
    raw = w.text[:off[-1]].cpu().numpy().tobytes()
    for b, t in enumerate(texts):
        if t is not None:
            assert raw[off[b]:off[b + 1]].decode("ascii") == t, b
    return texts


def _run(images, cap_atoms, cap_bonds, cap_text=None):
    w = SmilesWriter(*_rows(images, cap_atoms, cap_bonds), cap_text=cap_text)
    w.run()
    torch.cuda.synchronize()
    return w


def _random_images(seed, count):
    rng = np.random.default_rng(seed)
    return [random_rows(rng) + (0,) for _ in range(count)]


def test_golden_cases_through_assembler_and_writer(golden_dir):
    """every case of assemble_128.npz in one batch (capacities 128 / 2048): the device text is the host form's of molecules(), and
    it reads back as the graph of the rows"""
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
    w = SmilesWriter.from_assembler(asm)
    assert w.cap_text == B * w.image_bytes and w.image_bytes == 12 * cap_atoms + 7 * asm.cap_mol_bonds
    asm.run()
    w.run()
    torch.cuda.synchronize()
    got, mols = w.smiles(), asm.molecules()
    assert w.status() == [0] * B
    mc, ma, mq, mh = (t.cpu().numpy() for t in asm.rows.tensors)
    for b, (name, _) in enumerate(cases):
        assert got[b] == mols[b].smiles(), name
        n, m, k, _ = mc[b]
        rows = (ma[b, :n].tolist(), mq[b, :m].tolist(), mh[b, :k].tolist())
        assert same_graph(graph_of_text(O.parse(got[b])), graph_of_rows(rows)), name
    assert sum(len(t) > 100 for t in got) >= 3 and "" in got      # (the dense decoded images and the 110 atoms; one_atom_only)


def test_hand_made_rows_equal_the_host_form():
    """cap_atoms 512: EMPTY, zero atoms, TRUNCATED, the example table, a 512-atom chain, a degree-511 star, K19 and K20 in one
    batch, then 200 graphs of the host suite's recipe, 8 per batch, through the same buffers"""
    rng = np.random.default_rng(31)
    empty = EXAMPLES[0][1] + (L.MOL_EMPTY,)                 # (rows behind an EMPTY status are not text)
    truncated = random_rows(rng) + (L.MOL_TRUNCATED,)
    shuffled_star = star(512)
    rng.shuffle(shuffled_star[1])
    images = ([empty, NOTHING + (0,), truncated] + [rows + (0,) for _, rows, _ in EXAMPLES]
              + [chain(512) + (0,), shuffled_star + (0,), complete(19) + (0,), complete(20) + (0,)])
    w = _run(images, 512, 512)
    texts = _check(w, images)
    assert texts[:2] == [None, ""] and texts[3:14] == [t for _, _, t in EXAMPLES]
    assert texts[14] == "C" * 512 and texts[15] == "C" + "(C)" * 510 + "C" and len(texts[16]) == 797 and texts[17] is None
    assert w.status()[17] == L.TEXT_RING_LIMIT
    with pytest.raises(L.AbcNetHipError, match="image 17 .*RING_LIMIT"):
        w.smiles()
    rows = _rows([NOTHING + (0,)] * 8, 512, 512)
    w = SmilesWriter(*rows)
    graphs = _random_images(32, 200)
    for at in range(0, 200, 8):
        batch = graphs[at:at + 8]
        for dst, src in zip(rows, _rows(batch, 512, 512)):
            dst.copy_(src)
        w.run()
        torch.cuda.synchronize()
        assert w.smiles() == _check(w, batch), at


CAUSES = [("a vocabulary index of 14", lambda a, q: a.__setitem__(1, (0, 0, 14, 0, 0))),
          ("a vocabulary index of -1", lambda a, q: a.__setitem__(0, (0, 0, -1, 0, 0))),
          ("a charge of 16", lambda a, q: a.__setitem__(2, (0, 0, 1, 16, 0))),
          ("a charge of -16", lambda a, q: a.__setitem__(2, (0, 0, 1, -16, 0))),
          ("an order of 0", lambda a, q: q.__setitem__(0, (1, 2, 0, 0))),
          ("an order of 7", lambda a, q: q.__setitem__(0, (1, 2, 7, 0))),
          ("an end of 0", lambda a, q: q.__setitem__(1, (0, 3, 1, 1))),
          ("an end past n", lambda a, q: q.__setitem__(1, (2, len(a) + 1, 1, 1))),
          ("an end of -2^31", lambda a, q: q.__setitem__(1, (-2 ** 31, 2, 1, 1))),
          ("both ends on one atom", lambda a, q: q.__setitem__(1, (3, 3, 1, 1))),
          ("a pair listed twice", lambda a, q: q.append((q[0][1], q[0][0], 2, 3))),
          ("a pair listed twice, the same way", lambda a, q: q.append(q[-1]))]


def test_refused_rows():
    """each cause in its own image between intact ones: the neighbours keep their bytes, smiles() names the image"""
    rng = np.random.default_rng(33)
    images = []
    for _, spoil in CAUSES:
        images.append(random_rows(rng) + (0,))
        atoms, bonds, implh = random_rows(rng)
        while len(atoms) < 4 or len(bonds) < 3:
            atoms, bonds, implh = random_rows(rng)
        spoil(atoms, bonds)
        images.append((atoms, bonds, implh, 0))
    images.append(random_rows(rng) + (0,))
    w = _run(images, 64, 96)
    texts = _check(w, images)
    status = w.status()
    assert status[1::2] == [L.TEXT_BAD_ROW] * len(CAUSES) and status[0::2] == [0] * (len(CAUSES) + 1)
    assert all(t is not None for t in texts[0::2])
    with pytest.raises(L.AbcNetHipError, match="image 1 .*BAD_ROW"):
        w.smiles()
    # the edges that are NOT refused: index 13, charges -15 and 15, order 6, an end of n
    edge = ([(0, 0, 13, 15, 0), (0, 0, 0, -15, 0), (0, 0, 12, 0, 0)], [(3, 1, 6, 0), (2, 3, 1, 1)], [4, 0])
    w = _run([edge + (0,)], 8, 8)
    assert w.smiles() == _check(w, [edge + (0,)]) == ["[Si+15][H][C-15]"]


def test_capacity_is_a_prefix_rule():
    images = _random_images(34, 5) + [NOTHING + (L.MOL_EMPTY,)]
    want = [_host(im) for im in images]
    assert all(len(t) > 0 for t in want[:5])
    total = sum(len(t) for t in want[:5])
    rows = _rows(images, 64, 96)
    w = SmilesWriter(*rows, cap_text=total + 4096)
    # the same buffers behind a smaller cap_text: everything at or beyond it must stay as it is
    w.text.fill_(0xA5)
    w.d.cap_text = total - 1
    w.run()
    torch.cuda.synchronize()
    idx = w.index.cpu().tolist()
    off, status = idx[:7], idx[7:]
    assert [b - a for a, b in zip(off, off[1:])] == [len(t) for t in want[:4]] + [0, 0]
    assert status == [0, 0, 0, 0, L.TEXT_OVERFLOW, L.MOL_EMPTY | L.TEXT_OVERFLOW]
    raw = w.text.cpu().numpy()
    for b in range(4):
        assert raw[off[b]:off[b + 1]].tobytes().decode("ascii") == want[b], b
    assert off[-1] == total - len(want[4]) and (raw[off[-1]:] == 0xA5).all()
    with pytest.raises(L.AbcNetHipError, match="image 4 .*OVERFLOW"):
        w.smiles()
    # below the first image's length: nothing is written at all
    w.text.fill_(0xA5)
    w.d.cap_text = len(want[0]) - 1
    w.run()
    torch.cuda.synchronize()
    idx = w.index.cpu().tolist()
    assert idx[:7] == [0] * 7 and all(s & L.TEXT_OVERFLOW for s in idx[7:]) and (w.text.cpu().numpy() == 0xA5).all()
    # exactly the total: everything fits
    w.d.cap_text = total
    w.run()
    torch.cuda.synchronize()
    assert w.smiles() == want
    assert (w.text.cpu().numpy()[total:] == 0xA5).all()
    with pytest.raises(ValueError, match="cap_text"):
        SmilesWriter(*rows, cap_text=2 ** 31)
    with pytest.raises(ValueError, match="cap_text"):
        SmilesWriter(*rows, cap_text=0)


def test_a_short_batch_after_a_long_one_shows_nothing_stale():
    long_images = [chain(500) + (0,), complete(19) + (0,), star(300) + (0,)] + _random_images(35, 3)
    rows = _rows(long_images, 512, 512)
    w = SmilesWriter(*rows)
    w.run()
    torch.cuda.synchronize()
    assert w.smiles() == _check(w, long_images)
    short = [rows_ + (0,) for _, rows_, _ in EXAMPLES[:5]] + [NOTHING + (0,)]
    for dst, src in zip(rows, _rows(short, 512, 512)):
        dst.copy_(src)
    w.run()
    torch.cuda.synchronize()
    assert w.smiles() == _check(w, short) == [t for _, _, t in EXAMPLES[:5]] + [""]


def test_the_device_text_is_the_same_molecule_on_the_device():
    """the loop closed on the device: the device text, read by the oracle's reader, goes in as a graph record beside the rows it
    was written from, and the verified isomorphism stage calls every image the same"""
    # (the identity stage reads a record's atoms off its bonds, as the assembler's compaction leaves them: no atom without a bond)
    bonded = lambda im: {e for q in im[1] for e in q[:2]} == set(range(1, len(im[0]) + 1))
    images = [im for im in [rows + (0,) for _, rows, _ in EXAMPLES] + _random_images(36, 60) if bonded(im)]
    assert len(images) >= 24
    cnt, atoms, bonds, implh = _rows(images, 64, 96)
    w = SmilesWriter(cnt, atoms, bonds, implh)
    w.run()
    torch.cuda.synchronize()
    texts = w.smiles()
    class_of = {s: SYMBOLS.index(s, 1) for s in SYMBOLS}
    gi = GraphIdentity(cnt, atoms, bonds, max_atoms=64, max_bonds=96)
    gi.load([records_of_text(O.parse(t), class_of) for t in texts])
    gi.run()
    torch.cuda.synchronize()
    res = gi.result()
    assert res["counted"] == len(images) and res["same"] == len(images) and res["undecided"] == 0 and res["different"] == 0


def test_inference_runner_with_smiles():
    """eager, captured and replayed steps (another batch before the replay): the device text is the host form's of molecules(),
    and the mol block stage beside it still gives its own text"""
    from abcnet_amd.infer import InferenceRunner
    m = filled_unet(dropout_p=0.0)
    with pytest.raises(ValueError, match="smiles=True.*assemble=True"):
        InferenceRunner(m, 2, 128, 128, smiles=True)
    run = InferenceRunner(m, 2, 128, 128, use_graph=True, assemble=True, smiles=True)
    both = InferenceRunner(m, 2, 128, 128, use_graph=True, assemble=True, molblocks=True, smiles=True)
    assert both._stages.index("smiler") == both._stages.index("texter") + 1 == both._stages.index("assembler") + 2
    seen = 0
    for seed in (7, 8, 9):
        for r in (run, both):
            r.load_batch(synthetic_images(2, 128, seed=seed).to(DEV))
            r.step()
        torch.cuda.synchronize()
        mols = run.molecules()
        want = [mol.smiles() if mol is not None else None for mol in mols]
        assert run.smiles() == want and both.smiles() == want, seed
        assert both.molblocks() == [mol.molblock() if mol is not None else None for mol in mols], seed
        seen += sum(t is not None for t in want)
    print("images with a molecule over the three steps: %d of 6" % seen)
    assert run._graph is not None and both._graph is not None
    plain = InferenceRunner(m, 2, 128, 128, use_graph=False, assemble=True)
    with pytest.raises(L.AbcNetHipError, match="smiles=True"):
        plain.smiles()
