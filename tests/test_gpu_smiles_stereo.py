"""GPU parity of the stereo form of the device SMILES writer (abc_write_smiles_stereo, ops.SmilesWriter(stereo=True)) against the host
form decode.Molecule.smiles(stereo=True) and the second transcription of the rule (smiles_stereo_oracle), which
tests/test_smiles_stereo_host.py holds to each other and to the geometry.  Bytes and integers: exact, no tolerance anywhere."""
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
from abcnet_amd.decode import Molecule  # noqa: E402
from abcnet_amd.ops import GraphAssembler, SmilesWriter  # noqa: E402
from abcnet_amd.synthetic import synthetic_images  # noqa: E402
import smiles_stereo_oracle as S  # noqa: E402
from molrows import assemble_golden, filled_unet  # noqa: E402
from smiles_cases import chain, complete  # noqa: E402
from smiles_cases import random_rows as plain_random_rows  # noqa: E402
from smiles_stereo_cases import CASES, REFUSALS, WIDE, WIDE_4, random_images, wedged_chain  # noqa: E402

DEV = "cuda"
EINVAL, EUNSUPPORTED = -1, -2
NOTHING = ([], [], [])


def _rows(images, cap_atoms, cap_bonds):
    """hand-made rows [(atoms [n,5], bonds [m,4], implh [k], status)] as device tensors of the assembler's layout; the rows past
    the counts hold a pattern the writer must not read (an index the vocabulary does not have, a wedge no atom has)"""
    B = len(images)
    cnt = torch.zeros(B, 4, dtype=torch.int32)
    atoms = torch.full((B, cap_atoms, 5), 77, dtype=torch.int32)
    bonds = torch.full((B, cap_bonds, 4), 5, dtype=torch.int32)
    implh = torch.full((B, cap_atoms), 77, dtype=torch.int32)
    for b, (a, q, h, status) in enumerate(images):
        a, q, h = np.asarray(a, dtype=np.int64).reshape(-1, 5), np.asarray(q, dtype=np.int64).reshape(-1, 4), np.asarray(h, dtype=np.int64).reshape(-1)
        atoms[b, :len(a)] = torch.as_tensor(a, dtype=torch.int32)
        bonds[b, :len(q)] = torch.as_tensor(q, dtype=torch.int32)
        implh[b, :len(h)] = torch.as_tensor(h, dtype=torch.int32)
        cnt[b] = torch.tensor([len(a), len(q), len(h), status], dtype=torch.int32)
    return cnt.to(DEV), atoms.to(DEV), bonds.to(DEV), implh.to(DEV)


def _molecule(image):
    return Molecule.from_device_rows(np.asarray(image[0]).reshape(-1, 5), np.asarray(image[1]).reshape(-1, 4), image[2])


def _expected(image):
    """(text or None / "bad_row" / "ring_limit", codes, stats) of one image by the host form, which must agree with the oracle"""
    a, q, h, status = image
    if status & L.MOL_EMPTY:
        return None, [], (0, 0, 0, 0)
    if any(not 0 <= row[2] <= 13 for row in a):      # (from_device_rows cannot name such an atom's symbol)
        return "bad_row", [], (0, 0, 0, 0)
    try:
        m = _molecule(image)
        text, codes = m.smiles(stereo=True), m.stereo_centres()
    except ValueError as e:
        return ("ring_limit" if "ring limit" in str(e) else "bad_row"), [], (0, 0, 0, 0)
    want, _, want_codes, stats = S.write(a, q, h)
    assert text == want and codes == want_codes
    return text, codes, stats


def _check(w, images):
    """index, status words, bytes, stereo_stats and stereo_out of the last run against the host form and the oracle; returns the
    texts (None where none is written)"""
    want = [_expected(im) for im in images]
    bits = {"bad_row": L.TEXT_BAD_ROW, "ring_limit": L.TEXT_RING_LIMIT}
    texts = [None if t in bits else t for t, _, _ in want]
    idx = w.index.cpu().tolist()
    off, status = idx[:w.B + 1], idx[w.B + 1:]
    assert off[0] == 0 and [b - a for a, b in zip(off, off[1:])] == [0 if t is None else len(t) for t in texts]
    assert status == [(im[3] & (L.MOL_EMPTY | L.MOL_TRUNCATED)) | bits.get(t, 0) for im, (t, _, _) in zip(images, want)]
    raw = w.text[:off[-1]].cpu().numpy().tobytes()
    for b, t in enumerate(texts):
        if t is not None:
            assert raw[off[b]:off[b + 1]].decode("ascii") == t, b
    stats = torch.tensor([list(s) for _, _, s in want], dtype=torch.int32)
    codes = torch.zeros(w.B, w.cap_atoms, dtype=torch.int32)
    for b, (_, c, _) in enumerate(want):
        codes[b, :len(c)] = torch.tensor(c, dtype=torch.int32)
    assert torch.equal(w.stats.cpu(), stats)
    assert torch.equal(w.parities(), codes)
    res = w.stereo_stats()
    assert res["rows"] == stats.tolist() and [res[k] for k in L.SMILES_STEREO_COLUMNS] == stats.sum(0).tolist()
    return texts


def _run(images, cap_atoms, cap_bonds, cap_text=None, stereo=True):
    w = SmilesWriter(*_rows(images, cap_atoms, cap_bonds), cap_text=cap_text, stereo=stereo)
    w.run()
    torch.cuda.synchronize()
    return w


HAND = [im + (0,) for _, im, _ in CASES] + [im + (0,) for _, im, _ in REFUSALS] + [WIDE + (0,), WIDE_4 + (0,)]
RANDOM = [im + (0,) for im in random_images(41, 120)]      # (the images of the host suite, whose generator conditions it asserts)


@pytest.fixture(scope="module")
def device_texts():
    """every hand-made case and every random image through the device once, 64 at most per batch, capacities 32 / 48: checked
    against host form and oracle here, read back by the next test"""
    images = HAND + RANDOM
    texts = []
    for at in range(0, len(images), 64):
        batch = images[at:at + 64]
        w = _run(batch, 32, 48)
        assert w.image_bytes == 14 * 32 + 7 * 48
        got = _check(w, batch)
        assert w.smiles() == got
        texts += got
    return images, texts


def test_device_text_stats_and_codes_equal_host_form_and_oracle(device_texts):
    images, texts = device_texts
    assert texts[:len(CASES)][:3] == ["[C@H](N)(C)O", "[C@@H](N)(C)O", "C(N)(C)O"]
    assert [t for (_, _, t), got in zip(CASES, texts) if t is not None and t != got] == []
    assert all("@" not in t for t in texts[len(CASES):len(CASES) + len(REFUSALS)])
    assert sum("@" in t for t in texts[len(HAND):]) * 2 >= len(RANDOM)


def test_device_text_read_back_agrees_with_the_geometry(device_texts):
    images, texts = device_texts
    marked = 0
    for (a, q, h, _), text in zip(images, texts):
        preorder = S.preorder_of(len(a), q)
        seen = S.read(text, *S.in_text_order(a, q, preorder))
        assert len(seen) == text.count("@") - text.count("@@")
        for p, (written, geometric) in seen.items():
            assert written == geometric, (text, p)
        marked += len(seen)
    assert marked >= 60


def test_wide_indices():
    """cap_atoms 512: a chain of 511 carbons with a methyl on atom 500, the wedge from atom 500 to it"""
    image = wedged_chain() + (0,)
    w = _run([image, chain(512) + (0,)], 512, 512)
    texts = _check(w, [image, chain(512) + (0,)])
    codes = w.parities()
    assert codes[0, 499].item() in (1, -1) and codes[0].abs().sum().item() == 1 and codes[1].abs().sum().item() == 0
    mark = "@" if "[C@H]" in texts[0] else "@@"
    assert texts[0] == "C" * 499 + "[C%sH](" % mark + "C" * 11 + ")C" and texts[1] == "C" * 512
    seen = S.read(texts[0], *S.in_text_order(image[0], image[1], S.preorder_of(512, image[1])))
    assert list(seen) == [499] and seen[499][0] == seen[499][1] == mark


def _plain_images(seed, count):
    """the plain suite's recipe with every wedge made a single bond"""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(count):
        a, q, h = plain_random_rows(rng)
        out.append((a, [(e1, e2, 1 if o >= 5 else o, s) for e1, e2, o, s in q], h, 0))
    return out


def test_a_batch_without_wedges_has_the_plain_bytes():
    images = _plain_images(51, 24)
    tensors = _rows(images, 64, 96)
    plain, stereo = SmilesWriter(*tensors), SmilesWriter(*tensors, stereo=True)
    plain.run()
    stereo.run()
    torch.cuda.synchronize()
    assert plain.image_bytes == 12 * 64 + 7 * 96 and stereo.image_bytes == 14 * 64 + 7 * 96
    assert torch.equal(plain.index, stereo.index)
    n = int(plain.index[len(images)].item())
    assert n > 0 and torch.equal(plain.text[:n], stereo.text[:n])
    assert plain.smiles() == stereo.smiles() == [_molecule(im).smiles() for im in images]
    assert not stereo.stats.any().item() and not stereo.parities().any().item()
    assert stereo.stereo_stats() == dict(marked=0, flat=0, unqualified=0, wedge_rows=0, rows=[[0] * 4] * len(images))
    with pytest.raises(L.AbcNetHipError, match="stereo=True"):
        plain.stereo_stats()
    with pytest.raises(L.AbcNetHipError, match="stereo=True"):
        plain.parities()


def test_a_short_batch_after_a_long_one_shows_nothing_stale():
    long_images = RANDOM[:5] + [HAND[3]]
    tensors = _rows(long_images, 64, 96)
    w = SmilesWriter(*tensors, stereo=True)
    w.run()
    torch.cuda.synchronize()
    assert w.smiles() == _check(w, long_images) and w.stats.any().item() and w.parities().any().item()
    short = [NOTHING + (0,), HAND[2], (HAND[0][0], HAND[0][1], HAND[0][2], L.MOL_EMPTY), NOTHING + (0,), _plain_images(52, 1)[0], HAND[0]]
    for dst, src in zip(tensors, _rows(short, 64, 96)):
        dst.copy_(src)
    w.run()
    torch.cuda.synchronize()
    got = _check(w, short)
    assert got[:4] == ["", "C(N)(C)O", None, ""] and got[5] == "[C@H](N)(C)O"
    assert w.stats.cpu().tolist()[:4] == [[0] * 4, [0, 0, 1, 1], [0] * 4, [0] * 4]


def test_capacity_is_a_prefix_rule_inside_a_marked_token():
    images = [HAND[1], HAND[3], HAND[0], NOTHING + (L.MOL_EMPTY,)]
    want = [_expected(im)[0] for im in images]
    assert want[:3] == ["[C@@H](N)(C)O", "[C@@](F)(Cl)(Br)I", "[C@H](N)(C)O"]
    tensors = _rows(images, 32, 48)
    w = SmilesWriter(*tensors, stereo=True)
    # the same buffers behind a smaller cap_text, which ends behind the "@" of the second image's token: that image and all behind
    # it are left out whole, nothing at or beyond the end of the first is touched, the stats stay what they are
    w.text.fill_(0xA5)
    w.d.cap_text = len(want[0]) + 3
    w.run()
    torch.cuda.synchronize()
    idx = w.index.cpu().tolist()
    assert idx[:5] == [0] + [len(want[0])] * 4
    assert idx[5:] == [0, L.TEXT_OVERFLOW, L.TEXT_OVERFLOW, L.MOL_EMPTY | L.TEXT_OVERFLOW]
    raw = w.text.cpu().numpy()
    assert raw[:len(want[0])].tobytes().decode("ascii") == want[0] and (raw[len(want[0]):] == 0xA5).all()
    assert w.stats.cpu().tolist() == [[1, 0, 0, 1]] * 3 + [[0] * 4]
    with pytest.raises(L.AbcNetHipError, match="image 1 .*OVERFLOW"):
        w.smiles()
    # inside the first image's own token: nothing at all
    w.d.cap_text = 4
    w.text.fill_(0xA5)
    w.run()
    torch.cuda.synchronize()
    assert w.index.cpu().tolist()[:5] == [0] * 5 and (w.text.cpu().numpy() == 0xA5).all()
    # exactly the total
    total = sum(len(t) for t in want[:3])
    w.d.cap_text = total
    w.run()
    torch.cuda.synchronize()
    assert w.smiles() == want and (w.text.cpu().numpy()[total:] == 0xA5).all()


def test_refused_images_have_zero_stats():
    """BAD_ROW before and after the centres are looked at, RING_LIMIT after: wedge rows and would-be centres in each, zeros for all"""
    a, q, h = (list(v) for v in CASES[0][1])
    bad_atom = (a[:3] + [(25, 11, 14, 0, 0)], q, h, 0)                       # a vocabulary index of 14
    bad_order = (a, q[:2] + [(1, 4, 7, 2)], h, 0)                            # an order of 7
    twice = (a, q + [(2, 1, 6, 3)], h, 0)                                    # the pair of the wedge a second time (found in step 2)
    k20 = complete(20)
    ring_limit = (k20[0], [(e1, e2, 5, s) for e1, e2, _, s in k20[1]], [], 0)
    k19 = complete(19)                                                       # (every atom a candidate, every one of degree 18)
    all_wedges = (k19[0], [(e1, e2, 6, s) for e1, e2, _, s in k19[1]], [], 0)
    images = [HAND[0], bad_atom, bad_order, twice, ring_limit, all_wedges, HAND[1]]
    w = _run(images, 32, 256)
    texts = _check(w, images)
    assert w.status() == [0, L.TEXT_BAD_ROW, L.TEXT_BAD_ROW, L.TEXT_BAD_ROW, L.TEXT_RING_LIMIT, 0, 0]
    assert w.stats.cpu().tolist() == [[1, 0, 0, 1], [0] * 4, [0] * 4, [0] * 4, [0] * 4, [0, 0, 18, 171], [1, 0, 0, 1]]
    assert texts[0] == "[C@H](N)(C)O" and texts[6] == "[C@@H](N)(C)O" and len(texts[5]) == 797
    with pytest.raises(L.AbcNetHipError, match="image 1 .*BAD_ROW"):
        w.smiles()


def test_golden_cases_through_assembler_and_stereo_writer(golden_dir):
    """every case of assemble_128.npz in one batch: the device text is the host form's of molecules(), stats and codes too"""
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
    w = SmilesWriter.from_assembler(asm, stereo=True)
    assert w.cap_text == B * w.image_bytes and w.image_bytes == 14 * cap_atoms + 7 * asm.cap_mol_bonds
    asm.run()
    w.run()
    torch.cuda.synchronize()
    got, mols = w.smiles(), asm.molecules()
    assert w.status() == [0] * B
    codes, stats = w.parities(), w.stats.cpu().tolist()
    wedges = 0
    for b, (name, _) in enumerate(cases):
        c = mols[b].stereo_centres()
        assert got[b] == mols[b].smiles(stereo=True), name
        assert codes[b, :len(c)].tolist() == c and not codes[b, len(c):].any().item(), name
        assert stats[b] == [sum(v in (1, -1) for v in c), c.count(2), c.count(3), sum(o >= 5 for o in mols[b].orders)], name
        wedges += stats[b][3]
    print("golden cases: %d wedge rows, stats summed %s" % (wedges, w.stereo_stats()))


def test_guards():
    """a null stereo_stats: ABC_EINVAL and nothing launched; cap_atoms 513: ABC_EUNSUPPORTED"""
    lib = L.load()
    images = [HAND[0]]
    w = SmilesWriter(*_rows(images, 32, 48), stereo=True)
    w.text.fill_(0xA5)
    w.index.fill_(-7)
    w.stats.fill_(-7)
    w.codes.fill_(-7)
    w.work.fill_(-7)
    torch.cuda.synchronize()
    kept = w.d.stereo_stats
    w.d.stereo_stats = None
    assert lib.abc_write_smiles_stereo(C.byref(w.d), None) == EINVAL and b"null stereo_stats" in lib.abc_last_error()
    torch.cuda.synchronize()
    assert (w.text == 0xA5).all().item() and all((t == -7).all().item() for t in (w.index, w.stats, w.codes, w.work))
    w.d.stereo_stats = kept
    w.d.cap_atoms = 513
    assert lib.abc_write_smiles_stereo(C.byref(w.d), None) == EUNSUPPORTED and b"cap_atoms must be <= 512" in lib.abc_last_error()
    torch.cuda.synchronize()
    assert (w.text == 0xA5).all().item() and all((t == -7).all().item() for t in (w.index, w.stats, w.codes, w.work))
    w.d.cap_atoms = 32
    kept = w.d.stereo_out                 # optional: the text and the stats without it
    w.d.stereo_out = None
    w.run()
    torch.cuda.synchronize()
    assert w.smiles() == ["[C@H](N)(C)O"] and w.stats.cpu().tolist() == [[1, 0, 0, 1]] and (w.codes == -7).all().item()
    w.d.stereo_out = kept
    with pytest.raises(ValueError, match="cap_atoms"):
        SmilesWriter(*_rows(images, 513, 48), stereo=True)


def test_inference_runner_with_stereo():
    """eager, captured and replayed steps (another batch before the replay): the device text is molecules()[i].smiles(stereo=True),
    the stage stands where it stood, and a plain smiles=True runner beside it still gives its own text"""
    from abcnet_amd.infer import InferenceRunner
    m = filled_unet(dropout_p=0.0)
    with pytest.raises(ValueError, match="smiles_stereo=True.*smiles=True"):
        InferenceRunner(m, 2, 128, 128, assemble=True, smiles_stereo=True)
    run = InferenceRunner(m, 2, 128, 128, use_graph=True, assemble=True, smiles=True, smiles_stereo=True)
    plain = InferenceRunner(m, 2, 128, 128, use_graph=True, assemble=True, smiles=True)
    both = InferenceRunner(m, 2, 128, 128, use_graph=True, assemble=True, molblocks=True, smiles=True, smiles_stereo=True)
    assert run._stages == plain._stages and run.smiler.stereo and not plain.smiler.stereo
    assert both._stages.index("smiler") == both._stages.index("texter") + 1 == both._stages.index("assembler") + 2
    seen = wedges = 0
    for seed in (7, 8, 9):
        for r in (run, plain, both):
            r.load_batch(synthetic_images(2, 128, seed=seed).to(DEV))
            r.step()
        torch.cuda.synchronize()
        mols = run.molecules()
        want = [mol.smiles(stereo=True) if mol is not None else None for mol in mols]
        assert run.smiles() == want and both.smiles() == want, seed
        assert plain.smiles() == [mol.smiles() if mol is not None else None for mol in mols], seed
        centres = [mol.stereo_centres() if mol is not None else [] for mol in mols]
        rows_ = [[sum(v in (1, -1) for v in c), c.count(2), c.count(3), 0 if mol is None else sum(o >= 5 for o in mol.orders)]
                 for c, mol in zip(centres, mols)]
        assert run.stereo_stats()["rows"] == rows_ == both.stereo_stats()["rows"], seed
        seen += sum(t is not None for t in want)
        wedges += sum(r[3] for r in rows_)
    print("images with a molecule over the three steps: %d of 6, wedge rows %d" % (seen, wedges))
    assert run._graph is not None and both._graph is not None and plain._graph is not None
    with pytest.raises(L.AbcNetHipError, match="stereo=True"):
        plain.stereo_stats()
