"""GPU parity of the double-bond form of the device SMILES writer (abc_write_smiles_ez, ops.SmilesWriter(double_bonds=True)) against
the host form decode.Molecule.smiles(double_bonds=True) and the second transcription of the rule (smiles_ez_oracle), which
tests/test_smiles_ez_host.py holds to each other and to the drawing.  Bytes and integers: exact, no tolerance anywhere."""
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
import smiles_ez_oracle as Z  # noqa: E402
import smiles_stereo_oracle as S  # noqa: E402
import test_smiles_ez_host as H  # noqa: E402
from molrows import assemble_golden, filled_unet  # noqa: E402
from smiles_cases import complete  # noqa: E402
from smiles_cases import random_rows as plain_random_rows  # noqa: E402
from smiles_ez_cases import BOTH, CASES, FLAT_CASES, butenes, random_images, zigzag_polyene  # noqa: E402
from smiles_stereo_cases import CASES as WEDGE_CASES  # noqa: E402

DEV = "cuda"
EINVAL, EUNSUPPORTED = -1, -2
NOTHING = ([], [], [])
ZEROS = (0, 0, 0, 0)


def _rows(images, cap_atoms, cap_bonds):
    """hand-made rows [(atoms [n,5], bonds [m,4], implh [k], status)] as device tensors of the assembler's layout; the rows past
    the counts hold a pattern the writer must not read (an index the vocabulary does not have, a double bond no atom has)"""
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


def _molecule(image):
    return Molecule.from_device_rows(np.asarray(image[0]).reshape(-1, 5), np.asarray(image[1]).reshape(-1, 4), image[2])


def _expected(image, tetrahedral):
    """(text or None / "bad_row" / "ring_limit", codes per bond row, ez stats, centre codes, stereo stats) of one image by the host
    form, which must agree with the oracle"""
    a, q, h, status = image
    nothing = [], ZEROS, [], ZEROS
    if status & L.MOL_EMPTY:
        return (None,) + nothing
    if any(not 0 <= row[2] <= 13 for row in a):      # (from_device_rows cannot name such an atom's symbol)
        return ("bad_row",) + nothing
    try:
        m = _molecule(image)
        text, codes = m.smiles(double_bonds=True, stereo=tetrahedral), m.double_bond_codes()
    except ValueError as e:
        return ("ring_limit" if "ring limit" in str(e) else "bad_row",) + nothing
    want, want_codes, stats, _ = Z.write(a, q, h, tetrahedral=tetrahedral)
    assert text == want and codes == want_codes
    centres, centre_stats = [], ZEROS
    if tetrahedral:
        _, _, centres, centre_stats = S.write(a, q, h)
        assert centres == m.stereo_centres()
    return text, codes, stats, centres, centre_stats


def _check(w, images):
    """index, status words, bytes, ez_stats, ez_out (and stereo_stats, stereo_out) of the last run against the host form and the
    oracle; returns the texts (None where none is written)"""
    want = [_expected(im, w.stereo) for im in images]
    bits = {"bad_row": L.TEXT_BAD_ROW, "ring_limit": L.TEXT_RING_LIMIT}
    texts = [None if e[0] in bits else e[0] for e in want]
    idx = w.index.cpu().tolist()
    off, status = idx[:w.B + 1], idx[w.B + 1:]
    assert off[0] == 0 and [b - a for a, b in zip(off, off[1:])] == [0 if t is None else len(t) for t in texts]
    assert status == [(im[3] & (L.MOL_EMPTY | L.MOL_TRUNCATED)) | bits.get(e[0], 0) for im, e in zip(images, want)]
    raw = w.text[:off[-1]].cpu().numpy().tobytes()
    for b, t in enumerate(texts):
        if t is not None:
            assert raw[off[b]:off[b + 1]].decode("ascii") == t, b
    stats = torch.tensor([list(e[2]) for e in want], dtype=torch.int32)
    codes = torch.zeros(w.B, w.cap_mol_bonds, dtype=torch.int32)
    for b, e in enumerate(want):
        codes[b, :len(e[1])] = torch.tensor(e[1], dtype=torch.int32)
    assert torch.equal(w.ez_stats.cpu(), stats)
    assert torch.equal(w.double_bond_codes(), codes)
    res = w.double_bond_stats()
    assert res["rows"] == stats.tolist() and [res[k] for k in L.SMILES_EZ_COLUMNS] == stats.sum(0).tolist()
    if w.stereo:
        centres = torch.zeros(w.B, w.cap_atoms, dtype=torch.int32)
        for b, e in enumerate(want):
            centres[b, :len(e[3])] = torch.tensor(e[3], dtype=torch.int32)
        assert torch.equal(w.stats.cpu(), torch.tensor([list(e[4]) for e in want], dtype=torch.int32))
        assert torch.equal(w.parities(), centres)
    return texts


def _run(images, cap_atoms, cap_bonds, cap_text=None, stereo=False, double_bonds=True):
    w = SmilesWriter(*_rows(images, cap_atoms, cap_bonds), cap_text=cap_text, stereo=stereo, double_bonds=double_bonds)
    w.run()
    torch.cuda.synchronize()
    return w


HAND = ([im + (0,) for _, im, _, _ in CASES] + [im + (0,) for im, _, _, _ in BOTH] + [im + (0,) for _, im, _ in FLAT_CASES]
        + [im + (0,) for _, im, _ in WEDGE_CASES[:6]])
RANDOM = [im + (0,) for im in random_images(H.SEED, 132)]      # (the first images of the host suite's seed)


@pytest.fixture(scope="module", params=[False, True], ids=["double_bonds", "both"])
def device_texts(request):
    """every hand-made case and the seeded images through the device once, 32 per batch, capacities 32 / 64: checked against host
    form and oracle here, read back by the next test"""
    images = HAND + RANDOM
    assert len(images) == 5 * 32
    texts = []
    for at in range(0, len(images), 32):
        batch = images[at:at + 32]
        w = _run(batch, 32, 64, stereo=request.param)
        assert w.image_bytes == (14 if request.param else 12) * 32 + 7 * 64
        got = _check(w, batch)
        assert w.smiles() == got
        texts += got
    return request.param, images, texts


def test_device_text_stats_and_codes_equal_host_form_and_oracle(device_texts):
    tetrahedral, images, texts = device_texts
    if tetrahedral:
        assert texts[len(CASES):len(CASES) + 2] == [both for _, both, _, _ in BOTH]
    else:
        assert texts[:len(CASES)] == [t for _, _, t, _ in CASES]
        assert texts[len(CASES):len(CASES) + 2] == [double for _, _, _, double in BOTH]
    marked = sum(sum(c in (1, -1) for c in _molecule(im).double_bond_codes()) for im in RANDOM)
    print("seeded images: %d marked double bonds, %d texts with a symbol" % (marked, sum("/" in t for t in texts[len(HAND):])))
    assert marked >= 30


def test_device_text_read_back_agrees_with_the_drawing(device_texts):
    _, images, texts = device_texts
    seen = 0
    for (a, q, h, _), text in zip(images, texts):
        codes = _molecule((a, q, h)).double_bond_codes()
        conf = H.configurations((a, q, h), text, codes)      # (asserts every pair against the sign test on the drawing)
        assert len({frozenset(e for e, _ in key) for key in conf}) == sum(c in (1, -1) for c in codes)
        H.groups_start_with_a_slash((a, q, h), text, codes)
        seen += len(conf)
    assert seen >= 40


@pytest.mark.parametrize("tetrahedral", [False, True])
def test_wide_shapes(tetrahedral):
    """cap_atoms 512, one image each: a zigzag polyene of 512 carbons -- 255 conjugated double bonds in ONE group, the most a chain of
    512 atoms holds (a double bond at the chain's end has an end without a substituent) and the deepest propagation, with atoms 509 to
    512 in its last marked rows; 128 separate 2-butenes, 128 groups each normalised on its own"""
    for image, text in ((zigzag_polyene(512), "C" + "/C=C" * 255 + "/C"), (butenes(128), ".".join(["C/C=C\\C", "C/C=C/C"] * 64))):
        w = _run([image + (0,)], 512, 512, stereo=tetrahedral)
        assert _check(w, [image + (0,)]) == [text]
    codes = w.double_bond_codes()[0]
    assert codes[:384].tolist() == [0, 1, 0, 0, -1, 0] * 64 and w.ez_stats.cpu().tolist() == [[128, 0, 0, 0]]


def _plain_images(seed, count, wedges):
    """the plain suite's recipe with every double bond made a single bond (and every wedge, unless they are wanted)"""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(count):
        a, q, h = plain_random_rows(rng)
        out.append((a, [(e1, e2, 1 if o == 2 or (o >= 5 and not wedges) else o, s) for e1, e2, o, s in q], h, 0))
    return out


@pytest.mark.parametrize("tetrahedral", [False, True])
def test_a_batch_without_double_bonds_has_the_bytes_of_the_other_entry_points(tetrahedral):
    images = _plain_images(51, 24, tetrahedral) + ([HAND[-1], HAND[-2]] if tetrahedral else [])
    tensors = _rows(images, 64, 96)
    base, ez = SmilesWriter(*tensors, stereo=tetrahedral), SmilesWriter(*tensors, stereo=tetrahedral, double_bonds=True)
    base.run()
    ez.run()
    torch.cuda.synchronize()
    assert base.image_bytes == ez.image_bytes == (14 if tetrahedral else 12) * 64 + 7 * 96
    assert torch.equal(base.index, ez.index)
    n = int(base.index[len(images)].item())
    assert n > 0 and torch.equal(base.text[:n], ez.text[:n])
    assert base.smiles() == ez.smiles() == [_molecule(im).smiles(stereo=tetrahedral) for im in images]
    assert not ez.ez_stats.any().item() and not ez.double_bond_codes().any().item()
    assert ez.double_bond_stats() == dict(marked=0, flat=0, ring=0, twin=0, rows=[[0] * 4] * len(images))
    if tetrahedral:
        assert torch.equal(base.stats, ez.stats) and torch.equal(base.codes, ez.codes) and ez.stats.any().item()
    with pytest.raises(L.AbcNetHipError, match="double_bonds=True"):
        base.double_bond_stats()
    with pytest.raises(L.AbcNetHipError, match="double_bonds=True"):
        base.double_bond_codes()


def test_a_short_batch_after_a_long_one_shows_nothing_stale():
    long_images = RANDOM[:5] + [HAND[6]]
    tensors = _rows(long_images, 64, 96)
    w = SmilesWriter(*tensors, double_bonds=True)
    w.run()
    torch.cuda.synchronize()
    assert w.smiles() == _check(w, long_images) and w.ez_stats.any().item() and w.double_bond_codes().any().item()
    short = [NOTHING + (0,), HAND[12], (HAND[0][0], HAND[0][1], HAND[0][2], L.MOL_EMPTY), NOTHING + (0,), _plain_images(52, 1, False)[0], HAND[0]]
    for dst, src in zip(tensors, _rows(short, 64, 96)):
        dst.copy_(src)
    w.run()
    torch.cuda.synchronize()
    got = _check(w, short)
    assert got[:4] == ["", "CC=CC", None, ""] and got[5] == "C/C=C/C"
    assert w.ez_stats.cpu().tolist() == [[0] * 4, [0, 1, 0, 0], [0] * 4, [0] * 4, [0] * 4, [1, 0, 0, 0]]
    codes = w.double_bond_codes()
    assert codes[1, :3].tolist() == [0, 2, 0] and codes[5, :3].tolist() == [0, -1, 0] and codes.abs().sum().item() == 3


def test_capacity_is_a_prefix_rule_inside_a_marked_image():
    images = [HAND[1], HAND[6], HAND[0], NOTHING + (L.MOL_EMPTY,)]
    want = [_expected(im, False)[0] for im in images]
    assert want[:3] == ["C/C=C\\C", "F/C(/Cl)=C(\\Br)/I", "C/C=C/C"]
    w = SmilesWriter(*_rows(images, 32, 64), double_bonds=True)
    # the same buffers behind a smaller cap_text, which ends behind the "/" in front of "Cl" in the second image: that image and all
    # behind it are left out whole, nothing at or beyond the end of the first is touched, the stats stay what they are
    w.text.fill_(0xA5)
    w.d.cap_text = len(want[0]) + 5
    w.run()
    torch.cuda.synchronize()
    idx = w.index.cpu().tolist()
    assert idx[:5] == [0] + [len(want[0])] * 4
    assert idx[5:] == [0, L.TEXT_OVERFLOW, L.TEXT_OVERFLOW, L.MOL_EMPTY | L.TEXT_OVERFLOW]
    raw = w.text.cpu().numpy()
    assert raw[:len(want[0])].tobytes().decode("ascii") == want[0] and (raw[len(want[0]):] == 0xA5).all()
    assert w.ez_stats.cpu().tolist() == [[1, 0, 0, 0]] * 3 + [[0] * 4]
    with pytest.raises(L.AbcNetHipError, match="image 1 .*OVERFLOW"):
        w.smiles()
    # inside the first image, behind its first symbol: nothing at all
    w.d.cap_text = 2
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


@pytest.mark.parametrize("tetrahedral", [False, True])
def test_refused_and_empty_images_have_zero_stats(tetrahedral):
    """BAD_ROW before and after the candidates are looked at, RING_LIMIT after the walk, EMPTY: double bonds in each, zeros for all"""
    a, q, h = (list(v) for v in CASES[0][1])
    bad_atom = (a[:3] + [(30, 40, 14, 0, 0)], q, h, 0)                       # a vocabulary index of 14
    bad_order = (a, q[:2] + [(3, 4, 7, 2)], h, 0)                            # an order of 7
    twice = (a, q + [(3, 2, 2, 3)], h, 0)                                    # the pair of the double bond a second time (found in step 2)
    k20 = complete(20)
    ring_limit = (k20[0], [(e1, e2, 2 if s == 0 else 1, s) for e1, e2, _, s in k20[1]], [], 0)
    empty = (a, q, h, L.MOL_EMPTY)
    images = [HAND[0], bad_atom, bad_order, twice, ring_limit, empty, HAND[1]]
    w = _run(images, 32, 256, stereo=tetrahedral)
    texts = _check(w, images)
    assert w.status() == [0, L.TEXT_BAD_ROW, L.TEXT_BAD_ROW, L.TEXT_BAD_ROW, L.TEXT_RING_LIMIT, L.MOL_EMPTY, 0]
    assert w.ez_stats.cpu().tolist() == [[1, 0, 0, 0]] + [[0] * 4] * 5 + [[1, 0, 0, 0]]
    assert texts[0] == "C/C=C/C" and texts[6] == "C/C=C\\C"
    with pytest.raises(L.AbcNetHipError, match="image 1 .*BAD_ROW"):
        w.smiles()


def test_golden_cases_through_assembler_and_writer(golden_dir):
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
    w = SmilesWriter.from_assembler(asm, stereo=True, double_bonds=True)
    assert w.cap_text == B * w.image_bytes and w.image_bytes == 14 * cap_atoms + 7 * asm.cap_mol_bonds
    asm.run()
    w.run()
    torch.cuda.synchronize()
    got, mols = w.smiles(), asm.molecules()
    assert w.status() == [0] * B
    codes, stats = w.double_bond_codes(), w.ez_stats.cpu().tolist()
    doubles = 0
    for b, (name, _) in enumerate(cases):
        c = mols[b].double_bond_codes()
        assert got[b] == mols[b].smiles(stereo=True, double_bonds=True), name
        assert codes[b, :len(c)].tolist() == c and not codes[b, len(c):].any().item(), name
        assert stats[b] == [sum(v in (1, -1) for v in c), c.count(2), c.count(3), c.count(4)], name
        doubles += sum(o == 2 for o in mols[b].orders)
    print("golden cases: %d class-2 rows, stats summed %s" % (doubles, w.double_bond_stats()))


def test_guards():
    """a null ez_stats, a null stereo_stats with tetrahedral: ABC_EINVAL and nothing launched; cap_atoms 513: ABC_EUNSUPPORTED"""
    lib = L.load()
    images = [HAND[0]]
    w = SmilesWriter(*_rows(images, 32, 64), stereo=True, double_bonds=True)
    buffers = (w.index, w.stats, w.codes, w.ez_stats, w.ez_codes, w.work)

    def untouched():
        torch.cuda.synchronize()
        return (w.text == 0xA5).all().item() and all((t == -7).all().item() for t in buffers)
    w.text.fill_(0xA5)
    for t in buffers:
        t.fill_(-7)
    torch.cuda.synchronize()
    kept = w.d.ez_stats
    w.d.ez_stats = None
    assert lib.abc_write_smiles_ez(C.byref(w.d), None) == EINVAL and b"null ez_stats" in lib.abc_last_error() and untouched()
    w.d.ez_stats = kept
    kept = w.d.stereo_stats
    w.d.stereo_stats = None
    assert lib.abc_write_smiles_ez(C.byref(w.d), None) == EINVAL and b"null stereo_stats" in lib.abc_last_error() and untouched()
    w.d.stereo_stats = kept
    w.d.cap_atoms = 513
    assert lib.abc_write_smiles_ez(C.byref(w.d), None) == EUNSUPPORTED and b"cap_atoms must be <= 512" in lib.abc_last_error() and untouched()
    w.d.cap_atoms = 32
    assert lib.abc_write_smiles_ez(None, None) == EINVAL
    # without tetrahedral a null stereo_stats is nothing to refuse, and the optional ez_out may be left out
    w.d.tetrahedral, w.d.stereo_stats, w.d.stereo_out, w.d.ez_out = 0, None, None, None
    assert lib.abc_smiles_ez_text_bytes(C.byref(w.d)) == 12 * 32 + 7 * 64
    w.run()
    torch.cuda.synchronize()
    assert w.smiles() == ["C/C=C/C"] and w.ez_stats.cpu().tolist() == [[1, 0, 0, 0]]
    assert all((t == -7).all().item() for t in (w.stats, w.codes, w.ez_codes))
    with pytest.raises(ValueError, match="cap_atoms"):
        SmilesWriter(*_rows(images, 513, 64), double_bonds=True)


def test_inference_runner_with_double_bonds():
    """eager, captured and replayed steps (another batch before the replay): the device text is
    molecules()[i].smiles(double_bonds=True, ...), the stage stands where it stood, and a plain smiles=True runner beside it still
    gives its own text"""
    from abcnet_amd.infer import InferenceRunner
    m = filled_unet(dropout_p=0.0)
    with pytest.raises(ValueError, match="smiles_double_bonds=True.*smiles=True"):
        InferenceRunner(m, 2, 128, 128, assemble=True, smiles_double_bonds=True)
    with pytest.raises(ValueError, match="smiles_canonical=True, smiles_double_bonds=True"):
        InferenceRunner(m, 2, 128, 128, assemble=True, smiles=True, smiles_canonical=True, smiles_double_bonds=True)
    run = InferenceRunner(m, 2, 128, 128, use_graph=True, assemble=True, smiles=True, smiles_double_bonds=True)
    plain = InferenceRunner(m, 2, 128, 128, use_graph=True, assemble=True, smiles=True)
    both = InferenceRunner(m, 2, 128, 128, use_graph=True, assemble=True, molblocks=True, smiles=True, smiles_stereo=True, smiles_double_bonds=True)
    assert run._stages == plain._stages and run.smiler.double_bonds and not run.smiler.stereo and not plain.smiler.double_bonds
    assert both._stages.index("smiler") == both._stages.index("texter") + 1 == both._stages.index("assembler") + 2
    seen = doubles = 0
    for seed in (7, 8, 9):
        for r in (run, plain, both):
            r.load_batch(synthetic_images(2, 128, seed=seed).to(DEV))
            r.step()
        torch.cuda.synchronize()
        mols = run.molecules()
        assert run.smiles() == [mol.smiles(double_bonds=True) if mol is not None else None for mol in mols], seed
        assert both.smiles() == [mol.smiles(double_bonds=True, stereo=True) if mol is not None else None for mol in mols], seed
        assert plain.smiles() == [mol.smiles() if mol is not None else None for mol in mols], seed
        codes = [mol.double_bond_codes() if mol is not None else [] for mol in mols]
        rows_ = [[sum(v in (1, -1) for v in c), c.count(2), c.count(3), c.count(4)] for c in codes]
        assert run.double_bond_stats()["rows"] == rows_ == both.double_bond_stats()["rows"], seed
        got = run.double_bond_codes()
        for b, c in enumerate(codes):
            assert got[b, :len(c)].tolist() == c and not got[b, len(c):].any().item()
        seen += sum(mol is not None for mol in mols)
        doubles += sum(sum(o == 2 for o in mol.orders) for mol in mols if mol is not None)
    print("images with a molecule over the three steps: %d of 6, class-2 rows %d" % (seen, doubles))
    assert run._graph is not None and both._graph is not None and plain._graph is not None
    with pytest.raises(L.AbcNetHipError, match="double_bonds=True"):
        plain.double_bond_stats()
