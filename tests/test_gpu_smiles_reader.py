"""The SMILES reader on the device (csrc/smiles_read.hip, ops.SmilesReader, InferenceRunner.load_smiles) against its host form
(decode.parse_smiles): status, counts and rows are compared with torch.equal; then the records read serve the stages that read
records -- identity, similarity, aromaticity perception, canonical keys -- exactly as records loaded from the host do."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import abcnet_amd  # noqa: E402,F401
from abcnet_amd import _lib as L  # noqa: E402
from abcnet_amd.contract import GraphRecords  # noqa: E402
from abcnet_amd.decode import Molecule, parse_smiles  # noqa: E402
from abcnet_amd.ops import AromaticityPerceiver, GraphCanonicalizer, GraphIdentity, GraphSimilarity, SmilesReader, SmilesWriter  # noqa: E402
from abcnet_amd.synthetic import drawn_molecules  # noqa: E402
import smiles_oracle as O  # noqa: E402
import smiles_reader_cases as K  # noqa: E402
from molrows import trained_unet  # noqa: E402
from smiles_cases import EXAMPLES, SYMBOLS, random_rows, records_of_text, rows_of, ring  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
JUNK = 77


def _reader(B, max_atoms=64, max_bonds=64, cap_text=None):
    rec = GraphRecords(B, max_atoms, max_bonds, DEV)
    for t in rec.staging.dev.values():
        t.fill_(JUNK)                     # (rows past the counts are unspecified; the counts themselves are written by every load)
    return rec, SmilesReader(rec, cap_text=cap_text)


def _check(rec, reader, strings):
    """status, counts and the rows up to the counts of the last load against the host form, with torch.equal; returns the statuses"""
    torch.cuda.synchronize()
    B = rec.B
    want = [parse_smiles(s, rec.max_atoms, rec.max_bonds) for s in strings] + [parse_smiles("")] * (B - len(strings))
    atoms, bonds, cnt = (t.cpu() for t in rec.staging.dev.values())
    assert torch.equal(reader.status_words.cpu(), torch.tensor([w[0] for w in want], dtype=torch.int32))
    assert torch.equal(cnt, torch.tensor([[len(w[1]) for w in want], [len(w[2]) for w in want]], dtype=torch.int32))
    for b, (status, a, q) in enumerate(want):
        assert torch.equal(atoms[b, :len(a)], torch.from_numpy(a)), (b, strings[b][:60])
        assert torch.equal(bonds[b, :len(q)], torch.from_numpy(q)), (b, strings[b][:60])
    stats = reader.stat.cpu()
    raw = [len(s.encode("ascii", "replace")) for s in strings] + [0] * (B - len(strings))
    assert stats[:, 0].tolist() == raw and torch.equal(stats[:, 1:3].T.contiguous(), cnt)
    assert rec.loaded and reader.status() == [w[0] for w in want]
    return [w[0] for w in want]


def test_the_table_as_one_batch():
    strings = [row[0] for row in K.TABLE] + [s for s, _ in K.REFUSED]
    rec, reader = _reader(len(strings))
    reader.load(strings)
    status = _check(rec, reader, strings)
    assert status == [K.OK] * len(K.TABLE) + [want for _, want in K.REFUSED]
    # (a string's chains hold atoms - chains bonds: the others are ring bonds)
    assert reader.stats()["ring_bonds"] == sum(row[2] - row[1] + row[0].count(".") + 1 for row in K.TABLE)


def test_a_batch_of_one_and_a_short_batch_in_a_longer_op():
    rec, reader = _reader(1)
    reader.load(["CC(=O)Oc1ccccc1C(=O)O"])
    assert _check(rec, reader, ["CC(=O)Oc1ccccc1C(=O)O"]) == [K.OK]
    rec, reader = _reader(8)
    three = ["c1ccccc1", "C12CCC12", "[Na+].[O-]c1ccccc1"]
    reader.load(three)
    assert _check(rec, reader, three) == [K.OK, K.DUPLICATE, K.OK] + [K.EMPTY] * 5
    with pytest.raises(ValueError):
        reader.load(["C"] * 9)
    with pytest.raises(ValueError):
        reader.load([b"C"])
    with pytest.raises(ValueError, match="cap_text"):
        SmilesReader(rec, cap_text=4).load(["CCCCC"])


def test_a_short_batch_after_a_long_one_shows_nothing_stale():
    rec, reader = _reader(6, 512, 512)
    long_batch = ["C" * 500, "C1CC1" * 100, "c1ccccc1" * 60, "C(C)" * 120 + "C", "OCC" * 100, "N#CC" * 30]
    reader.load(long_batch)
    assert _check(rec, reader, long_batch) == [K.OK] * 6
    short = ["C", "C(", "CC"]
    reader.load(short)
    assert _check(rec, reader, short) == [K.OK, K.SYNTAX, K.OK, K.EMPTY, K.EMPTY, K.EMPTY]


def _straddle(token, length, at):
    """`token` at byte `at` of a chain of `length` bytes (ring 12 is opened by the first atom where the token closes it)"""
    s = ("C%12" + "C" * (at - 4) if token == "%12" else "C" * at) + token
    return s + "C" * (length - len(s))


def test_tokens_across_the_boundaries_of_the_threads_runs():
    """256 bytes: one byte per thread; 257: two; ABC_MAX_SMILES_READ_BYTES: sixteen -- `Cl`, a bracket atom and `%nn` lie across byte 256
    (the second round of the load loop) and so across two threads' runs"""
    strings = []
    for length in (256, 257, K.MAX_BYTES):
        for token in ("Cl", "[NH2+]", "%12"):
            at = min(255, length - len(token))
            strings.append(_straddle(token, length, at))
            assert len(strings[-1]) == length and strings[-1][at:at + len(token)] == token
    rec, reader = _reader(len(strings), K.MAX_BYTES, K.MAX_BYTES)
    reader.load(strings)
    assert _check(rec, reader, strings) == [K.OK] * len(strings)


def test_counts_at_the_capacities_and_one_over():
    rec, reader = _reader(6, 64, 8)
    strings = ["C1CCCCCCC1", "C1CCCCCCCC1", ".".join("C" * 64), ".".join("C" * 65), "C" * 9, "C" * 10]       # 8 / 9 bonds; 64 / 65 atoms; 8 / 9 bonds
    reader.load(strings)
    assert _check(rec, reader, strings) == [K.OK, K.TRUNCATED, K.OK, K.TRUNCATED, K.OK, K.TRUNCATED]


def test_deep_nesting_a_hundred_open_rings_and_a_chain_of_512():
    number = lambda k: str(k) if k < 10 else "%%%02d" % k
    deep = "C(" * 300 + "C" + ")" * 300
    rings = "".join("C" + number(k) for k in range(100)) + "".join("N" + number(k) for k in range(100))
    fan = "C" + "".join(number(k) for k in range(100)) + "".join("(CO%s)" % number(k) for k in range(99)) + "CO%99"      # 100 numbers on one atom
    strings = [deep, rings, fan, "C" * 512, "C" * 513]
    rec, reader = _reader(len(strings), 512, 512)
    reader.load(strings)
    assert _check(rec, reader, strings) == [K.OK, K.OK, K.OK, K.OK, K.TRUNCATED]
    assert reader.stats()["rows"][1] == [len(rings), 200, 299, 100]


def test_mutated_strings_equal_the_host_form():
    strings = K.mutated(2000)[:256]
    rec, reader = _reader(256, 32, 32, cap_text=16384)
    reader.load(strings)
    status = _check(rec, reader, strings)
    print({L.READ_STATUS_NAMES[v]: status.count(v) for v in sorted(set(status))})
    assert status.count(K.SYNTAX) > 64 and status.count(K.OK) > 16


# ------------------------------------------------------------------------------------------------- the readers of the records
def _rows(images, cap_atoms, cap_bonds):
    """hand-made rows [(atoms [n,5], bonds [m,4], implh [k])] as device tensors of the assembler's layout"""
    B = len(images)
    cnt = torch.zeros(B, 4, dtype=torch.int32)
    atoms = torch.full((B, cap_atoms, 5), JUNK, dtype=torch.int32)
    bonds = torch.full((B, cap_bonds, 4), JUNK, dtype=torch.int32)
    implh = torch.full((B, cap_atoms), JUNK, dtype=torch.int32)
    for b, (a, q, h) in enumerate(images):
        a, q, h = np.asarray(a, dtype=np.int64).reshape(-1, 5), np.asarray(q, dtype=np.int64).reshape(-1, 4), np.asarray(h, dtype=np.int64).reshape(-1)
        atoms[b, :len(a)] = torch.as_tensor(a, dtype=torch.int32)
        bonds[b, :len(q)] = torch.as_tensor(q, dtype=torch.int32)
        implh[b, :len(h)] = torch.as_tensor(h, dtype=torch.int32)
        cnt[b] = torch.tensor([len(a), len(q), len(h), 0], dtype=torch.int32)
    return cnt.to(DEV), atoms.to(DEV), bonds.to(DEV), implh.to(DEV)


def _bonded_images(seed, count):
    """(the identity stage reads a record's atoms off its bonds: no atom without a bond)"""
    rng = np.random.default_rng(seed)
    bonded = lambda im: {e for q in im[1] for e in q[:2]} == set(range(1, len(im[0]) + 1))
    return [im for im in [rows for _, rows, _ in EXAMPLES] + [random_rows(rng) for _ in range(count)] if bonded(im)]


def test_round_trip_on_the_device():
    """SmilesWriter's text of hand-made rows, read back by SmilesReader: the verified isomorphism says `same` of every image, and the
    canonical keys of the records read are those of the records the test's own reader makes of the text"""
    images = _bonded_images(61, 60)
    assert len(images) >= 24
    B = len(images)
    cnt, atoms, bonds, implh = _rows(images, 64, 96)
    w = SmilesWriter(cnt, atoms, bonds, implh)
    w.run()
    texts = w.smiles()
    assert texts == [Molecule.from_device_rows(np.asarray(a).reshape(-1, 5), np.asarray(q).reshape(-1, 4), h).smiles() for a, q, h in images]
    rec, reader = _reader(B, 64, 96)
    gi = GraphIdentity(cnt, atoms, bonds, records=rec)
    canon = GraphCanonicalizer.from_records(rec)
    reader.load(texts)
    gi.run()
    canon.run()
    assert _check(rec, reader, texts) == [K.OK] * B
    res = gi.result()
    assert res["counted"] == B and res["same"] == B and res["undecided"] == 0 and res["different"] == 0
    keys, stats = canon.keys(), canon.stats()
    class_of = {s: SYMBOLS.index(s, 1) for s in SYMBOLS}
    rec2 = GraphRecords(B, 64, 96, DEV)
    canon2 = GraphCanonicalizer.from_records(rec2)
    rec2.load([records_of_text(O.parse(t), class_of) for t in texts])
    canon2.run()
    torch.cuda.synchronize()
    decided = torch.from_numpy((stats["status"] == 0) & (canon2.stats()["status"] == 0))
    assert int(decided.sum()) >= B - 2 and torch.equal(keys[decided], canon2.keys()[decided])


def _totals(op):
    res = op.result()
    return {k: (v.tolist() if k == "rows" else v) for k, v in res.items() if not k.startswith("share") and k != "similarity"}


def test_scores_are_equal_whether_the_records_come_from_the_host_or_from_their_strings():
    images = _bonded_images(62, 40)
    B = len(images)
    rows = _rows(images, 64, 96)
    # the truth: the molecules of the next image round, as strings -- some equal (the examples against themselves), most different
    truth = [Molecule.from_device_rows(np.asarray(a).reshape(-1, 5), np.asarray(q).reshape(-1, 4), h).smiles()
             for a, q, h in images[:11] + images[12:] + images[11:12]]
    truth[3] = "C(("                       # a row the rule refuses: an empty record on both paths
    host, (dev, reader) = GraphRecords(B, 64, 96, DEV), _reader(B, 64, 96)
    host.load([parse_smiles(t, 64, 96)[1:] for t in truth])
    reader.load(truth)
    for perceive in (False, True):
        results = []
        for rec in (host, dev):
            ops = []
            if perceive:
                ap = AromaticityPerceiver.from_records(rec)
                ap.run()
                rec = ap.records()
            ops = [GraphSimilarity(*rows[:3], records=rec), GraphIdentity(*rows[:3], records=rec)]
            for op in ops:
                op.run()
            results.append([_totals(op) for op in ops])
        assert results[0] == results[1], perceive
        assert results[0][1]["counted"] == B and results[0][1]["same"] >= 9 and results[0][1]["different"] >= 1


def test_a_kekule_string_and_its_lower_case_form():
    """the molecule: benzene and pyridine drawn with order 4; the truth as a Kekule string and in lower case: `different` and `same`
    as read, `same` twice after the aromaticity perception of the records"""
    benzene = rows_of(["C"] * 6, ring(1, 6, 4))
    pyridine = rows_of(["N"] + ["C"] * 5, ring(1, 6, 4))
    rows = _rows([benzene, benzene, pyridine, pyridine], 16, 16)
    rec, reader = _reader(4, 16, 16)
    strings = ["C1=CC=CC=C1", "c1ccccc1", "N1=CC=CC=C1", "n1ccccc1"]
    reader.load(strings)
    assert _check(rec, reader, strings) == [K.OK] * 4
    plain = GraphIdentity(*rows[:3], records=rec)
    ap = AromaticityPerceiver.from_records(rec)
    perceived = GraphIdentity(*rows[:3], records=ap.records())
    plain.run()
    ap.run()
    perceived.run()
    col = L.GRAPH_IDENT_COLUMNS.index("same")
    assert plain.result()["rows"][:, col].tolist() == [0, 1, 0, 1] and plain.result()["different"] == 2
    assert perceived.result()["rows"][:, col].tolist() == [1, 1, 1, 1]


# ------------------------------------------------------------------------------------------------------------------ the runner
def _scores(run):
    ev = run.evaluation()
    return {key: {k: (v.tolist() if k == "rows" else v) for k, v in ev[key].items() if k == "rows" or v == v} for key in ("identity", "similarity")}


def test_runner_load_smiles_equals_load_graphs(golden_dir):
    """batch 4 at 96 x 96 (the size of test_runner_identifies_its_own_molecules), the trained fixture: the same strings through
    load_smiles (the device reader) and through decode.parse_smiles + load_graphs give equal identity and similarity tables, eager
    and replayed from the captured graph, with other strings in between; a runner that never calls load_smiles is as it was"""
    from abcnet_amd.infer import STAGES, InferenceRunner
    B, S = 4, 96
    m = trained_unet(golden_dir)
    kw = dict(use_graph=True, assemble=True, evaluate=True, score_similarity=True, score_identity=True)
    by_graphs, by_smiles = InferenceRunner(m, B, S, S, **kw), InferenceRunner(m, B, S, S, **kw)
    assert by_graphs.smiles_reader is None and by_smiles.smiles_reader is None and "smiles_reader" not in STAGES
    stages = list(by_smiles._stages)
    assert by_graphs._stages == stages and set(stages) <= set(STAGES)
    with pytest.raises(L.AbcNetHipError, match="load_smiles"):
        by_smiles.record_status()
    x, _ = drawn_molecules(B, S, seed=40)
    empty = (np.zeros((0, 4), np.int32), np.zeros((0, 3), np.int32))
    for r in (by_graphs, by_smiles):
        r.load_batch(x.to(DEV), n_valid=B)
    by_graphs.load_graphs([empty] * B)
    by_graphs.step()
    torch.cuda.synchronize()
    own = [mol.smiles() if mol is not None else "" for mol in by_graphs.molecules()]
    assert any(own), "every molecule is None: these weights say nothing"
    batches = [own, own, own[1:] + own[:1], ["c1ccccc1", "C((", "CC(=O)O", own[0]]]      # eager; capture + replay; two more replays
    for step, strings in enumerate(batches):
        for r in (by_graphs, by_smiles):
            r.reset_evaluation()
        by_graphs.load_graphs([parse_smiles(s, 256, 256)[1:] for s in strings])
        by_smiles.load_smiles(strings)
        by_graphs.step()
        by_smiles.step()
        torch.cuda.synchronize()
        a, b = _scores(by_graphs), _scores(by_smiles)
        assert a == b, step
        assert by_smiles.record_status() == [parse_smiles(s)[0] for s in strings], step
        same = a["identity"]["rows"]
        print(step, [r[L.GRAPH_IDENT_COLUMNS.index("same")] for r in same], a["similarity"]["dice_q20"])
        if step < 2:
            first = a
            assert a["identity"]["same"] >= 1                                   # a molecule against its own text
    assert by_smiles._graph is not None and by_smiles.steps == 4 and by_graphs.smiles_reader is None and by_smiles._stages == stages
    assert a != first                                                            # the replays followed the strings
    # overwriting the same records from the host afterwards is just another load
    by_smiles.reset_evaluation()
    by_smiles.load_graphs([parse_smiles(s, 256, 256)[1:] for s in own])
    by_smiles.step()
    assert _scores(by_smiles) == first


def test_runner_refusals(golden_dir):
    from abcnet_amd.infer import InferenceRunner
    m = trained_unet(golden_dir)
    graded = InferenceRunner(m, 2, 96, 96, assemble=True, evaluate=True, score_graphs=True, score_similarity=True)
    with pytest.raises(ValueError, match="score_graphs"):
        graded.load_smiles(["CC", "CO"])
    assert graded.smiles_reader is None
    plain = InferenceRunner(m, 2, 96, 96, assemble=True, evaluate=True)
    with pytest.raises(L.AbcNetHipError, match="score_similarity"):
        plain.load_smiles(["CC", "CO"])


def test_the_launcher_refuses_and_launches_nothing():
    rec, reader = _reader(2)
    reader.load(["CC", "CO"])
    torch.cuda.synchronize()
    reader.status_words.fill_(JUNK)
    lib = L.load()
    for field, value in (("text", None), ("status", None), ("rec_counts", None), ("B", 0), ("max_atoms", 0), ("max_bonds", 0), ("cap_text", 0)):
        d = L.SmilesReadDesc()
        C.memmove(C.byref(d), C.byref(reader.d), C.sizeof(d))
        setattr(d, field, value)
        assert lib.abc_read_smiles(C.byref(d), torch.cuda.current_stream().cuda_stream) == -1, field
        assert b"read_smiles" in lib.abc_last_error()
    torch.cuda.synchronize()
    assert reader.status_words.cpu().tolist() == [JUNK, JUNK]
