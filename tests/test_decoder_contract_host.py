"""CPU tier of the decoder's half of abcnet_amd.contract: the molecule-row and candidate-list checkers under every caller's name,
the device-free half of GraphRecords.load, the capacities of include/abcnet_hip.h against their mirrors in _lib.py at the Python
classes and at the launchers, and the table of self-sized descriptors of _lib.load()."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import abcnet_amd  # noqa: E402,F401
from abcnet_amd import _lib as L  # noqa: E402
from abcnet_amd import contract as K  # noqa: E402
from abcnet_amd.ops import GraphAssembler, GraphScore, GraphSimilarity  # noqa: E402
from molrows import ASSEMBLE_DEFAULTS, ASSEMBLE_POINTERS, SCORE_DEFAULTS, SCORE_POINTERS, fake_desc  # noqa: E402

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "abcnet_hip.h")


def z(*shape, dtype=torch.int32):
    return torch.zeros(shape, dtype=dtype)


# ------------------------------------------------------------------------------------------------------------- molecule rows
C4, A5, Q4, H = z(2, 4), z(2, 8, 5), z(2, 16, 4), z(2, 8)
# the malformed rows of test_graphscore_host, test_graphsim_host and test_molblock_host, once each: (rows, keywords)
BAD_ROWS = [((C4, z(2, 8, 4), Q4), {}), ((C4, A5, z(2, 16, 3)), {}), ((z(3, 4), A5, Q4), {}), ((z(2, 3), A5, Q4), {}),
            ((C4, A5, z(3, 16, 4)), {}), ((C4, z(2, 8), Q4), {}), ((C4, A5, z(2, 0, 4)), {}), ((None, A5, Q4), {}),
            ((C4, A5.numpy(), Q4), {}), ((C4, z(2, 2049, 5), Q4), dict(max_cap_atoms=2048)), ((C4, z(2, 513, 5), Q4), dict(max_cap_atoms=512)),
            ((C4, A5, Q4), dict(n_valid=z(2))), ((C4, A5, Q4, z(2, 9)), dict(need_implh=True)), ((C4, A5, Q4, None), dict(need_implh=True))]


@pytest.mark.parametrize("who", ["MolBlockWriter", "GraphScore", "a caller yet to come"])
def test_molecule_rows_refuse_malformed_rows_under_the_callers_name(who):
    for rows, kw in BAD_ROWS:
        with pytest.raises(ValueError, match="^" + who):           # (never AbcNetHipError: every tensor here is a host tensor)
            K.MoleculeRows.checked(who, *rows, **kw)
    # well-formed host tensors, at the limit too: there is no CPU form
    for rows, kw in (((C4, A5, Q4), {}), ((C4, A5, Q4, H), dict(need_implh=True)), ((C4, z(2, 512, 5), Q4), dict(max_cap_atoms=512)),
                     ((C4, A5, Q4), dict(n_valid=z(1))), ((K.MoleculeRows(C4, A5, Q4, H),), dict(need_implh=True))):
        with pytest.raises(L.AbcNetHipError, match="^" + who):
            K.MoleculeRows.checked(who, *rows, **kw)
    # an object goes through the same check as the tensors it holds
    with pytest.raises(ValueError, match="^" + who):
        K.MoleculeRows.checked(who, K.MoleculeRows(C4, z(2, 513, 5), Q4), max_cap_atoms=512)


def test_candidate_lists_refuse_malformed_lists_under_the_callers_name():
    c, a, q, r = z(2, 4), z(2, 8, 5), z(2, 16, 4), z(2, 16, dtype=torch.float32)
    for lists in ((c, z(2, 8, 4), q, r), (c, a, z(2, 16, 3), r), (z(3, 4), a, q, r), (z(2, 3), a, q, r), (c, a, z(3, 16, 4), r),
                  (c, z(2, 8), q, r), (c, a, q, z(2, 15, dtype=torch.float32)), (c, a, q, z(3, 16, dtype=torch.float32)),
                  (None, a, q, r), (c, a, q, r.numpy())):
        for who, call in (("someone", lambda *t: K.CandidateLists.checked("someone", *t)), ("GraphAssembler", GraphAssembler)):
            with pytest.raises(ValueError, match="^" + who):
                call(*lists)
    for lists in ((c, a, q, r), (K.CandidateLists(c, a, q, r),)):
        with pytest.raises(L.AbcNetHipError, match="^someone"):
            K.CandidateLists.checked("someone", *lists)


# ------------------------------------------------------------------------------------------------------------- graph records
def test_graph_records_validation_needs_no_device():
    a = np.array([[1, 1, 1, 0], [3, 1, 2, 0], [3, 5, 3, -1]], np.int64)
    q = np.array([[0, 1, 1], [1, 2, 2]], np.int64)
    ok = lambda graphs, B=2, max_atoms=3, max_bonds=2: K.GraphRecords.validate(graphs, B, max_atoms, max_bonds)
    got = ok([(a, q), (a[:0], q[:0])])
    assert [(x.dtype, y.dtype, x.flags.c_contiguous, y.flags.c_contiguous) for x, y in got] == [(np.int32, np.int32, True, True)] * 2
    assert got[0][0].tolist() == a.tolist() and got[0][1].tolist() == q.tolist() and ok([]) == []
    bond = lambda i, j: np.array([[i, j, 1]], np.int32)
    for what, graphs, kw in (("atoms width", [(a[:, :3], q)], {}), ("bonds width", [(a, q[:, :2])], {}), ("atoms 1-d", [(a[0], q)], {}),
                             ("atoms over capacity", [(a, q)], dict(max_atoms=2)), ("bonds over capacity", [(a, q)], dict(max_bonds=1)),
                             ("i == j", [(a, bond(1, 1))], {}), ("i > j", [(a, bond(2, 1))], {}), ("j == n", [(a, bond(0, 3))], {}),
                             ("i < 0", [(a, bond(-1, 1))], {}), ("more than B records", [(a, q)] * 3, {})):
        with pytest.raises(ValueError):
            print(what)
            ok(graphs, **kw)


# ------------------------------------------------------------------------------------------------------------------ the limits
def test_limits_are_the_headers_at_the_classes_and_at_the_launchers():
    header = open(HEADER).read()
    enum = dict((k, int(v)) for k, v in re.findall(r"(ABC_MAX_\w+) = (\d+)", header[header.index("enum abc_decoder_limit"):]))
    assert enum == {"ABC_MAX_CAP_ATOMS": L.MAX_CAP_ATOMS, "ABC_MAX_BOND_PEAKS": L.MAX_BOND_PEAKS,
                    "ABC_MAX_SCORE_RECORD": L.MAX_SCORE_RECORD, "ABC_MAX_SIM_ATOMS": L.MAX_SIM_ATOMS}
    assert (L.MAX_CAP_ATOMS, L.MAX_BOND_PEAKS, L.MAX_SCORE_RECORD, L.MAX_SIM_ATOMS) == (2048, 4096, 1024, 512)
    lib = L.load()
    q = z(2, 16, 4)

    def refused(fn, struct, pointers, defaults, **kw):
        assert fn(C.byref(fake_desc(struct, pointers, defaults, **kw)), None) == -1, kw
        return lib.abc_last_error()

    # the classes: one past the limit is a ValueError, the limit itself passes every shape check (and then finds no device)
    for cls, kw, limit in ((GraphScore, {}, L.MAX_CAP_ATOMS), (GraphSimilarity, {}, L.MAX_SIM_ATOMS)):
        with pytest.raises(ValueError, match=str(limit)):
            cls(z(2, 4), z(2, limit + 1, 5), q, **kw)
        with pytest.raises(L.AbcNetHipError):
            cls(z(2, 4), z(2, limit, 5), q, **kw)
    for cls, field, limit in ((GraphScore, "max_atoms", L.MAX_SCORE_RECORD), (GraphScore, "max_bonds", L.MAX_SCORE_RECORD),
                              (GraphSimilarity, "max_atoms", L.MAX_SIM_ATOMS)):
        with pytest.raises(ValueError, match=str(limit)):
            cls(z(2, 4), z(2, 8, 5), q, **{field: limit + 1})
        with pytest.raises(L.AbcNetHipError):
            cls(z(2, 4), z(2, 8, 5), q, **{field: limit})
    # the launchers.  (PeakExtractor and GraphAssembler have no refusal of their own for cap_atoms: their launchers refuse at run().)
    score = (lib.abc_graph_score_update, L.GraphScoreDesc, SCORE_POINTERS, SCORE_DEFAULTS)
    sim = (lib.abc_graph_similarity_update, L.GraphSimilarityDesc, SCORE_POINTERS, SCORE_DEFAULTS)
    assert b"cap_atoms" in refused(*score, cap_atoms=L.MAX_CAP_ATOMS + 1)
    assert b"max_atoms" in refused(*score, max_atoms=L.MAX_SCORE_RECORD + 1) and b"max_bonds" in refused(*score, max_bonds=L.MAX_SCORE_RECORD + 1)
    assert b"cap_atoms" in refused(*sim, cap_atoms=L.MAX_SIM_ATOMS + 1) and b"max_atoms" in refused(*sim, max_atoms=L.MAX_SIM_ATOMS + 1)
    assert b"cap_atoms" in refused(lib.abc_assemble_graphs, L.AssembleDesc, ASSEMBLE_POINTERS, ASSEMBLE_DEFAULTS, cap_atoms=L.MAX_CAP_ATOMS + 1)
    extract = (L.ExtractDesc, ("work", "work_masks", "counts", "atoms", "bonds", "bond_rho"), dict(B=2, h=8, w=8, cap_atoms=512, cap_bonds=64))
    assert b"cap_atoms" in refused(lib.abc_extract_peaks, *extract, cap_atoms=L.MAX_CAP_ATOMS + 1)
    # the bond-peak limit is no field of a descriptor, so nothing can refuse it: it is the extractor's scratch per image, and past
    # it a list is truncated (PeakExtractor.lists() reports that from counts[b][2], on the device: tests/test_gpu_extract.py)
    d = fake_desc(*extract)
    assert lib.abc_extract_work_masks(C.byref(d)) == 2 * L.MAX_BOND_PEAKS
    assert lib.abc_extract_work_ints(C.byref(d)) == 2 * (512 + L.MAX_BOND_PEAKS)


# ------------------------------------------------------------------------------------------------- the self-sized descriptors
def test_self_sized_table_names_the_five_descriptors():
    assert [st for st, _ in L.SELF_SIZED] == [L.EvalDesc, L.GraphScoreDesc, L.GraphSimilarityDesc, L.MolBlockDesc, L.ScanDesc]
    lib = L.load()
    for st, size_fn in L.SELF_SIZED:
        assert st not in L._STRUCTS and L.SYMBOLS[size_fn] == (C.c_int, [])
        assert getattr(lib, size_fn)() == C.sizeof(st)


# ------------------------------------------------------------------------------------------- the runner's constructor flags
RUNNER_FLAGS = ("assemble", "evaluate", "score_graphs", "score_similarity", "score_identity", "molblocks", "smiles", "aromatize",
                "smiles_stereo", "smiles_double_bonds", "smiles_canonical")


def _first_refusal(f):
    """the refusals of InferenceRunner.__init__ as they stood before the two tables (FLAG_NEEDS, FLAG_REFUSED), in their order"""
    for flag in ("score_graphs", "score_similarity", "score_identity"):
        if f[flag] and not (f["assemble"] and f["evaluate"]):
            return ("InferenceRunner(%s=True) scores the assembled molecules of an evaluating step: it needs "
                    "assemble=True and evaluate=True" % flag)
    for flag in ("molblocks", "smiles"):
        if f[flag] and not f["assemble"]:
            return ("InferenceRunner(%s=True) writes the text of the assembled molecules of the step: it needs "
                    "assemble=True" % flag)
    if f["aromatize"] and not f["assemble"]:
        return ("InferenceRunner(aromatize=True) perceives the aromatic rings of the assembled molecules of the step: it "
                "needs assemble=True")
    if f["smiles_stereo"] and not f["smiles"]:
        return "InferenceRunner(smiles_stereo=True) is a form of the SMILES stage: it needs smiles=True"
    if f["smiles_double_bonds"] and not f["smiles"]:
        return "InferenceRunner(smiles_double_bonds=True) is a form of the SMILES stage: it needs smiles=True"
    if f["smiles_canonical"] and f["smiles_double_bonds"]:
        return ("InferenceRunner(smiles_canonical=True, smiles_double_bonds=True): a text with double-bond marks on the "
                "canonical order would not be canonical (the drawn geometry is not in the invariant)")
    if f["smiles_canonical"] and not f["smiles"]:
        return "InferenceRunner(smiles_canonical=True) is a form of the SMILES stage: it needs smiles=True"
    if f["smiles_canonical"] and f["smiles_stereo"]:
        return ("InferenceRunner(smiles_canonical=True, smiles_stereo=True): a stereo text on the canonical order would not "
                "be canonical (wedge ownership and the drawn geometry are not in the invariant)")
    return None


def test_runner_flag_tables_refuse_every_combination_with_the_same_first_message():
    from abcnet_amd.infer import FLAG_NEEDS, FLAG_REFUSED, InferenceRunner, check_flags
    from molrows import Heads
    assert {f for group, needs, _ in FLAG_NEEDS for f in group + needs} | {f for a, b, _ in FLAG_REFUSED for f in (a, b)} == set(RUNNER_FLAGS)
    refused = seen = 0
    for bits in range(1 << len(RUNNER_FLAGS)):
        flags = {name: bool(bits >> i & 1) for i, name in enumerate(RUNNER_FLAGS)}
        want = _first_refusal(flags)
        if want is None:
            check_flags(flags)
            continue
        with pytest.raises(ValueError) as e:
            check_flags(flags)
        assert str(e.value) == want, flags
        refused += 1
        if bits % 7 == 0:                # (through the constructor too: the refusals come before it reads the model or a device)
            with pytest.raises(ValueError) as e:
                InferenceRunner(Heads(), 2, 64, 64, **flags)
            assert str(e.value) == want, flags
            seen += 1
    assert refused > 1500 and seen > 200
