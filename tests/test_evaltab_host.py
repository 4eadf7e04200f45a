"""CPU tier of the evaluation tables (test_accuracy.py:105-298): the torch oracle against the golden generated from the
reference text, the golden's own non-degeneracy, the mirror struct, and every refusal of abc_eval_tables_update -- all of
which happen before a launch."""
import ctypes as C
import os

import numpy as np
import pytest

import abcnet_amd  # noqa: F401
from abcnet_amd import _lib as L
from abcnet_amd.ops import METER_NAMES, eval_tables_from_counts
from abcnet_amd.synthetic import synthetic_targets

import evaltab_oracle as eo


@pytest.fixture(scope="module")
def gold(golden_dir):
    return np.load(os.path.join(golden_dir, "evaltab_128.npz"))


def test_oracle_matches_golden(gold):
    tg = synthetic_targets(2, 128, seed=3)
    res = eo.evaluate(eo.confusable_logits(tg, seed=19), tg)
    for k in eo.TABLES:
        assert np.array_equal(res[k], gold[k]), k
    assert METER_NAMES == [n[len("train_"):] for n in gold["names"]]
    # (the reference stores ratio * count in f32: 67.000002-style residue)
    for n, s, c in zip(METER_NAMES, gold["sum"], gold["count"]):
        num, den = res["meters"][n]
        assert abs(num - s) <= 1e-5 * max(1.0, abs(s)), (n, num, s)
        assert abs(den - c) <= 1e-5 * max(1.0, abs(c)), (n, den, c)
    # the (tp, tn, fp, fn) rows follow from the confusion matrices, which is how the device derives them
    for k, m in res["confusion"].items():
        tp, row, col = np.diag(m), m.sum(1), m.sum(0)
        assert np.array_equal(res[k], np.stack([tp, m.sum() - row - col + tp, col - tp, row - tp], axis=1)), k


def test_golden_is_not_degenerate(gold):
    assert eo.non_degenerate({k: gold[k] for k in eo.TABLES}) is None
    for k in ("atom_detection", "bond_detection"):
        assert not gold[k][:, 1].any()                 # column 1 is never written
        assert gold[k][1:, 2].sum() == 0 and gold[k][0, 2] > 0      # a false positive on an empty pixel is booked under class 0


def test_counts_layout_round_trip():
    counts = np.arange(1, L.EVAL_NCOUNT + 1)
    tab, conf = eval_tables_from_counts(counts)
    assert tab["atom_detection"].shape == (14, 4) and tab["bond_detection"].shape == (6, 4)
    assert tab["atom_detection"][0].tolist() == [1, 0, 2, 3] and tab["bond_detection"][5].tolist() == [58, 0, 59, 60]
    assert conf["atom_type"][0, 0] == 61 and conf["atom_charge"][0, 0] == 257 and conf["bond_type"][5, 5] == 301
    m = conf["atom_charge"]
    assert tab["atom_charge"][1].tolist() == [m[1, 1], m[0, 0] + m[0, 2] + m[2, 0] + m[2, 2], m[0, 1] + m[2, 1], m[1, 0] + m[1, 2]]


def test_mirror_struct_matches_library():
    lib = L.load()
    assert lib.abc_eval_desc_size() == C.sizeof(L.EvalDesc)
    for s in ("abc_eval_tables_blocks", "abc_eval_tables_update", "abc_eval_desc_size"):
        assert s in L.SYMBOLS
    assert L.EvalDesc not in L._STRUCTS


INPUTS = ["atom_mask", "bond_mask", "omega_mask", "rho_abs", "types", "charges", "hs", "t_atom", "t_types", "t_charges", "t_hs", "t_bond",
          "t_btypes", "t_rho", "t_omega"]
WORK = ["partial", "counts_last", "counts_totals", "meters_last", "meters_totals"]


def _desc():
    """a descriptor that would pass every check (the addresses are never dereferenced: each test breaks one field)"""
    d = L.EvalDesc()
    for i, f in enumerate(INPUTS + WORK + ["btypes"]):
        setattr(d, f, 0x1000 * (i + 1))
    d.B, d.h, d.w = 2, 32, 32
    return d


def _refused(d, word):
    lib = L.load()
    assert lib.abc_eval_tables_update(C.byref(d), None) == -1          # ABC_EINVAL, before any launch
    assert word in lib.abc_last_error().decode(), lib.abc_last_error()


@pytest.mark.parametrize("field", ["B", "h", "w"])
def test_empty_shape_is_refused(field):
    d = _desc()
    setattr(d, field, 0)
    _refused(d, "empty")
    assert L.load().abc_eval_tables_blocks(C.byref(d)) == -1


@pytest.mark.parametrize("field", WORK)
def test_null_workspace_is_refused(field):
    d = _desc()
    setattr(d, field, None)
    _refused(d, "workspace")


@pytest.mark.parametrize("field", INPUTS)
def test_null_input_is_refused(field):
    d = _desc()
    setattr(d, field, None)
    _refused(d, "null")


def test_bond_type_source_must_be_exactly_one():
    d = _desc()
    d.btype_idx = 0x100000
    _refused(d, "exactly one")
    d.btypes, d.btype_idx = None, None
    _refused(d, "exactly one")


def test_blocks_of_a_valid_shape():
    d = _desc()
    d.B, d.h, d.w = 3, 40, 40
    assert L.load().abc_eval_tables_blocks(C.byref(d)) == (3 * 40 * 40 + 255) // 256
